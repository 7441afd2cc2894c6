"""GPU (-m gpu): the posterior mean, variance, covariance and IVAR held to per-point error bounds.

Cases, metric, references, comparators and the bound rule: tests/posterior_ref.py (pinned on the CPU by tests/test_posterior_host.py).
Every evaluation set carries 20 points that ARE training points and 20 within 1e-7 of one: at noise 1e-6 their variances are
1e-6, and omega = max_j |got_j - ref_j| / (u S_j) judges them to the digits their inputs determine.

  tight rule        K, K(X, Z), k(z, z) and K(Z, Z) are the DEVICE's own fills taken back (the posterior's internal fills are the same
                    doubles: same KParams, same launch_kfill), the reference is formed from them in longdouble: the solve and the
                    reductions are judged alone.  device omega <= 8 x max(LAPACK, emulation b = 128) on the same arrays.
  from-points rule  the reference starts from the points (cov_ld); the error in excess of the assembly's first-order allowance is
                    held to the same bound.  Only the fills' distance form and centre come from the device (kfill_plan).

Run with -s: every case prints device, comparators and ratio per metric ("Posterior accuracy", quotes them)."""
import numpy as np
import pytest

import kernel_reference as KR
import posterior_ref as P

pytestmark = pytest.mark.gpu

IVAR_SIZES = (1, 2, 3, 130, 1023, 1024, 1025, 2049)


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def spec_of(dev, spec):
    return dev.KernelSpec(P.KIND_ID[spec["kind"]], spec["d"], KR.hyp_of(spec))


def boxed(dev, ctx, Z, X):
    """Z on the device carrying the bounding box of X and Z together: its symmetric fill then centres where the posterior's fills
    do (gpx_posterior_cov fills K(Z, Z) with the parameters of the whole call)."""
    return dev.points_slice(ctx, np.vstack([Z, X]), 0, Z.shape[0])


class Fit:
    """One case on the device: the fills taken back, the factor, alpha from potrs."""

    def __init__(self, dev, ctx, name, m=P.M_EVAL, moved=False, Z=None):
        c = P.case(name, m)
        self.c, self.sp = c, spec_of(dev, c["spec"])
        self.X = c["X2"] if moved else c["X"]
        self.Z = c["Z"] if Z is None else Z
        self.dX, self.dZ = dev.points(ctx, self.X), dev.points(ctx, self.Z)
        Kd = dev.kfill(ctx, self.sp, self.dX, nugget=c["nugget"])
        self.K = Kd.to_host()
        self.B = dev.kfill(ctx, self.sp, self.dX, Z=self.dZ).to_host()
        self.kd = dev.kdiag(ctx, self.sp, self.dZ)
        ctx.sync()
        self.L = dev.potrf(ctx, Kd)
        self.alpha = dev.potrs(ctx, self.L, c["y"])

    def kzz(self, dev, ctx):
        return dev.kfill(ctx, self.sp, boxed(dev, ctx, self.Z, self.X)).to_host()


def form_of(dev, ctx, sp, A, B=None):
    exact, centre = dev.kfill_plan(ctx, sp, A, B)
    return ("diff", None) if exact else ("expanded", centre)


@pytest.mark.parametrize("name", P.SMALL)
def test_tight_rule(dev, ctx, name):
    f = Fit(dev, ctx, name)
    c, sp = f.c, f.sp
    al = P.host_alpha(name)
    kzz = f.kzz(dev, ctx)
    mean_h, var = dev.posterior(ctx, sp, f.L, f.dX, al, f.dZ)
    mean_d, var2 = dev.posterior(ctx, sp, f.L, f.dX, f.alpha, f.dZ)
    assert np.array_equal(var, var2)
    assert np.array_equal(dev.posterior(ctx, sp, f.L, f.dX, None, f.dZ, want_mean=False)[1], var)
    cov = dev.posterior_cov(ctx, sp, f.L, f.dX, f.dZ)
    ivar = dev.ivar(ctx, sp, f.L, f.dX, f.dZ)
    fit_ivar = dev.fit_ivar(ctx, sp, dev.kfill(ctx, sp, f.dX, nugget=c["nugget"]), f.dX, f.dZ)
    assert fit_ivar == ivar, (fit_ivar, ivar)

    ref = P.reference(f.K, f.B, f.kd, c["y"], al, kzz)
    cmp_ = P.comparator_omegas(ref, f.K, f.B, f.kd, c["y"], al, kzz)
    got = P.omegas({"v": var, "m": mean_h, "M": mean_d, "c": cov, "I": ivar}, ref)
    got["v(diag cov)"] = P.omega(np.diag(cov), ref["val"]["v"], ref["scale"]["v"])
    got["v(on point)"] = P.omega(var, ref["val"]["v"], ref["scale"]["v"], where=slice(0, P.N_ON))
    got["v(near point)"] = P.omega(var, ref["val"]["v"], ref["scale"]["v"], where=slice(P.N_ON, P.N_ON + P.N_NEAR))
    for k in ("v(diag cov)", "v(on point)", "v(near point)"):
        cmp_[k] = cmp_["v"]
    print("\n%s (tight): smallest variance %.3e, rel(var) %.1e, rel(mean) %.1e"
          % (name, float(np.min(var)), P.rel(var, ref["val"]["v"]), P.rel(mean_d, ref["val"]["M"])))
    failures = P.check_all(name, got, cmp_)

    # the cost after a refit that kept leading rows: W of the old design updated in place, against a fresh reference
    _, W = dev.ivar(ctx, sp, f.L, f.dX, f.dZ, keep=True)
    g = Fit(dev, ctx, name, moved=True)
    ref2 = P.reference(g.K, g.B, g.kd)
    cmp2 = P.comparator_omegas(ref2, g.K, g.B, g.kd)
    for keep in (128, 256):
        L2 = dev.refit_rows(ctx, sp, g.dX, c["nugget"], f.L, keep)
        upd = dev.ivar_update(ctx, sp, L2, g.dX, g.dZ, dev.clone(ctx, W), keep)
        failures += P.check_all("%s ivar_update keep=%d" % (name, keep), P.omegas({"I": upd}, ref2), cmp2)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", P.FROM_POINTS)
def test_from_points_rule(dev, ctx, name):
    f = Fit(dev, ctx, name)
    c, sp = f.c, f.sp
    al = P.host_alpha(name)
    plans = [form_of(dev, ctx, sp, f.dX), form_of(dev, ctx, sp, f.dX, f.dZ), form_of(dev, ctx, sp, boxed(dev, ctx, f.Z, f.X))]
    ref = P.reference_from_points(c["spec"], f.X, f.Z, c["nugget"], c["y"], al, want_cov=True,
                                  forms=tuple(p[0] for p in plans), centers=tuple(p[1] for p in plans))
    h = ref["f64"]
    cmp_ = P.comparator_omegas(ref, h["K"], h["B"], h["kd"], c["y"], al, h["kzz"])
    mean_h, var = dev.posterior(ctx, sp, f.L, f.dX, al, f.dZ)
    mean_d, _ = dev.posterior(ctx, sp, f.L, f.dX, f.alpha, f.dZ, want_var=False)
    values = {"v": var, "m": mean_h, "M": mean_d, "c": dev.posterior_cov(ctx, sp, f.L, f.dX, f.dZ),
              "I": dev.ivar(ctx, sp, f.L, f.dX, f.dZ)}
    raw = P.omegas(values, ref, allowance=False)
    print("\n%s (from points, forms %s): omega before the allowance  %s"
          % (name, "/".join(p[0] for p in plans), "  ".join("%s %.2f" % kv for kv in raw.items())))
    failures = P.check_all(name + " from points", P.omegas(values, ref), cmp_)
    assert not failures, "\n".join(failures)


def test_large_case_out_of_place_solve(dev, ctx):
    """n = 2200 (2304 padded): the out-of-place cross solve through the block inverses, ragged last block.  Variance on the sampled
    columns against the refined reference; the mean from a given alpha on every column."""
    name = "m52-oop"
    f = Fit(dev, ctx, name)
    al = P.host_alpha(name)
    mean_h, var = dev.posterior(ctx, f.sp, f.L, f.dX, al, f.dZ)
    ivar = dev.ivar(ctx, f.sp, f.L, f.dX, f.dZ)
    del f.L
    ctx.trim()
    cols = P.sampled_cols()
    rs = P.reference_sampled(f.K, f.B, f.kd, cols)
    cmp_ = P.comparator_omegas(rs, f.K, f.B, f.kd, cols=cols)
    rm = P.reference_mean(f.B, al)
    cmp_["m"] = {"lapack": P.omega(f.B.T @ al, rm["val"]["m"], rm["scale"]["m"])}
    got = {"v": P.omega(var[cols], rs["val"]["v"], rs["scale"]["v"]), "m": P.omega(mean_h, rm["val"]["m"], rm["scale"]["m"])}
    print("\n%s (tight, %d sampled columns): smallest variance %.3e" % (name, cols.size, float(np.min(var))))
    failures = P.check_all(name, got, cmp_)
    assert ivar == P.pairwise_mean(var)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("m", IVAR_SIZES)
def test_ivar_is_the_halving_sum_of_the_variances(dev, ctx, m):
    """gpx_ivar = pairwise_mean (api.hip: h = ceil(m / 2), v[i] += v[i + h]) of gpx_posterior's variances, bit for bit: additions and
    one division, restated in NumPy."""
    c = P.case("se-well")
    sp = spec_of(dev, c["spec"])
    dX = dev.points(ctx, c["X"])
    L = dev.potrf(ctx, dev.kfill(ctx, sp, dX, nugget=c["nugget"]))
    Z = np.vstack([c["Z"][:min(m, 40)], np.random.default_rng(m).uniform(-1.0, 1.0, (max(m - 40, 0), 3))])
    dZ = dev.points(ctx, Z)
    _, var = dev.posterior(ctx, sp, L, dX, None, dZ, want_mean=False)
    assert dev.ivar(ctx, sp, L, dX, dZ) == P.pairwise_mean(var)
    assert dev.ivar(ctx, sp, L, dX, dZ, keep=True)[0] == P.pairwise_mean(var)


def test_chunk_seams(dev, ctx, monkeypatch):
    """m = 300 in chunks of 128, 128 and 44 evaluation points (GPX_CROSS_BYTES=1): the bits of the unchunked call, and the per-point
    bound in both."""
    name = "se-tiny-noise"
    f = Fit(dev, ctx, name, m=300)
    al = P.host_alpha(name)
    mean, var = dev.posterior(ctx, f.sp, f.L, f.dX, al, f.dZ)
    ivar = dev.ivar(ctx, f.sp, f.L, f.dX, f.dZ)
    monkeypatch.setenv("GPX_CROSS_BYTES", "1")
    mean_c, var_c = dev.posterior(ctx, f.sp, f.L, f.dX, al, f.dZ)
    ivar_c = dev.ivar(ctx, f.sp, f.L, f.dX, f.dZ)
    monkeypatch.delenv("GPX_CROSS_BYTES")
    assert np.array_equal(mean_c, mean) and np.array_equal(var_c, var) and ivar_c == ivar
    ref = P.reference(f.K, f.B, f.kd, alpha=al)
    cmp_ = P.comparator_omegas(ref, f.K, f.B, f.kd, alpha=al)
    print()
    failures = P.check_all(name + " m=300 chunked", P.omegas({"v": var_c, "m": mean_c, "I": ivar_c}, ref), cmp_)
    assert not failures, "\n".join(failures)


_FULL_SET = {}


def full_set_comparators(dev, ctx, name):
    """The comparators' figures on all M_EVAL evaluation points of a case (device fills, tight rule), once per module."""
    if name not in _FULL_SET:
        f = Fit(dev, ctx, name)
        al = P.host_alpha(name)
        _FULL_SET[name] = P.comparator_omegas(P.reference(f.K, f.B, f.kd, alpha=al), f.K, f.B, f.kd, alpha=al)
    return _FULL_SET[name]


@pytest.mark.parametrize("m", [1, 128, 129])
def test_slices_of_the_evaluation_set(dev, ctx, m):
    """Z[:1], Z[:128], Z[:129]: one point, one full tile, one point into the second tile.  (No bit identity across different Z is
    claimed: the fills centre on the bounding box of X and Z.)  On one point a comparator's omega is a single draw (0.1 where the
    130 points give 4 .. 6), so the comparators' figures on the case's full evaluation set stand beside those on the slice."""
    name = "se-tiny-noise"
    f = Fit(dev, ctx, name, Z=np.ascontiguousarray(P.case(name)["Z"][:m]))
    al = P.host_alpha(name)
    mean, var = dev.posterior(ctx, f.sp, f.L, f.dX, al, f.dZ)
    ivar = dev.ivar(ctx, f.sp, f.L, f.dX, f.dZ)
    ref = P.reference(f.K, f.B, f.kd, alpha=al)
    cmp_ = P.comparator_omegas(ref, f.K, f.B, f.kd, alpha=al)
    full = full_set_comparators(dev, ctx, name)
    for k in ("v", "m"):
        cmp_[k]["full set"] = max(full[k][r] for r in P.ROUTES)
    cmp_["I"]["v/sqrt(m)"] = max(cmp_["v"].values()) / np.sqrt(float(m))
    print()
    failures = P.check_all("%s Z[:%d]" % (name, m), P.omegas({"v": var, "m": mean, "I": ivar}, ref), cmp_)
    assert not failures, "\n".join(failures)


def test_sign_of_the_variance_on_training_points(dev, ctx):
    """noise 1e-6: at a z that IS a training point the variance is noise (1 - ...) > 0, and the device returns it positive (its
    distance from the reference is under the tight rule above); the class API returns the same numbers -- the abs() of
    evaluate(compvar=1) never fires."""
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelSquaredExponential
    name = "se-tiny-noise"
    f = Fit(dev, ctx, name)
    c = f.c
    mean, var = dev.posterior(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ)
    ref = P.reference(f.K, f.B, f.kd)
    on = np.asarray(ref["val"]["v"][:P.N_ON], dtype=float)
    print("\non-point variances: reference %.3e .. %.3e, device %.3e .. %.3e" % (on.min(), on.max(), var[:P.N_ON].min(), var[:P.N_ON].max()))
    assert np.all(on > 0.0) and np.all(on <= c["nugget"])
    assert np.all(var > 0.0), var.min()
    gp = GP(KernelSquaredExponential(c["spec"]["cl"], c["spec"]["signalSize"], 3), c["nugget"])
    gp.train(c["X"], c["y"])
    gmean, gvar = gp.evaluate(c["Z"], compvar=1)
    assert np.array_equal(np.ravel(gvar), var)
    assert np.array_equal(np.ravel(gmean), mean)
