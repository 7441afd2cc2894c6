"""GPU (-m gpu): the point gradients of the posterior variance and of IVAR (gpexp_amd/csrc/grad.hip: gpx_var_grad, gpx_var_grad_newpt,
gpx_ivar_grad, gpx_ivar_grad_w, gpx_ivar_grad_rows) held to per-entry error bounds, through gpexp_amd.device only.

Quantities, metric, allowance, comparators and the bound rule: tests/pointgrad_ref.py (pinned on the CPU by
tests/test_pointgrad_host.py).  K and K(X, Z) are the DEVICE's own fills taken back (the gradient's internal fill is the same doubles:
same KParams, same launch_kfill), the reference is formed from them in longdouble; Dz and Dx come from the points, and the device's
own error in them is allowed for.  device omega <= 8 x max(LAPACK, emulation b = 128, 1) on the same arrays.

Run with -s: every case prints device, comparators and ratio per metric ("Point-gradient accuracy", quotes them).

MEASURED ON THE MI355X (device omega / largest comparator or 1; the bound is 8):
  entry point           metric        worst ratio   where (device omega / largest comparator)
  gpx_var_grad          omega_G       1.62          m52-tiny-noise n = 127, M = 127 (2.13 / 1.32)
  gpx_var_grad_newpt    omega_N       2.36          se-tiny-noise n = 129, M = 129 (3.06 / 1.30)
  gpx_ivar_grad         omega_I       1.02          mehler-1d n = 129, M = 129 (1.83 / 1.79)
  gpx_ivar_grad_w       omega_I       0.89          mehler-1d (1.44 / 1.63); 1e-12 of the plain call everywhere
  gpx_ivar_grad_rows    omega_I       0.03          m32-per-point n = 257, r0 = 128 (0.026 / 1)

  case (n = 300, M = 130)      omega_G device / top comparator   omega_N        omega_I          on-point G, N   near-point G, N
  se-well                      1.5 / 1 (floor)                   0 / 2.0        0 / 1            1.5, 0          0.57, 0
  se-tiny-noise                0.013 / 1                         3.4 / 3.4      8e-6 / 1         0.013, 0.62     0.007, 3.4
  m52-tiny-noise               0.61 / 1.2                        2.1 / 3.4      0.002 / 1        0.43, 2.0       0.61, 2.1
  m32-per-point                2.7 / 2.2                         5.1 / 6.1      0.023 / 1        0.55, 2.8       2.7, 5.1
  mehler-1d (n = 150, d = 1)   5.5 / 7.4                         3.9 / 2.2      1.4 / 1.6        5.1, 2.7        4.8, 2.5
  m32-per-point + nd, dups     2.9 / 3.9                         2.3 / 2.3      0.35 / 1         2.7, 2.3        2.9, 1.8
  m52-tiny-noise M = 257       1.4 / 1.7 (chunked = one chunk)   3.2 / 3.2                       column 256: 0.05, 0.04
  m52-large n = 4100, 16 cols  0.44 / 1                          4.8 / 2.3

A 0 is an error inside the allowance for the device's own Dz / Dx (<= 0.07 u S in G and I, 1.4 .. 4.7 u S in N).  Edge sweep
(n, M) = (1, 1) .. (257, 130), three kinds: omega_G 0 .. 2.1, omega_N 0 .. 5.2, omega_I <= 0.14, exactly 0 at n = 1; ratios <= 2.36.
sum_m var_grad = M ivar_grad: the gap is < 0.001 of the sum of the two bounds on every case.  No defect of grad.hip was found.
"""
import numpy as np
import pytest

import kernel_reference as KR
import pointgrad_ref as G
import posterior_ref as P

pytestmark = pytest.mark.gpu

ON, NEAR = slice(0, G.N_ON), slice(G.N_ON, G.N_ON + G.N_NEAR)


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


class Fit:
    """One problem on the device: the fills taken back, the factor."""

    def __init__(self, dev, ctx, p):
        spec = p["spec"]
        self.p, self.sp = p, dev.KernelSpec(P.KIND_ID[spec["kind"]], spec["d"], KR.hyp_of(spec))
        self.dX, self.dZ = dev.points(ctx, p["X"]), dev.points(ctx, p["Z"])
        Kd = dev.kfill(ctx, self.sp, self.dX, nugget=p["nugget"])
        self.K = Kd.to_host()
        self.B = dev.kfill(ctx, self.sp, self.dX, Z=self.dZ).to_host()
        ctx.sync()
        self.L = dev.potrf(ctx, Kd)

    def three(self, dev, ctx, nd=None):
        """{G, N, I} of the three plain entry points."""
        a = (ctx, self.sp, self.L, self.dX, self.dZ)
        return {"G": dev.var_grad(*a, noise_deriv=nd), "N": dev.var_grad_newpt(*a), "I": dev.ivar_grad(*a, noise_deriv=nd)}

    def rows(self, dev, ctx, ref, got, r0s):
        """omega_I of gpx_ivar_grad_w and of gpx_ivar_grad_rows at every r0, from the forward solve the cost kept; the kept-solve
        gradient against the plain one at the 1e-12 of the existing tests."""
        out = {}
        _, W = dev.ivar(ctx, self.sp, self.L, self.dX, self.dZ, keep=True)
        assert W is not None
        gw = dev.ivar_grad(ctx, self.sp, self.L, self.dX, self.dZ, W=W)
        assert P.rel(gw, got["I"]) <= 1e-12
        out["I(W=)"] = G.omegas({"I": gw}, ref)["I"]
        d = self.sp.d
        for r0 in r0s:
            g = dev.ivar_grad_rows(ctx, self.sp, self.L, self.dX, self.dZ, W, r0)
            assert g.shape == ((self.p["X"].shape[0] - r0) * d,)
            out["I(rows %d)" % r0] = G.omega(g, ref["val"]["I"][r0:], ref["scale"]["I"][r0:], ref["allow"]["I"][r0:])
        return out


def judge(label, f, got, split=True):
    """Reference and comparators on the fit's own arrays; {metric: device omega} with the on-point / near-point columns apart."""
    ref = G.reference(f.K, f.B, f.p)
    cmp_ = G.comparator_omegas(ref, f.K, f.B)
    om = G.omegas(got, ref)
    if split and f.p["Z"].shape[0] >= G.N_ON + G.N_NEAR:
        for k in ("G", "N"):
            om["%s(on point)" % k] = G.omegas({k: got[k]}, ref, where=ON)[k]
            om["%s(near point)" % k] = G.omegas({k: got[k]}, ref, where=NEAR)[k]
    return ref, cmp_, om


def finish(label, om, cmp_):
    print()
    failures = G.check_all(label, om, cmp_)
    assert not failures, "\n".join(failures)


# ---- A and F: the cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASES + ("mehler-1d",))
def test_cases(dev, ctx, name):
    """n = 300, M = 130 (Mehler, d = 1: n = 150): every entry point; gpx_ivar_grad_rows at r0 = 128, 256 (not offered for Mehler).
    And the two routes to the IVAR gradient against each other: sum_m var_grad = M x ivar_grad within the sum of the two bounds."""
    f = Fit(dev, ctx, G.problem(name))
    got = f.three(dev, ctx)
    ref, cmp_, om = judge(name, f, got)
    om.update(f.rows(dev, ctx, ref, got, () if name == "mehler-1d" else (128, 256)))
    n, d = f.p["X"].shape
    m = f.p["Z"].shape[0]
    gap = np.abs(np.sum(got["G"].reshape(n, d, m), axis=2) - m * got["I"].reshape(n, d))
    room = m * (G.U * G.MARGIN * ref["scale"]["I"] * (max(cmp_["G"].values()) + max(cmp_["I"].values())) + 2.0 * ref["allow"]["I"])
    # the test's own arithmetic: NumPy's pairwise sum over m (depth log2 m) and the product with m
    room = room + (np.log2(m) + 2.0) * G.U * np.sum(np.abs(np.asarray(ref["val"]["G"], dtype=float)), axis=2)
    print("\n%s: |sum_m var_grad - M ivar_grad| / (sum of the two bounds) <= %.3f" % (name, float(np.max(gap[room > 0] / room[room > 0]))))
    assert np.all(gap <= room)
    finish(name, om, cmp_)


# ---- B: heteroscedastic, duplicated rows ---------------------------------------------------------------------------------------------
def test_noise_derivative_and_coincidence_mask(dev, ctx):
    """m32-per-point with rows 17 and 140 copies of row 3 and nd = NoiseFunc.deriv(X): the mask and the -A_jj beta^2 term."""
    f = Fit(dev, ctx, G.problem("m32-per-point", hetero=True))
    got = f.three(dev, ctx, nd=f.p["nd"])
    ref, cmp_, om = judge("m32-per-point +nd", f, got)
    assert int(ref["f64"]["mask"].sum()) == 300 + 6
    finish("m32-per-point +nd", om, cmp_)


# ---- C: the edge sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", G.EDGES)
@pytest.mark.parametrize("kind", sorted(G.EDGE_KINDS))
def test_edge_shapes(dev, ctx, kind, n, m):
    """The leading n rows / M columns of a case: one workgroup per point with 1 .. 257 terms in its strided loop, 32-tiles of
    mirror_lower_tri_kernel with one live row, a single free row of gpx_ivar_grad_rows (n = 129, r0 = 128)."""
    name = G.EDGE_KINDS[kind]
    f = Fit(dev, ctx, G.problem(name, n, m))
    got = f.three(dev, ctx)
    ref, cmp_, om = judge(name, f, got, split=False)
    r0s = [r for r in (128, 256) if r < n]
    if r0s:
        om.update(f.rows(dev, ctx, ref, got, r0s))
    if n == 1:
        assert all(np.all(v == 0.0) for v in got.values())
    finish("%s n=%d M=%d" % (name, n, m), om, cmp_)


def test_edge_shape_mehler(dev, ctx):
    f = Fit(dev, ctx, G.problem("mehler-1d", 129, 129))
    ref, cmp_, om = judge("mehler-1d", f, f.three(dev, ctx), split=False)
    finish("mehler-1d n=129 M=129", om, cmp_)


# ---- D: chunk seams ------------------------------------------------------------------------------------------------------------------
def test_chunk_seams(dev, ctx, monkeypatch):
    """M = 257 in chunks of 128 + 128 + 1 evaluation points (GPX_CROSS_BYTES = 1): held to the bound, and equal to the one-chunk call
    to the 1e-13 of the existing tests."""
    name = "m52-tiny-noise"
    f = Fit(dev, ctx, G.problem(name, m=257))
    a = (ctx, f.sp, f.L, f.dX, f.dZ)
    one = {"G": dev.var_grad(*a), "N": dev.var_grad_newpt(*a)}
    monkeypatch.setenv("GPX_CROSS_BYTES", "1")
    got = {"G": dev.var_grad(*a), "N": dev.var_grad_newpt(*a)}
    monkeypatch.delenv("GPX_CROSS_BYTES")
    for k in got:
        assert P.rel(got[k], one[k]) <= 1e-13, (k, P.rel(got[k], one[k]))
    ref, cmp_, om = judge(name, f, got)
    for k in ("G", "N"):
        om["%s(one chunk)" % k] = G.omegas({k: one[k]}, ref)[k]
        om["%s(column 256)" % k] = G.omegas({k: got[k]}, ref, where=slice(256, 257))[k]
    finish(name + " M=257 chunked", om, cmp_)


# ---- E: the large-factor path --------------------------------------------------------------------------------------------------------
def test_large_factor_path(dev, ctx):
    """n = 4100 (4224 padded: the smallest n whose two solves for beta go through the factor's block inverses), M = 130, Matern-5/2,
    noise 1e-4.  G and N on 16 sampled columns against beta refined to 2^-60 (posterior_ref.reference_sampled)."""
    name = "m52-large"
    f = Fit(dev, ctx, G.problem(name))
    a = (ctx, f.sp, f.L, f.dX, f.dZ)
    Gd, Nd = dev.var_grad(*a), dev.var_grad_newpt(*a)
    del f.L
    ctx.trim()
    cols = P.sampled_cols()
    ref = G.reference_sampled(f.K, f.B, f.p, cols)
    cmp_ = G.comparator_omegas(ref, f.K, f.B)
    n, d = f.p["X"].shape
    got = {"G": Gd.reshape(n, d, -1)[:, :, cols], "N": Nd.reshape(-1, d)[cols]}
    finish(name + " (16 sampled columns)", G.omegas(got, ref), cmp_)
