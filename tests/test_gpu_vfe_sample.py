"""GPU (-m gpu): posterior sampling on VFE models (gpx_vfe_paths_create, gpx_vfe_posterior_cov, gpx_vfe_psampler_create and the
classes above them) held to tests/vfe_sample_ref.py.

 1. plumbing, tight: values and gradients against a longdouble replay from the device's OWN V (path_ref with X := S) within
    path_ref.MARGIN x its per-element bound, the arg-best exactly, two calls the same bits;
 2. the weights and the paths end to end against the longdouble reference from (X, S, y, noise, base): 1e-8 x max |reference|
    (tests/test_gpu_vfe.py's figure for VFE quantities against NumPy); on the noise-1e-2 cases and BLOCKED only -- a float64 LAPACK
    restatement stays within 3.5e-10 (V) and 2.7e-11 (values) of longdouble there, and is at 1.4e-6 / 4e-8 at noise 1e-4;
 3. the distribution, deterministically: the paths of the unit base draws give the linear map J, and J J^T is the finite-feature
    covariance, 1e-8 x max |cov|;
 4. bits: rows of a larger base, and three chunks of Z in a child process;
 5. the exact sampler: covariance, mean bits, factor, draws, arg-best, the refusal of a repeated point;
 6. the class API;  7. the allocator's books.

Every test prints its figures before it asserts (run with -s).  Measured on an MI355X:
  1. values / gradients / the gradient call's values against the replay from the device's own V, as a share of the bound (the cap is
     8 x the bound): at most 0.051 / 0.072 / 0.053 (se, d = 1, nu = 1); nu = 1152: 0.001 / 0.000 / 0.000;
  2. |V - ref| / max |V_ref| and |f - ref| / max |ref| per case, in the order of PLUMBING: 8.6e-15 / 1.7e-14, 1.5e-14 / 5.4e-14,
     2.0e-12 / 6.0e-13, 9.4e-13 / 3.7e-13, 3.0e-10 / 1.0e-10 (nu = 129), 9.8e-13 / 4.2e-13, 1.2e-12 / 6.6e-13; BLOCKED (nu = 1152)
     1.5e-9 / 3.1e-10 -- all under the cap 1e-8;
  3. zero path against the mean at most 1.3e-12, against the device's own predictor 1.6e-15, J J^T against the finite-feature covariance
     at most 6.1e-15;
  5. posterior_cov against the reference at most 9.4e-12 (nu = 129; 1.7e-14 on the smallest case), its diagonal against posterior's
     variance at most 5.9e-14 (Mehler), draws at most 0.31 of their bound, the factor at most 0.12 of its bound on 20 of the 21 cases
     and 0.46 on se-d1-N5-nu1-noise0.01-M129: 129 points on a line under a squared exponential with ONE inducing point, a covariance of
     low numerical rank whose other eigenvalues are the jitter 1e-10 (condition 1.8e11, two 128-tiles).  There ONE refinement step
     leaves 79 x the bound (9.1e-12), and the constructor, which measures the residual on the device, repeats the step (sample.hip,
     psampler_factor's `verify`); the other cases are left after the first step with the bits they had."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as FR
import path_ref as PR
import sample_ref as SR
import vfe_sample_ref as VS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))

# (kind, d, lengths, signalSize, N, nu, noise, seed), generated as fitc_grad_ref.case does; the hyper-parameters are those of
# fitc_grad_ref.CASES for the same kind and dimension where it has them (se d = 1 and 8, matern32 d = 2)
SMALL = [("se", 1, [0.1], 1.0, 5, 1, 1e-2, 31),
         ("matern32", 2, [0.5], 1.4, 9, 3, 1e-2, 32),
         ("matern52", 3, [0.7], 1.1, 40, 17, 1e-2, 33),
         ("se", 8, [1.0, 1.2, 0.8, 1.5, 0.9, 1.1, 1.3, 0.7], 1.0, 130, 40, 1e-2, 34),
         ("matern32", 2, [0.5], 1.4, 257, 129, 1e-2, 35),          # nu one past a 128 tile
         ("matern52", 32, [4.0], 1.2, 40, 16, 1e-2, 36)]
LOW_NOISE = ("matern52", 3, [0.7], 1.1, 40, 17, 1e-6, 37)           # the replay checks only (1 and 5)
PATHS = (1, 16, 17, 33)
FEATS = (1, 5, 64, 257)
# (case, paths, features, M)
PLUMBING = [(c, PATHS[i % 4], FEATS[(i + 1) % 4], 33 if i != 1 else 1) for i, c in enumerate(SMALL)] + \
           [(SMALL[2], 33, 1, 1), (LOW_NOISE, 17, 64, 33)]
BLOCKED = (FR.BLOCKED, 17, 64, 17)
TOL = 1e-8


def case_id(c):
    return "%s-d%d-N%d-nu%d-noise%g" % (c[0], c[1], c[4], c[5], c[6])


def plumb_id(p):
    return "%s-P%d-L%d-M%d" % (case_id(p[0]), p[1], p[2], p[3])


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def eval_points(c, S, m):
    """m points in the cube, one of them ON an inducing point."""
    Z = np.random.default_rng(500 + c[7] + m).uniform(-1.0, 1.0, (m, c[1]))
    Z[min(1, m - 1)] = S[0]
    return Z


_REFERENCE = {}


def reference_model(c):
    """The longdouble model of a case, computed once and shared (read-only)."""
    if repr(c) not in _REFERENCE:
        spec, X, S, y, noise = FR.case(c)
        _REFERENCE[repr(c)] = VS.model(spec, X, S, y, noise)
    return _REFERENCE[repr(c)]


class Model(object):
    """One case on the device: the VFE model, alpha, and the host-side arguments of `paths` paths with `feats` features."""

    def __init__(self, dev, ctx, c, paths=1, feats=1, m=33, seed=0):
        self.c = c
        self.spec, self.X, self.S, self.y, self.noise = FR.case(c)
        self.nu, self.d, self.P, self.L = self.S.shape[0], c[1], paths, feats
        self.sp = dev.KernelSpec(FR.KIND_ID[self.spec["kind"]], self.d, FR.hyp_of(self.spec))
        self.dX, self.dS = dev.points(ctx, self.X), dev.points(ctx, self.S)
        self.model = dev.VfeModel(ctx, self.sp, self.dX, self.dS, self.noise)
        self.alpha = self.model.solve(self.y)[0]
        b = PR.base_draws(self.spec, paths, feats, 2 * self.nu, seed=900 + seed)
        self.omega, self.phase, self.w = PR.frequencies(self.spec, b["g"], b["u"]), b["phase"], b["w"]
        self.cw = PR.feature_weights(self.spec, self.w)
        self.xi1, self.xi2 = b["xi"][:, :self.nu].copy(), b["xi"][:, self.nu:].copy()
        self.Z = eval_points(c, self.S, m)
        self.dZ = dev.points(ctx, self.Z)

    def sampler(self, rows=None, w=None, xi1=None, xi2=None):
        w, xi1, xi2 = (self.w if w is None else w), (self.xi1 if xi1 is None else xi1), (self.xi2 if xi2 is None else xi2)
        if rows is not None:
            w, xi1, xi2 = w[rows], xi1[rows], xi2[rows]
        return self.model.path_sampler(self.dS, self.alpha, self.omega, self.phase, w, np.sqrt(self.noise) * xi1, xi2)


# ---- 1, 2: plumbing against the device's own V; V and the paths against the reference ---------------------------------------------
def _check_paths(dev, ctx, m, label, end_to_end):
    failures = []

    def attempt(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:          # (every figure is printed before the first assertion surfaces)
            failures.append(str(e))
    smp = m.sampler()
    try:
        assert (smp.S, smp.nfeat, smp.n) == (m.P, m.L, m.nu)
        V = smp.coefficients()
        assert V.shape == (m.P, m.nu) and np.all(np.isfinite(V))
        out = smp.evaluate(m.dZ)
        assert out.shape == (m.P, m.Z.shape[0])
        assert np.array_equal(smp.evaluate(m.dZ), out) and np.array_equal(smp.coefficients(), V)          # two calls, same bits
        ref = PR.paths(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z)
        bound = PR.value_bound(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z)
        attempt(PR.check_within, out, ref, bound, label + " values")
        for minimize in (True, False):
            idx, val, rows = smp.argbest(m.dZ, minimize=minimize, want_values=True)
            assert np.array_equal(rows, out)
            PR.check_argbest(idx, val, out, minimize, label)
            idx2, val2 = smp.argbest(m.dZ, minimize=minimize)
            assert np.array_equal(idx2, idx) and np.array_equal(val2, val)
        path = np.arange(m.Z.shape[0]) % m.P
        g, gv = smp.gradient(m.dZ, path, want_values=True)
        assert np.array_equal(smp.gradient(m.dZ, path), g)
        attempt(PR.check_within, g, PR.gradient(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z, path),
                PR.gradient_bound(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z, path), label + " gradient")
        attempt(PR.check_within, gv, ref[path, np.arange(len(path))], bound[path, np.arange(len(path))], label + " gradient's values")
        if end_to_end:
            Vref = VS.weights(m.spec, m.S, m.noise, reference_model(m.c), m.cw, m.omega, m.phase, m.xi1, m.xi2)
            fref = VS.paths(m.spec, m.cw, m.omega, m.phase, Vref, m.S, m.Z)
            rv = float(np.max(np.abs(V - Vref)) / np.max(np.abs(Vref)))
            rf = float(np.max(np.abs(out - fref)) / np.max(np.abs(fref)))
            print("  %-48s |V - ref| / max |ref| = %.3e   |f - ref| / max |ref| = %.3e   (cap %g)" % (label, rv, rf, TOL))
            attempt(_assert, rv <= TOL, "%s: V is %.3e x max |V_ref| from the reference" % (label, rv))
            attempt(_assert, rf <= TOL, "%s: the paths are %.3e x max |ref| from the reference" % (label, rf))
        assert not failures, "\n".join(failures)
    finally:
        smp.close()


def _assert(cond, msg):
    assert cond, msg


@pytest.mark.parametrize("p", PLUMBING, ids=plumb_id)
def test_values_gradients_argbest_and_weights(dev, ctx, p):
    c, paths, feats, mm = p
    _check_paths(dev, ctx, Model(dev, ctx, c, paths, feats, mm), plumb_id(p), end_to_end=c[6] == 1e-2)


def test_blocked(dev, ctx):
    """nu = 1152: the right solves cross the 1024-order block inverses."""
    c, paths, feats, mm = BLOCKED
    _check_paths(dev, ctx, Model(dev, ctx, c, paths, feats, mm), plumb_id(BLOCKED), end_to_end=True)


# ---- 3: the distribution, deterministically ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL[:4], ids=case_id)
def test_linear_map_of_the_base_draws(dev, ctx, c):
    m = Model(dev, ctx, c, 1, 5, 33)
    w, xi1, xi2 = VS.unit_draws(5, m.nu)
    smp = m.sampler(w=w, xi1=xi1, xi2=xi2)
    try:
        mean, J = VS.linear_map(smp.evaluate(m.dZ))
    finally:
        smp.close()
    rm = reference_model(c)
    mref = VS.mean(m.spec, m.S, rm, m.Z)
    cref = VS.feature_cov(m.spec, m.S, m.noise, rm, m.omega, m.phase, m.Z)
    r_mean = float(np.max(np.abs(mean - mref)) / np.max(np.abs(mref)))
    r_cov = float(np.max(np.abs(VS.mm(J, J.T) - cref)) / np.max(np.abs(cref)))
    pm = m.model.posterior(m.alpha, m.dZ, want_var=False)[0]
    r_pred = float(np.max(np.abs(mean - pm)) / np.max(np.abs(pm)))
    print("  %-32s zero path - mean: %.3e (predictor: %.3e)   J J^T - cov: %.3e   (cap %g)" % (case_id(c), r_mean, r_pred, r_cov, TOL))
    assert r_mean <= TOL and r_pred <= TOL and r_cov <= TOL


# ---- 4: bits ------------------------------------------------------------------------------------------------------------------------------
BITS = (SMALL[4], 33, 64, 257)


def chunk_digest():
    from gpexp_amd import device as dev
    ctx = dev.context()
    m = Model(dev, ctx, *BITS)
    smp = m.sampler()
    res = [smp.evaluate(m.dZ)]
    for minimize in (True, False):
        res += list(smp.argbest(m.dZ, minimize=minimize))
    smp.close()
    h = hashlib.sha256()
    for a in res:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe_sample as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


def test_bits_do_not_depend_on_the_company_or_the_chunking(dev, ctx):
    m = Model(dev, ctx, *BITS)
    smp = m.sampler()
    try:
        full, Vfull = smp.evaluate(m.dZ), smp.coefficients()
        for rows in ([0], [16], [32], [5, 32, 0]):                                  # rows of the larger base: the smaller call's bits
            one = m.sampler(rows=rows)
            try:
                assert np.array_equal(one.coefficients(), Vfull[rows]), rows
                assert np.array_equal(one.evaluate(m.dZ), full[rows]), rows
            finally:
                one.close()
        assert np.array_equal(smp.evaluate(dev.points(ctx, m.Z[[200, 3, 64]])), full[:, [200, 3, 64]])
    finally:
        smp.close()
    # GPX_CROSS_BYTES so small that the 257 points go in three chunks (128 + 128 + 1); a fresh child, not an exec
    assert run_child("print('RESULT ' + t.chunk_digest(), flush=True)", {"GPX_CROSS_BYTES": "1000"}) == chunk_digest()


# ---- 5: the exact sampler ------------------------------------------------------------------------------------------------------------------
MEHLER = ("mehler", 2, None, None, 40, 17, 1e-2, 41)
EXACT = [(c, m) for c in SMALL[:5] + [MEHLER, LOW_NOISE] for m in (1, 17, 129)]


class Exact(object):
    """One case of the exact sampler on the device (a Mehler model included: points and values as fitc_grad_ref.case makes them)."""

    def __init__(self, dev, ctx, c, m):
        if c[0] == "mehler":
            _, self.X, self.S, self.y, self.noise = FR.case(("se", c[1], [1.0], 1.0) + c[4:])
            self.X, self.S = 0.8 * self.X, 0.8 * self.S
            self.spec = SR.kernel_spec("mehler", c[1])
            self.sp = SR.device_spec(dev, self.spec)
        else:
            self.spec, self.X, self.S, self.y, self.noise = FR.case(c)
            self.sp = dev.KernelSpec(FR.KIND_ID[self.spec["kind"]], c[1], FR.hyp_of(self.spec))
        self.m = m
        self.Z = eval_points(c, self.S, m)
        self.dZ = dev.points(ctx, self.Z)
        self.model = dev.VfeModel(ctx, self.sp, dev.points(ctx, self.X), dev.points(ctx, self.S), self.noise)
        self.alpha = self.model.solve(self.y)[0]
        self.nugget = 1e-10 * float(np.max(dev.kdiag(ctx, self.sp, self.dZ)))

    def factor(self):
        """F itself: the draws of Xi = I from the sampler of alpha = 0 (beta_u = 0: mean_j + F_jk is then F_jk exactly)."""
        s0 = self.model.posterior_sampler(np.zeros(len(self.y)), self.dZ, self.nugget)
        try:
            return np.ascontiguousarray(s0.draw(np.eye(self.m)).T)
        finally:
            s0.close()


@pytest.mark.parametrize("cm", EXACT, ids=lambda cm: "%s-M%d" % (case_id(cm[0]), cm[1]))
def test_exact_sampler(dev, ctx, cm):
    c, mm = cm
    e = Exact(dev, ctx, c, mm)
    label = "%s-M%d" % (case_id(c), mm)
    failures = []
    cov = e.model.posterior_cov(e.dZ)
    assert cov.shape == (mm, mm) and np.array_equal(cov, cov.T) and np.array_equal(e.model.posterior_cov(e.dZ), cov)
    mean, var = e.model.posterior(e.alpha, e.dZ)
    cref = VS.exact_cov(e.spec, e.S, VS.model(e.spec, e.X, e.S, None, e.noise), e.Z)
    scale = float(np.max(np.abs(cref)))
    r_cov, r_diag = float(np.max(np.abs(cov - cref))) / scale, float(np.max(np.abs(np.diag(cov) - var))) / scale
    print("  %-40s |cov - ref| / max |ref| = %.3e   |diag - variance| / max |ref| = %.3e   (cap %g)" % (label, r_cov, r_diag, TOL))
    if c[6] == 1e-2:
        if not r_cov <= TOL:
            failures.append("%s: posterior_cov is %.3e x max |cov| from the reference" % (label, r_cov))
    if not r_diag <= TOL:
        failures.append("%s: the diagonal of posterior_cov is %.3e x max |cov| from posterior's variance" % (label, r_diag))
    F = e.factor()
    smp = e.model.posterior_sampler(e.alpha, e.dZ, e.nugget)
    try:
        assert np.array_equal(smp.draw(np.zeros((1, mm)))[0], mean)                                        # posterior's bits
        assert np.array_equal(smp.draw(np.eye(mm)), mean[None, :] + F.T)                                   # draw - mean IS F
        Chat = cov.copy()
        Chat[np.diag_indices(mm)] += e.nugget
        try:
            SR.check_factor(F, Chat, label)
        except AssertionError as err:
            failures.append(str(err))
        xi = SR.base_samples(33, mm)
        out = smp.draw(xi)
        SR.check_draw(out, mean, F, xi, label)
        assert np.array_equal(smp.draw(xi), out)
        for minimize in (True, False):
            idx, val, rows = smp.argbest(xi, minimize=minimize, want_samples=True)
            assert np.array_equal(rows, out)
            SR.check_argbest(idx, val, out, minimize, label)
        assert not failures, "\n".join(failures)
    finally:
        smp.close()


@pytest.mark.parametrize("drop_before", [False, True])
def test_repeated_points_without_jitter_are_refused_and_the_policy_survives(dev, ctx, drop_before):
    """Eight points, each given twice: without a nugget every second copy meets a pivot that is 0 in exact arithmetic, and
    round-to-nearest leaves it on either side of 0 by chance (tests/test_gpu_sample.py) -- eight chances, so one of the copies, points
    8 .. 15, is refused.  (0, report) is used whatever policy the context holds, and that policy is in force again afterwards."""
    from gpexp_amd._lib import NotPositiveDefinite
    e = Exact(dev, ctx, SMALL[2], 8)
    dZ = dev.points(ctx, np.vstack([e.Z, e.Z]))
    prev = dev.potrf_policy(ctx, 1e-13 * 1.3, True) if drop_before else dev.potrf_policy(ctx, 0.0, False)
    try:
        with pytest.raises(NotPositiveDefinite) as err:
            e.model.posterior_sampler(e.alpha, dZ, 0.0)
        assert 9 <= err.value.pivot <= 16, err.value.pivot
        assert "larger jitter" in str(err.value) and "point %d" % (err.value.pivot - 1) in str(err.value)
        e.model.posterior_sampler(e.alpha, dZ, e.nugget).close()                       # the default nugget factors, policy or not
        twin = np.vstack([e.X, e.X[7:8]])
        K = dev.kfill(ctx, e.sp, dev.points(ctx, twin), nugget=0.0)
        if drop_before:
            dev.potrf(ctx, K)
            assert dev.potrf_dropped(ctx) >= 1                                          # the drop policy is still on
        else:
            try:
                dev.potrf(ctx, K)
            except NotPositiveDefinite:
                pass
            assert dev.potrf_dropped(ctx) == 0                                          # nothing dropped: (0, report) is still on
    finally:
        dev.potrf_policy(ctx, *prev)


# ---- 6: the class API ------------------------------------------------------------------------------------------------------------------------
class _Space(object):
    def __init__(self, d):
        self.dimension = d


def _trained(kind, n=60, d=2, noise=1e-2, **kw):
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern, KernelMehlerND, KernelSquaredExponential
    c = SR.points_case(kind if kind != "mehler" else "se", n, 300, d, noise)
    spec = SR.kernel_spec(kind, d)
    if kind == "se":
        k = KernelSquaredExponential(spec["cl"], spec["signalSize"], d)
    elif kind == "mehler":
        k = KernelMehlerND(spec["t"], d)
    else:
        k = KernelIsoMatern(spec["rho"], spec["signalSize"], d, nu={"matern32": 1.5, "matern52": 2.5}[kind])
    np.random.seed(5)                                  # the inducing points are drawn with np.random.permutation
    g = GP(k, noise, **kw)
    g.train(c["X"], c["y"])
    return g, c


@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_class_api(kind):
    from gpexp_amd.experimentalDesign import costFuncEI
    from gpexp_amd.gp import PathBase
    g, c = _trained(kind, FITC=0.5, sparse="vfe")
    Z, nu = c["Z"], g.fitcnodes.shape[0]
    assert nu == 30
    base = PathBase.draw(5, 64, 2 * nu, 2, g.kernel, rng=1)
    smp = g.vfePathSampler(base=base)
    try:
        assert smp.base is base and smp.nPaths == 5
        f = smp.evaluate(Z)
        assert f.shape == (5, 300) and np.array_equal(g.vfeSamplePaths(Z, base=base), f)
        idx, val = smp.argbest(Z)
        PR.check_argbest(idx, val, f, True, "class argbest")
        assert smp.gradient(Z[:7], np.arange(7) % 5).shape == (7, 2)
    finally:
        smp.close()
    with pytest.raises(ValueError, match="closed"):
        smp.evaluate(Z)
    # zero draws: every path is the predictor's mean
    zero = PathBase(base.g, base.u, base.phase, 0.0 * base.w, 0.0 * base.xi)
    mean = g.evaluate(Z)
    f0 = g.vfeSamplePaths(Z, base=zero)
    assert np.max(np.abs(f0 - mean[None, :])) <= TOL * np.max(np.abs(mean))
    # the exact sampler, its covariance and its draws
    Zs = Z[:40]
    cov = g.vfePosteriorCovariance(Zs)
    assert cov.shape == (40, 40) and np.max(np.abs(np.diag(cov) - g.evaluateVariance(Zs))) <= TOL * np.max(np.abs(cov))
    xi = SR.base_samples(6, 40)
    js = g.vfePosteriorSampler(Zs)
    try:
        smpl = js.draw(baseSamples=xi)
        assert smpl.shape == (6, 40) and np.array_equal(g.vfeSamplePosterior(Zs, baseSamples=xi), smpl)
        assert np.array_equal(js.draw(baseSamples=np.zeros((1, 40)))[0], g.evaluate(Zs))
    finally:
        js.close()
    assert g.vfeSamplePosterior(Zs, nSamples=3).shape == (3, 40)                   # baseSamples=None: drawn with NumPy
    cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
    g2 = cf.gaussianProcess                                  # (the cost trains a copy on the same inducing points)
    for minimize in (True, False):
        ti, tv = cf.vfeThompsonBatch(Zs, 6, baseSamples=xi, minimize=minimize)
        rows = g2.vfeSamplePosterior(Zs, baseSamples=xi)
        SR.check_argbest(ti, tv, rows, minimize, "vfeThompsonBatch")
        pts, vals, ids = cf.vfeThompsonPaths(Z, 5, base=base, minimize=minimize)
        assert pts.shape == (5, 2) and vals.shape == (5,) and ids.shape == (5,) and ids.dtype == np.int64
        assert np.array_equal(pts, Z[ids])
        PR.check_argbest(ids, vals, g2.vfeSamplePaths(Z, base=base), minimize, "vfeThompsonPaths")
        again = cf.vfeThompsonPaths(Z, 5, base=base, minimize=minimize)
        assert all(np.array_equal(a, b) for a, b in zip(again, (pts, vals, ids)))
        pp, pv, pi = cf.vfeThompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, maxiter=20)
        assert np.array_equal(pi, ids) and pp.shape == (5, 2)
        assert np.all(pv <= vals) if minimize else np.all(pv >= vals)
        assert np.all(pp >= Z.min(axis=0)) and np.all(pp <= Z.max(axis=0))
        again = cf.vfeThompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, maxiter=20)
        assert all(np.array_equal(a, b) for a, b in zip(again, (pp, pv, pi)))
        lb, ub = np.array([-0.5, -0.4]), np.array([0.6, 0.5])
        bp, bv, bi = cf.vfeThompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, lbounds=lb, rbounds=ub, maxiter=20)
        assert np.all(bp >= lb) and np.all(bp <= ub) and np.all((Z[bi] >= lb) & (Z[bi] <= ub))
    assert cf.vfeThompsonPaths(Z, 2, nFeatures=16)[0].shape == (2, 2)              # base=None: drawn with NumPy
    # the old names still refuse this model
    for call in (lambda: g.pathSampler(2, 8), lambda: g.posteriorSampler(Zs), lambda: cf.thompsonPaths(Z, 2),
                 lambda: cf.thompsonBatch(Zs, 2), lambda: g.evaluate(Zs, compvar=2)):
        with pytest.raises(NotImplementedError):
            call()


def test_refusals_on_trained_models(monkeypatch):
    import gpexp_amd.gp as gpm
    from gpexp_amd.experimentalDesign import costFuncEI
    from gpexp_amd._lib import GpxError, NotPositiveDefinite
    from gpexp_amd import device as dev
    for kw in (dict(), dict(FITC=0.5)):                                 # dense and FITC models: ValueError
        g, c = _trained("se", **kw)
        cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
        for call in (lambda: g.vfePathSampler(2, 8), lambda: g.vfeSamplePaths(c["Z"]), lambda: g.vfePosteriorSampler(c["Z"][:9]),
                     lambda: g.vfeSamplePosterior(c["Z"][:9]), lambda: g.vfePosteriorCovariance(c["Z"][:9]),
                     lambda: cf.vfeThompsonPaths(c["Z"], 2), lambda: cf.vfeThompsonBatch(c["Z"][:9], 2)):
            with pytest.raises(ValueError, match="VFE models"):
                call()
    g, c = _trained("mehler", FITC=0.5, sparse="vfe")                 # Mehler: no paths, but the joint sampler and the covariance
    with pytest.raises(NotImplementedError, match="spectral density"):
        g.vfePathSampler(2, 8)
    assert g.vfePosteriorCovariance(c["Z"][:9]).shape == (9, 9) and g.vfeSamplePosterior(c["Z"][:9], 2).shape == (2, 9)
    g, c = _trained("se", FITC=0.5, sparse="vfe")
    with pytest.raises(NotPositiveDefinite, match="larger jitter"):
        g.vfePosteriorSampler(np.vstack([c["Z"][:8], c["Z"][:8]]), jitter=0.0)
    monkeypatch.setattr(gpm._dist, "session", lambda: object())       # base=None / baseSamples=None under a session
    with pytest.raises(ValueError, match="session"):
        g.vfePathSampler(2, 8)
    with pytest.raises(ValueError, match="session"):
        g.vfeSamplePosterior(c["Z"][:9], 2)
    monkeypatch.undo()
    # the C ABI: a FITC model, a Mehler model, nfeat < 1 and nPaths < 1 are argument errors
    ctx = dev.context()
    se = dev.KernelSpec(dev.K_SE, 2, [0.5, 0.6, 1.0])
    X, S = dev.points(ctx, c["X"]), dev.points(ctx, c["X"][:20])
    om, ph, w, al = np.zeros((2, 2)), np.zeros(2), np.zeros((1, 2)), np.zeros(60)
    fitc = dev.FitcModel(ctx, se, X, S, 1e-2)
    with pytest.raises(GpxError, match="gpx_paths_create"):
        dev.VfeModel.path_sampler(fitc, S, al, om, ph, w, None, None)
    with pytest.raises(GpxError, match="FITC model"):
        dev.VfeModel.posterior_cov(fitc, S)
    with pytest.raises(GpxError, match="gpx_psampler_create"):
        dev.VfeModel.posterior_sampler(fitc, al, S, 1e-6)
    meh = dev.VfeModel(ctx, dev.KernelSpec(dev.K_MEHLER, 2, [0.3, 0.5]), X, S, 1e-2)
    with pytest.raises(GpxError, match="stationary kernels only"):
        meh.path_sampler(S, al, om, ph, w, None, None)
    vfe = dev.VfeModel(ctx, se, X, S, 1e-2)
    h = dev.c_vp()
    args = (dev.dptr(al), dev.dptr(om), dev.dptr(ph))
    assert ctx.lib.gpx_vfe_paths_create(ctx.h, vfe.h, S.h, *args, 0, dev.dptr(w), None, None, 1, dev.C.byref(h)) == -1
    assert ctx.lib.gpx_vfe_paths_create(ctx.h, vfe.h, S.h, *args, 2, dev.dptr(w), None, None, 0, dev.C.byref(h)) == -1
    smp = vfe.path_sampler(S, al, om, ph, w, None, None)               # both draws NULL: zeros
    try:
        assert np.array_equal(smp.coefficients(), np.zeros((1, 20)))    # alpha = 0 and zero draws: V = 0 exactly
    finally:
        smp.close()


# ---- 7: the allocator ------------------------------------------------------------------------------------------------------------------------
def guarded_case():
    from gpexp_amd import device as dev
    ctx = dev.context()
    m = Model(dev, ctx, *BITS)
    e = Exact(dev, ctx, SMALL[4], 129)
    m.sampler().close()                             # (the factors' block inverses are built on the first solve and stay)
    e.model.posterior_sampler(e.alpha, e.dZ, e.nugget).close()
    ctx.sync()
    before = ctx.pool_stats()[1]
    smp = m.sampler()
    V = smp.coefficients()
    out = smp.evaluate(m.dZ)
    idx, val = smp.argbest(m.dZ)
    smp.close()
    js = e.model.posterior_sampler(e.alpha, e.dZ, e.nugget)
    xi = SR.base_samples(5, 129)
    draws = js.draw(xi)
    js.close()
    cov = e.model.posterior_cov(e.dZ)
    ctx.sync()
    after = ctx.pool_stats()[1]
    PR.check_within(out, PR.paths(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z), PR.value_bound(m.spec, m.cw, m.omega, m.phase, V, m.S, m.Z),
                    "guarded values")
    PR.check_argbest(idx, val, out, True, "guarded")
    assert np.all(np.isfinite(draws)) and np.all(np.isfinite(cov))
    return "%d %d %d" % (int(ctx.lib.gpx_dbg_guard_violations(ctx.h)), before, after)


def test_allocator_books_balance(dev, ctx):
    m = Model(dev, ctx, SMALL[2], 17, 64, 33)
    m.sampler().close()
    ctx.sync()
    before = ctx.pool_stats()[1]
    smp = m.sampler()
    smp.evaluate(m.dZ)
    smp.close()
    ctx.sync()
    assert ctx.pool_stats()[1] == before


def test_under_allocation_guard_and_nan_fill():
    """Guard bands + NaN-filled blocks: no padding reaches a result, no block is overrun, and the pool's outstanding bytes return to
    their value after create / coefficients / evaluate / argbest / close, the exact sampler and the covariance."""
    viol, before, after = run_child("print('RESULT ' + t.guarded_case(), flush=True)", {"GPX_ALLOC_GUARD": "2"}).split()
    assert viol == "0"
    assert before == after, (before, after)
