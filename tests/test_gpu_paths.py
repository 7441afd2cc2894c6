"""GPU (-m gpu): pathwise posterior sampling (gpx_paths_*) held to tests/path_ref.py -- the update weights V by the residual of the
solve against the device's own factor, values and gradients by a longdouble replay from the device's OWN V within the per-element
bound x 8 (chol_stability_ref.MARGIN), the arg-best exactly -- plus bit-for-bit independence of S, of the company and of the chunking,
the class API, the refusals and the allocator's books.

Measured on an MI355X, largest |device - replay| / bound of the VALUES per case, in the order of CASES (the cap is 8 x the bound):
squared exponential 0.083, 0.082, 0.076, 0.051, 0.018, 0.003; Matern 3/2 0.031, 0.062, 0.002, 0.005, 0.040, 0.019; Matern 5/2 0.009,
0.003, 0.158, 0.115, 0.075, 0.015.  Gradients: at most 0.152 (Matern 5/2, S = 33, L = 1, N = 3, M = 257, d = 1), the values the
gradient call returns at most 0.125; the residual of V at most 0.017 of its bound; the central-difference line 0.001 of its
tolerance.  Every test prints its figures before it asserts (run with -s)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import path_ref as PR
import sample_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))

# (kind, S, L, N, M, d, noise): a covering subset -- every S in {1, 15, 16, 17, 33, 64}, L in {1, 3, 4, 5, 64, 257}, N in {0 (prior),
# 1, 3, 4, 5, 130}, M in {1, 15, 16, 17, 257}, d in {1, 2, 3, 8, 9, 32}, both noises, each with every kernel at least once
_AX = dict(S=(1, 15, 16, 17, 33, 64), L=(1, 3, 4, 5, 64, 257), N=(0, 1, 3, 4, 5, 130), M=(1, 15, 16, 17, 257, 16),
           d=(1, 2, 3, 8, 9, 32), noise=(1e-2, 1e-6, 1e-2, 1e-6, 1e-2, 1e-6))
CASES = [(kind, _AX["S"][(i + a) % 6], _AX["L"][(i + 2 * a) % 6], _AX["N"][(i + 3 * a) % 6], _AX["M"][(i + 4 * a) % 6],
          _AX["d"][(i + 5 * a) % 6], _AX["noise"][(i + a) % 6])
         for a, kind in enumerate(("se", "matern32", "matern52")) for i in range(6)]


def case_id(c):
    return "%s-S%d-L%d-N%d-M%d-d%d-noise%g" % c


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


class Model(object):
    """One case on the device: the factor of K(X) + noise I, alpha, the base draws and the sampler's host-side arguments."""

    def __init__(self, dev, ctx, case, seed=0):
        kind, S, L, n, m, d, noise = case
        self.case, self.S, self.L, self.n, self.m, self.d, self.noise = case, S, L, n, m, d, noise
        c = SR.points_case(kind, max(n, 4), max(m, 1), d, noise, seed=seed)
        self.spec, self.X, self.y, self.Z = c["spec"], c["X"][:n], c["y"][:n], c["Z"]
        if n > 3 and m > 2:
            self.Z[1] = self.X[3]                                   # a point ON a training point
        self.sp = SR.device_spec(dev, self.spec)
        self.b = PR.base_draws(self.spec, S, L, n, seed=77 + seed)
        self.omega = PR.frequencies(self.spec, self.b["g"], self.b["u"])
        self.phase, self.w = self.b["phase"], self.b["w"]
        self.c = PR.feature_weights(self.spec, self.w)
        self.eps = np.sqrt(noise) * self.b["xi"]
        self.dZ = dev.points(ctx, self.Z)
        if n:
            self.dX = dev.points(ctx, self.X)
            self.Lf = dev.potrf(ctx, dev.kfill(ctx, self.sp, self.dX, nugget=noise))
            self.alpha = dev.potrs(ctx, self.Lf, self.y)
        else:
            self.dX = self.Lf = self.alpha = None

    def sampler(self, dev, ctx, rows=None):
        w, eps = (self.w, self.eps) if rows is None else (self.w[rows], self.eps[rows])
        return dev.PathSampler(ctx, self.sp, self.Lf, self.dX, self.alpha, self.omega, self.phase, w, eps if self.n else None)

    def Xr(self):
        return self.X if self.n else None


# ---- V, values, arg-best, gradients: every case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_weights_values_argbest_and_gradients(dev, ctx, case):
    m = Model(dev, ctx, case)
    label = case_id(case)
    smp = m.sampler(dev, ctx)
    failures = []

    def attempt(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:        # (every figure is printed before the first assertion surfaces)
            failures.append(str(e))
    try:
        V = smp.coefficients()
        assert V.shape == (m.S, m.n)
        if m.n:
            # the solve, against the device's own factor: Khat (alpha - V_s) = r_s, r = the longdouble replay of f~(X) + eps
            Ld = np.tril(m.Lf.to_host(tri=1))[:m.n, :m.n]
            Kh = CR_ld(Ld)
            r = PR.prior_paths(m.c, m.omega, m.phase, m.X) + m.eps.astype(PR.LD)
            r_err = PR.MARGIN * PR.value_bound(m.spec, m.c, m.omega, m.phase, None, None, m.X) + PR.U * np.abs(r).astype(float)
            worst = 0.0
            for s in range(m.S):
                x = m.alpha - V[s]
                res = float(np.max(np.abs(Kh @ x.astype(PR.LD) - r[s])))
                cap = PR.solve_residual_bound(Ld, x, r[s].astype(float), float(np.max(np.abs(Kh).astype(float) @ np.abs(V[s]))),
                                              float(np.max(r_err[s])))
                worst = max(worst, res / cap)
            print("  %-48s max residual / bound = %.3f" % (label + " V", worst))
            attempt(lambda: _assert(worst <= 1.0, "%s: the residual of V reaches %.3f x its bound" % (label, worst)))
        else:
            assert V.size == 0
        out = smp.evaluate(m.dZ)
        assert out.shape == (m.S, m.m)
        assert np.array_equal(smp.evaluate(m.dZ), out)                                         # two calls, same bits
        ref = PR.paths(m.spec, m.c, m.omega, m.phase, V, m.Xr(), m.Z)
        bound = PR.value_bound(m.spec, m.c, m.omega, m.phase, V, m.Xr(), m.Z)
        attempt(PR.check_within, out, ref, bound, label + " values")
        for minimize in (True, False):
            idx, val, rows = smp.argbest(m.dZ, minimize=minimize, want_values=True)
            assert np.array_equal(rows, out)
            PR.check_argbest(idx, val, out, minimize, label)
            idx2, val2 = smp.argbest(m.dZ, minimize=minimize)
            assert np.array_equal(idx2, idx) and np.array_equal(val2, val)
        # gradients: point p belongs to path p mod S
        path = np.arange(m.m) % m.S
        g, gv = smp.gradient(m.dZ, path, want_values=True)
        assert g.shape == (m.m, m.d) and np.all(np.isfinite(g))
        assert np.array_equal(smp.gradient(m.dZ, path), g)
        gref = PR.gradient(m.spec, m.c, m.omega, m.phase, V, m.Xr(), m.Z, path)
        attempt(PR.check_within, g, gref, PR.gradient_bound(m.spec, m.c, m.omega, m.phase, V, m.Xr(), m.Z, path), label + " gradient")
        attempt(PR.check_within, gv, ref[path, np.arange(m.m)], bound[path, np.arange(m.m)], label + " gradient's values")
        assert not failures, "\n".join(failures)
    finally:
        smp.close()


def _assert(cond, msg):
    assert cond, msg


def CR_ld(Ld):
    """Khat = Ld Ld^T in longdouble."""
    Ll = Ld.astype(PR.LD)
    return Ll @ Ll.T


def test_central_differences_of_evaluate(dev, ctx):
    """A sanity line, not the bound: central differences of `evaluate` at h = 1e-5 against `gradient`, tolerance h^2 x the size of
    the third derivative (every feature term differentiates to |c| |omega_l|^3, the squared-exponential kernel term to at most
    |v| sig 3 scale_l^3) plus the rounding of the difference quotient, 2 x the value cap / (2 h)."""
    m = Model(dev, ctx, ("se", 3, 64, 40, 17, 2, 1e-2))
    smp = m.sampler(dev, ctx)
    try:
        V, h = smp.coefficients(), 1e-5
        path = np.arange(m.m) % m.S
        g = smp.gradient(m.dZ, path)
        sc = PR.DR._params_f64(m.spec)[1]
        cap = PR.MARGIN * PR.value_bound(m.spec, m.c, m.omega, m.phase, V, m.X, m.Z)[path, np.arange(m.m)]
        for l in range(m.d):
            E = np.zeros((1, m.d))
            E[0, l] = h
            fp = smp.evaluate(dev.points(ctx, m.Z + E))[path, np.arange(m.m)]
            fm = smp.evaluate(dev.points(ctx, m.Z - E))[path, np.arange(m.m)]
            third = (np.abs(m.c) @ np.abs(m.omega[:, l]) ** 3)[path] + 3.0 * m.spec["signalSize"] * sc[l] ** 3 * np.sum(np.abs(V), axis=1)[path]
            tol = h * h * third + 2.0 * cap / (2.0 * h)
            err = np.abs((fp - fm) / (2.0 * h) - g[:, l])
            print("  central differences, coordinate %d: max err / tol = %.3f" % (l, float(np.max(err / tol))))
            assert np.all(err <= tol)
    finally:
        smp.close()


# ---- bit for bit: S, the company, the chunking -------------------------------------------------------------------------------------------
BITS_CASE = ("matern32", 33, 64, 130, 257, 3, 1e-2)


def chunk_digest():
    from gpexp_amd import device as dev
    ctx = dev.context()
    m = Model(dev, ctx, BITS_CASE)
    smp = m.sampler(dev, ctx)
    out = smp.evaluate(m.dZ)
    res = [out]
    for minimize in (True, False):
        res += list(smp.argbest(m.dZ, minimize=minimize))
    smp.close()
    h = hashlib.sha256()
    for a in res:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_paths as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


def test_bits_do_not_depend_on_S_company_or_chunking(dev, ctx):
    m = Model(dev, ctx, BITS_CASE)
    smp = m.sampler(dev, ctx)
    try:
        full, Vfull = smp.evaluate(m.dZ), smp.coefficients()
        for s in (0, 16, 32):                                                       # row s of S = 33 against the S = 1 sampler
            one = m.sampler(dev, ctx, rows=[s])
            try:
                assert np.array_equal(one.coefficients()[0], Vfull[s])
                assert np.array_equal(one.evaluate(m.dZ)[0], full[s])
            finally:
                one.close()
        some = m.sampler(dev, ctx, rows=[5, 32, 0])                                 # other company, another position
        try:
            assert np.array_equal(some.evaluate(m.dZ), full[[5, 32, 0]])
        finally:
            some.close()
        # a point's value does not change when other points are added to or taken from Z
        assert np.array_equal(smp.evaluate(dev.points(ctx, m.Z[:17])), full[:, :17])
        assert np.array_equal(smp.evaluate(dev.points(ctx, m.Z[[200, 3, 64]])), full[:, [200, 3, 64]])
        assert np.array_equal(smp.evaluate(dev.points(ctx, m.Z[100:101])), full[:, 100:101])
    finally:
        smp.close()
    # GPX_CROSS_BYTES so small that the 257 points go in three chunks (128 + 128 + 1); a fresh child, not an exec
    assert run_child("print('RESULT ' + t.chunk_digest(), flush=True)", {"GPX_CROSS_BYTES": "1000"}) == chunk_digest()


def tie_case():
    """Arg-best across chunk boundaries with exact ties: candidate 3 repeated bit for bit at 130 and 256 (three different chunks of
    128 under the small budget), made the winner of every path by construction: prior paths with ONE feature of frequency 0, so
    that every path is constant -- every candidate ties, and the first index must win for the minimum and for the maximum."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    spec = SR.kernel_spec("se", 2)
    sp = SR.device_spec(dev, spec)
    Z = np.random.default_rng(3).uniform(-1.0, 1.0, (257, 2))
    Z[130] = Z[256] = Z[3]
    out = []
    # (a) constant paths: all 257 candidates tie
    smp = dev.PathSampler(ctx, sp, None, None, None, np.zeros((1, 2)), np.array([0.3]), np.array([[1.0], [-2.0]]), None)
    for minimize in (True, False):
        idx, val, rows = smp.argbest(dev.points(ctx, Z), minimize=minimize, want_values=True)
        PR.check_argbest(idx, val, rows, minimize, "constant paths")
        out.append(idx.tolist())
    smp.close()
    # (b) general paths: the repeated candidate's value is repeated bit for bit; where it wins, index 3 wins
    m = Model(dev, ctx, ("se", 64, 5, 5, 257, 2, 1e-2))
    Zm = m.Z.copy()
    Zm[130] = Zm[256] = Zm[3]
    smp = m.sampler(dev, ctx)
    for minimize in (True, False):
        idx, val, rows = smp.argbest(dev.points(ctx, Zm), minimize=minimize, want_values=True)
        assert np.array_equal(rows[:, 3], rows[:, 130]) and np.array_equal(rows[:, 3], rows[:, 256])
        PR.check_argbest(idx, val, rows, minimize, "general paths")
        assert not np.any(np.isin(idx, (130, 256)))
        out.append(idx.tolist())
    smp.close()
    return repr(out)


def test_argbest_across_chunks_and_ties():
    small = run_child("print('RESULT ' + t.tie_case(), flush=True)", {"GPX_CROSS_BYTES": "1000"})
    assert small == tie_case()
    assert eval(small)[0] == [0, 0] and eval(small)[1] == [0, 0]


ARGBEST_M = (1, 255, 256, 257)    # below, at and above the 256 threads a row is dealt to; 257: three chunks under the small budget


@pytest.mark.parametrize("budget", [None, "1"], ids=["one-chunk", "chunks-of-128"])
@pytest.mark.parametrize("m", ARGBEST_M)
def test_argbest_of_rows_with_ties_zeros_and_nan(dev, ctx, m, budget, monkeypatch):
    """The row arg-best and its merge across chunks on rows made to order: prior paths on three features -- a constant, cos(z_0), and
    cos(1e308 z_1), which is cos(inf) = NaN where z_1 = 10 and 1 where z_1 = 0.  The candidates at 127, 128 and m - 1 repeat candidate
    1 bit for bit, where cos(z_0) = 1: the winner of the maximum of path 1 and of the minimum of path 2, tied across the chunk
    boundaries.  Path 0 is constant (every candidate ties), path 3 is exactly 0 (weights 0), path 4 is NaN everywhere (a NaN weight).
    Evaluated twice: without NaN candidates, and with NaN at candidate 0 and at 130 (the start of the first and inside the second
    chunk).  Checked on the rows the device itself returns: the first arg-best among the entries that are not NaN, the value there bit
    for bit, index 0 and NaN for a row of NaNs.  (A -0 cannot come out of the evaluation, whose sums start from +0: the tie of +0
    with -0 reaches the reduction as a tie of +0 with +0, path 3.)"""
    if budget:
        monkeypatch.setenv("GPX_CROSS_BYTES", budget)
    sp = SR.device_spec(dev, dict(SR.kernel_spec("se", 2), signalSize=1.0))
    omega, phase = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1e308]]), np.zeros(3)
    w = np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -1.0, 0.0], [0.0, -0.0, 0.0], [np.nan, 0.0, 0.0]])
    Z = np.zeros((m, 2))
    Z[:, 0] = np.random.default_rng(m).uniform(0.5, 3.0, m)
    Z[[j for j in (1, 127, 128, m - 1) if j < m], 0] = 0.0
    Znan = Z.copy()
    Znan[[j for j in (0, 130) if j < m], 1] = 10.0
    smp = dev.PathSampler(ctx, sp, None, None, None, omega, phase, w, None)
    try:
        for pts, with_nan in ((Z, False), (Znan, True)):
            for minimize in (True, False):
                idx, val, rows = smp.argbest(dev.points(ctx, pts), minimize=minimize, want_values=True)
                assert np.all(rows[0] == rows[0, -1]) or with_nan
                assert np.all(np.isnan(rows[4])) and np.array_equal(np.isnan(rows[0]), pts[:, 1] != 0.0)
                assert np.all(rows[3][pts[:, 1] == 0.0] == 0.0)
                if m > 128 and not with_nan:
                    assert rows[1, 1] == rows[1, 127] == rows[1, 128] == rows[1, m - 1] == rows[1].max()
                    assert rows[2, 1] == rows[2, 127] == rows[2, 128] == rows[2, m - 1] == rows[2].min()
                SR.check_argbest_bits(idx, val, rows, minimize, "m = %d, %s" % (m, "min" if minimize else "max"))
                assert idx[4] == 0 and np.isnan(val[4])
                if m > 1:
                    assert idx[0] == idx[3] == (1 if with_nan else 0)
                    if not with_nan:
                        assert idx[2 if minimize else 1] == 1
                idx2, val2 = smp.argbest(dev.points(ctx, pts), minimize=minimize)
                assert np.array_equal(idx2, idx) and np.array_equal(val2, val, equal_nan=True)
    finally:
        smp.close()


# ---- the class API ---------------------------------------------------------------------------------------------------------------------------
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
    g = GP(k, noise, **kw)
    g.train(c["X"], c["y"])
    return g, c


@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_class_api(kind):
    from gpexp_amd.experimentalDesign import costFuncEI
    from gpexp_amd.gp import PathBase
    g, c = _trained(kind)
    Z = c["Z"]
    base = PathBase.draw(5, 64, 60, 2, g.kernel, rng=1)
    smp = g.pathSampler(base=base)
    try:
        assert smp.base is base and smp.nPaths == 5
        f = smp.evaluate(Z)
        assert f.shape == (5, 300) and np.array_equal(g.samplePaths(Z, base=base), f)
        idx, val = smp.argbest(Z)
        PR.check_argbest(idx, val, f, True, "class argbest")
        assert smp.gradient(Z[:7], np.arange(7) % 5).shape == (7, 2)
    finally:
        smp.close()
    with pytest.raises(ValueError, match="closed"):
        smp.evaluate(Z)
    # w = 0, xi = 0: the right-hand side is exactly 0, V = coeff exactly, and every path is the posterior mean K(Z, X) coeff
    zero = PathBase(base.g, base.u, base.phase, 0.0 * base.w, 0.0 * base.xi)
    spec, V0, c0 = SR.kernel_spec(kind, 2), np.tile(g.coeff, (5, 1)), np.zeros((5, 64))
    om = PR.frequencies(spec, base.g, base.u)
    PR.check_within(g.samplePaths(Z, base=zero), PR.paths(spec, c0, om, base.phase, V0, c["X"], Z),
                    PR.value_bound(spec, c0, om, base.phase, V0, c["X"], Z), "%s posterior mean" % kind)
    pr = g.priorPathSampler(base=PathBase.draw(3, 64, 0, 2, g.kernel, rng=2))
    try:
        assert pr.evaluate(Z).shape == (3, 300)
    finally:
        pr.close()
    cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
    for minimize in (True, False):
        pts, vals, ids = cf.thompsonPaths(Z, 5, base=base, minimize=minimize)
        assert pts.shape == (5, 2) and vals.shape == (5,) and ids.shape == (5,) and ids.dtype == np.int64
        assert np.array_equal(pts, Z[ids])
        again = cf.thompsonPaths(Z, 5, base=base, minimize=minimize)
        assert all(np.array_equal(a, b) for a, b in zip(again, (pts, vals, ids)))
        pp, pv, pi = cf.thompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, maxiter=20)
        assert np.array_equal(pi, ids) and pp.shape == (5, 2)
        assert np.all(pv <= vals) if minimize else np.all(pv >= vals)
        assert np.all(pp >= Z.min(axis=0)) and np.all(pp <= Z.max(axis=0))
        again = cf.thompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, maxiter=20)
        assert all(np.array_equal(a, b) for a, b in zip(again, (pp, pv, pi)))
        lb, ub = np.array([-0.5, -0.4]), np.array([0.6, 0.5])
        bp, bv, bi = cf.thompsonPaths(Z, 5, base=base, minimize=minimize, polish=True, lbounds=lb, rbounds=ub, maxiter=20)
        assert np.all(bp >= lb) and np.all(bp <= ub) and np.all((Z[bi] >= lb) & (Z[bi] <= ub))
    assert cf.thompsonPaths(Z, 2, nFeatures=16)[0].shape == (2, 2)                 # base=None: drawn with NumPy


def test_refusals_on_trained_models(monkeypatch):
    import gpexp_amd.gp as gpm
    from gpexp_amd.experimentalDesign import costFuncEI
    from gpexp_amd._lib import GpxError
    for kw in (dict(FITC=0.5), dict(FITC=0.5, sparse="vfe")):
        g, c = _trained("se", **kw)
        cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
        for call in (lambda: g.pathSampler(2, 8), lambda: cf.thompsonPaths(c["Z"], 2)):
            with pytest.raises(NotImplementedError, match="FITC / VFE"):
                call()
    g, c = _trained("se")
    cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
    monkeypatch.setattr(gpm._dist, "session", lambda: object())      # the branch itself: base=None under a session
    with pytest.raises(ValueError, match="session"):
        cf.thompsonPaths(c["Z"], 2)
    monkeypatch.undo()
    # the C ABI: a Mehler kind, nfeat < 1 and S < 1 are argument errors
    from gpexp_amd import device as dev
    ctx = dev.context()
    om, ph, w = np.zeros((2, 2)), np.zeros(2), np.zeros((1, 2))
    with pytest.raises(GpxError, match="stationary"):
        dev.PathSampler(ctx, dev.KernelSpec(dev.K_MEHLER, 2, [0.3, 0.5]), None, None, None, om, ph, w, None)
    se = dev.KernelSpec(dev.K_SE, 2, [0.5, 0.6, 1.0])
    h = dev.c_vp()
    assert ctx.lib.gpx_paths_create(ctx.h, *se.args(), None, None, None, dev.dptr(om), dev.dptr(ph), 0, dev.dptr(w), None, 1,
                                    dev.C.byref(h)) == -1
    assert ctx.lib.gpx_paths_create(ctx.h, *se.args(), None, None, None, dev.dptr(om), dev.dptr(ph), 2, dev.dptr(w), None, 0,
                                    dev.C.byref(h)) == -1


# ---- the allocator ---------------------------------------------------------------------------------------------------------------------------
def guarded_case():
    from gpexp_amd import device as dev
    ctx = dev.context()
    m = Model(dev, ctx, BITS_CASE)
    m.sampler(dev, ctx).close()                    # (the factor's block inverses are built on the first solve and stay)
    ctx.sync()
    before = ctx.pool_stats()[1]
    smp = m.sampler(dev, ctx)
    V = smp.coefficients()
    out = smp.evaluate(m.dZ)
    idx, val = smp.argbest(m.dZ)
    path = np.arange(m.m) % m.S
    g = smp.gradient(m.dZ, path)
    smp.close()
    ctx.sync()
    after = ctx.pool_stats()[1]
    PR.check_within(out, PR.paths(m.spec, m.c, m.omega, m.phase, V, m.X, m.Z), PR.value_bound(m.spec, m.c, m.omega, m.phase, V, m.X, m.Z),
                    "guarded values")
    PR.check_argbest(idx, val, out, True, "guarded")
    PR.check_within(g, PR.gradient(m.spec, m.c, m.omega, m.phase, V, m.X, m.Z, path),
                    PR.gradient_bound(m.spec, m.c, m.omega, m.phase, V, m.X, m.Z, path), "guarded gradient")
    return "%d %d %d" % (int(ctx.lib.gpx_dbg_guard_violations(ctx.h)), before, after)


def test_under_allocation_guard_and_nan_fill():
    """Guard bands + NaN-filled blocks: no padding reaches a result, no block is overrun, and the pool's outstanding bytes return to
    their value after create / coefficients / evaluate / argbest / gradient / close."""
    viol, before, after = run_child("print('RESULT ' + t.guarded_case(), flush=True)", {"GPX_ALLOC_GUARD": "2"}).split()
    assert viol == "0"
    assert before == after, (before, after)
