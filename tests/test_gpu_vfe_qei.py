"""GPU (-m gpu): Monte-Carlo joint expected improvement on VFE models (gpx_vfe_acq_qei, test hook gpx_dbg_vfe_qei_blocks and the
classes above them) held to tests/vfe_qei_ref.py, tests/vfe_sample_ref.py and the q-EI contracts of tests/sample_ref.py.

 B1  the blocks: the means are gpx_vfe_posterior's bits; C_b is bitwise symmetric, within 1e-8 x max |cov| of the longdouble
     reference (float64 on the nu = 2049 case) and within 6 (nu + 2) u sqrt(k_ii k_jj) of the device's own posterior_cov of the
     same batch (vfe_qei_ref.route_bound: both routes solve bit-identical columns); F_b lower triangular under the factor contract;
 B2  the costs against the longdouble replay from the device's own blocks, the arg-min, want_costs=False;
 B3  q = 1 against gpx_vfe_acq's closed-form EI;   B4  B = 1, q = 16 against the exact sampler's draws;
 B5  bits: permutation, two calls, three chunks in a child process;   B6  the NaN rule;   B7  refusals through the C ABI;
 B8  the class API;   B9  the allocator's books.

Every test prints its worst figure before it asserts (run with -s)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as FR
import sample_ref as SR
import vfe_qei_ref as QR
import vfe_sample_ref as VS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
GRID = [(q, b) for q in QR.QS for b in QR.BS]


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def test_cases_are_those_of_the_vfe_sampling_tests():
    import test_gpu_vfe_sample as T
    assert QR.SMALL == T.SMALL + [T.LOW_NOISE]


class Model(object):
    """One case on the device: the VFE model and alpha.  Built once per case and shared (read-only), as are the host references."""
    _made, _ref = {}, {}

    def __init__(self, dev, ctx, c):
        self.c = c
        self.spec, self.X, self.S, self.y, self.noise = QR.build(c)
        self.nu, self.d = self.S.shape[0], c[1]
        self.sp = SR.device_spec(dev, self.spec) if c[0] == "mehler" else \
            dev.KernelSpec(FR.KIND_ID[self.spec["kind"]], self.d, FR.hyp_of(self.spec))
        self.dX, self.dS = dev.points(ctx, self.X), dev.points(ctx, self.S)
        self.model = dev.VfeModel(ctx, self.sp, self.dX, self.dS, self.noise)
        self.alpha = self.model.solve(self.y)[0]
        self.fBest = float(np.max(self.y))

    @classmethod
    def of(cls, dev, ctx, c):
        if repr(c) not in cls._made:
            cls._made[repr(c)] = cls(dev, ctx, c)
        return cls._made[repr(c)]

    def reference(self, dtype=VS.LD):
        """The host model of the case (longdouble; float64 where asked), with beta_u."""
        key = (repr(self.c), dtype is VS.LD)
        if key not in self._ref:
            self._ref[key] = VS.model(self.spec, self.X, self.S, self.y, self.noise, dtype)
        return self._ref[key]

    def pts(self, dev, ctx, Zb):
        """Zb on the device carrying the box [-1, 1]^d: the fills centre on the bounding box of their point sets, so two calls whose
        batches differ would otherwise differ in the last bits of every cross covariance."""
        d = Zb.shape[1]
        return dev.points_slice(ctx, np.vstack([Zb, -np.ones((1, d)), np.ones((1, d))]), 0, Zb.shape[0])

    def qei(self, dev, ctx, Zb, q, xi, nugget, **kw):
        return self.model.acq_qei(self.alpha, self.pts(dev, ctx, Zb), q, xi, self.fBest, nugget, **kw)

    def blocks(self, dev, ctx, Zb, q, nugget):
        return self.model.dbg_qei_blocks(self.alpha, self.pts(dev, ctx, Zb), q, nugget)


# ---- B1, B2: the hook's blocks and the costs -------------------------------------------------------------------------------------------
def check_blocks_and_costs(dev, ctx, c, q, b, s, dtype=VS.LD):
    m = Model.of(dev, ctx, c)
    label = "%s q=%d B=%d S=%d" % (QR.case_id(c), q, b, s)
    Zb = QR.batches(c, m.S, q, b)
    nugget = QR.default_nugget(m.spec, Zb)
    xi = SR.base_samples(s, q, seed=q + b)
    best, best_cost, costs, nbad = m.qei(dev, ctx, Zb, q, xi, nugget)
    mu, Cb, Fb = m.blocks(dev, ctx, Zb, q, nugget)
    failures = []
    assert costs.shape == (b,) and mu.shape == (b, q) and Cb.shape == (b, q, q) and Fb.shape == (b, q, q)
    dZ = m.pts(dev, ctx, Zb)
    # (a) the means: gpx_vfe_posterior's bits;  (b) bitwise symmetric
    assert np.array_equal(mu.ravel(), m.model.posterior(m.alpha, dZ, want_var=False)[0]), label
    assert np.array_equal(Cb, np.transpose(Cb, (0, 2, 1))), label
    # (c) against the reference
    ref = QR.blocks_ref(m.spec, m.S, m.reference(dtype), Zb, q, dtype)
    r_ref = QR.worst_rel(Cb, ref)
    # (d) against the device's own posterior_cov of the same batch, at most 8 batches
    r_dev = 0.0
    for i in range(min(b, 8)):
        Zq = Zb[i * q:(i + 1) * q]
        cov = m.model.posterior_cov(m.pts(dev, ctx, Zq))
        kd = dev.kdiag(ctx, m.sp, m.pts(dev, ctx, Zq))
        r_dev = max(r_dev, float(np.max(np.abs(Cb[i] - cov) / QR.route_bound(m.nu, kd))))
    # (e) the factor
    ratio = QR.worst_factor_ratio(Fb, Cb, nugget)
    print("  %-52s |C_b - ref| / max |cov| = %.3e (cap %g)   |C_b - posterior_cov| / bound = %.3f   |F F^T - Chat| / bound = %.3f"
          % (label, r_ref, QR.TOL, r_dev, ratio))
    if not r_ref <= QR.TOL:
        failures.append("%s: C_b is %.3e x max |cov| from the reference" % (label, r_ref))
    if not r_dev <= 1.0:
        failures.append("%s: C_b misses the device's own posterior_cov by %.3f x the route bound" % (label, r_dev))
    if not ratio <= 1.0:
        failures.append("%s: the factor misses its contract by %.3f" % (label, ratio))
    # B2: the costs against the replay from the device's own blocks
    assert nbad == 0 and np.all(np.isfinite(costs)), (label, nbad, costs)
    worst = 0.0
    for i in range(b):
        try:
            worst = max(worst, SR.check_qei(costs[i], mu[i], Fb[i], xi, m.fBest, "%s batch %d" % (label, i)))
        except AssertionError as e:
            failures.append(str(e))
    print("  %-52s worst |cost - replay| / bound = %.3f" % (label, worst))
    assert not failures, "\n".join(failures)
    assert best == int(np.argmin(costs)) and best_cost == costs[best]
    assert m.qei(dev, ctx, Zb, q, xi, nugget, want_costs=False)[:2] == (best, best_cost)


@pytest.mark.parametrize("q,b", GRID, ids=["q%d-B%d" % g for g in GRID])
def test_blocks_and_costs(dev, ctx, q, b):
    c, s = QR.setting(q, b)
    check_blocks_and_costs(dev, ctx, c, q, b, s)


@pytest.mark.parametrize("q,b,s", [(5, 3, 130), (32, 1, 3)], ids=["q5-B3", "q32-B1"])
def test_blocks_and_costs_out_of_place(dev, ctx, q, b, s):
    """nu = 2049: the solves run out of place, Wu and Wa in separate blocks.  The reference is the float64 model (the longdouble one
    is too slow at this size)."""
    check_blocks_and_costs(dev, ctx, QR.OOP, q, b, s, dtype=float)


# ---- B3: q = 1 against the closed form ----------------------------------------------------------------------------------------------------
Q1_SEED = 44          # the first seed whose 40 points have every |g| <= 3 on the host reference (g = 0.44 .. 2.77)


def test_q1_against_closed_form_ei(dev, ctx):
    """q = 1 with the stratified base samples xi_s = Phi^-1((s + 1/2) / S), S = 4096, against gpx_vfe_acq's closed-form EI at the same
    40 points of the d = 8 case.  Tolerance per point: 2 x the distance of the REFERENCE's longdouble replay (host mean and variance
    from vfe_sample_ref) from the closed form -- the midpoint rule's own error, which comes from the kink of max(0, .) at xi = g =
    (fBest - mu) / s and is there while g lies inside the samples' range: every g in [-3, 3] is asserted on the host reference."""
    c = QR.SMALL[3]
    m = Model.of(dev, ctx, c)
    Zb = np.random.default_rng(700 + Q1_SEED).uniform(-1.0, 1.0, (40, c[1]))
    nugget = QR.default_nugget(m.spec, Zb)
    xi = SR.stratified_normal(4096)
    ref = m.reference()
    mean = np.asarray(VS.mean(m.spec, m.S, ref, Zb), dtype=float)
    var = np.asarray(np.diag(VS.exact_cov(m.spec, m.S, ref, Zb)), dtype=float) + nugget
    g = (m.fBest - mean) / np.sqrt(var)
    assert np.all(np.abs(g) <= 3.0), g
    _, _, costs, nbad = m.qei(dev, ctx, Zb, 1, xi, nugget)
    closed = m.model.acq(m.alpha, m.pts(dev, ctx, Zb), dev.ACQ_EI, m.fBest)[2]
    tol = np.array([2.0 * abs(float(SR.qei_replay(mean[i:i + 1], np.sqrt(var[i:i + 1, None]), xi, m.fBest))
                              - float(SR.closed_form_ei(mean[i], var[i], m.fBest))) for i in range(40)])
    err = np.abs(costs - closed)
    print("  q=1: g %.2f .. %.2f, tolerance / |cost| %.2e .. %.2e, worst error / tolerance %.3f"
          % (np.min(g), np.max(g), np.min(tol / np.abs(closed)), np.max(tol / np.abs(closed)), np.max(err / tol)))
    assert nbad == 0 and np.all(err <= tol)


# ---- B4: B = 1 against the exact sampler ------------------------------------------------------------------------------------------------
def test_one_batch_against_the_exact_sampler(dev, ctx):
    """One batch of q = 16 points: the sample average -mean(max(0, fBest - min_j)) taken on the host from the exact sampler's draws
    (gpx_vfe_psampler_create, same points, base samples and nugget) against the device cost, within the q-EI bound (B2) plus the draw
    bound of sample_ref with M = q.  The two factors are different factorisations of the same matrix; each route is first held to its
    own replay, and the costs are compared, not the factors."""
    c, q, s = QR.SMALL[3], 16, 128
    m = Model.of(dev, ctx, c)
    Zq = np.random.default_rng(44).uniform(-1.0, 1.0, (q, c[1]))
    nugget = QR.default_nugget(m.spec, Zq)
    xi = SR.base_samples(s, q, seed=11)
    cost = m.qei(dev, ctx, Zq, q, xi, nugget)[2][0]
    mu, Cb, Fb = m.blocks(dev, ctx, Zq, q, nugget)
    own = SR.check_qei(cost, mu[0], Fb[0], xi, m.fBest, "B=1")
    dZ = m.pts(dev, ctx, Zq)
    zero = m.model.posterior_sampler(np.zeros(len(m.y)), dZ, nugget)         # alpha = 0: draw - mean IS F
    smp = m.model.posterior_sampler(m.alpha, dZ, nugget)
    try:
        F2 = np.ascontiguousarray(zero.draw(np.eye(q)).T)
        rows = smp.draw(xi)
        mean2 = smp.draw(np.zeros((1, q)))[0]
    finally:
        zero.close()
        smp.close()
    SR.check_draw(rows, mean2, F2, xi, "B=1 draws")
    via = -float(np.mean(np.maximum(m.fBest - np.min(rows, axis=1), 0.0)))
    tol = SR.qei_bound(mu[0], Fb[0], xi, cost) + float(np.max(SR.draw_bound(mean2, F2, xi)))
    cov2 = m.model.posterior_cov(dZ)
    r_cov = float(np.max(np.abs(Cb[0] - cov2) / QR.route_bound(m.nu, dev.kdiag(ctx, m.sp, dZ))))
    print("  B=1 against the sampler: cost %.17g (own replay: %.3f of its bound), through the sampler %.17g, |difference| %.3e, "
          "tolerance %.3e; the two covariances: %.3f of the route bound" % (cost, own, via, abs(cost - via), tol, r_cov))
    assert np.array_equal(mean2, mu[0]) and r_cov <= 1.0
    assert abs(cost - via) <= tol


# ---- B5: bits -------------------------------------------------------------------------------------------------------------------------------
def perm_case():
    from gpexp_amd import device as dev
    ctx = dev.context()
    c = QR.SMALL[2]
    m = Model.of(dev, ctx, c)
    Zb = QR.batches(c, m.S, 5, 257).copy()
    for pos in (128, 256):
        Zb[pos * 5:(pos + 1) * 5] = Zb[:5]
    return dev, ctx, m, Zb, QR.default_nugget(m.spec, Zb), SR.base_samples(130, 5, seed=6)


def chunk_digest():
    dev, ctx, m, Zb, nugget, xi = perm_case()
    best, best_cost, costs, _ = m.qei(dev, ctx, Zb, 5, xi, nugget)
    h = hashlib.sha256(np.ascontiguousarray(costs).tobytes())
    h.update(np.array([best], dtype=np.int64).tobytes() + np.array([best_cost]).tobytes())
    return h.hexdigest()


def test_permutation_copies_and_chunking():
    dev, ctx, m, Zb, nugget, xi = perm_case()
    best, best_cost, costs, _ = m.qei(dev, ctx, Zb, 5, xi, nugget)
    print("  257 batches: costs %.6g .. %.6g, best %d" % (np.min(costs), np.max(costs), best))
    assert costs[0] == costs[128] == costs[256]                                 # copies of batch 0, three workgroup positions
    perm = np.random.default_rng(4).permutation(257)
    Zp = Zb.reshape(257, 5, -1)[perm].reshape(257 * 5, -1)
    bp, bcp, cp, _ = m.qei(dev, ctx, Zp, 5, xi, nugget)
    assert np.array_equal(cp, costs[perm])                                      # bit for bit
    assert bcp == best_cost and bp == int(np.argmin(cp)) and best == int(np.argmin(costs))     # the FIRST minimum, in either order
    assert m.qei(dev, ctx, Zb, 5, xi, nugget)[2].tobytes() == costs.tobytes()   # two calls
    # GPX_CROSS_BYTES so small that a chunk holds 128 points: 24 batches a chunk, eleven chunks; a fresh child, not an exec
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe_qei as t\n"
                        "print('RESULT ' + t.chunk_digest(), flush=True)" % (ROOT, TESTS)],
                       env=dict(os.environ, GPX_CROSS_BYTES="1000"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:] == chunk_digest()


# ---- B6: the NaN rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 5, 32])
def test_singular_batch_gets_nan_and_is_skipped(dev, ctx, q):
    c = QR.SMALL[1]
    m = Model.of(dev, ctx, c)
    Zb = np.random.default_rng(q).uniform(-1.0, 1.0, (7 * q, c[1]))             # (no repeats: nugget 0 factors them)
    xi = SR.base_samples(64, q, seed=2)
    _, _, clean, nb0 = m.qei(dev, ctx, Zb, q, xi, 0.0)
    print("  q=%d nugget 0: n_bad %d, costs %s" % (q, nb0, clean))
    assert nb0 == 0 and np.all(np.isfinite(clean))
    j = int(np.argmin(clean))                                                   # spoil the winner
    twin = Zb.copy()
    twin[j * q + q - 1] = twin[j * q]                                           # two identical points in batch j
    best, best_cost, costs, nbad = m.qei(dev, ctx, twin, q, xi, 0.0)
    assert nbad == 1 and np.isnan(costs[j])
    keep = np.arange(7) != j
    assert np.array_equal(costs[keep], clean[keep])                             # the others: bit for bit
    assert best == int(np.flatnonzero(keep)[np.argmin(clean[keep])]) and best_cost == costs[best]
    assert np.all(np.isfinite(m.qei(dev, ctx, twin, q, xi, QR.default_nugget(m.spec, twin))[2]))   # the default nugget factors the twin
    every = np.repeat(Zb[:7], q, axis=0)                                        # every batch: q copies of one point
    best, best_cost, costs, nbad = m.qei(dev, ctx, every, q, xi, 0.0)
    assert nbad == 7 and np.all(np.isnan(costs)) and best == -1 and np.isnan(best_cost)


# ---- B7: refusals through the C ABI ------------------------------------------------------------------------------------------------------------
def test_errors(dev, ctx):
    from gpexp_amd._lib import GpxError
    c = QR.SMALL[1]
    m = Model.of(dev, ctx, c)
    Zb = QR.batches(c, m.S, 4, 3)
    dZ, xi4 = dev.points(ctx, Zb), SR.base_samples(8, 4)

    def call(q, xi, model=m.model, nugget=1e-10):
        return dev.VfeModel.acq_qei(model, m.alpha, dZ, q, xi, m.fBest, nugget)

    before = call(4, xi4)[2]
    for q, xi, msg in ((0, np.zeros((8, 0)), "batch size q"), (33, np.zeros((8, 33)), "batch size q"),
                       (5, np.zeros((8, 5)), "multiple of q"), (4, np.zeros((0, 4)), "at least one base sample")):
        with pytest.raises(GpxError, match=msg):
            call(q, xi)
    with pytest.raises(GpxError, match="nugget must not be negative"):
        call(4, xi4, nugget=-1e-12)
    fitc = dev.FitcModel(ctx, m.sp, m.dX, m.dS, m.noise)
    with pytest.raises(GpxError, match="FITC model.*gpx_acq_qei"):
        call(4, xi4, model=fitc)
    with pytest.raises(GpxError, match="FITC model"):
        dev.VfeModel.dbg_qei_blocks(fitc, m.alpha, dZ, 4, 1e-10)

    def raw(S, coeff):
        best, bc, nb = dev.c_i64(), dev.C.c_double(), dev.c_i64()
        costs = np.empty(3)
        dev.check(ctx.lib.gpx_vfe_acq_qei(ctx.h, m.model.h, S.h, dev.dptr(coeff), dZ.h, 4, dev.dptr(xi4), 8, m.fBest, 1e-10,
                                          dev.dptr(costs), dev.C.byref(best), dev.C.byref(bc), dev.C.byref(nb)))
        return costs
    with pytest.raises(GpxError, match="point sets do not match"):
        raw(m.dX, m.alpha)                                                      # a dense factor's points in place of S
    with pytest.raises(GpxError, match="NULL argument"):
        raw(m.dS, None)
    assert np.array_equal(raw(m.dS, m.alpha), before) and np.array_equal(call(4, xi4)[2], before)
    print("  every refusal is an argument error with its message; the model still answers with the same bits")


# ---- B8: the class API -----------------------------------------------------------------------------------------------------------------------
class _Space(object):
    def __init__(self, d):
        self.dimension = d


@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_class_api(kind):
    import test_gpu_vfe_sample as T
    from gpexp_amd.experimentalDesign import costFuncEI
    g, c = T._trained(kind, FITC=0.5, sparse="vfe")
    cf = costFuncEI(g, c["X"], c["y"], 2, _Space(2))
    C = c["Z"]
    xi = SR.base_samples(128, 4, seed=9)
    lies = ("believer", "min", "max", "mean")
    idx, cost, lie = cf.vfeSelectBatchJoint(C, 4, baseSamples=xi)
    proposals = [cf.selectBatch(C, 4, lie=name)[0] for name in lies]
    assert lie in lies and np.array_equal(idx, proposals[lies.index(lie)])
    # The winner's cost is its own vfeJointEI -- in the call that holds the same point sets, bit for bit.  A call on ONE proposal has
    # another bounding box, the fills centre on it, and its cost differs in the last bits (Model.pts carries the cube for that reason;
    # the class API uploads the points as they are): both are the same quantity computed twice, so that call is held to the figure
    # every VFE quantity is held to against its reference, 1e-8 x the largest cost, not to equality.
    stacked = np.stack([C[p] for p in proposals])
    four = cf.vfeJointEI(stacked, baseSamples=xi)
    alone = np.array([cf.vfeJointEI(C[p], baseSamples=xi)[0] for p in proposals])
    print("  %s: the proposals' joint costs %s, winner %r; one call per proposal differs by at most %.3e" % (kind, four, lie, np.max(np.abs(alone - four))))
    assert four.shape == (4,) and cost == np.min(four) and cost == four[lies.index(lie)]
    assert np.max(np.abs(alone - four)) <= 1e-8 * np.max(np.abs(four))                  # (the project's figure for VFE quantities)
    assert cf.vfeBestJointBatch(stacked, baseSamples=xi) == (int(np.argmin(four)), np.min(four))
    assert cf.vfeJointEI(stacked, nSamples=16).shape == (4,)                    # baseSamples=None: drawn with NumPy
    for call in (lambda: cf.jointEI(stacked, baseSamples=xi), lambda: cf.bestJointBatch(stacked, baseSamples=xi),
                 lambda: cf.selectBatchJoint(C, 4, baseSamples=xi)):
        with pytest.raises(NotImplementedError):
            call()


# ---- B9: the allocator's books ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [QR.SMALL[4], QR.OOP], ids=QR.case_id)
def test_allocator_books_balance(dev, ctx, c):
    m = Model.of(dev, ctx, c)
    Zb = QR.batches(c, m.S, 5, 3)
    xi, nugget = SR.base_samples(8, 5), QR.default_nugget(m.spec, Zb)
    m.qei(dev, ctx, Zb, 5, xi, nugget)              # (the factors' block inverses are built on the first solve and stay)
    ctx.sync()
    before = ctx.pool_stats()[1]
    m.qei(dev, ctx, Zb, 5, xi, nugget)
    m.blocks(dev, ctx, Zb, 5, nugget)
    ctx.sync()
    after = ctx.pool_stats()[1]
    print("  %s: outstanding pool bytes %d before, %d after" % (QR.case_id(c), before, after))
    assert after == before
