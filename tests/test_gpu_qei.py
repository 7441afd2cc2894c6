"""GPU (-m gpu): Monte-Carlo joint expected improvement (gpx_acq_qei) held to the contracts of tests/sample_ref.py: the blocks the
kernel works on (test hook gpx_dbg_qei_blocks) against a longdouble reference and the factor's backward-error bound, the costs
against a longdouble replay from the device's OWN blocks, q = 1 against gpx_acq's closed form, B = 1 against the sampler, bit-for-bit
invariance under permutation and chunking, the NaN rule, the errors, and selectBatchJoint."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_stability_ref as CR
import design_replay_ref as DR
import sample_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
QS, BS = (1, 2, 5, 16, 32), (1, 3, 257)
KINDS = ("se", "matern32", "matern52", "mehler")


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def setting(q, b):
    """(kind, N, d, noise, S) of the case (q, B): the kernels, sizes, noises and sample counts of the issue dealt over the grid; the
    257-batch cases keep N = 40 (their longdouble reference solves N x 257 q right-hand sides)."""
    i = QS.index(q) * len(BS) + BS.index(b)
    kind = KINDS[i % 4]
    n = 40 if b == 257 else (40, 200)[i % 2]
    noise = 1e-2 if kind == "mehler" else (1e-2, 1e-6)[(i // 2) % 2]
    if kind == "mehler":
        d = (2, 1)[i % 2]
    else:                                 # (one dimension only with the well-conditioned noise: the nugget rule was tried on d = 2, 8)
        d = (2, 8)[i % 2] if noise == 1e-6 else (1, 2, 8)[i % 3]
    return kind, n, d, noise, (130, 3, 128, 1)[i % 4]


class Model(object):
    def __init__(self, dev, ctx, kind, n, d, noise, q, nb, seed=0):
        self.c = c = SR.points_case(kind, n, 1, d, noise, seed=seed)
        self.sp, self.q, self.nb, self.n = SR.device_spec(dev, c["spec"]), q, nb, n
        rng = np.random.default_rng(100 * q + nb + seed)
        Zb = rng.uniform(-1.0, 1.0, (nb * q, d))
        if q >= 2:
            Zb[1] = c["X"][3]                 # batch 0: a point ON a training point ...
        if q >= 5:
            Zb[q - 1] = Zb[0]                 # ... and its last point repeats its first
        self.Zb = Zb
        self.dX = dev.points(ctx, c["X"])
        self.K = dev.kfill(ctx, self.sp, self.dX, nugget=noise)
        self.Khost = self.K.to_host()
        ctx.sync()
        self.L = dev.potrf(ctx, self.K)
        self.alpha = dev.potrs(ctx, self.L, c["y"])
        self.fBest = float(np.max(c["y"]))
        self.nugget = 1e-10 * SR.prior_max(c["spec"], Zb)

    def pts(self, dev, ctx, Zb):
        """Zb on the device carrying the box [-1, 1]^d: the fills centre on the bounding box of their point sets, so two calls whose
        batches differ in one point would otherwise differ in the last bits of EVERY cross covariance."""
        d = Zb.shape[1]
        return dev.points_slice(ctx, np.vstack([Zb, -np.ones((1, d)), np.ones((1, d))]), 0, Zb.shape[0])

    def qei(self, dev, ctx, xi, Zb=None, nugget=None, **kw):
        Zb = self.Zb if Zb is None else Zb
        return dev.acq_qei(ctx, self.sp, self.L, self.dX, self.alpha, self.pts(dev, ctx, Zb), self.q, xi, self.fBest,
                           self.nugget if nugget is None else nugget, **kw)

    def blocks(self, dev, ctx, Zb=None, nugget=None):
        Zb = self.Zb if Zb is None else Zb
        return dev.dbg_qei_blocks(ctx, self.sp, self.L, self.dX, self.alpha, self.pts(dev, ctx, Zb), self.q,
                                  self.nugget if nugget is None else nugget)


def worst_factor_ratio(Fb, Cb, nugget):
    q = Fb.shape[1]
    worst = 0.0
    for b in range(Fb.shape[0]):
        assert np.all(np.triu(Fb[b], 1) == 0.0), "batch %d: F_b is not lower triangular" % b
        Chat = Cb[b].copy()
        Chat[np.diag_indices(q)] += nugget
        worst = max(worst, SR.factor_residual(Fb[b], Chat) / SR.factor_bound(q))
    return worst


# ---- 1, 2: the hook's blocks and the costs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("q", QS)
def test_blocks_and_costs(dev, ctx, q, b):
    kind, n, d, noise, s = setting(q, b)
    m = Model(dev, ctx, kind, n, d, noise, q, b)
    xi = SR.base_samples(s, q, seed=q + b)
    best, best_cost, costs, nbad = m.qei(dev, ctx, xi)
    mu, Cb, Fb = m.blocks(dev, ctx)
    assert nbad == 0 and costs.shape == (b,) and np.all(np.isfinite(costs))
    dZ = m.pts(dev, ctx, m.Zb)
    assert np.array_equal(mu.ravel(), dev.posterior(ctx, m.sp, m.L, m.dX, m.alpha, dZ, want_var=False)[0])     # gpx_posterior's bits
    assert np.array_equal(Cb, np.transpose(Cb, (0, 2, 1)))
    # C_b against the longdouble reference from the device's own fills, under posterior_ref's covariance metric and bound
    Bx = dev.kfill(ctx, m.sp, m.dX, Z=dZ).to_host()
    P3 = m.Zb.reshape(b, q, d)
    kzz = dev.kernel_eval(ctx, m.sp, np.repeat(P3, q, axis=1).reshape(-1, d), np.tile(P3, (1, q, 1)).reshape(-1, d)).reshape(b, q, q)
    val, scale = SR.block_cov_reference(m.Khost, Bx, kzz, q)
    refs = {r: SR.block_cov_omega(SR.block_cov_route(r, m.Khost, Bx, kzz, q), val, scale) for r in ("lapack", "b128")}
    CR.check_bound("q=%d B=%d %s omega_c" % (q, b, kind), SR.block_cov_omega(Cb, val, scale), refs)
    # F_b: lower triangular, backward error of the factorisation
    ratio = worst_factor_ratio(Fb, Cb, m.nugget)
    print("  q=%d B=%d: worst |F F^T - Chat| / bound %.3f" % (q, b, ratio))
    assert ratio <= 1.0
    # the costs against the replay from the device's own blocks
    worst = max(SR.check_qei(costs[i], mu[i], Fb[i], xi, m.fBest, "batch %d" % i) for i in range(b))
    print("  q=%d B=%d S=%d: worst |cost - replay| / bound %.3f" % (q, b, s, worst))
    assert best == int(np.argmin(costs)) and best_cost == costs[best]
    assert m.qei(dev, ctx, xi, want_costs=False)[:2] == (best, best_cost)


# ---- 3: q = 1 against the closed form ----------------------------------------------------------------------------------------------
def test_q1_against_closed_form_ei(dev, ctx):
    """q = 1 with the stratified base samples xi_s = Phi^-1((s + 1/2) / S), S = 4096, against gpx_acq's closed-form EI at the same
    points.  Tolerance per point: 2 x the distance of the REFERENCE's longdouble replay (host mean and variance) from the closed
    form, i.e. the midpoint rule's own error, which comes from the kink of max(0, .) at xi = g = (fBest - mu) / s and is there
    only while g lies inside the samples' range (|xi| <= 3.7): the 40 points are far from the 40 training points in 8 dimensions
    (s near the prior's), g = 0.78 .. 1.31, asserted.  Measured on the reference: 2.9e-5 .. 4.4e-5 of |cost|; the device's own
    rounding (1e-16) is what the factor 2 is for."""
    m = Model(dev, ctx, "matern32", 40, 8, 1e-2, 1, 40)
    xi = SR.stratified_normal(4096)
    _, _, costs, nbad = m.qei(dev, ctx, xi)
    closed = dev.acq(ctx, m.sp, m.L, m.dX, m.alpha, m.pts(dev, ctx, m.Zb), dev.ACQ_EI, m.fBest)[2]
    mean, Cm = SR.host_posterior(m.c, m.Zb)
    var = np.diag(Cm) + m.nugget
    g = (m.fBest - mean) / np.sqrt(var)
    assert np.all(np.abs(g) < 3.0)
    tol = np.array([2.0 * abs(float(SR.qei_replay(mean[i:i + 1], np.sqrt(var[i:i + 1, None]), xi, m.fBest))
                              - float(SR.closed_form_ei(mean[i], var[i], m.fBest))) for i in range(40)])
    err = np.abs(costs - closed)
    print("  q=1: g %.2f .. %.2f, tolerance / |cost| %.2e .. %.2e, worst error / tolerance %.3f"
          % (np.min(g), np.max(g), np.min(tol / np.abs(closed)), np.max(tol / np.abs(closed)), np.max(err / tol)))
    assert nbad == 0 and np.all(err <= tol)


# ---- 4: B = 1 against the sampler ---------------------------------------------------------------------------------------------------
def reference_costs(m, Zq, xi):
    """(float64 NumPy replay, longdouble replay) of one batch from the points."""
    c, spec, nug = m.c, m.c["spec"], m.nugget
    mu, Cm = SR.host_posterior(c, Zq)
    c64 = float(SR.qei_replay(mu, np.linalg.cholesky(Cm + nug * np.eye(len(Zq))), xi, m.fBest, dtype=np.float64))
    K = DR.cov_ld(spec, c["X"])
    K[np.diag_indices(m.n)] += SR.LD(c["noise"])
    L = DR.chol_ld(K)
    Bl = DR.cov_ld(spec, c["X"], Zq)
    W = DR.solve_lower_ld(L, Bl)
    al = SR.P.solve_upper_ld(L, DR.solve_lower_ld(L, np.asarray(c["y"], dtype=SR.LD)[:, None]))[:, 0]
    Cl = DR.cov_ld(spec, Zq) - np.dot(W.T, W)
    Cl[np.diag_indices(len(Zq))] += SR.LD(nug)
    return c64, float(SR.qei_replay(np.dot(Bl.T, al), DR.chol_ld(Cl), xi, m.fBest))


def test_one_batch_against_the_sampler(dev, ctx):
    """B = 1, well conditioned (Matern 3/2, noise 1e-2, separated points): the cost against the sampler's draws at the same q points,
    base samples and nugget, reduced on the host.  Two factorisation codes meet here, so the tolerance is 8 x the distance between
    the REFERENCE's float64 NumPy replay and its longdouble replay from the points: measured 2.9e-15, tolerance 2.3e-14."""
    q, s = 5, 128
    m = Model(dev, ctx, "matern32", 200, 2, 1e-2, 1, 1)
    m.q = q
    Zq = np.array([[-0.8, -0.7], [0.75, -0.6], [0.0, 0.1], [-0.7, 0.8], [0.8, 0.7]])
    xi = SR.base_samples(s, q, seed=11)
    cost = m.qei(dev, ctx, xi, Zb=Zq)[2][0]
    smp = dev.PosteriorSampler(ctx, m.sp, m.L, m.dX, m.alpha, m.pts(dev, ctx, Zq), m.nugget)
    try:
        rows = smp.draw(xi)
    finally:
        smp.close()
    via = -float(np.mean(np.maximum(m.fBest - np.min(rows, axis=1), 0.0)))
    c64, cld = reference_costs(m, Zq, xi)
    tol = 8.0 * abs(c64 - cld)
    print("  B=1 against the sampler: cost %.17g, through the sampler %.17g, |difference| %.3e, tolerance %.3e"
          % (cost, via, abs(cost - via), tol))
    assert tol > 0.0 and abs(cost - via) <= tol


# ---- 5: permutation and chunking ----------------------------------------------------------------------------------------------------
def perm_case():
    from gpexp_amd import device as dev
    ctx = dev.context()
    m = Model(dev, ctx, "se", 40, 2, 1e-2, 5, 257)
    m.Zb = m.Zb.copy()
    for pos in (128, 256):
        m.Zb[pos * 5:(pos + 1) * 5] = m.Zb[:5]
    return dev, ctx, m, SR.base_samples(130, 5, seed=6)


def chunk_digest():
    dev, ctx, m, xi = perm_case()
    best, best_cost, costs, _ = m.qei(dev, ctx, xi)
    h = hashlib.sha256(np.ascontiguousarray(costs).tobytes())
    h.update(np.array([best], dtype=np.int64).tobytes() + np.array([best_cost]).tobytes())
    return h.hexdigest()


def test_permutation_copies_and_chunking():
    dev, ctx, m, xi = perm_case()
    best, best_cost, costs, _ = m.qei(dev, ctx, xi)
    assert costs[0] == costs[128] == costs[256]                                 # copies of batch 0, three workgroup positions
    perm = np.random.default_rng(4).permutation(257)
    Zp = m.Zb.reshape(257, 5, 2)[perm].reshape(-1, 2)
    bp, bcp, cp, _ = m.qei(dev, ctx, xi, Zb=Zp)
    assert np.array_equal(cp, costs[perm])                                      # bit for bit
    assert bcp == best_cost and bp == int(np.argmin(cp)) and best == int(np.argmin(costs))     # the FIRST minimum, in either order
    assert m.qei(dev, ctx, xi)[2].tobytes() == costs.tobytes()                  # two calls
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_qei as t\nprint('RESULT ' + t.chunk_digest(), flush=True)" % (ROOT, TESTS)],
                       env=dict(os.environ, GPX_CROSS_BYTES="100000"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:] == chunk_digest()


# ---- 6: the NaN rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 5, 32])
def test_singular_batch_gets_nan_and_is_skipped(dev, ctx, q):
    m = Model(dev, ctx, "matern32", 40, 2, 1e-2, q, 7, seed=1)
    Zb = np.random.default_rng(q).uniform(-1.0, 1.0, (7 * q, 2))               # (no repeats: nugget 0 factors them)
    xi = SR.base_samples(64, q, seed=2)
    _, _, clean, nb0 = m.qei(dev, ctx, xi, Zb=Zb, nugget=0.0)
    assert nb0 == 0 and np.all(np.isfinite(clean))
    j = int(np.argmin(clean))                                                  # spoil the winner
    twin = Zb.copy()
    twin[j * q + q - 1] = twin[j * q]                                          # two identical points in batch j
    best, best_cost, costs, nbad = m.qei(dev, ctx, xi, Zb=twin, nugget=0.0)
    assert nbad == 1 and np.isnan(costs[j])
    keep = np.arange(7) != j
    assert np.array_equal(costs[keep], clean[keep])                             # the others: bit for bit
    assert best == int(np.flatnonzero(keep)[np.argmin(clean[keep])]) and best_cost == costs[best]
    assert np.all(np.isfinite(m.qei(dev, ctx, xi, Zb=twin)[2]))                 # the default nugget factors the twin
    every = np.repeat(Zb[:7], q, axis=0)                                        # every batch: q copies of one point
    best, best_cost, costs, nbad = m.qei(dev, ctx, xi, Zb=every, nugget=0.0)
    assert nbad == 7 and np.all(np.isnan(costs)) and best == -1 and np.isnan(best_cost)


# ---- 7: errors --------------------------------------------------------------------------------------------------------------------------
def test_errors(dev, ctx):
    from gpexp_amd._lib import GpxError
    m = Model(dev, ctx, "matern32", 40, 2, 1e-2, 4, 3)
    dZ = dev.points(ctx, m.Zb)

    def call(q, xi, Z=dZ, nugget=1e-10):
        return dev.acq_qei(ctx, m.sp, m.L, m.dX, m.alpha, Z, q, xi, m.fBest, nugget)

    before = call(4, SR.base_samples(8, 4))[2]
    for q, xi in ((0, np.zeros((8, 0))), (33, np.zeros((8, 33))), (5, np.zeros((8, 5))), (4, np.zeros((0, 4)))):
        with pytest.raises(GpxError):
            call(q, xi)
    with pytest.raises(GpxError):
        call(4, SR.base_samples(8, 4), nugget=-1e-12)
    assert np.array_equal(call(4, SR.base_samples(8, 4))[2], before)
    np.random.seed(3)
    from gpExp.experimentalDesign import costFuncEI
    from gpExp.gp import GP
    from gpExp.kernels import KernelIsoMatern
    for kw in (dict(FITC=0.5), dict(FITC=0.5, sparse="vfe")):
        cf = costFuncEI(GP(KernelIsoMatern(0.7, 1.1, 2, nu=1.5), 1e-2, **kw), m.c["X"], m.c["y"], 2, Space(2))
        for fn in (lambda: cf.jointEI(m.Zb.reshape(3, 4, 2)), lambda: cf.bestJointBatch(m.Zb.reshape(3, 4, 2)),
                   lambda: cf.selectBatchJoint(m.Zb, 2), lambda: cf.thompsonBatch(m.Zb, 2),
                   lambda: cf.gaussianProcess.samplePosterior(m.Zb), lambda: cf.gaussianProcess.samplePrior(m.Zb)):
            with pytest.raises(NotImplementedError):
                fn()


# ---- 8: the class API ----------------------------------------------------------------------------------------------------------------
class Space(object):
    def __init__(self, d):
        self.dimension = d


def test_select_batch_joint_and_thompson(dev, ctx):
    from gpExp.experimentalDesign import costFuncEI
    from gpExp.gp import GP
    from gpExp.kernels import KernelIsoMatern
    c = SR.points_case("matern32", 200, 300, 2, 1e-2)
    cf = costFuncEI(GP(KernelIsoMatern(0.7, 1.1, 2, nu=1.5), 1e-2), c["X"], c["y"], 2, Space(2))
    C = np.random.default_rng(12).uniform(-1.0, 1.0, (300, 2))
    xi = SR.base_samples(128, 4, seed=9)
    idx, cost, lie = cf.selectBatchJoint(C, 4, baseSamples=xi)
    lies = ("believer", "min", "max", "mean")
    proposals = [cf.selectBatch(C, 4, lie=name)[0] for name in lies]
    four = np.array([cf.jointEI(C[p], baseSamples=xi)[0] for p in proposals])
    assert lie in lies and np.array_equal(idx, proposals[lies.index(lie)])
    assert cost == np.min(four) and cost == four[lies.index(lie)]
    assert np.array_equal(cf.jointEI(np.stack([C[p] for p in proposals]), baseSamples=xi), four)
    # Thompson picks: the first arg-min of the device's own joint draws
    xt = SR.base_samples(6, 300, seed=10)
    pick, val = cf.thompsonBatch(C, 6, baseSamples=xt)
    rows = cf.gaussianProcess.samplePosterior(C, baseSamples=xt)
    SR.check_argbest(pick, val, rows, True, "thompsonBatch")
    assert cf.gaussianProcess.samplePrior(C[:7], nSamples=3).shape == (3, 7)
    with pytest.raises(NotImplementedError):
        cf.gaussianProcess.generateSamples(C[:7])
