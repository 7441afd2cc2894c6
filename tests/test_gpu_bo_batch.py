"""q-point batch acquisition on the MI355X (selectBatch -> gpx_acq_batch: Kriging believer / constant liar by rank-one conditioning
of resident state) against the literal refit loop in NumPy (bo_batch_compose.refit_path), today's one-pick API, and itself."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bo_compose as bc
import bo_batch_compose as bb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
ACQS = {"ucb": (bc.UCB, 2.0), "pi": (bc.PI, "best"), "ei": (bc.EI, "best")}


class Space(object):
    def __init__(self, d):
        self.dimension = d


def kernel_of(spec):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    if spec["kind"] == "se":
        return KernelSquaredExponential(spec["cl"], spec["signalSize"], spec["d"])
    return KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)


def make_cost(acq, kernel, d, X, y, noise, kappa=2.0, **kw):
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    gp = GP(kernel, noise)
    if acq == bc.UCB:
        return costFuncGPUCbound(gp, kappa, X, y, 2, Space(d))
    if acq == bc.PI:
        return costFuncPI(gp, X, y, 2, Space(d))
    return costFuncEI(gp, X, y, 2, Space(d), **kw)


def lie_value(lie, y):
    return lie if lie == "believer" else float(getattr(np, lie)(y))


def self_consistent(idx, costs, allc):
    """1(ii), 1(iii): the device's picks are the first minima of its own rows, bit for bit; distinct; masked entries NaN."""
    from gpexp_amd.experimentalDesign import firstMinIndex
    q = len(idx)
    assert idx.dtype == np.int64 and idx.shape == (q,) and costs.shape == (q,) and allc.shape[0] == q
    for t in range(q):
        assert idx[t] == firstMinIndex(allc[t]), t
        assert costs[t] == allc[t, idx[t]], t
        assert np.all(np.isnan(allc[t, idx[:t]])), t
        assert np.count_nonzero(np.isnan(allc[t])) == t, t
    assert len(set(idx.tolist())) == q


def check_small(name, acqname, lie, q=8):
    """Test 1 for one configuration; returns the device's output."""
    acq, rule = ACQS[acqname]
    spec, X, y, C, noise = bb.problem(name)
    cf = make_cost(acq, kernel_of(spec), spec["d"], X, y, noise)
    idx, costs, allc = cf.selectBatch(C, q, lie=lie, returnAllCosts=True)
    self_consistent(idx, costs, allc)
    lv = lie_value(lie, y)
    _, rows, _ = bb.refit_path(spec, X, y, noise, C, acq, rule, lv, q, forced=idx)
    errs = [bb.row_err(allc[t], rows[t]) for t in range(q)]
    print("%s %s %s: worst row error against the forced refit loop %.3e" % (name, acqname, lie, max(errs)))
    assert max(errs) <= 1e-9, errs
    if acq != bc.PI:
        free, _, _ = bb.refit_path(spec, X, y, noise, C, acq, rule, lv, q)
        print("    device picks %s   refit-loop picks %s" % (idx.tolist(), free))
        assert idx.tolist() == free
    return idx, costs, allc


def digest(idx, costs, allc):
    h = hashlib.sha256()
    for a in (idx, costs, allc):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_bo_batch as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


# ---- 1. against the refit loop, small ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se3", "m52", "m32"])
@pytest.mark.parametrize("acqname", ["ucb", "pi", "ei"])
@pytest.mark.parametrize("lie", ["believer", "min", "max"])
def test_small_against_refit_loop(name, acqname, lie):
    check_small(name, acqname, lie)


# ---- 2. row 0 is today's API ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se3", "m52"])
@pytest.mark.parametrize("acqname", ["ei", "ucb"])
def test_row0_is_evaluate_batch(name, acqname):
    acq, _ = ACQS[acqname]
    spec, X, y, C, noise = bb.problem(name)
    cf = make_cost(acq, kernel_of(spec), spec["d"], X, y, noise)
    idx, costs, allc = cf.selectBatch(C, 3, returnAllCosts=True)
    one = cf.evaluateBatch(C)
    err = bb.row_err(allc[0], one)
    j, c = cf.bestCandidate(C)
    print("%s %s: row 0 against evaluateBatch %.3e" % (name, acqname, err))
    assert err <= 1e-13
    assert idx[0] == j
    assert abs(costs[0] - c) <= 1e-13 * np.max(np.abs(one))


# ---- 3. blocked-factor size ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acqname,lie", [("ei", "believer"), ("ucb", "min")])
def test_blocked_factor_size(acqname, lie):
    acq, rule = ACQS[acqname]
    spec, X, y, C, noise = bb.problem("big")
    cf = make_cost(acq, kernel_of(spec), spec["d"], X, y, noise)
    idx, costs, allc = cf.selectBatch(C, 16, lie=lie, returnAllCosts=True)
    self_consistent(idx, costs, allc)
    free, rows, _ = bb.refit_path(spec, X, y, noise, C, acq, rule, lie_value(lie, y), 16)
    print("big %s %s: device picks %s\n    refit-loop picks %s" % (acqname, lie, idx.tolist(), free))
    assert idx.tolist() == free
    want = np.array([rows[t][free[t]] for t in range(16)])
    err = np.abs(costs - want) / np.abs(want)
    print("    winner costs: worst relative error %.3e" % np.max(err))
    assert np.max(err) <= 1e-9


# ---- 4. lie semantics ----------------------------------------------------------------------------------------------------------
def test_lie_semantics():
    from gpexp_amd import device as dev
    spec, X, y, C, noise = bb.problem("m52")
    cf = make_cost(bc.EI, kernel_of(spec), 4, X, y, noise)
    gp = cf.gaussianProcess
    ctx = dev.context()

    def call(lie, value, **kw):
        return dev.acq_batch(ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, dev.points(ctx, C), float(gp.noise), dev.ACQ_EI,
                             float(np.max(y)), True, lie, value, 8, **kw)

    idx, costs, lies = call(dev.LIE_BELIEVER, 0.0)
    _, _, want = bb.refit_path(spec, X, y, noise, C, bc.EI, "best", "believer", 8, forced=idx)
    err = np.max(np.abs(lies - want) / np.maximum(1.0, np.abs(want)))
    print("believed values against the refit loop's posterior means: %.3e" % err)
    assert err <= 1e-9
    idx2, _, lies2, allc2 = call(dev.LIE_CONSTANT, 0.3, want_all=True)
    assert np.array_equal(lies2, np.full(8, 0.3))
    self_consistent(idx2, allc2[np.arange(8), idx2], allc2)
    # a given fBest= is the caller's constant: no tracking, although the believed value (max y) lies above it
    fb = float(np.median(y))
    cf2 = make_cost(bc.EI, kernel_of(spec), 4, X, y, noise, fBest=fb)
    idx3, costs3, allc3 = cf2.selectBatch(C, 8, lie="max", returnAllCosts=True)
    self_consistent(idx3, costs3, allc3)
    _, rows, _ = bb.refit_path(spec, X, y, noise, C, bc.EI, fb, float(np.max(y)), 8, forced=idx3)
    errs = [bb.row_err(allc3[t], rows[t]) for t in range(8)]
    print("fixed fBest: worst row error %.3e" % max(errs))
    assert max(errs) <= 1e-9
    _, tracked, _ = bb.refit_path(spec, X, y, noise, C, bc.EI, "best", float(np.max(y)), 8, forced=idx3)
    assert bb.row_err(allc3[1], tracked[1]) > 1e-6          # (the tracked rule is a different cost: the check discriminates)


# ---- 5. Mehler kernel ----------------------------------------------------------------------------------------------------------
def test_mehler_kernel():
    from gpExp.kernels import KernelMehlerND
    from oracle import gpexp_oracle as orc
    rng = np.random.default_rng(14)
    X, C = rng.uniform(-1, 1, (60, 2)), rng.uniform(-1, 1, (300, 2))
    y = np.sin(3 * X[:, 0]) + 0.5 * np.cos(2 * X.sum(axis=1))
    spec, noise = dict(kind="mehler", t=[0.3, 0.5], d=2), 1e-2
    cond = np.linalg.cond(orc.cov_matrix(spec, X, nugget=noise))
    print("Mehler: cond(K + noise I) = %.3e" % cond)
    assert cond <= 1e4                                      # where pinv and the factor agree
    cf = make_cost(bc.UCB, KernelMehlerND([0.3, 0.5], 2), 2, X, y, noise)
    idx, costs, allc = cf.selectBatch(C, 4, returnAllCosts=True)
    self_consistent(idx, costs, allc)

    def posterior_of(Xa, ya):
        model = orc.fit(spec, Xa, ya, noise)
        return lambda Z: orc.posterior(spec, model, Z)

    _, rows, _ = bb.refit_path(spec, X, y, noise, C, bc.UCB, 2.0, "believer", 4, forced=idx, posterior_of=posterior_of)
    errs = [bb.row_err(allc[t], rows[t]) for t in range(4)]
    print("Mehler: worst row error %.3e" % max(errs))
    assert max(errs) <= 1e-9, errs


# ---- 6. duplicates and near-zero noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [1e-3, 1e-8])
def test_duplicates_and_near_zero_noise(noise):
    spec = bb.CONFIGS["se3"][0]
    rng = np.random.default_rng(7)
    X, C = rng.uniform(-1, 1, (60, 3)), rng.uniform(-1, 1, (200, 3))
    C[150] = C[20]
    C[3] = X[5]
    y = np.sin(3 * X[:, 0])
    cf = make_cost(bc.UCB, kernel_of(spec), 3, X, y, noise)
    idx, costs, allc = cf.selectBatch(C, 10, returnAllCosts=True)
    assert np.all(np.isfinite(costs))
    for t in range(10):
        assert np.all(np.isfinite(np.delete(allc[t], idx[:t])))
    assert len(set(idx.tolist())) == 10
    free, _, _ = bb.refit_path(spec, X, y, noise, C, bc.UCB, 2.0, "believer", 10)
    print("noise %g: device picks %s   refit-loop picks %s" % (noise, idx.tolist(), free))
    assert idx.tolist() == free


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------
def case_digest():
    spec, X, y, C, noise = bb.problem("m52")
    cf = make_cost(bc.EI, kernel_of(spec), 4, X, y, noise)
    return digest(*cf.selectBatch(C, 8, lie="min", returnAllCosts=True))


def test_determinism():
    a, b = case_digest(), case_digest()
    assert a == b
    assert run_child("print('RESULT ' + t.case_digest(), flush=True)", {"GPX_CHAOS": "7"}) == a


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_errors():
    from gpexp_amd._lib import GpxError
    spec, X, y, C, noise = bb.problem("m32")
    cf = make_cost(bc.EI, kernel_of(spec), 2, X, y, noise)
    before = cf.evaluateBatch(C)
    with pytest.raises(ValueError):
        cf.selectBatch(C[:5], 6)
    with pytest.raises(GpxError):
        cf.selectBatch(C, 0)
    nan = make_cost(bc.EI, kernel_of(spec), 2, X, y, noise, fBest=float("nan"))
    with pytest.raises(GpxError, match=r"pick 1\b"):
        nan.selectBatch(C, 4)
    np.random.seed(3)
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI
    fitc = costFuncEI(GP(kernel_of(spec), noise, FITC=0.5), X, y, 2, Space(2))
    with pytest.raises(NotImplementedError):
        fitc.selectBatch(C, 4)
    idx, _ = cf.selectBatch(C, 4)
    assert len(idx) == 4
    assert np.array_equal(cf.evaluateBatch(C), before)


# ---- 9. allocator --------------------------------------------------------------------------------------------------------------
def guarded_case():
    from gpexp_amd import device as dev
    check_small("se3", "ei", "believer")
    ctx = dev.context()
    ctx.sync()
    return int(ctx.lib.gpx_dbg_guard_violations(ctx.h))


def test_under_allocation_guard_and_nan_fill():
    """Guard bands + NaN-filled blocks: U's unused rows and the padding columns of W_C (M = 500 in 512) never reach a result."""
    assert run_child("print('RESULT %d' % t.guarded_case(), flush=True)", {"GPX_ALLOC_GUARD": "2"}) == "0"
