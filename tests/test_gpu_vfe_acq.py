"""Bayesian-optimisation costs, their gradient and q-point batches on a VFE model on the device (gpx_vfe_acq / gpx_vfe_acq_grad /
gpx_vfe_acq_batch, VfeModel.acq*, and the batched methods of costFuncGPUCbound / costFuncPI / costFuncEI on
GP(..., FITC=fraction, sparse="vfe")) against the NumPy forms of tests/vfe_acq_ref.py, which tests/test_vfe_acq_host.py ties to
central differences and to the literal refit loop.

Shapes: those at which the predictor's kernels can go wrong (tests/test_gpu_vfe.py's list) -- the six cases of fitc_grad_ref
(nu = 129 / N = 257 one past a 128 tile, nu = 40 below one tile, nu = 257), BLOCKED (nu = 1152: Lu and La cross the 1024-order block
inverses) and one case past the out-of-place solve branch (nu = 2049 pads to 2176 >= 2048); M = 300 candidates (no multiple of
128, five of them training points) and M = 1.  The backward sweeps of the gradient use chol_trsm_right_n at every order: there is no
further branch at padded order 4096 (the dense path's `bytesT` one), hence no nu = 4100 case.

Tolerances: costs against bo_compose.costs of vfe_ref.predict 1e-8 of the largest |cost| (the predictor's own figure in
tests/test_gpu_vfe.py); against bo_compose.costs of the device's own posterior 1e-12 (only the epilogue is left: device erfc / exp
against SciPy); gradients 1e-6 against central differences (h = 1e-5) and 1e-8 of the largest entry against vfe_acq_ref.grad (dF/dS's
figure); batch rows 1e-9 against the refit loop forced to the device's picks (tests/test_gpu_bo_batch.py's figure)."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bo_batch_compose as bb
import bo_compose as bc
import fitc_grad_ref as ref
import vfe_acq_ref as aref
import vfe_ref as vref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
CASES["blocked-m52-d8-nu1152"] = ref.BLOCKED
CASES["oop-m52-d8-nu2049"] = ("matern52", 8, [1.5], 1.2, 2304, 2049, 0.05, 19)
ACQS = ["ucb", "pi", "ei"]


class Space(object):
    def __init__(self, d):
        self.dimension = d


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, y, noise, Z, mean, var, Zg): Z the 300 candidates of the value tests with vfe_ref's posterior there, Zg the 24 of
    the gradient tests.  Computed once per case, shared, never modified."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    Z = np.random.default_rng(31).uniform(-1.2, 1.2, (300, spec["d"]))
    Z[:5] = X[:5]
    mean, var = vref.predict(spec, X, S, y, noise, Z)
    Zg = aref.grad_inputs(spec, X, y)
    for a in (X, S, y, Z, mean, var, Zg):
        a.setflags(write=False)
    return spec, X, S, y, noise, Z, mean, var, Zg


@functools.lru_cache(maxsize=None)
def reference_gradients(cid):
    """{acq name: (24, d) closed-form gradient at Zg}: one model for the three costs."""
    spec, X, S, y, noise = problem(cid)[:5]
    setup = aref.grad_setup(spec, X, S, y, noise, problem(cid)[8])
    return {name: aref.grad_of(setup, acq, param_of(y)) for name, (acq, param_of) in aref.ACQ_PARAMS.items()}


@functools.lru_cache(maxsize=None)
def batch_candidates(cid):
    C = np.random.default_rng(41).uniform(-1.0, 1.0, (400, problem(cid)[0]["d"]))
    C.setflags(write=False)
    return C


def kernel_spec(spec):
    from gpexp_amd import device as dev
    return dev.KernelSpec(ref.KIND_ID[spec["kind"]], spec["d"], ref.hyp_of(spec))


def device_model(cid, cls="VfeModel"):
    """(dev, ctx, model, coeff)"""
    from gpexp_amd import device as dev
    spec, X, S, y, noise = problem(cid)[:5]
    ctx = dev.context()
    model = getattr(dev, cls)(ctx, kernel_spec(spec), dev.points(ctx, X), dev.points(ctx, S), noise)
    return dev, ctx, model, model.solve(y)[0]


def make_gp(spec, noise, S=None, **kw):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    from gpExp.gp import GP
    if spec["kind"] == "se":
        k = KernelSquaredExponential(list(spec["cl"]), spec["signalSize"], spec["d"])
    else:
        k = KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)
    gp = GP(k, noise, **kw)
    if S is not None:
        gp.fitcnodes = np.array(S)
    return gp


def make_cost(cid, acqname, sparse="vfe", **kw):
    """The class-API cost on the case's data with the case's inducing points."""
    from gpExp.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    spec, X, S, y, noise = problem(cid)[:5]
    X, y = np.array(X), np.array(y)
    gp = make_gp(spec, noise, S, FITC=0.5, **({"sparse": sparse} if sparse else {}))
    if acqname == "ucb":
        cf = costFuncGPUCbound(gp, 2.0, X, y, 2, Space(spec["d"]))
    elif acqname == "pi":
        cf = costFuncPI(gp, X, y, 2, Space(spec["d"]))
    else:
        cf = costFuncEI(gp, X, y, 2, Space(spec["d"]), **kw)
    cf.callersGP = gp
    return cf


def vrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def self_consistent(idx, costs, allc):
    """The device's picks are the first minima of its own rows, bit for bit; distinct; masked entries NaN."""
    from gpexp_amd.experimentalDesign import firstMinIndex
    q = len(idx)
    assert idx.dtype == np.int64 and idx.shape == (q,) and costs.shape == (q,) and allc.shape[0] == q
    for t in range(q):
        assert idx[t] == firstMinIndex(allc[t]), t
        assert costs[t] == allc[t, idx[t]], t
        assert np.all(np.isnan(allc[t, idx[:t]])), t
        assert np.count_nonzero(np.isnan(allc[t])) == t, t
    assert len(set(idx.tolist())) == q


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe_acq as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


# ---- 1. values and arg-min ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_values_and_argmin(cid):
    from gpexp_amd.experimentalDesign import firstMinIndex
    spec, X, S, y, noise, Z, mean_ref, var_ref = problem(cid)[:8]
    dev, ctx, model, coeff = device_model(cid)
    Zd = dev.points(ctx, Z)
    dmean, dvar = model.posterior(coeff, Zd)
    for name in ACQS:
        acq, param_of = aref.ACQ_PARAMS[name]
        p = param_of(y)
        best, best_cost, costs = model.acq(coeff, Zd, acq, p)
        want = bc.costs(acq, p, mean_ref, var_ref)
        own = bc.costs(acq, p, dmean, dvar)
        e_ref, e_own = vrel(costs, want), vrel(costs, own)
        print("%s %s: costs against vfe_ref %.2e, against the device's own posterior %.2e" % (cid, name, e_ref, e_own))
        assert costs.shape == (300,) and np.all(np.isfinite(costs))
        assert e_ref <= 1e-8, (name, e_ref)
        assert e_own <= 1e-12, (name, e_own)
        j = firstMinIndex(costs)
        assert best == j and best_cost == costs[j]
        assert model.acq(coeff, Zd, acq, p, want_costs=False) == (best, best_cost, None)
        # M = 1
        b1, c1, one = model.acq(coeff, dev.points(ctx, Z[7:8]), acq, p)
        assert b1 == 0 and c1 == one[0] and abs(one[0] - want[7]) <= 1e-8 * np.max(np.abs(want))
        # duplicated candidates: the first copy wins
        assert model.acq(coeff, dev.points(ctx, np.vstack((Z, Z[j:j + 1]))), acq, p, want_costs=False)[0] == j
        assert model.acq(coeff, dev.points(ctx, np.vstack((Z[j:j + 1], Z))), acq, p, want_costs=False)[0] == 0
    best, best_cost, costs = model.acq(coeff, Zd, dev.ACQ_EI, float("nan"))
    assert best == -1 and np.isnan(best_cost) and np.all(np.isnan(costs))


# ---- 2. chunking -------------------------------------------------------------------------------------------------------------------
def chunk_digest(cid="m32-d8-nu257"):
    y, Z = problem(cid)[3], problem(cid)[5]
    dev, ctx, model, coeff = device_model(cid)
    h = hashlib.sha256()
    for name in ACQS:
        acq, param_of = aref.ACQ_PARAMS[name]
        best, best_cost, costs = model.acq(coeff, dev.points(ctx, Z), acq, param_of(y))
        c2, grad = model.acq_grad(coeff, dev.points(ctx, Z), acq, param_of(y))
        for a in (np.array([best], dtype=np.int64), np.array([best_cost]), costs, c2, grad):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_chunked_calls_return_the_same_bits():
    """A child process whose GPX_CROSS_BYTES allows 128 candidates per chunk (nu = 257 pads to 384 rows): M = 300 runs as three
    chunks of 128, 128 and 44.  Costs, winner and gradients: the bits of the unchunked call."""
    here = chunk_digest()
    assert run_child("print('RESULT ' + t.chunk_digest(), flush=True)", {"GPX_CROSS_BYTES": str(384 * 8 * 128)}) == here


# ---- 3. gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
@pytest.mark.parametrize("acqname", ACQS)
def test_gradient(cid, acqname):
    spec, X, S, y = problem(cid)[:4]
    Zg = np.array(problem(cid)[8])
    d = spec["d"]
    cf = make_cost(cid, acqname)
    costs, G = cf.evaluateBatchWithDerivative(Zg)
    assert G.shape == (24, d) and np.all(np.isfinite(G))
    assert np.array_equal(costs, cf.evaluateBatch(Zg))                      # acq_grad's costs: acq's bits
    assert np.array_equal(cf.derivativeBatch(Zg), G)
    fd = aref.central_differences(cf.evaluateBatch, Zg)
    e_fd, e_ref = vrel(G, fd), vrel(G, reference_gradients(cid)[acqname])
    print("%s %s: gradient against central differences %.2e, against the closed form in NumPy %.2e" % (cid, acqname, e_fd, e_ref))
    assert np.max(np.abs(fd)) > 1e-3
    assert e_fd <= 1e-6, e_fd
    assert e_ref <= 1e-8, e_ref
    # (one candidate alone: the fill is centred on another bounding box, so the last bits may differ)
    assert np.max(np.abs(cf.derivative(np.vstack((X[:1], Zg[5:6]))) - G[5])) <= 1e-10 * np.max(np.abs(G))


def mehler_cost():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncGPUCbound
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (150, 2))
    y = np.sin(X.sum(1))
    np.random.seed(23)
    gp = GP(KernelMehlerND([0.5, 0.3], 2), 0.05, FITC=0.5, sparse="vfe")
    return costFuncGPUCbound(gp, 2.0, X, y, 2, Space(2)), rng.uniform(-1.0, 1.0, (300, 2))


def test_mehler_has_values_and_batches_and_no_gradient():
    from gpexp_amd._lib import GpxError
    cf, C = mehler_cost()
    costs = cf.evaluateBatch(C)
    assert costs.shape == (300,) and np.all(np.isfinite(costs))
    mean, var = cf.gaussianProcess.evaluate(C, compvar=1)
    assert vrel(costs, bc.costs(bc.UCB, 2.0, mean, var)) <= 1e-12
    with pytest.raises(GpxError, match="Mehler"):
        cf.derivativeBatch(C)
    idx, c, allc = cf.selectBatch(C, 4, returnAllCosts=True)
    self_consistent(idx, c, allc)
    assert np.array_equal(allc[0], costs)


# ---- 4. batch ----------------------------------------------------------------------------------------------------------------------
def check_batch(cid, acqname, lie, q, **kw):
    """The device's batch against the refit loop; returns the device's output."""
    spec, X, S, y, noise = problem(cid)[:5]
    C = np.array(batch_candidates(cid))
    acq = aref.ACQ_PARAMS[acqname][0]
    rule = 2.0 if acq == bc.UCB else kw.get("fBest", "best")
    cf = make_cost(cid, acqname, **kw)
    idx, costs, allc = cf.selectBatch(C, q, lie=lie, returnAllCosts=True)
    self_consistent(idx, costs, allc)
    assert np.array_equal(allc[0], cf.evaluateBatch(C))                      # row 0: today's one-pick call, bit for bit
    lv = lie if lie == "believer" or not isinstance(lie, str) else float(getattr(np, lie)(y))
    free = None
    if acq != bc.PI:        # PI saturates to ties on these inputs: the forced comparison only
        free, rows, _ = aref.refit_path(spec, X, S, y, noise, C, acq, rule, lv, q)
        print("%s %s %s: device picks %s   refit-loop picks %s" % (cid, acqname, lie, idx.tolist(), free))
        assert idx.tolist() == free
    else:
        _, rows, _ = aref.refit_path(spec, X, S, y, noise, C, acq, rule, lv, q, forced=idx)
    errs = [bb.row_err(allc[t], rows[t]) for t in range(q)]
    print("%s %s %s: worst row error against the refit loop at the device's picks %.3e" % (cid, acqname, lie, max(errs)))
    assert max(errs) <= 1e-9, errs
    return cf, C, idx, costs, allc


@pytest.mark.parametrize("cid", ["se-d3", "m32-d2", "m52-d8"])
@pytest.mark.parametrize("acqname", ACQS)
@pytest.mark.parametrize("lie", ["believer", "min", "max"])
def test_batch_against_the_refit_loop(cid, acqname, lie):
    check_batch(cid, acqname, lie, 8)


@pytest.mark.parametrize("acqname,lie", [("ei", "believer"), ("ucb", "min")])
def test_batch_at_the_blocked_size(acqname, lie):
    check_batch("blocked-m52-d8-nu1152", acqname, lie, 4)


def test_batch_lie_semantics():
    """Constant liar with a number, the believed values, and a given fBest= (the caller's constant: no tracking)."""
    cid = "m52-d8"
    spec, X, S, y, noise = problem(cid)[:5]
    C = np.array(batch_candidates(cid))
    dev, ctx, model, coeff = device_model(cid)
    Cd = dev.points(ctx, C)
    idx, costs, lies = model.acq_batch(coeff, Cd, dev.ACQ_EI, float(np.max(y)), True, dev.LIE_BELIEVER, 0.0, 8)
    _, _, want = aref.refit_path(spec, X, S, y, noise, C, bc.EI, "best", "believer", 8, forced=idx)
    assert np.max(np.abs(lies - want) / np.maximum(1.0, np.abs(want))) <= 1e-9
    idx2, costs2, lies2, allc2 = model.acq_batch(coeff, Cd, dev.ACQ_EI, float(np.max(y)), True, dev.LIE_CONSTANT, 0.3, 8, want_all=True)
    assert np.array_equal(lies2, np.full(8, 0.3))
    self_consistent(idx2, costs2, allc2)
    check_batch(cid, "ei", 0.3, 8)
    fb = float(np.median(y))
    cf, _, idx3, costs3, allc3 = check_batch(cid, "ei", "max", 8, fBest=fb)
    _, tracked, _ = aref.refit_path(spec, X, S, y, noise, C, bc.EI, "best", float(np.max(y)), 8, forced=idx3)
    assert bb.row_err(allc3[1], tracked[1]) > 1e-6          # (the tracked rule is a different cost: the check discriminates)


def test_batch_errors_and_fallback(monkeypatch):
    from gpexp_amd import device as dev
    from gpexp_amd._lib import GpxError
    cf, C, idx, costs, allc = check_batch("se-d3", "ei", "believer", 8)
    with pytest.raises(ValueError):
        cf.selectBatch(C[:5], 6)
    with pytest.raises(GpxError):
        cf.selectBatch(C, 0)
    nan = make_cost("se-d3", "ei", fBest=float("nan"))
    with pytest.raises(GpxError, match=r"pick 1\b"):
        nan.selectBatch(C, 4)
    # the refit fallback (resident state "does not fit"): per pick a VFE model on the grown data with the same inducing points
    ctx = dev.context()
    monkeypatch.setattr(ctx, "_hbm_bytes", 1024.0, raising=False)
    idx2, costs2, allc2 = cf.selectBatch(C, 8, returnAllCosts=True)
    assert idx2.tolist() == idx.tolist()
    assert max(bb.row_err(allc2[t], allc[t]) for t in range(8)) <= 1e-9
    assert np.array_equal(allc2[0], allc[0])


# ---- 5. class API ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_class_api(cid):
    from gpExp.experimentalDesign import optimizeAcquisition
    spec, X, S, y, noise = problem(cid)[:5]
    d = spec["d"]
    C = np.array(batch_candidates(cid))
    for acqname in ACQS:
        cf = make_cost(cid, acqname)
        coeff = cf.gaussianProcess.coeff.copy()
        c = cf.evaluateBatch(C)
        assert isinstance(c, np.ndarray) and c.shape == (400,) and c.dtype == np.float64
        j, cj = cf.bestCandidate(C)
        assert isinstance(j, int) and isinstance(cj, float) and cj == c[j]
        cc, G = cf.evaluateBatchWithDerivative(C[:7])
        assert cc.shape == (7,) and G.shape == (7, d) and np.array_equal(cf.derivativeBatch(C[:7]), G)
        assert cf.derivative(C[:3]).shape == (d,) and np.max(np.abs(cf.derivative(C[:3]) - G[2])) <= 1e-10 * np.max(np.abs(G))
        out = cf.selectBatch(C, 3, lie="mean")
        assert len(out) == 2 and out[0].dtype == np.int64 and out[0].shape == (3,) and out[1].shape == (3,)
        assert cf.selectBatch(C, 3, lie="mean", returnAllCosts=True)[2].shape == (3, 400)
        p1 = optimizeAcquisition(cf, C, nStarts=4, maxiter=10)
        p2 = optimizeAcquisition(cf, C, nStarts=4, maxiter=10)
        assert p1[0].shape == (1, d) and p1[1] <= cj and p1[2] == j
        assert np.all(p1[0] >= C.min(axis=0)) and np.all(p1[0] <= C.max(axis=0))
        assert np.array_equal(p1[0], p2[0]) and p1[1] == p2[1] and p1[2] == p2[2]
        # the cost's GP copy and the caller's GP are unmodified
        assert np.array_equal(cf.gaussianProcess.coeff, coeff) and np.array_equal(cf.evaluateBatch(C), c)
        assert np.array_equal(cf.gaussianProcess.fitcnodes, S) and cf.gaussianProcess.pts.shape == X.shape
        assert cf.callersGP._fitc is None and cf.callersGP.coeff is None and np.array_equal(cf.callersGP.fitcnodes, S)
    # the same calls on a FITC model still raise
    np.random.seed(3)
    fitc = make_cost(cid, "ei", sparse=None)
    assert np.isfinite(fitc.evaluate(C[:1]))
    for call in (fitc.evaluateBatch, fitc.bestCandidate, fitc.evaluateBatchWithDerivative, fitc.derivativeBatch, fitc.derivative,
                 lambda z: optimizeAcquisition(fitc, z), lambda z: fitc.selectBatch(z, 2)):
        with pytest.raises(NotImplementedError):
            call(C)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    dev, ctx, model, coeff = device_model("se-d3")
    fitc = device_model("se-d3", "FitcModel")[2]
    Zd = dev.points(ctx, np.array(problem("se-d3")[5][:7]))
    for call in (lambda m, co: dev.VfeModel.acq(m, co, Zd, dev.ACQ_EI, 0.5), lambda m, co: dev.VfeModel.acq_grad(m, co, Zd, dev.ACQ_EI, 0.5),
                 lambda m, co: dev.VfeModel.acq_batch(m, co, Zd, dev.ACQ_EI, 0.5, True, dev.LIE_BELIEVER, 0.0, 2)):
        with pytest.raises(dev.GpxError, match="VFE models only"):
            call(fitc, coeff)
        with pytest.raises(dev.GpxError, match="NULL"):
            call(model, None)
        call(model, coeff)
    with pytest.raises(dev.GpxError, match="acq must be"):
        model.acq(coeff, Zd, 7, 0.5)
    with pytest.raises(dev.GpxError, match="lie must be"):
        model.acq_batch(coeff, Zd, dev.ACQ_EI, 0.5, True, 5, 0.0, 2)
    with pytest.raises(dev.GpxError, match="more picks"):
        model.acq_batch(coeff, Zd, dev.ACQ_EI, 0.5, True, dev.LIE_BELIEVER, 0.0, 8)
    with pytest.raises(dev.GpxError, match="do not match"):
        model.acq(coeff, dev.points(ctx, np.zeros((4, 2))), dev.ACQ_EI, 0.5)


# ---- 7. determinism and memory discipline --------------------------------------------------------------------------------------
def digest(cids=("se-d8", "m32-d8-nu257")):
    from gpexp_amd import device as dev
    h = hashlib.sha256()
    for cid in cids:
        y, Z = problem(cid)[3], problem(cid)[5]
        dev, ctx, model, coeff = device_model(cid)
        Zd = dev.points(ctx, Z)
        p = float(np.max(y))
        out = model.acq(coeff, Zd, dev.ACQ_EI, p)
        out = (np.array(out[:2]), out[2]) + model.acq_grad(coeff, Zd, dev.ACQ_PI, p) + \
            model.acq_batch(coeff, Zd, dev.ACQ_EI, p, True, dev.LIE_BELIEVER, 0.0, 6, want_all=True)
        for a in out:
            h.update(np.ascontiguousarray(a).tobytes())
    ctx = dev.context()
    ctx.sync()
    return "%s %d" % (h.hexdigest(), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    assert digest().split()[0] == digest().split()[0]


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled, so the padding of every work matrix and vector holds NaN unless the call wrote it): the same bits, no violation."""
    here = digest().split()[0]
    bits, violations = run_child("print('RESULT ' + t.digest(), flush=True)", {"GPX_CHAOS": "7", "GPX_ALLOC_GUARD": "2"}).split()
    assert violations == "0"
    assert bits == here


@pytest.mark.parametrize("cid", ["se-d3", "oop-m52-d8-nu2049"])
def test_outstanding_bytes_return_to_their_value(cid):
    """gpx_dbg_pool_stats' outstanding bytes, in pool keys, are exactly where they were after each of the three entries, run twice
    (the second time every block comes from the pool), and after a call that fails AFTER its resident state was allocated: a batch
    whose every cost is NaN (fBest = NaN) gives up at pick 1.  The explicit block inverses of chol(Quu) and chol(A) are the model's,
    built on its first solve: one predictor call comes first."""
    y, Z = problem(cid)[3], problem(cid)[5]
    dev, ctx, model, coeff = device_model(cid)
    Zd = dev.points(ctx, Z)
    p = float(np.max(y))
    model.posterior(coeff, Zd)
    calls = dict(acq=lambda: model.acq(coeff, Zd, dev.ACQ_EI, p), acq_grad=lambda: model.acq_grad(coeff, Zd, dev.ACQ_EI, p),
                 acq_batch=lambda: model.acq_batch(coeff, Zd, dev.ACQ_EI, p, True, dev.LIE_BELIEVER, 0.0, 5, want_all=True))
    for name, call in calls.items():
        for rep in range(2):
            before = ctx.pool_stats()[1]
            call()
            after = ctx.pool_stats()[1]
            print("%s %s, call %d: outstanding %d -> %d bytes" % (cid, name, rep, before, after))
            assert after == before, (name, rep, after - before)
    before = ctx.pool_stats()[1]
    with pytest.raises(dev.GpxError, match=r"pick 1\b"):
        model.acq_batch(coeff, Zd, dev.ACQ_EI, float("nan"), True, dev.LIE_BELIEVER, 0.0, 5)
    assert ctx.pool_stats()[1] == before
    assert np.all(np.isfinite(calls["acq_batch"]()[1]))
