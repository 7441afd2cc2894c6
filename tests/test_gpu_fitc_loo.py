"""Leave-one-out cross-validation of FITC models on the device (gpx_fitc_loo, gpx_fitc_loo_grad, FitcModel.loo / loo_grad,
GP.fitcLooPredict / fitcLooLogLike and findOptParamsLogLike(objective="loo") on FITC models) against the NumPy restatement of
tests/fitc_loo_ref.py, which tests/test_fitc_loo_host.py ties to a dense N x N evaluation (gradient <= 1e-10 per entry; seen
<= 4e-13), to central differences and to the conditional with the point deleted.

Tolerances: the value at 1e-10 relative, the mean at 1e-8 of max|mean|, every variance and every gradient entry at 1e-8 relative
to that entry -- what tests/test_gpu_fitc.py and tests/test_gpu_fitc_grad.py hold FITC quantities to against Cholesky-accurate
NumPy.  The two CPU forms agree to 1.5e-10 at worst (BLOCKED, the mean), so the margin is the device's.  Per-entry relative errors
are meaningful: no gradient entry of these cases is below 1e-2 of the largest, and p_i g_i >= 0.08, so ginv - ssq does not
cancel.  The entries have no size gate of their own (every product goes through launch_gemm); the `blocked` case is there for the
gates of the solves they call: chol(Quu) and chol(A) of order 1152 cross the 1024-order block inverses."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as ref
import fitc_loo_ref as lref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
CASES["blocked-m52-d8-nu1152"] = ref.BLOCKED


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, y, noise, reference dict): computed once per case, shared, never modified."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    want = lref.loo(spec, X, S, y, noise)
    for a in (X, S, y, want["mean"], want["var"], want["grad"]):
        a.setflags(write=False)
    return spec, X, S, y, noise, want


def device_model(cid):
    from gpexp_amd import device as dev
    spec, X, S, y, noise = problem(cid)[:5]
    ctx = dev.context()
    ks = dev.KernelSpec(ref.KIND_ID[spec["kind"]], spec["d"], ref.hyp_of(spec))
    return dev, ctx, ks, dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, S), noise)


def make_gp(spec, noise, **kw):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    from gpExp.gp import GP
    if spec["kind"] == "se":
        k = KernelSquaredExponential(list(spec["cl"]), spec["signalSize"], spec["d"])
    else:
        k = KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)
    return GP(k, noise, **kw)


def entry_relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_predictions_value_and_gradient_match_the_numpy_form(cid):
    y, want = problem(cid)[3], problem(cid)[5]
    dev, ctx, ks, model = device_model(cid)
    mean, var, lp = model.loo(y)
    lp2, g = model.loo_grad(ks, y)
    errs = dict(value=abs(lp - want["value"]) / abs(want["value"]),
                mean=float(np.max(np.abs(mean - want["mean"])) / np.max(np.abs(want["mean"]))),
                var=entry_relerr(var, want["var"]), grad=entry_relerr(g, want["grad"]))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert mean.shape == var.shape == y.shape and g.shape == want["grad"].shape
    assert lp2 == lp                                        # the same bits from both entries
    assert model.loo(y, want_pred=False) == (None, None, lp)
    assert errs["value"] <= 1e-10, errs
    assert errs["mean"] <= 1e-8, errs
    assert errs["var"] <= 1e-8, errs
    assert errs["grad"] <= 1e-8, (errs, g, want["grad"])


def test_mehler_predicts_but_has_no_gradient():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpexp_amd import device as dev
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (150, 2))
    y = np.sin(X.sum(1))
    np.random.seed(23)
    gp = GP(KernelMehlerND([0.5, 0.3], 2), 0.05, FITC=0.5)
    mean, var = gp.fitcLooPredict(X, y)
    assert gp.fitcnodes.shape == (75, 2)
    assert mean.shape == var.shape == (150,) and np.all(np.isfinite(mean)) and np.all(var > 0.0)
    assert np.isfinite(gp.fitcLooLogLike(X, y))
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        gp.fitcLooLogLike(X, y, returnDeriv=1)
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, gp.fitcnodes), 0.05)
    m2, v2, lp = model.loo(y)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var) and lp == gp.fitcLooLogLike(X, y)
    # ... and the predictions are the conditional of N(0, Q + G) (dense, from the model's own matrices)
    cov = model.dense(prec=False)[0]
    for i in (0, 77, 149):
        keep = np.arange(150) != i
        sol = np.linalg.solve(cov[np.ix_(keep, keep)], np.column_stack([y[keep], cov[keep, i]]))
        assert abs(mean[i] - cov[keep, i] @ sol[:, 0]) <= 1e-8 * np.max(np.abs(mean))
        assert abs(var[i] - (cov[i, i] - cov[keep, i] @ sol[:, 1])) <= 1e-8 * var[i]
    with pytest.raises(dev.GpxError, match="Mehler"):
        model.loo_grad(ks, y)


# ---- 2. class API ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_class_api_equals_the_model_calls_and_leaves_the_trained_state_alone(cid):
    from gpexp_amd import device as dev
    spec, X, _, y, noise = problem(cid)[:5]
    X, y = np.array(X), np.array(y)
    Z = np.random.default_rng(5).uniform(-1.0, 1.0, (30, spec["d"]))
    np.random.seed(21)
    gp = make_gp(spec, noise, FITC=0.5)
    mean, var = gp.fitcLooPredict(X, y)
    nodes = gp.fitcnodes.copy()
    assert nodes.shape == (len(X) // 2, spec["d"])
    v0 = gp.fitcLooLogLike(X, y)
    v1, derivs = gp.fitcLooLogLike(X, y, returnDeriv=1)
    assert v1 == v0
    assert list(derivs.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise"]
    assert np.array_equal(gp.fitcnodes, nodes)
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, nodes), noise)
    m2, s2, lp = model.loo(y)
    lp2, g = model.loo_grad(ks, y)
    assert np.array_equal(mean, m2) and np.array_equal(var, s2) and v0 == lp and lp2 == lp
    assert np.array_equal(np.array(list(derivs.values())), g)       # 'noise' included: no 2 * noise
    # ... and against the NumPy form with these inducing points
    want = lref.loo(spec, X, nodes, y, noise)
    assert abs(v0 - want["value"]) <= 1e-10 * abs(want["value"]) and entry_relerr(g, want["grad"]) <= 1e-8
    # looPredict stays the dense call
    with pytest.raises(NotImplementedError):
        gp.looPredict(X, y)
    # the trained state: the same with and without the calls in between
    gp.train(X, y)
    m1, s1 = gp.evaluate(Z, compvar=1)
    other = make_gp(spec, noise, FITC=0.5)
    other.fitcnodes = nodes.copy()
    other.train(X, y)
    m0, s0 = other.evaluate(Z, compvar=1)
    assert np.array_equal(m1, m0) and np.array_equal(s1, s0) and np.array_equal(gp.fitcnodes, nodes)


# ---- 3. determinism --------------------------------------------------------------------------------------------------------------
def digest(cids=("se-d8", "m32-d8-nu257")):
    out = []
    for cid in cids:
        dev, ctx, ks, model = device_model(cid)
        y = problem(cid)[3]
        mean, var, lp = model.loo(y)
        lp2, g = model.loo_grad(ks, y)
        out.append(np.concatenate([mean, var, [lp, lp2], g]).tobytes().hex())
    ctx.sync()
    return "%s %d" % ("".join(out), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    a, b = digest().split()[0], digest().split()[0]
    assert a == b


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled, so the padding of every vector and work matrix holds NaN unless the call wrote it): the same bits, no violation."""
    here = digest().split()[0]
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_fitc_loo as t\nprint('RESULT ' + t.digest(), flush=True)" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPX_CHAOS="7", GPX_ALLOC_GUARD="2"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    bits, violations = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:].split()
    assert violations == "0"
    assert bits == here


# ---- 4. scratch --------------------------------------------------------------------------------------------------------------------
def small_model():
    """N = 300, nu = 64 (S the first 64 nodes), squared exponential in 3 dimensions."""
    from gpexp_amd import device as dev
    rng = np.random.default_rng(31)
    X = rng.uniform(-1.0, 1.0, (300, 3))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(300)
    ctx = dev.context()
    ks = dev.KernelSpec(dev.K_SE, 3, [0.3, 0.45, 0.6, 1.7])
    return ctx, ks, dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, X[:64].copy()), 0.1), y


@pytest.mark.parametrize("which", ["N300-nu64", "blocked"])
def test_every_block_of_scratch_goes_back_under_its_size(which):
    if which == "blocked":
        ctx, ks, model = device_model("blocked-m52-d8-nu1152")[1:]
        y = problem("blocked-m52-d8-nu1152")[3]
    else:
        ctx, ks, model, y = small_model()
    model.solve(y)    # the first solve against chol(A) caches its block inverses IN THE MODEL: resident state, not scratch
    for name, call in (("loo", lambda: model.loo(y)), ("loo_grad", lambda: model.loo_grad(ks, y))):
        for rep in range(2):
            before = ctx.pool_stats()[1]
            call()
            after = ctx.pool_stats()[1]
            print("%s call %d: outstanding %d -> %d bytes" % (name, rep, before, after))
            assert after == before, "%s call %d left %d bytes of pool keys outstanding" % (name, rep, after - before)


# ---- 5. optimiser ----------------------------------------------------------------------------------------------------------------
def test_hyper_parameter_search_on_the_leave_one_out_objective():
    spec, X, _, y, _ = problem("m52-d8")[:5]
    X, y = np.array(X), np.array(y)
    np.random.seed(22)
    gp = make_gp(spec, 1e-5, FITC=0.5)     # the driver starts the noise variance at 1e-5
    start = -gp.fitcLooLogLike(X, y)
    nodes = gp.fitcnodes.copy()
    params, val = gp.findOptParamsLogLike(X, y, maxiter=15, analyticGradient=True, objective="loo")
    assert set(params) == {"rho", "signalSize", "noise"}
    assert np.array_equal(gp.fitcnodes, nodes)
    here = -gp.fitcLooLogLike(X, y)
    print("FITC leave-one-out (analytic gradient): start %.6f -> %.6f at %s" % (start, val, params))
    assert abs(val - here) <= 1e-12 * abs(here)
    assert val <= start


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------
def test_mismatched_arguments_are_refused():
    dev, ctx, ks, model = device_model("se-d3")
    spec, X, S, y = problem("se-d3")[:4]
    lp, good = model.loo_grad(ks, y)
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.loo_grad(dev.KernelSpec(dev.K_SE, 2, [0.3, 0.45, 1.7]), y)
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.loo_grad(dev.KernelSpec(dev.K_SE, 3, [0.3, 0.45, 0.7, 1.7]), y)
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.loo_grad(dev.KernelSpec(dev.K_MATERN52, 3, [0.3, 1.7]), y)
    for attr, other in (("S", S[:100]), ("X", X[:200])):   # point sets that are not the model's
        keep = getattr(model, attr)
        try:
            setattr(model, attr, dev.points(ctx, other))
            with pytest.raises(dev.GpxError, match="inducing points of the model"):
                model.loo_grad(ks, y)
        finally:
            setattr(model, attr, keep)
    again = model.loo_grad(ks, y)
    assert again[0] == lp and np.array_equal(again[1], good)
