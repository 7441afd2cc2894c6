"""Hyper-parameter gradient of the FITC marginal likelihood on the device (gpx_fitc_lml_grad, FitcModel.lml_grad,
GP.loglikeParams(returnDeriv=1) and findOptParamsLogLike(analyticGradient=True) on FITC models) against the NumPy restatement of
tests/fitc_grad_ref.py, which tests/test_fitc_grad_host.py ties to central differences of the oracle (<= 1e-6) and to a dense
N x N evaluation (<= 1e-9; seen <= 4e-13).

Tolerances: the value at 1e-10 relative, every gradient entry at 1e-8 relative to that entry -- what tests/test_gpu_fitc.py
holds FITC quantities to against Cholesky-accurate NumPy.  The two CPU forms agree to 1e-12 on these inputs, so the margin is
the device's.  The entry point has no size gate of its own (every product goes through launch_gemm); the `blocked` case is there
for the gates of the solves it calls: chol(Quu) and chol(A) of order 1152 cross the 1024-order block inverses."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as ref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
CASES["blocked-m52-d8-nu1152"] = ref.BLOCKED


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, y, noise, value, gradient): computed once per case, shared, never modified."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    value, grad = ref.fitc_value_grad(spec, X, S, y, noise)
    for a in (X, S, y, grad):
        a.setflags(write=False)
    return spec, X, S, y, noise, value, grad


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
def test_value_and_gradient_match_the_numpy_form(cid):
    value, grad = problem(cid)[5:]
    dev, ctx, ks, model = device_model(cid)
    y = problem(cid)[3]
    lp, g = model.lml_grad(ks, y)
    quad = model.solve(y)[1]
    errs = dict(value=abs(lp - value) / abs(value), grad=entry_relerr(g, grad))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert g.shape == grad.shape
    # as gpx_fitc_solve + gpx_fitc_logdet give it: the same quad and log det, three terms added on the host (a few ulps of the largest)
    two_calls = -0.5 * quad - 0.5 * model.logdet() - len(y) / 2.0 * np.log(2.0 * np.pi)
    assert abs(lp - two_calls) <= 1e-13 * abs(two_calls)
    assert errs["value"] <= 1e-10, errs
    assert errs["grad"] <= 1e-8, (errs, g, grad)


# ---- 2. class API ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_loglike_params_returns_the_gradient_on_a_fitc_model(cid):
    from gpexp_amd import device as dev
    spec, X, _, y, noise = problem(cid)[:5]
    X, y = np.array(X), np.array(y)
    Z = np.random.default_rng(5).uniform(-1.0, 1.0, (30, spec["d"]))
    np.random.seed(21)
    gp = make_gp(spec, noise, FITC=0.5)
    v0 = gp.loglikeParams(X, y)
    nodes = gp.fitcnodes.copy()
    assert nodes.shape == (len(X) // 2, spec["d"])
    v1, derivs = gp.loglikeParams(X, y, returnDeriv=1)
    assert v1 == v0
    assert list(derivs.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise"]
    assert np.array_equal(gp.fitcnodes, nodes)
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, nodes), noise)
    lp, g = model.lml_grad(ks, y)
    got = np.array(list(derivs.values()))
    assert abs(lp - v0) <= 1e-13 * abs(v0)
    assert np.array_equal(got[:-1], g[:-1]) and got[-1] == g[-1] * 2.0 * noise
    # ... and against the NumPy form with these inducing points
    rv, rg = ref.fitc_value_grad(spec, X, nodes, y, noise)
    assert abs(v0 - rv) <= 1e-10 * abs(rv) and entry_relerr(g, rg) <= 1e-8
    # the trained state: the same with and without the call in between
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
        lp, g = model.lml_grad(ks, problem(cid)[3])
        out.append(np.concatenate([[lp], g]).tobytes().hex())
    ctx.sync()
    return "%s %d" % ("".join(out), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    a, b = digest().split()[0], digest().split()[0]
    assert a == b


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled, so the padding of R, T and of every vector holds NaN unless the call wrote it): the same bits, no violation."""
    here = digest().split()[0]
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_fitc_grad as t\nprint('RESULT ' + t.digest(), flush=True)" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPX_CHAOS="7", GPX_ALLOC_GUARD="2"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    bits, violations = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:].split()
    assert violations == "0"
    assert bits == here


# ---- 4. optimiser ----------------------------------------------------------------------------------------------------------------
def test_hyper_parameter_search_with_the_analytic_gradient():
    spec, X, _, y, _ = problem("m52-d8")[:5]
    X, y = np.array(X), np.array(y)
    np.random.seed(22)
    gp = make_gp(spec, 1e-5, FITC=0.5)     # the driver starts the noise variance at 1e-5
    start = -gp.loglikeParams(X, y)
    nodes = gp.fitcnodes.copy()
    params, val = gp.findOptParamsLogLike(X, y, maxiter=15, analyticGradient=True)
    assert set(params) == {"rho", "signalSize", "noise"}
    assert np.array_equal(gp.fitcnodes, nodes)
    here = -gp.loglikeParams(X, y)
    print("FITC lml (analytic gradient): start %.6f -> %.6f at %s" % (start, val, params))
    assert abs(val - here) <= 1e-12 * abs(here)
    assert val <= start


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------
def test_mehler_has_no_gradient():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpexp_amd import device as dev
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (150, 2))
    y = np.sin(X.sum(1))
    np.random.seed(23)
    gp = GP(KernelMehlerND([0.5, 0.3], 2), 0.05, FITC=0.5)
    assert np.isfinite(gp.loglikeParams(X, y))
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        gp.loglikeParams(X, y, returnDeriv=1)
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, gp.fitcnodes), 0.05)
    with pytest.raises(dev.GpxError, match="Mehler"):
        model.lml_grad(ks, y)


def test_mismatched_arguments_are_refused():
    dev, ctx, ks, model = device_model("se-d3")
    spec, X, S, y = problem("se-d3")[:4]
    good = model.lml_grad(ks, y)[1]
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.lml_grad(dev.KernelSpec(dev.K_SE, 2, [0.3, 0.45, 1.7]), y)
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.lml_grad(dev.KernelSpec(dev.K_SE, 3, [0.3, 0.45, 0.7, 1.7]), y)
    with pytest.raises(dev.GpxError, match="fitted with"):
        model.lml_grad(dev.KernelSpec(dev.K_MATERN52, 3, [0.3, 1.7]), y)
    for attr, other in (("S", S[:100]), ("X", X[:200])):   # point sets that are not the model's
        keep = getattr(model, attr)
        try:
            setattr(model, attr, dev.points(ctx, other))
            with pytest.raises(dev.GpxError, match="inducing points of the model"):
                model.lml_grad(ks, y)
        finally:
            setattr(model, attr, keep)
    assert np.array_equal(model.lml_grad(ks, y)[1], good)
    assert model.lml_grad(ks, y, want_value=False)[0] is None
    assert np.array_equal(model.lml_grad(ks, y, want_value=False)[1], good)
