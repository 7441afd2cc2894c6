"""The VFE sparse objective on the device (gpx_vfe_fit / gpx_vfe_bound / gpx_vfe_grad / gpx_vfe_posterior, VfeModel and
GP(..., FITC=fraction, sparse="vfe")) against the NumPy restatement of tests/vfe_ref.py, which tests/test_vfe_host.py ties to
central differences, to a dense N x N evaluation and to the bound property.

Tolerances: the value at 1e-10 relative, every hyper-gradient entry at 1e-8 relative to that entry, dF/dS at 1e-8 of its largest
entry -- the figures tests/test_gpu_fitc_grad.py and tests/test_gpu_fitc_inducing.py hold FITC to; the predictor's mean and variance
within 1e-8 of the largest reference entry, tests/test_gpu_fitc.py's figure for FITC posteriors against Cholesky-accurate NumPy
(the variance's minimum on these cases is >= 2.4e-2 signalSize: the tolerance does not sit on a cancellation).

Shapes: the cases of fitc_grad_ref plus BLOCKED -- nu = 129 / N = 257 one past a 128 tile, nu = 40 below one tile, nu = 1152 where
Lu and La cross the 1024-order block inverses; M = 300 evaluation points (no multiple of 128, five of them training points) and
M = 1."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as ref
import vfe_ref as vref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
CASES["blocked-m52-d8-nu1152"] = ref.BLOCKED


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, y, noise, Z, value, gradient, dF/dS, mean, var): computed once per case, shared, never modified."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    Z = np.random.default_rng(31).uniform(-1.2, 1.2, (300, spec["d"]))
    Z[:5] = X[:5]
    value, grad = vref.value_grad(spec, X, S, y, noise)
    gs = vref.grad_S(spec, X, S, y, noise)
    mean, var = vref.predict(spec, X, S, y, noise, Z)
    for a in (X, S, y, Z, grad, gs, mean, var):
        a.setflags(write=False)
    return spec, X, S, y, noise, Z, value, grad, gs, mean, var


def kernel_spec(spec):
    from gpexp_amd import device as dev
    return dev.KernelSpec(ref.KIND_ID[spec["kind"]], spec["d"], ref.hyp_of(spec))


def device_model(cid, cls="VfeModel"):
    from gpexp_amd import device as dev
    spec, X, S, y, noise = problem(cid)[:5]
    ctx = dev.context()
    ks = kernel_spec(spec)
    return dev, ctx, ks, getattr(dev, cls)(ctx, ks, dev.points(ctx, X), dev.points(ctx, S), noise)


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


def max_relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. value and gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_value_and_gradients_match_the_numpy_form(cid):
    y, value, grad, gs_ref = problem(cid)[3], *problem(cid)[6:9]
    dev, ctx, ks, model = device_model(cid)
    bound = model.bound(y)
    lp, g = model.grad(ks, y)
    lp2, g2, gs = model.grad(ks, y, want_inducing=True)
    errs = dict(value=abs(bound - value) / abs(value), grad=entry_relerr(g, grad), grad_s=max_relerr(gs, gs_ref))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert g.shape == grad.shape and gs.shape == gs_ref.shape and np.all(np.isfinite(gs))
    assert lp == bound and lp2 == bound and np.array_equal(g2, g)      # gpx_vfe_bound's bits
    assert errs["value"] <= 1e-10, errs
    assert errs["grad"] <= 1e-8, (errs, g, grad)
    assert errs["grad_s"] <= 1e-8, errs
    # each output alone
    assert model.grad(ks, y, want_value=False)[0] is None and np.array_equal(model.grad(ks, y, want_value=False)[1], g)
    only_s = np.empty(gs.shape)
    yy = np.ascontiguousarray(y, dtype=float)
    dev.check(ctx.lib.gpx_vfe_grad(ctx.h, model.h, *ks.args(), model.X.h, model.S.h, dev.dptr(yy), None, None, dev.dptr(only_s)))
    assert np.array_equal(only_s, gs)
    with pytest.raises(dev.GpxError, match="at least one"):
        dev.check(ctx.lib.gpx_vfe_grad(ctx.h, model.h, *ks.args(), model.X.h, model.S.h, dev.dptr(yy), None, None, None))


# ---- 2. predictor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_predictor_matches_the_numpy_form(cid):
    y, Z, mean_ref, var_ref = problem(cid)[3], problem(cid)[5], *problem(cid)[9:11]
    dev, ctx, ks, model = device_model(cid)
    coeff = model.solve(y)[0]
    mean, var = model.posterior(coeff, dev.points(ctx, Z))
    errs = dict(mean=max_relerr(mean, mean_ref), var=max_relerr(var, var_ref))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()), "min var %.3e" % np.min(var))
    assert errs["mean"] <= 1e-8 and errs["var"] <= 1e-8, errs
    assert np.all(var > 0.0)
    # M = 1, and each output alone: the same bits
    m1, v1 = model.posterior(coeff, dev.points(ctx, Z[7:8]))
    assert abs(m1[0] - mean_ref[7]) <= 1e-8 * np.max(np.abs(mean_ref)) and abs(v1[0] - var_ref[7]) <= 1e-8 * np.max(np.abs(var_ref))
    assert v1[0] > 0.0
    assert np.array_equal(model.posterior(coeff, dev.points(ctx, Z), want_var=False)[0], mean)
    assert np.array_equal(model.posterior(None, dev.points(ctx, Z), want_mean=False)[1], var)


def predictor_digest(cid="m32-d8-nu257"):
    y, Z = problem(cid)[3], problem(cid)[5]
    dev, ctx, ks, model = device_model(cid)
    mean, var = model.posterior(model.solve(y)[0], dev.points(ctx, Z))
    return np.concatenate([mean, var]).tobytes().hex()


def test_chunked_predictor_returns_the_same_bits():
    """A child process whose GPX_CROSS_BYTES allows 128 evaluation points per chunk (nu = 257 pads to 384 rows): M = 300 runs as
    three chunks of 128, 128 and 44."""
    here = predictor_digest()
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe as t\nprint('RESULT ' + t.predictor_digest(), flush=True)" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPX_CROSS_BYTES=str(384 * 8 * 128)), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:] == here


# ---- 3. class API ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_class_api_on_a_vfe_model(cid):
    from gpexp_amd import device as dev
    spec, X, _, y, noise = problem(cid)[:5]
    X, y = np.array(X), np.array(y)
    Z = np.random.default_rng(5).uniform(-1.0, 1.0, (30, spec["d"]))
    np.random.seed(21)
    gp = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    v0 = gp.loglikeParams(X, y)
    nodes = gp.fitcnodes.copy()
    assert nodes.shape == (len(X) // 2, spec["d"])
    assert gp.computeLogLike(X, y) == v0
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.VfeModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, nodes), noise)
    lp, g, gs = model.grad(ks, y, want_inducing=True)
    assert v0 == model.bound(y) and lp == v0
    v1, d1 = gp.loglikeParams(X, y, returnDeriv=1)
    v2, d2 = gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    assert v1 == v0 and v2 == v0
    assert list(d1.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise"]
    assert list(d2.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise", "fitcnodes"]
    got = np.array(list(d1.values()))
    assert np.array_equal(got[:-1], g[:-1]) and got[-1] == g[-1] * 2.0 * noise
    assert all(np.array_equal(d2[k], d1[k]) for k in d1)
    assert d2["fitcnodes"].shape == nodes.shape and np.array_equal(d2["fitcnodes"], gs)
    assert np.array_equal(gp.fitcnodes, nodes)
    # ... and against the NumPy form with these inducing points
    rv, rg = vref.value_grad(spec, X, nodes, y, noise)
    assert abs(v0 - rv) <= 1e-10 * abs(rv) and entry_relerr(g, rg) <= 1e-8
    assert max_relerr(gs, vref.grad_S(spec, X, nodes, y, noise)) <= 1e-8
    # the trained state: the same with and without the likelihood calls in between; evaluate = the device predictor
    gp.train(X, y)
    m1, s1 = gp.evaluate(Z, compvar=1)
    gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    m2, s2 = gp.evaluate(Z, compvar=1)
    other = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    other.fitcnodes = nodes.copy()
    other.train(X, y)
    m0, s0 = other.evaluate(Z, compvar=1)
    assert np.array_equal(m1, m0) and np.array_equal(s1, s0) and np.array_equal(m2, m0) and np.array_equal(s2, s0)
    coeff = model.solve(y)[0]
    assert np.array_equal(gp.coeff, coeff)
    pm, pv = model.posterior(coeff, dev.points(ctx, Z))
    assert np.array_equal(m0, pm) and np.array_equal(s0, np.abs(pv))
    assert np.array_equal(gp.evaluate(Z), pm) and np.array_equal(gp.evaluateVariance(Z), pv)
    # the dense attributes: Q + noise I and its inverse
    cov, prec = gp.covarianceMatrix, gp.precisionMatrix
    Kuf = ref.kparts(spec, nodes, X)[0]
    Q = Kuf.T @ np.linalg.solve(ref.kparts(spec, nodes, nodes)[0] + noise * np.eye(len(nodes)), Kuf)
    assert max_relerr(cov, Q + noise * np.eye(len(X))) <= 1e-10
    assert max_relerr(prec @ cov, np.eye(len(X))) <= 1e-8


def test_vfe_differs_from_fitc_and_matches_its_reference():
    """The anchor: the same data and inducing points under sparse="vfe" and under FITC give different objectives and different
    predictive variances, and the VFE ones are vfe_ref's."""
    spec, X, S, y, noise, Z = problem("se-d3")[:6]
    X, y, Z = np.array(X), np.array(y), np.array(Z)
    vfe = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    fitc = make_gp(spec, noise, FITC=0.5)
    vfe.fitcnodes, fitc.fitcnodes = np.array(S), np.array(S)
    fv, ff = vfe.loglikeParams(X, y), fitc.loglikeParams(X, y)
    vfe.train(X, y)
    fitc.train(X, y)
    vv, vf = vfe.evaluateVariance(Z), fitc.evaluateVariance(Z)
    rv = problem("se-d3")[6]
    rm, rvar = problem("se-d3")[9:11]
    print("F %.6f  FITC likelihood %.6f;  max |var difference| %.3e" % (fv, ff, np.max(np.abs(vv - vf))))
    assert abs(fv - ff) > 1e-3 * abs(ff)
    assert np.max(np.abs(vv - vf)) > 1e-3 * np.max(np.abs(rvar))
    assert abs(fv - rv) <= 1e-10 * abs(rv)
    assert max_relerr(vv, rvar) <= 1e-8 and max_relerr(vfe.evaluate(Z), rm) <= 1e-8


def test_ivar_cost_and_a_one_point_bo_cost_work_through_the_predictor():
    from gpExp.approximation import Space
    from gpExp.experimentalDesign import costFunctionGP_IVAR, costFuncEI
    spec, X, S, y, noise, Z = problem("se-d3")[:6]
    X, y, Z = np.array(X), np.array(y), np.array(Z)
    d = spec["d"]
    rng = np.random.default_rng(2)
    space = Space(d, lambda size: rng.uniform(-1, 1, size), lambda p: np.ones(len(p)))
    gp = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    gp.fitcnodes = np.array(S)
    cf = costFunctionGP_IVAR(gp, len(X), space, mcPoints=Z)
    cost = cf.evaluate(X)
    assert abs(cost - np.mean(problem("se-d3")[10])) <= 1e-8 * np.max(np.abs(problem("se-d3")[10]))
    with pytest.raises(NotImplementedError, match="VFE"):
        cf.derivative(X)
    gp2 = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    gp2.fitcnodes = np.array(S)
    ei = costFuncEI(gp2, X, y, 2, space)
    assert np.isfinite(ei.evaluate(Z[10:11]))


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
def digest(cids=("se-d8", "m32-d8-nu257")):
    out = []
    for cid in cids:
        dev, ctx, ks, model = device_model(cid)
        y, Z = problem(cid)[3], problem(cid)[5]
        lp, g, gs = model.grad(ks, y, want_inducing=True)
        mean, var = model.posterior(model.solve(y)[0], dev.points(ctx, Z))
        out.append(np.concatenate([[lp, model.bound(y)], g, gs.ravel(), mean, var]).tobytes().hex())
    ctx.sync()
    return "%s %d" % ("".join(out), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    a, b = digest().split()[0], digest().split()[0]
    assert a == b


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled, so the padding of every work matrix and vector holds NaN unless the call wrote it): the same bits, no violation."""
    here = digest().split()[0]
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe as t\nprint('RESULT ' + t.digest(), flush=True)" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPX_CHAOS="7", GPX_ALLOC_GUARD="2"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    bits, violations = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:].split()
    assert violations == "0"
    assert bits == here


# ---- 5. optimiser ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inducing", [False, True], ids=["hyper", "hyper+inducing"])
def test_hyper_parameter_search_on_the_bound(inducing):
    spec, X, _, y, _ = problem("m52-d8")[:5]
    X, y = np.array(X), np.array(y)
    np.random.seed(22)
    gp = make_gp(spec, 1e-5, FITC=0.5, sparse="vfe")     # the driver starts the noise variance at 1e-5
    start = -gp.loglikeParams(X, y)
    nodes = gp.fitcnodes.copy()
    params, val = gp.findOptParamsLogLike(X, y, maxiter=15, analyticGradient=True, optimizeInducing=inducing)
    assert set(params) == {"rho", "signalSize", "noise"}
    here = -gp.loglikeParams(X, y)
    print("-F (analytic gradient%s): start %.6f -> %.6f at %s" % (", inducing points too" if inducing else "", start, val, params))
    assert abs(val - here) <= 1e-12 * abs(here)
    assert val <= start
    assert gp.fitcnodes.shape == nodes.shape
    assert np.all(gp.fitcnodes >= X.min(axis=0)) and np.all(gp.fitcnodes <= X.max(axis=0))
    if not inducing:
        assert np.array_equal(gp.fitcnodes, nodes)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_each_model_kind_is_refused_by_the_other_kinds_entries():
    dev, ctx, ks, vfe = device_model("se-d3")
    fitc = device_model("se-d3", "FitcModel")[3]
    spec, X, S, y, noise, Z = problem("se-d3")[:6]
    Zd = dev.points(ctx, Z[:7])
    coeff = vfe.solve(y)[0]
    for call, name in ((lambda: vfe.lml_grad(ks, y), "gpx_vfe_grad"), (lambda: vfe.lml_grad(ks, y, want_inducing=True), "gpx_vfe_grad"),
                       (lambda: vfe.loo(y), "gpx_vfe_"), (lambda: vfe.loo_grad(ks, y), "gpx_vfe_"),
                       (lambda: dev.FitcModel.posterior(vfe, coeff, Zd), "gpx_vfe_posterior"), (lambda: vfe.var_grad(ks, Zd), "gpx_vfe_posterior"),
                       (lambda: vfe.var_grad_newpt(ks, Zd), "gpx_vfe_posterior")):
        with pytest.raises(dev.GpxError, match=name):
            call()
    # the gpx_vfe_* entries on a FITC model (VfeModel's methods on the FITC handle)
    for call, name in ((lambda: dev.VfeModel.bound(fitc, y), "gpx_fitc_solve"), (lambda: dev.VfeModel.grad(fitc, ks, y), "gpx_fitc_lml_grad"),
                       (lambda: dev.VfeModel.posterior(fitc, coeff, Zd), "gpx_fitc_posterior")):
        with pytest.raises(dev.GpxError, match=name):
            call()
    with pytest.raises(dev.GpxError, match="noise"):
        dev.VfeModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, S), 0.0)
    # what works on both as it is
    assert np.isfinite(vfe.logdet()) and np.isfinite(fitc.logdet())
    assert np.array_equal(fitc.lml_grad(ks, y)[1], device_model("se-d3", "FitcModel")[3].lml_grad(ks, y)[1])


def test_unsupported_methods_on_a_vfe_model_raise():
    spec, X, S, y, noise, Z = problem("se-d3")[:6]
    X, y, Z = np.array(X), np.array(y), np.array(Z[:9])
    gp = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    gp.fitcnodes = np.array(S)
    gp.train(X, y)
    coeff = gp.coeff.copy()
    for call in (lambda: gp.evaluate(Z, compvar=2), lambda: gp.evaluateVarianceDerivative(Z), lambda: gp.evaluateVarianceDerivWRTnewpt(Z),
                 lambda: gp.varianceGradient(Z), lambda: gp.varianceGradientWRTnewpt(Z), lambda: gp.fitcLooPredict(X, y),
                 lambda: gp.fitcLooLogLike(X, y), lambda: gp.findOptParamsLogLike(X, y, objective="loo"),
                 lambda: gp.loglikeParams(X, y, noiseIn=np.full(len(X), noise))):
        with pytest.raises(NotImplementedError, match="VFE"):
            call()
    # per-point noise in train: the FITC branch's behaviour, the trained state left alone
    gp.addNodesAndComputeCovariance(X, noiseIn=np.full(len(X), noise))
    assert np.array_equal(gp.coeff, coeff) and np.all(np.isfinite(gp.evaluate(Z)))


def test_mehler_fits_and_predicts_and_has_no_gradient():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpexp_amd import device as dev
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (150, 2))
    y = np.sin(X.sum(1))
    np.random.seed(23)
    gp = GP(KernelMehlerND([0.5, 0.3], 2), 0.05, FITC=0.5, sparse="vfe")
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        gp.loglikeParams(X, y, returnDeriv=1)
    assert gp.fitcnodes is None
    assert np.isfinite(gp.loglikeParams(X, y))
    gp.train(X, y)
    mean, var = gp.evaluate(X[:20], compvar=1)
    assert np.all(np.isfinite(mean)) and np.all(var >= 0.0) and np.max(np.abs(mean - y[:20])) < 0.5
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.VfeModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, gp.fitcnodes), 0.05)
    with pytest.raises(dev.GpxError, match="Mehler"):
        model.grad(ks, y)
