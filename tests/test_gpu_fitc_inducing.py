"""Gradient of the FITC marginal likelihood w.r.t. the inducing-point locations on the device (gpx_fitc_lml_grad_inducing,
FitcModel.lml_grad(want_inducing=True), GP.loglikeParams(inducingDeriv=True) and findOptParamsLogLike(optimizeInducing=True))
against the NumPy restatement of tests/fitc_inducing_ref.py, which tests/test_fitc_inducing_host.py ties to central differences
(<= 1e-5 of the largest entry; seen <= 2.1e-6) and to a dense N x N evaluation (<= 1e-10; seen <= 5.4e-12, 2.2e-10 on BLOCKED).

Tolerance: max|dev - ref| <= 1e-8 max|ref| -- what tests/test_gpu_fitc_grad.py holds FITC gradients to; the smallest entries of
dL/dS are ~1e-6 of the largest, so the error is taken against the largest entry of the reference matrix.  The two CPU forms agree
>= 45 times tighter, so the margin is the device's (seen on an MI355X: <= 1.2e-11 on the small cases, 6.3e-10 on BLOCKED).

Shapes.  The cases of fitc_grad_ref cover a ragged nu (129, 130, 257), a ragged N (257, 300, 385), nu below one row tile (40),
d = 1 and d = 8 and, with the rule of two column tiles per segment at these sizes, between one segment (the nu = 40 launch against
S) and 18 (BLOCKED against X), the last one ragged or single-tiled.  Beyond d = 8 the kernel walks a strip in several passes
(register arrays of 16 and of 32 coordinates): `se-d9` and `m52-d17` are the smallest cases that take those two paths."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as ref
import fitc_inducing_ref as iref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
CASES["blocked-m52-d8-nu1152"] = ref.BLOCKED
# (kind, d, lengths, signalSize, N, nu, noise, seed), as fitc_grad_ref.CASES
CASES["se-d9"] = ("se", 9, [1.0, 1.2, 0.8, 1.5, 0.9, 1.1, 1.3, 0.7, 1.4], 1.0, 150, 70, 0.05, 18)
CASES["m52-d17"] = ("matern52", 17, [2.5], 1.1, 150, 70, 0.05, 19)
# (case, where the inducing points are): perturbed off the training points everywhere; coincident pairs (S a subset of X) on the
# zero-distance Matern branch and on d = 8
PARITY = [(cid, "perturbed") for cid in CASES] + [("m32-d2", "subset"), ("se-d8", "subset")]


@functools.lru_cache(maxsize=None)
def problem(cid, where="perturbed"):
    """(spec, X, S, y, noise, dL/dS): computed once per case, shared, never modified."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    if where == "perturbed":
        S = iref.perturbed(S)
    gs = iref.grad_S(spec, X, S, y, noise)
    for a in (X, S, y, gs):
        a.setflags(write=False)
    return spec, X, S, y, noise, gs


def device_model(cid, where="perturbed"):
    from gpexp_amd import device as dev
    spec, X, S, y, noise = problem(cid, where)[:5]
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


def max_relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,where", PARITY, ids=["%s-%s" % p for p in PARITY])
def test_inducing_gradient_matches_the_numpy_form(cid, where):
    y, gs_ref = problem(cid, where)[3], problem(cid, where)[5]
    dev, ctx, ks, model = device_model(cid, where)
    lp0, g0 = model.lml_grad(ks, y)
    lp, g, gs = model.lml_grad(ks, y, want_inducing=True)
    err = max_relerr(gs, gs_ref)
    print("%s %s: dL/dS %.2e of max|ref| = %.3e" % (cid, where, err, np.max(np.abs(gs_ref))))
    assert gs.shape == gs_ref.shape and np.all(np.isfinite(gs))
    # the value and the hyper-parameter gradient of the same call: gpx_fitc_lml_grad's, bit for bit
    assert lp == lp0 and np.array_equal(g, g0)
    assert err <= 1e-8, err


# ---- 2. class API ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_loglike_params_returns_the_inducing_gradient(cid):
    from gpexp_amd import device as dev
    spec, X, _, y, noise = problem(cid)[:5]
    X, y = np.array(X), np.array(y)
    Z = np.random.default_rng(5).uniform(-1.0, 1.0, (30, spec["d"]))
    np.random.seed(21)
    gp = make_gp(spec, noise, FITC=0.5)
    v0, d0 = gp.loglikeParams(X, y, returnDeriv=1)
    nodes = gp.fitcnodes.copy()
    v1, d1 = gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    assert list(d1.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise", "fitcnodes"]
    assert list(d0.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise"]
    assert v1 == v0 and all(np.array_equal(d1[k], d0[k]) for k in d0)
    assert np.array_equal(gp.fitcnodes, nodes)
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, nodes), noise)
    gs = model.lml_grad(ks, y, want_inducing=True)[2]
    assert d1["fitcnodes"].shape == nodes.shape and np.array_equal(d1["fitcnodes"], gs)
    # ... and against the NumPy form with these inducing points (a subset of X: coincident pairs)
    assert max_relerr(gs, iref.grad_S(spec, X, nodes, y, noise)) <= 1e-8
    # the trained state: the same with and without the call in between
    gp.train(X, y)
    m1, s1 = gp.evaluate(Z, compvar=1)
    gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    m2, s2 = gp.evaluate(Z, compvar=1)
    other = make_gp(spec, noise, FITC=0.5)
    other.fitcnodes = nodes.copy()
    other.train(X, y)
    m0, s0 = other.evaluate(Z, compvar=1)
    assert np.array_equal(m1, m0) and np.array_equal(s1, s0) and np.array_equal(m2, m0) and np.array_equal(s2, s0)
    assert np.array_equal(gp.fitcnodes, nodes)
    with pytest.raises(ValueError, match="inducingDeriv"):
        gp.loglikeParams(X, y, returnDeriv=0, inducingDeriv=True)
    with pytest.raises(ValueError, match="inducingDeriv"):
        make_gp(spec, noise).loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)


# ---- 3. determinism --------------------------------------------------------------------------------------------------------------
def digest(cids=("se-d8", "m32-d8-nu257")):
    out = []
    for cid in cids:
        dev, ctx, ks, model = device_model(cid)
        lp, g, gs = model.lml_grad(ks, problem(cid)[3], want_inducing=True)
        out.append(np.concatenate([[lp], g, gs.ravel()]).tobytes().hex())
    ctx.sync()
    return "%s %d" % ("".join(out), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    a, b = digest().split()[0], digest().split()[0]
    assert a == b


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled, so the padding of R and T and the partial sums hold NaN unless the call wrote them): the same bits, no violation."""
    here = digest().split()[0]
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_fitc_inducing as t\nprint('RESULT ' + t.digest(), flush=True)" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPX_CHAOS="7", GPX_ALLOC_GUARD="2"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    bits, violations = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:].split()
    assert violations == "0"
    assert bits == here


# ---- 4. optimiser ----------------------------------------------------------------------------------------------------------------
def test_joint_search_over_hyper_parameters_and_inducing_points():
    spec, X, _, y, _ = problem("m52-d8")[:5]
    X, y = np.array(X), np.array(y)
    np.random.seed(22)
    gp = make_gp(spec, 1e-5, FITC=0.5)     # the driver starts the noise variance at 1e-5
    start = -gp.loglikeParams(X, y)
    nodes = gp.fitcnodes.copy()
    params, val = gp.findOptParamsLogLike(X, y, maxiter=15, optimizeInducing=True, analyticGradient=True)
    assert set(params) == {"rho", "signalSize", "noise"}
    here = -gp.loglikeParams(X, y)
    print("FITC lml (hyper-parameters + inducing points): start %.6f -> %.6f at %s; max move of a point %.3e"
          % (start, val, params, np.max(np.abs(gp.fitcnodes - nodes))))
    assert val <= start
    assert abs(val - here) <= 1e-12 * abs(val)
    assert gp.fitcnodes.shape == nodes.shape and not np.array_equal(gp.fitcnodes, nodes)
    assert np.all(gp.fitcnodes >= X.min(axis=0)) and np.all(gp.fitcnodes <= X.max(axis=0))
    # the same start without the keyword leaves the draw alone
    np.random.seed(22)
    other = make_gp(spec, 1e-5, FITC=0.5)
    other.findOptParamsLogLike(X, y, maxiter=15, optimizeInducing=False, analyticGradient=True)
    assert np.array_equal(other.fitcnodes, nodes)
    for kw in (dict(analyticGradient=False), dict(analyticGradient=True, objective="loo")):
        with pytest.raises(ValueError, match="optimizeInducing"):
            other.findOptParamsLogLike(X, y, maxiter=2, optimizeInducing=True, **kw)
    with pytest.raises(ValueError, match="optimizeInducing"):
        make_gp(spec, 1e-5).findOptParamsLogLike(X, y, maxiter=2, optimizeInducing=True, analyticGradient=True)


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
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    assert np.isfinite(gp.loglikeParams(X, y))
    ctx = dev.context()
    ks = gp.kernel._spec()
    model = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, gp.fitcnodes), 0.05)
    with pytest.raises(dev.GpxError, match="Mehler"):
        model.lml_grad(ks, y, want_inducing=True)


def test_mismatched_arguments_are_refused():
    dev, ctx, ks, model = device_model("se-d3")
    spec, X, S, y = problem("se-d3")[:4]
    good = model.lml_grad(ks, y, want_inducing=True)
    for bad in (dev.KernelSpec(dev.K_SE, 2, [0.3, 0.45, 1.7]), dev.KernelSpec(dev.K_SE, 3, [0.3, 0.45, 0.7, 1.7]),
                dev.KernelSpec(dev.K_MATERN52, 3, [0.3, 1.7])):
        with pytest.raises(dev.GpxError, match="fitted with"):
            model.lml_grad(bad, y, want_inducing=True)
    for attr, other in (("S", S[:100]), ("X", X[:200])):   # point sets that are not the model's
        keep = getattr(model, attr)
        try:
            setattr(model, attr, dev.points(ctx, other))
            with pytest.raises(dev.GpxError, match="inducing points of the model"):
                model.lml_grad(ks, y, want_inducing=True)
        finally:
            setattr(model, attr, keep)
    # grad_s is required; logp and grad are not
    yy = np.ascontiguousarray(y, dtype=float)
    gs = np.empty(S.shape)

    def call(lp, g, s):
        return ctx.lib.gpx_fitc_lml_grad_inducing(ctx.h, model.h, *ks.args(), model.X.h, model.S.h, dev.dptr(yy), lp, g, s)

    with pytest.raises(dev.GpxError, match="NULL"):
        dev.check(call(None, None, None))
    dev.check(call(None, None, dev.dptr(gs)))
    assert np.array_equal(gs, good[2])
    again = model.lml_grad(ks, y, want_value=False, want_inducing=True)
    assert again[0] is None and np.array_equal(again[1], good[1]) and np.array_equal(again[2], good[2])
