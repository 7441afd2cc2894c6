"""Leave-one-out cross-validation on the device (gpx_loo / gpx_loo_grad, GP.looPredict / looLogLike, objective="loo") against the
NumPy closed form of tests/loo_ref.py, which tests/test_loo_host.py ties to N actual refits (<= 4e-14) and to central differences.

Tolerance 1e-9 (helpers.rel: relative to the largest entry), what tests/test_gpu_f1.py holds gradients to: the closed form is
within 1e-13 of the refits at these condition numbers (<= 6e3), so the margin belongs to the device."""
import functools
import warnings

import numpy as np
import pytest

from helpers import rel
import loo_ref as ref

pytestmark = pytest.mark.gpu

# id -> (kind, d, n, noise, seed, per-point nugget).  150: ragged against the 128-wide tiles; 300 / SE d = 8: eight products, three
# row tiles; 127 / 128 / 129: the padding edge; 1, 2: the smallest; 1100: the blocked chol_trtri / potri recursion (9 tiles)
CASES = {
    "m52-d3-n150": ("m52", 3, 150, 0.05, 1, False),
    "m32-d1-n150": ("m32", 1, 150, 0.05, 2, False),
    "se-d8-n300": ("se", 8, 300, 1e-3, 3, False),
    "m52-n127": ("m52", 3, 127, 0.05, 6, False),
    "m52-n128": ("m52", 3, 128, 0.05, 7, False),
    "m52-n129": ("m52", 3, 129, 0.05, 8, False),
    "m52-n1": ("m52", 2, 1, 0.05, 5, False),
    "m52-n2": ("m52", 2, 2, 0.05, 9, False),
    "m52-d8-n1100": ("m52", 8, 1100, 0.05, 10, False),
    "per-point": ("m52", 3, 150, 0.02, 4, True),
}


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(hyp, X, nugget, y, closed-form mean, var, L_LOO, gradient): computed once per case, shared, never modified."""
    kind, d, n, noise, seed, pp = CASES[cid]
    hyp, X, nugget, y = ref.case(kind, d, n, noise, seed, pp)
    out = (hyp, X, nugget, y) + ref.loo_all(kind, d, hyp, X, nugget, y)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def make_gp(kind, d, hyp, nugget):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    from gpExp.gp import GP
    if kind == "se":
        k = KernelSquaredExponential(list(hyp[:d]), float(hyp[d]), d)
    else:
        k = KernelIsoMatern(float(hyp[0]), float(hyp[1]), d, nu=1.5 if kind == "m32" else 2.5)
    per_point = np.ndim(nugget) > 0
    return GP(k, 0.01 if per_point else float(nugget)), (np.array(nugget) if per_point else None)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_predictions_value_and_gradient_match_the_closed_form(cid):
    kind, d = CASES[cid][0], CASES[cid][1]
    hyp, X, nugget, y, m0, v0, l0, g0 = problem(cid)
    gp, noiseIn = make_gp(kind, d, hyp, nugget)
    mean, var = gp.looPredict(X, y, noiseIn=noiseIn)
    val = gp.looLogLike(X, y, noiseIn=noiseIn)
    val2, derivs = gp.looLogLike(X, y, returnDeriv=1, noiseIn=noiseIn)
    assert list(derivs.keys()) == list(gp.kernel.hyperParam.keys()) + ["noise"]
    g = np.array(list(derivs.values()))
    # the mean is y_i - alpha_i / p_i: its rounding error is relative to |y|, and at n = 1 the mean itself is 0 (the reference
    # holds 1e-16 there), so its error is measured against the larger of the two scales -- for n > 1 they are the same size
    mean_err = float(np.max(np.abs(mean - m0)) / max(np.max(np.abs(m0)), np.max(np.abs(y))))
    errs = dict(mean=mean_err, var=rel(var, v0), logp=abs(val - l0) / abs(l0), logp_grad_path=abs(val2 - l0) / abs(l0),
                grad=rel(g, g0))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert mean.shape == var.shape == y.shape
    assert max(errs.values()) <= 1e-9, errs


def test_single_point_is_the_prior():
    hyp, X, nugget, y = problem("m52-n1")[:4]
    gp, _ = make_gp("m52", 2, hyp, nugget)
    mean, var = gp.looPredict(X, y)
    assert abs(mean[0]) <= 1e-14 * abs(y[0]) and abs(var[0] - (hyp[1] + nugget)) <= 1e-14


def test_brute_force_through_the_library():
    """looPredict against N actual GP.train / evaluate(compvar=1) refits with one point left out (+ noise: the prediction is of
    the observation)."""
    kind, d, n, noise = "m52", 2, 40, 0.05
    hyp, X, nugget, y = ref.case(kind, d, n, noise, 11)
    gp, _ = make_gp(kind, d, hyp, nugget)
    mean, var = gp.looPredict(X, y)
    bm, bv = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        g, _ = make_gp(kind, d, hyp, nugget)
        g.train(X[keep], y[keep])
        m, v = g.evaluate(X[i:i + 1], compvar=1)
        bm[i], bv[i] = m[0], v[0] + noise
    errs = (rel(mean, bm), rel(var, bv))
    print("vs refits: mean %.2e var %.2e" % errs)
    assert max(errs) <= 1e-9


def _device_problem(cid):
    from gpexp_amd import device as dev
    kind, d = CASES[cid][0], CASES[cid][1]
    hyp, X, nugget, y = problem(cid)[:4]
    ctx = dev.context()
    spec = dev.KernelSpec({"se": dev.K_SE, "m32": dev.K_MATERN32, "m52": dev.K_MATERN52}[kind], d, hyp)
    Xd = dev.points(ctx, X)
    L = dev.potrf(ctx, dev.kfill(ctx, spec, Xd, nugget=nugget))
    return dev, ctx, spec, L, Xd, nugget, y


def test_row_slabs_are_independent():
    dev, ctx, spec, L, Xd, nugget, y = _device_problem("se-d8-n300")
    l0, g0 = dev.loo_grad(ctx, spec, L, Xd, nugget, y, slab_rows=0)
    l1, g1 = dev.loo_grad(ctx, spec, L, Xd, nugget, y, slab_rows=128)
    l2, g2 = dev.loo_grad(ctx, spec, L, Xd, nugget, y, slab_rows=256)
    print("slabs of 128 / 256 vs whole: %.2e %.2e" % (rel(g1, g0), rel(g2, g0)))
    assert l1 == l0 and rel(g1, g0) <= 1e-13 and rel(g2, g0) <= 1e-13
    with pytest.raises(dev.GpxError, match="slab_rows"):
        dev.loo_grad(ctx, spec, L, Xd, nugget, y, slab_rows=100)


@pytest.mark.parametrize("cid", ["se-d8-n300", "per-point"])
def test_two_calls_agree_bit_for_bit(cid):
    dev, ctx, spec, L, Xd, nugget, y = _device_problem(cid)
    a = dev.loo(ctx, L, y)
    b = dev.loo(ctx, L, y)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    la, ga = dev.loo_grad(ctx, spec, L, Xd, nugget, y)
    lb, gb = dev.loo_grad(ctx, spec, L, Xd, nugget, y)
    assert la == lb and np.array_equal(ga, gb)


def test_kept_factor_path_and_untouched_state():
    """Right after `train` on the same points (n >= 256: the fit keeps its factor) the calls reuse that factor; they equal the
    calls on a fresh GP, and neither `coeff` nor `pts` changes."""
    hyp, X, nugget, y = problem("se-d8-n300")[:4]
    fresh, _ = make_gp("se", 8, hyp, nugget)
    v0, d0 = fresh.looLogLike(X, y, returnDeriv=1)
    gp, _ = make_gp("se", 8, hyp, nugget)
    gp.train(X, y)
    assert gp._cached_factor(np.asarray(X), nugget, gp.kernel._spec()) is not None
    coeff, pts = gp.coeff.copy(), gp.pts.copy()
    v1, d1 = gp.looLogLike(X, y, returnDeriv=1)
    m1, s1 = gp.looPredict(X, y)
    assert abs(v1 - v0) <= 1e-13 * abs(v0)
    assert rel(list(d1.values()), list(d0.values())) <= 1e-13
    assert rel(m1, fresh.looPredict(X, y)[0]) <= 1e-13
    assert np.array_equal(gp.coeff, coeff) and np.array_equal(gp.pts, pts)
    # other points than the trained ones: still no change of the trained state
    gp.looPredict(X[:100], y[:100])
    assert np.array_equal(gp.coeff, coeff) and np.array_equal(gp.pts, pts)


def test_mehler_predicts_and_has_no_gradient():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpexp_amd._lib import GpxError
    rng = np.random.default_rng(12)
    n, t, noise = 150, [0.5, 0.3], 0.05
    X = rng.uniform(-1.0, 1.0, (n, 2))
    y = np.sin(X.sum(1)) + np.sqrt(noise) * rng.standard_normal(n)
    gp = GP(KernelMehlerND(t, 2), noise)
    mean, var = gp.looPredict(X, y)
    m0, v0, l0 = ref.loo_closed(ref.cov0_mehler(t, X) + noise * np.eye(n), y)
    errs = (rel(mean, m0), rel(var, v0), abs(gp.looLogLike(X, y) - l0) / abs(l0))
    print("mehler: mean %.2e var %.2e logp %.2e" % errs)
    assert max(errs) <= 1e-9
    with pytest.raises(GpxError, match="loo_grad"):
        gp.looLogLike(X, y, returnDeriv=1)


def test_fitc_is_refused():
    hyp, X, nugget, y = problem("m52-d3-n150")[:4]
    from gpExp.kernels import KernelIsoMatern
    from gpExp.gp import GP
    gp = GP(KernelIsoMatern(0.9, 1.3, 3, nu=2.5), 0.05, FITC=0.5)
    with pytest.raises(NotImplementedError):
        gp.looPredict(X, y)
    with pytest.raises(NotImplementedError):
        gp.looLogLike(X, y)


def test_dropped_points_are_refused():
    hyp, X, nugget, y = problem("m52-d3-n150")[:4]
    Xd = np.vstack([X, X[:1]])
    yd = np.concatenate([y, y[:1]])
    gp, _ = make_gp("m52", 3, hyp, 0.0)
    with pytest.warns(RuntimeWarning, match="dropped"):
        with pytest.raises(ValueError, match="dropped"):
            gp.looPredict(Xd, yd)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the policy warns once per GP object
        with pytest.raises(ValueError, match="dropped"):
            gp.looLogLike(Xd, yd, returnDeriv=1)


@pytest.mark.parametrize("analytic", [False, True])
def test_hyper_parameter_search_on_the_loo_objective(analytic):
    """Numerical gradients over the kernel parameters at a fixed noise; analytic gradients with the noise variance searched too
    (from the driver's start value 1e-5), which is where the LOO gradient's unscaled 'noise' entry matters."""
    kind, d, n, noise = "m52", 2, 200, 0.05
    hyp, X, nugget, y = ref.case(kind, d, n, noise, 13)
    gp, _ = make_gp(kind, d, [0.5, 1.0], 1e-5 if analytic else nugget)
    start = -gp.looLogLike(X, y)   # the search starts from the kernel's parameters and this noise
    params, val = gp.findOptParamsLogLike(X, y, useNoise=None if analytic else noise, maxiter=15, analyticGradient=analytic,
                                          objective="loo")
    assert set(params) == ({"rho", "signalSize", "noise"} if analytic else {"rho", "signalSize"})
    assert all(gp.kernel.hyperParam[k] == params[k] for k in ("rho", "signalSize"))
    assert not analytic or gp.noise == params["noise"]
    here = -gp.looLogLike(X, y)
    print("loo objective (analytic=%s): start %.6f -> %.6f at %s" % (analytic, start, val, params))
    assert abs(val - here) <= 1e-12 * abs(here)
    assert val <= start
    with pytest.raises(ValueError):
        gp.findOptParamsLogLike(X, y, objective="bogus")
