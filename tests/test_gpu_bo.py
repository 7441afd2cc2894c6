"""Bayesian-optimisation costs on the MI355X (gpx_acq / gpx_acq_grad behind costFuncGPUCbound / costFuncPI / costFuncEI,
experimentalDesign.py:889-1003): the reference's one-point `evaluate` against its own outputs, the batched values, the device
arg-min, the candidate gradients and the L-BFGS-B driver."""
import json
import os
import warnings

import numpy as np
import pytest

import bo_compose as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gpexp_golden_bo")


class Space(object):
    def __init__(self, d):
        self.dimension = d


def kernel_of(spec):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    if spec["kind"] == "se":
        return KernelSquaredExponential(spec["cl"], spec["signalSize"], spec["d"])
    return KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)


def make_cost(acq, spec, X, y, noise, param=None, **kw):
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    gp = GP(kernel_of(spec), noise, **kw)
    d = spec["d"]
    if acq == bc.UCB:
        return costFuncGPUCbound(gp, param, X, y, 2, Space(d))
    if acq == bc.PI:
        return costFuncPI(gp, X, y, 2, Space(d))
    if param is None:
        return costFuncEI(gp, X, y, 2, Space(d))
    return costFuncEI(gp, X, y, 2, Space(d), fBest=param)


def problem(spec, n, seed, noise=1e-3):
    rng = np.random.default_rng(seed)
    d = spec["d"]
    X = rng.uniform(-1, 1, (n, d))
    y = np.sin(3.0 * X[:, 0]) + 0.5 * np.cos(2.0 * X.sum(1)) + 0.05 * rng.standard_normal(n)
    return X, y, rng


def vrel(a, b):
    """max |a - b| relative to the largest |b| of the vector."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


SPECS = {
    "se_iso": lambda d: dict(kind="se", cl=[0.5], signalSize=1.4, d=d),
    "se_ard": lambda d: dict(kind="se", cl=list(0.5 + 0.15 * np.arange(d)), signalSize=0.8, d=d),
    "matern32": lambda d: dict(kind="matern32", rho=0.7, signalSize=1.3, d=d),
    "matern52": lambda d: dict(kind="matern52", rho=0.7, signalSize=0.6, d=d),
}
ACQS = [(bc.UCB, 2.0), (bc.PI, None), (bc.EI, None)]


def param_of(acq, param, y):
    return param if param is not None else float(np.max(y))


# ---- 1. the reference's evaluate, against the reference's own outputs ------------------------------------------------------------
def test_evaluate_matches_reference_fixture():
    arrs = np.load(GOLD + ".npz")
    with open(GOLD + ".json") as f:
        index = json.load(f)
    for case, ix in index.items():
        X, y, Q, junk = (arrs[case + "/" + k] for k in ("X", "y", "Q", "junk"))
        runs = [("ucb%d" % i, make_cost(bc.UCB, ix["kernel"], X, y, ix["noise"], k)) for i, k in enumerate(ix["kappas"])]
        runs += [("pi", make_cost(bc.PI, ix["kernel"], X, y, ix["noise"])),
                 ("ei", make_cost(bc.EI, ix["kernel"], X, y, ix["noise"])),
                 ("ei_fbest", make_cost(bc.EI, ix["kernel"], X, y, ix["noise"], ix["fBest"]))]
        for key, cf in runs:
            want = arrs["%s/%s" % (case, key)]
            with warnings.catch_warnings():
                warnings.simplefilter("error", DeprecationWarning)   # (the reference's float(array) raises one)
                got = [cf.evaluate(np.vstack((junk, Q[i:i + 1]))) for i in range(len(Q))]
            if key.startswith("ei"):
                assert all(type(v) is np.float64 for v in got), key
            else:
                assert all(type(v) is float for v in got), key
            err = np.abs(np.array(got) - want) / np.maximum(1.0, np.abs(want))
            assert np.max(err) < 1e-10, (case, key, float(np.max(err)))


def test_constructor_leaves_callers_gp_untouched():
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI
    spec = SPECS["se_ard"](2)
    X, y, rng = problem(spec, 40, 11)
    gp = GP(kernel_of(spec), 1e-3)
    gp.train(X[:20], y[:20])
    coeff, pts, L = gp.coeff, gp.pts, gp._L
    Q = rng.uniform(-1, 1, (16, 2))
    before = gp.evaluate(Q, compvar=1)
    cf = costFuncEI(gp, X, y, 2, Space(2))
    assert gp.coeff is coeff and gp.pts is pts and gp._L is L
    assert cf.gaussianProcess is not gp and cf.gaussianProcess.pts.shape == (40, 2)
    after = gp.evaluate(Q, compvar=1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- 2. evaluateBatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname,d", [("se_iso", 1), ("se_ard", 3), ("matern32", 2), ("matern52", 3)])
@pytest.mark.parametrize("acq,param", ACQS)
def test_evaluate_batch(kname, d, acq, param):
    from oracle import gpexp_oracle as orc
    spec = SPECS[kname](d)
    # cond(K) <= 1e4: where the reference's pinv and the Cholesky factor agree to 1e-10
    X, y, rng = problem(spec, 40 if d == 1 else 150, 21 + d)
    # candidates inside the training points' bounding box: a one-point call then centres the cross-covariance fill on the same
    # midpoint as the batch (gpx_kparams_sets), so the two agree to the last bits of the cost epilogue, not of the placement
    Q = rng.uniform(X.min(axis=0), X.max(axis=0), (300, d))
    Q[:5] = X[:5]
    cf = make_cost(acq, spec, X, y, 1e-2, param)
    p = param_of(acq, param, y)
    batch = cf.evaluateBatch(Q)
    assert batch.shape == (300,)
    per_point = np.array([cf.evaluate(Q[i:i + 1]) for i in range(len(Q))])
    assert vrel(batch, per_point) <= 1e-13
    model = orc.fit(spec, X, y, 1e-2)
    mean, var = orc.posterior(spec, model, Q)
    assert vrel(batch, bc.costs(acq, p, mean, var)) < 1e-10


# ---- 3. bestCandidate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq,param", ACQS)
def test_best_candidate(acq, param, monkeypatch):
    spec = SPECS["matern52"](2)
    X, y, rng = problem(spec, 200, 31)
    C = rng.uniform(-1, 1, (1000, 2))
    cf = make_cost(acq, spec, X, y, 1e-3, param)
    costs = cf.evaluateBatch(C)
    from gpexp_amd.experimentalDesign import firstMinIndex
    j, c = cf.bestCandidate(C)
    assert j == firstMinIndex(costs) and c == costs[j]
    # duplicates: the first copy wins
    C2 = np.vstack((C[:7], C[j:j + 1], C, C[j:j + 1]))
    j2, c2 = cf.bestCandidate(C2)
    assert j2 == min(j, 7) and c2 == c
    # chunked (>= 3 chunks of Z: 128 candidates each at N = 200) equals unchunked, bit for bit
    monkeypatch.setenv("GPX_CROSS_BYTES", str(256 * 8 * 128))
    jc, cc = cf.bestCandidate(C)
    costs_c = cf.evaluateBatch(C)
    assert (jc, cc) == (j, c)
    assert np.array_equal(costs_c, costs)


def test_best_candidate_nan_rule():
    """A cost that is NaN never wins; all-NaN gives -1 (EI with fBest = NaN)."""
    spec = SPECS["se_iso"](1)
    X, y, rng = problem(spec, 40, 41)
    cf = make_cost(bc.EI, spec, X, y, 1e-3, float("nan"))
    C = rng.uniform(-1, 1, (300, 1))
    assert np.all(np.isnan(cf.evaluateBatch(C)))
    j, c = cf.bestCandidate(C)
    assert j == -1 and np.isnan(c)


# ---- 4. derivativeBatch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", ["se_iso", "se_ard", "matern32", "matern52"])
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("acq,param", ACQS)
def test_derivative_batch(kname, d, acq, param):
    spec = SPECS[kname](d)
    X, y, rng = problem(spec, 10 if d == 1 else 120, 51 + d)   # (d = 1: sparse, so that s is not tiny everywhere)
    Z = rng.uniform(-1, 1, (24, d))
    Z[0] = X[3] + 1e-7          # next to a training point (Matern: smooth at r = 0)
    # around the best observation, where PI / EI with fBest = max(y) are not saturated (elsewhere Phi(g) = 1 to the last bit)
    Z[1:12] = X[np.argmax(y)] + 0.05 * rng.standard_normal((11, d))
    cf = make_cost(acq, spec, X, y, 1e-3, param)
    p = param_of(acq, param, y)
    G = cf.derivativeBatch(Z)
    assert G.shape == (24, d)
    # central differences of evaluateBatch, every perturbed point in ONE call
    h = 1e-5
    P = np.repeat(Z[:, None, :], 2 * d, axis=1)
    for l in range(d):
        P[:, 2 * l, l] += h
        P[:, 2 * l + 1, l] -= h
    c = cf.evaluateBatch(P.reshape(-1, d)).reshape(24, 2 * d)
    fd = (c[:, 0::2] - c[:, 1::2]) / (2 * h)
    assert np.max(np.abs(fd)) > 1e-3
    assert vrel(G, fd) < 1e-6, vrel(G, fd)
    model = bc.DenseModel(spec, X, y, 1e-3)
    assert vrel(G, model.grad(acq, p, Z)) < 1e-9
    assert np.max(np.abs(cf.derivative(np.vstack((X[:1], Z[5:6]))) - G[5])) <= 1e-10 * np.max(np.abs(G))


def test_derivative_mehler_raises():
    from gpExp.gp import GP
    from gpExp.kernels import KernelMehlerND
    from gpExp.experimentalDesign import costFuncPI
    from gpexp_amd._lib import GpxError
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, (40, 2))
    y = np.sin(X.sum(1))
    cf = costFuncPI(GP(KernelMehlerND([0.3, 0.5], 2), 1e-3), X, y, 2, Space(2))
    Z = rng.uniform(-1, 1, (5, 2))
    assert np.all(np.isfinite(cf.evaluateBatch(Z)))
    with pytest.raises(GpxError):
        cf.derivativeBatch(Z)


def test_fitc_batched_calls_raise():
    from gpExp.experimentalDesign import optimizeAcquisition
    spec = SPECS["se_ard"](2)
    X, y, rng = problem(spec, 60, 71)
    np.random.seed(3)
    cf = make_cost(bc.EI, spec, X, y, 1e-3, FITC=0.5)
    Z = rng.uniform(-1, 1, (5, 2))
    assert np.isfinite(cf.evaluate(Z))            # the reference's path: GP.evaluate on the FITC model
    for call in (cf.evaluateBatch, cf.bestCandidate, cf.derivativeBatch, cf.derivative,
                 lambda z: optimizeAcquisition(cf, z)):
        with pytest.raises(NotImplementedError):
            call(Z)


# ---- 5. full size ------------------------------------------------------------------------------------------------------------------
def test_full_size_matern52():
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI, firstMinIndex
    spec = SPECS["matern52"](8)
    spec["rho"] = 1.5
    X, y, rng = problem(spec, 8192, 81, noise=1e-2)
    Z = rng.uniform(-1, 1, (131072, 8))
    gp = GP(kernel_of(spec), 1e-2)
    cf = costFuncEI(gp, X, y, 2, Space(8))
    costs = cf.evaluateBatch(Z)
    mean, var = cf.gaussianProcess.evaluate(Z, compvar=1)
    want = bc.costs(bc.EI, float(np.max(y)), mean, var)
    err = np.abs(costs - want) / np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want)))
    assert np.max(err) < 1e-10, float(np.max(err))
    j, c = cf.bestCandidate(Z)
    assert j == firstMinIndex(costs) and c == costs[j]
    sample = np.sort(rng.choice(len(Z), 64, replace=False))
    G = cf.derivativeBatch(Z)
    model = bc.DenseModel(spec, X, y, 1e-2)
    assert vrel(G[sample], model.grad(bc.EI, float(np.max(y)), Z[sample])) < 1e-9


# ---- 6. optimizeAcquisition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq,param", ACQS)
def test_optimize_acquisition(acq, param):
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI, optimizeAcquisition
    spec = SPECS["se_ard"](2)
    X, y, rng = problem(spec, 50, 91)
    gp = GP(kernel_of(spec), 1e-3)
    gp.train(X[:10], y[:10])
    coeff, pts = gp.coeff, gp.pts
    if acq == bc.UCB:
        cf = costFuncGPUCbound(gp, param, X, y, 2, Space(2))
    elif acq == bc.PI:
        cf = costFuncPI(gp, X, y, 2, Space(2))
    else:
        cf = costFuncEI(gp, X, y, 2, Space(2))
    assert gp.coeff is coeff and gp.pts is pts
    C = rng.uniform(-1, 1, (2000, 2))
    lb, ub = np.array([-1.0, -0.8]), np.array([0.9, 1.0])
    pt, cost, idx = optimizeAcquisition(cf, C, nStarts=6, lbounds=lb, rbounds=ub, maxiter=40)
    inside = np.flatnonzero(np.all((C >= lb) & (C <= ub), axis=1))      # the discrete pass sees the candidates in the box
    jd, cd = cf.bestCandidate(C[inside])
    assert idx == inside[jd]
    assert pt.shape == (1, 2) and np.all(pt >= lb) and np.all(pt <= ub)
    assert np.isfinite(cost) and cost <= cd
    assert abs(cf.evaluateBatch(pt)[0] - cost) <= 1e-10 * max(1.0, abs(cost))
    pt2, cost2, idx2 = optimizeAcquisition(cf, C, nStarts=6, lbounds=lb, rbounds=ub, maxiter=40)
    assert np.array_equal(pt, pt2) and cost == cost2 and idx == idx2
