"""CPU-only checks of the VFE objective, gradients and predictor the device code implements (tests/vfe_ref.py), and of the ABI
addition and the constructor's validation.

Tolerances.  Central differences of the restatement's own value at relative step 1e-4: truncation ~ h^2 f''' / 6 ~ 1e-8 relative,
cancellation ~ eps cond |F| / (h theta) ~ 1e-8..1e-7 on these inputs (each case asserts cond(Quu) <= 1e4 as a condition of
validity) -- tests/test_fitc_grad_host.py's figure and reasoning: 1e-6 per entry, relative to the entry (seen 9e-9 .. 3.4e-7; every
entry of every case is >= 8e-3 of the largest, so the per-entry relative error is well defined).  dF/dS against central differences
(h = 1e-5): 1e-5 of the largest entry, as tests/test_fitc_inducing_host.py (its smallest entries are ~1e-5 of the largest).  The
nu x N value against the dense N x N form: 1e-10 relative (seen <= 2e-13; 1.3e-11 on BLOCKED).  Predictor: both forms of the mean to
1e-10 of the largest, the variance against the N x N form to 1e-10 signalSize (seen <= 8e-12 and <= 3e-14).
"""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as ref
import vfe_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gpx_vfe_fit", "gpx_vfe_bound", "gpx_vfe_grad", "gpx_vfe_posterior")
ALL = list(ref.CASES) + [ref.BLOCKED]
ALL_IDS = list(ref.IDS) + ["blocked"]


def entry_relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_gradient_matches_central_differences(c):
    spec, X, S, y, noise = ref.case(c)
    cond = ref.cond_quu(spec, S, noise)
    assert cond <= 1e4, cond
    g = vref.value_grad(spec, X, S, y, noise)[1]
    theta = np.concatenate([ref.hyp_of(spec), [noise]])
    assert g.shape == theta.shape
    fd = np.empty(theta.size)
    for k in range(theta.size):
        h = 1e-4 * theta[k]
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd[k] = (vref.value(ref.spec_with(spec, tp[:-1]), X, S, y, float(tp[-1]))
                 - vref.value(ref.spec_with(spec, tm[:-1]), X, S, y, float(tm[-1]))) / (2.0 * h)
    err = entry_relerr(g, fd)
    print("cond(Quu) %.2e  gradient vs central differences %.2e  smallest/largest entry %.2e"
          % (cond, err, np.min(np.abs(g)) / np.max(np.abs(g))))
    assert err <= 1e-6, (g, fd)


@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_inducing_gradient_matches_central_differences(c):
    spec, X, S, y, noise = ref.case(c)
    assert ref.cond_quu(spec, S, noise) <= 1e4
    g = vref.grad_S(spec, X, S, y, noise)
    assert g.shape == S.shape
    rng = np.random.default_rng(7)
    h, worst = 1e-5, 0.0
    # eight entries: the largest one, the first one, six drawn
    for idx in [int(np.argmax(np.abs(g))), 0] + [int(v) for v in rng.choice(g.size, 6, replace=False)]:
        u, l = divmod(idx, S.shape[1])
        Sp, Sm = S.copy(), S.copy()
        Sp[u, l] += h
        Sm[u, l] -= h
        fd = (vref.value(spec, X, Sp, y, noise) - vref.value(spec, X, Sm, y, noise)) / (2.0 * h)
        worst = max(worst, abs(fd - g[u, l]) / np.max(np.abs(g)))
    print("dF/dS vs central differences: worst %.2e of max|grad| = %.3e" % (worst, np.max(np.abs(g))))
    assert worst <= 1e-5


@pytest.mark.parametrize("c", ALL, ids=ALL_IDS)
def test_value_matches_the_dense_form_and_is_a_monotone_lower_bound(c):
    spec, X, S, y, noise = ref.case(c)
    assert ref.cond_quu(spec, S, noise) <= 1e4
    f = vref.value(spec, X, S, y, noise)
    fd = vref.dense_value(spec, X, S, y, noise)
    exact = vref.exact_loglike(spec, X, y, noise)
    fewer = vref.value(spec, X, S[:-5], y, noise)
    print("nu x N vs dense %.2e;  F %.6f <= exact %.6f;  F without the last five inducing points %.6f" %
          (abs(f - fd) / abs(fd), f, exact, fewer))
    assert abs(f - fd) <= 1e-10 * abs(fd)
    assert f <= exact
    assert fewer <= f


@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_both_forms_of_the_predictor_agree_and_the_variance_is_positive(c):
    spec, X, S, y, noise = ref.case(c)
    assert ref.cond_quu(spec, S, noise) <= 1e4
    s = float(ref.hyp_of(spec)[-1])
    Z = np.random.default_rng(31).uniform(-1.2, 1.2, (300, spec["d"]))
    mean, var = vref.predict(spec, X, S, y, noise, Z)
    dmean, dvar = vref.predict_dense(spec, X, S, y, noise, Z)
    em = float(np.max(np.abs(mean - dmean)) / np.max(np.abs(dmean)))
    ev = float(np.max(np.abs(var - dvar)) / s)
    print("mean %.2e  variance %.2e of signalSize  min variance %.3e signalSize" % (em, ev, np.min(var) / s))
    assert em <= 1e-10 and ev <= 1e-10
    assert np.all(var > 0.0)


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", txt))
    assert set(ENTRIES) <= syms
    assert "#define GPX_ABI_VERSION 2" in txt


def test_binding_lists_the_entry_points():
    from gpexp_amd import _lib
    assert set(ENTRIES) <= set(_lib.exported_symbols())


def test_constructor_validates_the_sparse_keyword():
    from gpexp_amd.kernels import KernelSquaredExponential
    from gpexp_amd.gp import GP
    k = KernelSquaredExponential([0.5, 0.5], 1.0, 2)
    assert GP(k, 0.1, FITC=0.5).sparse == "fitc" and GP(k, 0.1, FITC=0.5, sparse="fitc").sparse == "fitc"
    assert GP(k, 0.1).sparse == "fitc"
    g = GP(k, 0.1, FITC=0.5, sparse="vfe")
    assert g.sparse == "vfe" and g.FITC == 0.5 and g.fitcnodes is None
    with pytest.raises(ValueError, match="sparse"):
        GP(k, 0.1, FITC=0.5, sparse="dtc")
    with pytest.raises(ValueError, match="FITC"):
        GP(k, 0.1, sparse="vfe")


def test_unsupported_calls_raise_before_any_device_work():
    from gpexp_amd.kernels import KernelMehlerND, KernelSquaredExponential
    from gpexp_amd.gp import GP
    X, y = np.zeros((4, 2)), np.zeros(4)
    g = GP(KernelMehlerND([0.5, 0.5], 2), 0.1, FITC=0.5, sparse="vfe")
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        g.loglikeParams(X, y, returnDeriv=1)
    assert g.fitcnodes is None
    v = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.1, FITC=0.5, sparse="vfe")
    for call in (lambda: v.fitcLooPredict(X, y), lambda: v.fitcLooLogLike(X, y), lambda: v.looPredict(X, y),
                 lambda: v.findOptParamsLogLike(X, y, objective="loo"), lambda: v.loglikeParams(X, y, noiseIn=np.full(4, 0.1)),
                 lambda: v.evaluate(X, compvar=2), lambda: v.evaluateVarianceDerivative(X),
                 lambda: v.evaluateVarianceDerivWRTnewpt(X), lambda: v.varianceGradient(X)):
        with pytest.raises(NotImplementedError, match="VFE"):
            call()
    assert v.fitcnodes is None
