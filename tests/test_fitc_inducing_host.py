"""CPU-only checks of the gradient of the FITC likelihood w.r.t. the inducing-point locations that the device code implements
(tests/fitc_inducing_ref.py), and of the ABI addition.

Every error is relative to the largest |entry| of the reference matrix: the smallest entries of dL/dS are ~1e-6 of the largest,
so per-entry relative errors mean nothing for this matrix.

Tolerances.  Central differences (h = 1e-5) of fitc_grad_ref._model(...)["value"]: truncation ~ h^2 f''' / 6 ~ 1e-10 of the
gradient, cancellation ~ eps |L| / h ~ 1e-16 * 1e2..1e3 / 1e-5 ~ 1e-9..1e-8 absolute against largest entries of 1..1e2; 1e-5 of
the largest entry leaves the margin to that trade of the difference quotient, not to the formula (seen: <= 2.1e-6).  The nu x N
form against the dense form (M explicit, Cholesky of Q + G): both solve systems of condition <= ~1e4, 1e-10 is cond * eps with
two decades to spare (seen: <= 5.4e-12).  On BLOCKED (N = 2304) the gap is printed, not asserted: it belongs to the reference side
(seen: 2.2e-10) and says how much of the device test's 1e-8 the reference itself uses up.
"""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as ref
import fitc_inducing_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLACEMENTS = ["subset", "perturbed"]


def inducing(S, where):
    return S if where == "subset" else iref.perturbed(S)


def max_relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_gradient_matches_central_differences(c, where):
    spec, X, S, y, noise = ref.case(c)
    S = inducing(S, where)
    g = iref.grad_S(spec, X, S, y, noise)
    assert g.shape == S.shape
    rng = np.random.default_rng(7)
    h, worst = 1e-5, 0.0
    # eight entries: the largest one, the first one, six drawn
    flat = [int(np.argmax(np.abs(g))), 0] + [int(v) for v in rng.choice(g.size, 6, replace=False)]
    for idx in flat:
        u, l = divmod(idx, S.shape[1])
        Sp, Sm = S.copy(), S.copy()
        Sp[u, l] += h
        Sm[u, l] -= h
        fd = (iref.value(spec, X, Sp, y, noise) - iref.value(spec, X, Sm, y, noise)) / (2.0 * h)
        worst = max(worst, abs(fd - g[u, l]) / np.max(np.abs(g)))
    print("dL/dS vs central differences (%s): worst %.2e of max|grad| = %.3e" % (where, worst, np.max(np.abs(g))))
    assert worst <= 1e-5


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_rectangular_form_matches_dense_form(c, where):
    spec, X, S, y, noise = ref.case(c)
    S = inducing(S, where)
    err = max_relerr(iref.grad_S(spec, X, S, y, noise), iref.grad_S_dense(spec, X, S, y, noise))
    print("nu x N form vs dense form (%s): %.2e" % (where, err))
    assert err <= 1e-10


def test_blocked_case_gap_between_the_forms_is_reported():
    spec, X, S, y, noise = ref.case(ref.BLOCKED)
    S = iref.perturbed(S)
    T = iref.weights(spec, X, S, y, noise)[1]
    err = max_relerr(iref.grad_S(spec, X, S, y, noise), iref.grad_S_dense(spec, X, S, y, noise))
    print("BLOCKED: nu x N form vs dense form %.2e;  |T - T^T| / max|T| = %.2e" % (err, np.max(np.abs(T - T.T)) / np.max(np.abs(T))))
    assert np.isfinite(err)


def test_header_declares_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "gpx_fitc_lml_grad_inducing" in set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", txt))


def test_binding_lists_the_entry_point():
    from gpexp_amd import _lib
    assert "gpx_fitc_lml_grad_inducing" in _lib.exported_symbols()


def test_inducing_derivative_is_refused_where_it_does_not_exist():
    from gpexp_amd.kernels import KernelSquaredExponential
    from gpexp_amd.gp import GP
    X, y = np.zeros((4, 2)), np.zeros(4)
    dense = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.1)
    with pytest.raises(ValueError, match="inducingDeriv"):
        dense.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
    sparse = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.1, FITC=0.5)
    with pytest.raises(ValueError, match="inducingDeriv"):
        sparse.loglikeParams(X, y, returnDeriv=0, inducingDeriv=True)
    for kw in (dict(analyticGradient=False), dict(analyticGradient=True, objective="loo")):
        with pytest.raises(ValueError, match="optimizeInducing"):
            sparse.findOptParamsLogLike(X, y, optimizeInducing=True, **kw)
    with pytest.raises(ValueError, match="optimizeInducing"):
        dense.findOptParamsLogLike(X, y, optimizeInducing=True, analyticGradient=True)
