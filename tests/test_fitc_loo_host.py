"""CPU-only checks of the FITC leave-one-out formulas the device code implements (tests/fitc_loo_ref.py), of the ABI addition and
of the refusals that need no device.

Tolerances.  The nu x N form against the dense form (P from the Cholesky factor of Q + G, M explicit): both solve systems of
condition <= ~1e4, so 1e-10 per gradient entry is cond * eps with two decades to spare (seen <= 4e-13), 1e-12 on the value (a sum
of N terms of order one).  Per-entry relative errors are meaningful here: no gradient entry is below 1e-2 of the largest.  Central
differences (h = 1e-5 theta) of the dense value: truncation ~ h^2 f''' / 6 ~ 1e-10, cancellation ~ eps |L| / h ~ 1e-9..1e-8 of
entries of 1..1e3; 1e-6 of the largest entry leaves that trade its margin (seen <= 1.1e-9).  Mean and variance against the
conditional with row and column i deleted: two solves of condition <= ~1e4, 1e-9 (seen <= 1e-12).  On BLOCKED (N = 2304) the gaps
are printed, not asserted: they are the reference's own share of the device test's tolerances (seen: gradient 8e-12, mean 1.5e-10
of max|mean|, var 2e-11).
"""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as ref
import fitc_loo_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpx_fitc_loo", "gpx_fitc_loo_grad")


def entry_relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("c", lref.CASES, ids=lref.IDS)
def test_rectangular_form_matches_dense_form(c):
    args = lref.case(c)
    a, b = lref.loo(*args), lref.loo_dense(*args)
    ev, eg = abs(a["value"] - b["value"]) / abs(b["value"]), entry_relerr(a["grad"], b["grad"])
    print("nu x N form vs dense form: value %.2e gradient %.2e  min|g|/max|g| %.2e  min p g %.3f" %
          (ev, eg, np.min(np.abs(b["grad"])) / np.max(np.abs(b["grad"])), np.min(ref._model(*args)["g"] / a["var"])))
    assert a["grad"].shape == (len(ref.hyp_of(args[0])) + 1,)
    assert ev <= 1e-12
    assert eg <= 1e-10, (a["grad"], b["grad"])
    assert np.max(np.abs(a["mean"] - b["mean"])) <= 1e-10 * np.max(np.abs(b["mean"]))
    assert entry_relerr(a["var"], b["var"]) <= 1e-10


def test_blocked_case_gap_between_the_forms_is_reported():
    args = lref.case(lref.BLOCKED)
    a, b = lref.loo(*args), lref.loo_dense(*args)
    print("BLOCKED: nu x N form vs dense form: value %.2e gradient %.2e mean %.2e of max|mean| var %.2e" %
          (abs(a["value"] - b["value"]) / abs(b["value"]), entry_relerr(a["grad"], b["grad"]),
           np.max(np.abs(a["mean"] - b["mean"])) / np.max(np.abs(b["mean"])), entry_relerr(a["var"], b["var"])))
    assert np.all(np.isfinite(a["grad"])) and np.all(np.isfinite(b["grad"]))


@pytest.mark.parametrize("c", lref.CASES, ids=lref.IDS)
def test_gradient_matches_central_differences_of_the_dense_value(c):
    spec, X, S, y, noise = lref.case(c)
    g = lref.loo(spec, X, S, y, noise)["grad"]
    theta = np.concatenate([ref.hyp_of(spec), [noise]])
    fd = np.empty(theta.size)
    for k in range(theta.size):
        h = 1e-5 * theta[k]
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd[k] = (lref.dense_value(ref.spec_with(spec, tp[:-1]), X, S, y, float(tp[-1]))
                 - lref.dense_value(ref.spec_with(spec, tm[:-1]), X, S, y, float(tm[-1]))) / (2.0 * h)
    err = float(np.max(np.abs(g - fd)) / np.max(np.abs(g)))
    print("gradient vs central differences: %.2e of max|grad| = %.3e" % (err, np.max(np.abs(g))))
    assert err <= 1e-6, (g, fd)


@pytest.mark.parametrize("c", lref.CASES, ids=lref.IDS)
def test_predictions_match_the_conditional_with_the_point_deleted(c):
    args = lref.case(c)
    a = lref.loo(*args)
    n = len(args[3])
    idx = [0, n - 1] + [int(v) for v in np.random.default_rng(9).choice(np.arange(1, n - 1), 6, replace=False)]
    worst = 0.0
    for i in idx:
        mu, var = lref.delete_one(*args, i)
        worst = max(worst, abs(a["mean"][i] - mu), abs(a["var"][i] - var))
    print("mean / var vs delete-one over %d indices: %.2e" % (len(idx), worst))
    assert worst <= 1e-9


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", txt))
    assert set(NAMES) <= syms
    assert "#define GPX_ABI_VERSION 2" in txt


def test_binding_lists_the_entry_points():
    from gpexp_amd import _lib
    assert set(NAMES) <= set(_lib.exported_symbols())


def test_refusals_that_need_no_device():
    from gpexp_amd.kernels import KernelMehlerND, KernelSquaredExponential
    from gpexp_amd.gp import GP
    X, y = np.zeros((4, 2)), np.zeros(4)
    dense = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.1)
    with pytest.raises(ValueError, match="looPredict"):
        dense.fitcLooPredict(X, y)
    with pytest.raises(ValueError, match="looLogLike"):
        dense.fitcLooLogLike(X, y)
    mehler = GP(KernelMehlerND([0.5, 0.5], 2), 0.1, FITC=0.5)
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        mehler.fitcLooLogLike(X, y, returnDeriv=1)
    assert mehler.fitcnodes is None      # refused before the inducing points were drawn, let alone any device work
    sparse = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.1, FITC=0.5)
    with pytest.raises(ValueError, match="optimizeInducing"):
        sparse.findOptParamsLogLike(X, y, optimizeInducing=True, analyticGradient=True, objective="loo")
    with pytest.raises(NotImplementedError, match="fitcLooPredict"):
        sparse.looPredict(X, y)
    with pytest.raises(NotImplementedError, match="fitcLooLogLike"):
        sparse.looLogLike(X, y)
