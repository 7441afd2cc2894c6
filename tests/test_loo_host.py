"""CPU-only checks of the leave-one-out formulas the device code implements (tests/loo_ref.py), and of the ABI additions.

Tolerances: the closed form and N actual refits solve the same well-conditioned systems (cond(K) <= 6e3 in these cases: a
relative error of cond * eps ~ 1e-12 at the very most; measured <= 3.3e-14); the gradient is compared with central differences
of step 1e-5, whose own truncation + cancellation error (measured <= 2.4e-6 of the largest entry) sets the bound, not the
formula's."""
import os
import re

import numpy as np
import pytest

import loo_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kind, d, n, noise, seed, per-point nugget)
CASES = [("m52", 3, 150, 0.05, 1, False),
         ("m32", 1, 150, 0.05, 2, False),
         ("se", 8, 300, 1e-3, 3, False),
         ("m52", 3, 150, 0.02, 4, True)]
IDS = ["m52-d3", "m32-d1", "se-d8", "per-point"]


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_closed_form_matches_refits(c):
    kind, d, n, noise, seed, pp = c
    hyp, X, nugget, y = ref.case(kind, d, n, noise, seed, pp)
    K = ref.cov(kind, d, hyp, X, nugget)
    m0, v0, l0 = ref.loo_closed(K, y)
    m1, v1, l1 = ref.loo_brute(K, y)
    errs = (relerr(m0, m1), relerr(v0, v1), abs(l0 - l1) / abs(l1))
    print("cond %.2e  mean %.2e  var %.2e  logp %.2e" % ((np.linalg.cond(K),) + errs))
    assert max(errs) <= 1e-12, errs


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gradient_matches_central_differences(c):
    kind, d, n, noise, seed, pp = c
    hyp, X, nugget, y = ref.case(kind, d, n, noise, seed, pp)
    g = ref.loo_all(kind, d, hyp, X, nugget, y)[3]
    fd = ref.loo_grad_fd(kind, d, hyp, X, nugget, y, h=1e-5)
    assert g.shape == fd.shape == (ref.nlen(kind, d) + 2,)
    err = relerr(g, fd)
    print("gradient vs central differences: %.2e" % err)
    assert err <= 1e-5, (g, fd)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_signal_and_noise_shortcuts(c):
    """signalSize and noise need no N^3 product: P K0 = I - P D turns their row quantities into row reductions over P."""
    kind, d, n, noise, seed, pp = c
    hyp, X, nugget, y = ref.case(kind, d, n, noise, seed, pp)
    K = ref.cov(kind, d, hyp, X, nugget)
    generic = ref.loo_grad_closed(K, ref.dcov(kind, d, hyp, X)[-2:], y)
    short = ref.loo_grad_shortcuts(K, ref.nugget_vector(nugget, n), float(hyp[-1]), y)
    err = relerr(short, generic)
    print("shortcut vs generic: %.2e" % err)
    assert err <= 1e-12


def test_single_point():
    """n = 1: nothing to condition on -- the prior: mean 0, variance signalSize + noise."""
    hyp, X, nugget, y = ref.case("m52", 2, 1, 0.05, 5)
    m, v, lp = ref.loo_closed(ref.cov("m52", 2, hyp, X, nugget), y)
    assert abs(m[0]) <= 1e-15 and abs(v[0] - (hyp[-1] + 0.05)) <= 1e-15
    assert abs(lp - (-0.5 * np.log(v[0]) - y[0] ** 2 / (2 * v[0]) - 0.5 * ref.LOG2PI)) <= 1e-15


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", txt))
    assert "gpx_loo" in syms and "gpx_loo_grad" in syms
    assert "#define GPX_ABI_VERSION 2" in txt


def test_binding_lists_the_entry_points():
    from gpexp_amd import _lib
    syms = _lib.exported_symbols()
    assert "gpx_loo" in syms and "gpx_loo_grad" in syms


def test_objective_is_validated_before_any_device_work():
    from gpexp_amd.kernels import KernelIsoMatern
    from gpexp_amd.gp import GP
    g = GP(KernelIsoMatern(0.5, 1.0, 2, nu=2.5), 0.1)
    with pytest.raises(ValueError, match="objective"):
        g.findOptParamsLogLike(np.zeros((4, 2)), np.zeros(4), objective="bogus")
    with pytest.raises(NotImplementedError):
        GP(KernelIsoMatern(0.5, 1.0, 2), 0.1, FITC=0.5).looPredict(np.zeros((4, 2)), np.zeros(4))
