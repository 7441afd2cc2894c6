"""CPU-only checks of the FITC hyper-parameter gradient the device code implements (tests/fitc_grad_ref.py), and of the ABI
addition.

Tolerances.  Central differences of the oracle's FITC likelihood at relative step 1e-4: truncation ~ h^2 f''' / 6 ~ 1e-8
relative, cancellation ~ eps cond(Q + G) |L| / (h theta) ~ 1e-8..1e-7 on these inputs (cond(Quu) <= 1e3; the oracle goes through
pinv(Quu) and a dense slogdet, which is why the cases keep Quu well conditioned: each asserts cond(Quu) <= 1e4 as a condition of
validity); 1e-6 per entry, relative to the entry, leaves a margin of ~4 over the largest figure seen.  The nu x N form against
the dense form (M explicit, Cholesky of Q + G): both solve systems of condition <= ~1e4, so 1e-9 is cond * eps with three
decades to spare.
"""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as ref
from oracle import gpexp_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def entry_relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def central_differences(spec, X, S, y, noise, rel=1e-4):
    theta = np.concatenate([ref.hyp_of(spec), [noise]])
    out = np.empty(theta.size)
    for k in range(theta.size):
        h = rel * theta[k]
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fp = oracle.fitc_loglike(ref.spec_with(spec, tp[:-1]), X, y, float(tp[-1]), S)
        fm = oracle.fitc_loglike(ref.spec_with(spec, tm[:-1]), X, y, float(tm[-1]), S)
        out[k] = (fp - fm) / (2.0 * h)
    return out


@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_gradient_matches_central_differences_of_the_oracle(c):
    spec, X, S, y, noise = ref.case(c)
    cond = ref.cond_quu(spec, S, noise)
    assert cond <= 1e4, cond
    value, g = ref.fitc_value_grad(spec, X, S, y, noise)
    assert g.shape == (len(ref.hyp_of(spec)) + 1,)
    ov = oracle.fitc_loglike(spec, X, y, noise, S)
    fd = central_differences(spec, X, S, y, noise)
    err = entry_relerr(g, fd)
    print("cond(Quu) %.2e  value %.3e  gradient vs central differences %.2e" % (cond, abs(value - ov) / abs(ov), err))
    assert abs(value - ov) <= 1e-10 * abs(ov)
    assert err <= 1e-6, (g, fd)


@pytest.mark.parametrize("c", ref.CASES, ids=ref.IDS)
def test_rectangular_form_matches_dense_form(c):
    spec, X, S, y, noise = ref.case(c)
    g = ref.fitc_value_grad(spec, X, S, y, noise)[1]
    gd = ref.fitc_grad_dense(spec, X, S, y, noise)
    err = entry_relerr(g, gd)
    print("nu x N form vs dense form: %.2e" % err)
    assert err <= 1e-9, (g, gd)


def test_header_declares_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", txt))
    assert "gpx_fitc_lml_grad" in syms
    assert "#define GPX_ABI_VERSION 2" in txt


def test_binding_lists_the_entry_point():
    from gpexp_amd import _lib
    assert "gpx_fitc_lml_grad" in _lib.exported_symbols()


def test_mehler_with_fitc_raises_before_any_device_work():
    from gpexp_amd.kernels import KernelMehlerND
    from gpexp_amd.gp import GP
    g = GP(KernelMehlerND([0.5, 0.5], 2), 0.1, FITC=0.5)
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        g.loglikeParams(np.zeros((4, 2)), np.zeros(4), returnDeriv=1)
