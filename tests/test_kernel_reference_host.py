"""What the element-wise bound of tests/kernel_reference.py rests on, checked without a GPU:

  * the 256 literals of kExp2Tab in kfill.hip are the correctly rounded 2^(j/256);
  * fast_exp, emulated in exact rational arithmetic (every fma rounded once) with the constants parsed out of the source,
    stays within (2 + 0.2 |x|) 2^-52 of exp over [-745, 0]: whoever changes the table size or the polynomial degree re-derives
    the 0.2 |x| and the 8 of the bound;
  * the float64 oracle (differences first) and a float64 emulation of the expanded form staged as stage_points stages it
    both meet the bound with error / bound <= 0.5 on the structured sets of the GPU test: the bound is not vacuous and the
    device keeps real headroom;
  * the harness reports a single entry off by 3e-14 relative, a far-tail entry off by 1e-3 relative, and a zeroed entry.
"""
import decimal
import math
import os
import re
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

from oracle import gpexp_oracle as orc
import kernel_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KFILL = os.path.join(ROOT, "gpexp_amd", "csrc", "kfill.hip")
NUM = r"[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?"


@pytest.fixture(scope="module")
def source():
    with open(KFILL) as f:
        return f.read()


def parse_table(src):
    m = re.search(r"kExp2Tab\[EXP_TAB\]\s*=\s*\{(.*?)\};", src, re.S)
    assert m, "kExp2Tab not found in kfill.hip"
    return [float(t) for t in re.findall(NUM, m.group(1))]


def parse_fast_exp(src):
    """Constants of fast_exp as the doubles the compiler sees."""
    body = re.search(r"double fast_exp\(double xin.*?\n}\n", src, re.S)
    assert body, "fast_exp not found in kfill.hip"
    b = body.group(0)
    c = {}
    c["tab_size"] = int(re.search(r"constexpr int EXP_TAB = (\d+);", src).group(1))
    c["shift"] = float(re.search(r"SHIFT = (%s);" % NUM, b).group(1))
    c["clamp"] = float(re.search(r"vmax1\(xin, (%s)\)" % NUM, b).group(1))
    c["inv"] = float(re.search(r"sh = fma\(x, (%s), SHIFT\)" % NUM, b).group(1))
    c["step"] = float(re.search(r"r = fma\(m, (%s), x\)" % NUM, b).group(1))
    c["poly"] = [float(re.search(r"double p = (%s);" % NUM, b).group(1))]
    c["poly"] += [float(v) for v in re.findall(r"p = fma\(p, r, (%s)\);" % NUM, b)]
    return c


def fma(a, b, c):
    """Correctly rounded a * b + c (int / int true division rounds to nearest even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fast_exp_emulated(xin, c, tab, f=1.0):
    """f * exp(xin) as the device forms it: the factor goes in before the exponent."""
    x = max(xin, c["clamp"])
    sh = fma(x, c["inv"], c["shift"])
    m = sh - c["shift"]                      # exact: both are integers below 2^53
    mi = (int(m) + 2 ** 31) % 2 ** 32 - 2 ** 31  # the low dword of the shifted sum, as a signed int
    r = fma(m, c["step"], x)
    tj = tab[mi & (c["tab_size"] - 1)]
    p = c["poly"][0]
    for coef in c["poly"][1:]:
        p = fma(p, r, coef)
    return math.ldexp((tj * p) * f, mi >> 8)


def test_exp2_table_is_correctly_rounded(source):
    tab = parse_table(source)
    assert len(tab) == 256
    with decimal.localcontext(decimal.Context(prec=60)):
        ln2 = Decimal(2).ln()
        for j, v in enumerate(tab):
            want = (ln2 * j / 256).exp()
            assert v == float(want), "kExp2Tab[%d] = %r is not the nearest double to 2^(%d/256) = %s" % (j, v, j, want)
            # and not a tie that float() resolved by luck: the true value is well inside the rounding interval
            assert j == 0 or abs(Decimal(v) - want) < Decimal(math.ulp(v)) / 2


def test_fast_exp_emulation_meets_its_share_of_the_bound(source):
    c = parse_fast_exp(source)
    tab = parse_table(source)
    assert c["shift"] == 1.5 * 2.0 ** 52 and c["clamp"] == -5.0e6 and len(c["poly"]) == 5 and c["tab_size"] == len(tab)
    rng = np.random.default_rng(20240)
    xs = np.concatenate([rng.uniform(-1.0, 0.0, 20000), rng.uniform(-40.0, -1.0, 20000),
                         rng.uniform(-745.0, -40.0, 20000), [0.0, -0.0, -745.2, -750.0, -1e9]])
    tiny = Decimal(2) ** -1022
    step = Decimal(2) ** -1074
    deep = 0
    worst = (0.0, 0.0)   # (excess over 1.5 units, x) of error / |x| for the normal results: the slope the bound rounds up
    with decimal.localcontext(decimal.Context(prec=70, Emin=-999999999, Emax=999999999)):
        for x in xs:
            x = float(x)
            got = fast_exp_emulated(x, c, tab)
            if x <= -745.2:
                assert got == 0.0, "fast_exp(%r) = %r, want exactly 0" % (x, got)
                continue
            want = Decimal(x).exp()
            err = abs(Decimal(got) - want)
            if want >= tiny:
                units = float(err / want) * 2.0 ** 52
                assert units <= 2.0 + 0.2 * abs(x), "fast_exp(%r): %.3g units of 2^-52" % (x, units)
                if x < -1.0:
                    worst = max(worst, ((units - 1.5) / abs(x), x))
            else:
                # a denormal result just below 2^-1022 still has ~2^52 grid steps in it, so the relative error of the
                # range reduction (110 units at x = -708.4) is 110 steps there and falls under half a step by x = -714:
                # the relative bound of the normal results carries on, plus the half step of v_ldexp's rounding to the
                # grid; from x = -714 down that is "less than one denormal step" and nothing else
                rel_part = Decimal((2.0 + 0.2 * abs(x)) * 2.0 ** -52) * want
                assert err <= rel_part + step / 2, ("fast_exp(%r) = %r: denormal result off by %.4g steps"
                                                    % (x, got, float(err / step)))
                if rel_part < step / 2:
                    assert err < step
                    deep += 1
    assert deep >= 500   # results held to one step of the denormal grid alone
    assert fast_exp_emulated(0.0, c, tab) == 1.0 and fast_exp_emulated(-0.0, c, tab) == 1.0
    # the measured slope (0.155) has not drifted to the 0.2 the bound uses
    assert worst[0] <= 0.17, "error growth %.3f units per unit of |x| at x = %r" % worst


def test_fast_exp_factor_goes_in_before_the_exponent(source):
    """f * exp(x) for a factor well above 1 (Matern-3/2: f = sig (1 + t) = 746 at t = 745) whose result is denormal: the
    product is rounded to the denormal grid once, so the error stays a relative part (one more rounding than exp alone) plus
    half a grid step -- f times an already rounded denormal exp(x) would be off by f / 2 steps."""
    c = parse_fast_exp(source)
    tab = parse_table(source)
    assert re.search(r"return ldexp\(\(tj \* p\) \* f, mi >> 8\);", source), "the emulation no longer matches fast_exp"
    rng = np.random.default_rng(20241)
    step = Decimal(2) ** -1074
    most = Decimal(0)
    with decimal.localcontext(decimal.Context(prec=70, Emin=-999999999, Emax=999999999)):
        for t in np.concatenate([rng.uniform(700.0, 760.0, 3000), rng.uniform(760.0, 1100.0, 200)]):
            t = float(t)
            f = 1.3 * t + 1.3
            want = Decimal(f) * Decimal(-t).exp()
            err = abs(Decimal(fast_exp_emulated(-t, c, tab, f)) - want)
            assert err <= Decimal((3.0 + 0.2 * t) * 2.0 ** -52) * want + step / 2, (t, float(err / step))
            if want < Decimal(2) ** -1040:
                most = max(most, err / step)
    assert most < 1
    # beyond the clamp no finite factor brings the result back: Matern-5/2 of points 1e9 ... 1e150 length scales apart
    for t in (1e4, 1e9, 1e50, 1e150):
        assert fast_exp_emulated(-t, c, tab, 1.3 * (1.0 + t + t * t / 3.0)) == 0.0
    assert fast_exp_emulated(-1e200, c, tab, 8.0e307) == 0.0


# ---- the bound against float64 arithmetic ---------------------------------------------------------------------------------
def spec_for(kind, d, sig=1.3):
    if kind == "se":
        return dict(kind="se", cl=list(0.4 + 0.03 * np.arange(d)), signalSize=sig, d=d)
    if kind == "mehler":
        return dict(kind="mehler", t=list(0.2 + 0.01 * np.arange(d)), d=d)
    return dict(kind=kind, rho=0.9, signalSize=sig, d=d)


def device_scale(spec):
    """scale / c1 / c2 / sig in float64 exactly as gpx_make_kparams forms them."""
    d, hyp = spec["d"], kr.hyp_of(spec)
    if spec["kind"] == "se":
        return hyp[d], np.array([1.0 / h for h in hyp[:d]]), None, None
    if spec["kind"] == "matern32":
        return hyp[1], np.full(d, math.sqrt(3.0) / hyp[0]), None, None
    if spec["kind"] == "matern52":
        return hyp[1], np.full(d, math.sqrt(5.0) / hyp[0]), None, None
    sig, c1, c2 = 1.0, [], []
    for t in hyp:
        om = 1.0 - t * t
        c1.append(t * t / (2.0 * om))
        c2.append(t / om)
        sig *= om ** -0.5
    return sig, np.ones(d), np.array(c1), np.array(c2)


def expanded_float64(spec, A, B, center):
    """The augmented operands of stage_points and their dot product in slot order, plain float64 (no fma), then kvalue."""
    kind, d = spec["kind"], spec["d"]
    sig, scale, c1, c2 = device_scale(spec)
    if kind == "mehler":
        pa = np.zeros(len(A))
        pb = np.zeros(len(B))
        for k in range(d):
            pa = pa + (c1[k] * A[:, k]) * A[:, k]
            pb = pb + (c1[k] * B[:, k]) * B[:, k]
        Ap = np.hstack([c2[None, :] * A, pa[:, None], np.ones((len(A), 1))])
        Bp = np.hstack([-B, np.ones((len(B), 1)), pb[:, None]])
    else:
        wa = (A - center[None, :]) * scale[None, :]
        wb = (B - center[None, :]) * scale[None, :]
        na = np.zeros(len(A))
        nb = np.zeros(len(B))
        for k in range(d):
            na = na + wa[:, k] * wa[:, k]
            nb = nb + wb[:, k] * wb[:, k]
        Ap = np.hstack([wa, na[:, None], np.ones((len(A), 1))])
        Bp = np.hstack([-2.0 * wb, np.ones((len(B), 1)), nb[:, None]])
    acc = np.zeros((len(A), len(B)))
    for k in range(d + 2):
        acc = acc + Ap[:, k][:, None] * Bp[:, k][None, :]
    if kind == "se":
        return sig * np.exp(-0.5 * acc)
    if kind == "mehler":
        return sig * np.exp(-acc)
    s = np.maximum(acc, 1e-300)
    t = np.sqrt(s)
    if kind == "matern32":
        return (t * sig + sig) * np.exp(-t)
    return (s * (sig * (1.0 / 3.0)) + (t * sig + sig)) * np.exp(-t)


HOST_CASES = [(kind, d, half) for kind in ("se", "matern32", "matern52") for d, half in ((1, 4.0), (2, 2.0), (3, 1.5),
                                                                                         (8, 0.9), (32, 0.45))]
HOST_CASES += [("mehler", 1, 2.0), ("mehler", 3, 1.5), ("mehler", 8, 1.0), ("mehler", 32, 0.5)]


@pytest.mark.parametrize("kind,d,half", HOST_CASES)
def test_float64_arithmetic_meets_the_bound_with_headroom(kind, d, half):
    """S * sens of the stationary cases: 2 d (half * scale)^2 * sens, up to ~119 at d = 32 for SE."""
    spec = spec_for(kind, d)
    X, Z = kr.structured_sets(spec, half, 60, 40, seed=1000 + d)
    center = 0.5 * X.min(0) + 0.5 * X.max(0) if kind != "mehler" else np.zeros(d)
    nug = 0.05 + 0.01 * np.arange(len(X))
    sym = kr.Reference(spec, X)
    rect = kr.Reference(spec, X, Z)
    worst = []
    # difference form: the oracle
    K = orc.cov_matrix(spec, X, nug, row_loop=False)
    worst.append(sym.worst(K, "diff", nugget=nug))
    worst.append(rect.worst(orc.cross_matrix(spec, Z, X).T, "diff"))
    I = np.arange(min(len(X), len(Z)))
    paired = kr.Reference(spec, X, Z, pairs=(I, I))
    worst.append(paired.worst(orc.kernel_eval(spec, X[I], Z[I]), "diff"))
    # expanded form: float64 emulation of the staging and the dot product
    Ke = expanded_float64(spec, X, X, center)
    Ke[np.diag_indices(len(X))] = sym.sig if kind != "mehler" else np.diag(Ke)
    worst.append(sym.worst(Ke, "expanded", center))
    worst.append(rect.worst(expanded_float64(spec, X, Z, center), "expanded", center))
    for r, what in worst:
        assert r <= 0.5, what
    # and not vacuous: float64 arithmetic uses a visible part of it somewhere
    assert max(r for r, _ in worst) >= 0.01, worst


def test_bound_terms():
    """Spot values of the formula: a pair at distance 0, and the pure-exp term far out."""
    spec = dict(kind="se", cl=[1.0], signalSize=1.0, d=1)
    ref = kr.Reference(spec, np.array([[0.0]]), np.array([[0.0], [2.0], [40.0]]))
    b = [float(v) for v in ref.bound("diff")]
    u = 2.0 ** -53
    assert ref.kf[0] == 1.0 and b[0] == 8 * 2 * u + 2.0 ** -1073
    assert np.isclose(b[1], (8 + 0.2 * 2.0) * 2 * u * math.exp(-2.0) + 0.5 * math.exp(-2.0) * 18 * u * 4.0, rtol=1e-12)
    assert ref.kf[2] == 0.0 and b[2] == 2.0 ** -1073          # x = 800
    be = [float(v) for v in ref.bound("expanded", center=np.array([20.0]))]
    assert np.isclose(be[1], (8 + 0.4) * 2 * u * math.exp(-2.0) + 0.5 * math.exp(-2.0) * 18 * u * (400 + 324 + 720),
                      rtol=1e-12)


def test_harness_reports_injected_errors():
    spec = spec_for("se", 3)
    X, Z = kr.structured_sets(spec, 2.5, 80, 30, seed=5)
    ref = kr.Reference(spec, X, Z)
    good = orc.cross_matrix(spec, Z, X).T
    assert ref.failures(good, "diff") == []
    ref.check(good, "diff")
    sig = spec["signalSize"]
    s = 2.0 * ref.x.reshape(good.shape)
    # 1. a well-conditioned entry off by 3e-14 relative
    i, j = np.argwhere((s > 0.01) & (s < 1.0))[0]
    bad = good.copy()
    bad[i, j] *= 1.0 + 3e-14
    assert ref.failures(bad, "diff") == [(i, j)]
    with pytest.raises(AssertionError, match=r"pair \(%d, %d\)" % (i, j)):
        ref.check(bad, "diff")
    # 2. a far-tail entry off by 1e-3 relative: invisible to max|a - b| / max|b|
    tail = np.argwhere((good < 1e-12 * sig) & (good > 1e-200))
    assert len(tail) > 0
    i, j = tail[0]
    bad = good.copy()
    bad[i, j] *= 1.001
    assert np.max(np.abs(bad - good)) / np.max(np.abs(good)) < 1e-13
    assert ref.failures(bad, "diff") == [(i, j)]
    with pytest.raises(AssertionError, match=r"pair \(%d, %d\)" % (i, j)):
        ref.check(bad, "diff")
    # 3. an entry replaced by 0.0
    i, j = np.argwhere(good > 1e-6 * sig)[-1]
    bad = good.copy()
    bad[i, j] = 0.0
    assert ref.failures(bad, "diff") == [(i, j)]
    with pytest.raises(AssertionError, match=r"pair \(%d, %d\)" % (i, j)):
        ref.check(bad, "diff")
    # and a NaN is never within a bound
    bad = good.copy()
    bad[3, 4] = np.nan
    assert ref.failures(bad, "diff") == [(3, 4)]
