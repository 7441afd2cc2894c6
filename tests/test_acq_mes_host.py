"""CPU: the references, the float64 composition, the bound and the mutants of tests/acq_mes_ref.py, the census of the new entry points,
and the Gumbel sampler of the optimum value (gpexp_amd.experimentalDesign.gumbelOptima)."""
import os
import re

import numpy as np
import pytest

import acq_mes_ref as M
import acq_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = M.LD
SEAM = M.T0 * np.sqrt(2.0)
GAMMAS = (-1e6, -1e3, -100.0, -38.6, -20.0, -SEAM - 1e-9, -SEAM + 1e-9, -1.0, 0.0, 1.0, 9.0, 20.0, 37.0, 38.5)
NEW_ENTRIES = ("gpx_acq_mes", "gpx_acq_mes_grad", "gpx_acq_mes_batch", "gpx_vfe_acq_mes", "gpx_vfe_acq_mes_grad", "gpx_vfe_acq_mes_batch")


def _mp_terms(mp, g):
    """(h, h') by mpmath at the working precision; log Phi from the upper tail Q for gamma > 9, where ncdf rounds to 1."""
    g = mp.mpf(g)
    if g > 9:
        Q = mp.erfc(g / mp.sqrt(2)) / 2
        logPhi, lam = mp.log1p(-Q), mp.npdf(g) / (1 - Q)
    else:
        Phi = mp.erfc(-g / mp.sqrt(2)) / 2
        logPhi, lam = mp.log(Phi), mp.npdf(g) / Phi
    return g * lam / 2 - logPhi, -(lam / 2) * (1 + g * (g + lam))


def test_longdouble_terms_against_60_digits():
    mp = pytest.importorskip("mpmath")
    with mp.workdps(60):
        h, hp = M.terms_ld(np.array(GAMMAS, dtype=LD))
        for i, g in enumerate(GAMMAS):
            # the longdouble gamma of the seam points is the float64 one: both sides start from the same number
            wh, whp = _mp_terms(mp, mp.mpf(float(np.float64(g))))
            for name, got, want in (("h", h[i], wh), ("h'", hp[i], whp)):
                mant, ex = np.frexp(got)           # (a longdouble below 1e-308 has no two-double image: scale the mantissa's)
                got_mp = mp.ldexp(mp.mpf(float(mant)) + mp.mpf(float(mant - LD(float(mant)))), int(ex))
                err = abs(got_mp - want) / abs(want)
                print("gamma %-12g %-2s %.6e  rel err %.2e (%.2f x 2^-64)" % (g, name, float(got), float(err), float(err) * 2.0 ** 64))
                # a few 2^-64; at gamma = 37 / 38.5 the values' own e^(-gamma^2 / 2) carries gamma^2 2^-64 of the argument's rounding
                assert err < (64 + (g * g if g > 0 else 0.0)) * 2.0 ** -64, (g, name, float(err))
    assert M.terms_ld(np.array([np.inf]))[0][0] == 0 and M.terms_ld(np.array([np.inf]))[1][0] == 0
    assert np.isposinf(M.terms_ld(np.array([-np.inf]))[0][0]) and np.isnan(M.terms_ld(np.array([np.nan]))[0][0])


def test_seam_and_term_count_are_the_fewest_that_serve():
    """T0 and CF_TERMS are acq.hip's (and the class layer's); with CF_TERMS the truncation of D and of C2 at t = T0 is below u / 8
    against mpmath, with one term fewer it is not."""
    mp = pytest.importorskip("mpmath")
    src = open(os.path.join(ROOT, "gpexp_amd", "csrc", "acq.hip")).read()
    assert float(re.search(r"constexpr double MES_T0 = ([0-9.]+);", src).group(1)) == M.T0
    assert int(re.search(r"constexpr int MES_CF_TERMS = (\d+);", src).group(1)) == M.CF_TERMS
    import gpexp_amd.experimentalDesign as ED
    assert (ED._MES_T0, ED._MES_CF_TERMS) == (M.T0, M.CF_TERMS)
    with mp.workdps(60):
        t = mp.mpf(M.T0)
        D = 1 / (mp.sqrt(mp.pi) * mp.exp(t * t) * mp.erfc(t)) - t
        C2 = mp.mpf(1) / 2 / D - t

        def trunc(n):
            f = t
            for k in range(n, 2, -1):
                f = t + mp.mpf(k) / 2 / f
            c2 = 1 / f
            return float(abs(mp.mpf(1) / 2 / (t + c2) - D) / D), float(abs(c2 - C2) / C2)

        ok, short = trunc(M.CF_TERMS), trunc(M.CF_TERMS - 1)
        print("T0 = %g: %d terms D %.2e C2 %.2e; %d terms D %.2e C2 %.2e; u / 8 = %.2e" % ((M.T0, M.CF_TERMS) + ok + (M.CF_TERMS - 1,) + short + (M.U / 8,)))
        assert max(ok) < M.U / 8 <= max(short)


def _rows():
    for K in M.EPI_K:
        for sign in M.SIGNS:
            for mean, var in M.epilogue_rows_mes(257, sign):
                yield K, sign, M.ystar_of(K), mean, var


def test_float64_composition_within_its_bound_and_mutants_outside():
    worst = {"A": 0.0, "a": 0.0, "b": 0.0}
    caught = {m: 0.0 for m in M.MES_MUTANTS}
    for K, sign, ys, mean, var in _rows():
        ref = M.reference_costs_mes(ys, sign, mean, var, second=False)
        R = M.epilogue_bound_mes(ys, sign, mean, var)
        got = dict(zip("Aab", M.costs_f64_mes(ys, sign, mean, var)))
        for k in "Aab":
            w = A.judged(ref[k], R[k])
            q = A.bound_ratio(got[k], ref[k], R[k], w)
            worst[k] = max(worst[k], q)
            assert q <= 1.0, (K, sign, k, q)
            # outside the judged set reference and composition carry the same pattern, but for h'(-inf): NaN by the formulation
            assert np.all(~np.isfinite(got[k][~w]) | (got[k][~w] == np.asarray(ref[k], dtype=float)[~w])), (K, sign, k)
        for m in M.MES_MUTANTS:
            if m == "mean-ystar" and K == 1:
                continue
            mut = dict(zip("Aab", M.costs_f64_mes(ys, sign, mean, var, m)))
            for k in ("b",) if m == "abs-b" else "Aab":
                caught[m] = max(caught[m], A.bound_ratio(mut[k], ref[k], R[k], A.judged(ref[k], R[k])))
    print("float64 composition / bound: cost %.3f  a %.3f  b %.3f;  mutants: %s" % (worst["A"], worst["a"], worst["b"], {m: "%.3g" % v for m, v in caught.items()}))
    for m, v in caught.items():
        assert v > 1.0, "mutant %s (%s) passes the bound: %.3g" % (m, M.MES_MUTANTS[m], v)


def test_every_grid_row_is_judged():
    """No row of the grid part is left out: reference and bound are finite for every finite gamma, -1e150 and 38.6 included."""
    for K, sign, ys, mean, var in _rows():
        grid = np.isfinite(mean) & np.isfinite(var) & (var > 0)
        ref = M.reference_costs_mes(ys, sign, mean, var, second=False)
        R = M.epilogue_bound_mes(ys, sign, mean, var)
        for k in "Aab":
            assert np.all(A.judged(ref[k], R[k])[grid]), (K, sign, k)


def test_reference_derivatives_against_differences():
    """a = dA/dmu and b = dA/dvar of the reference against central differences of A in longdouble (gamma in [-30, 6], both signs of
    var and of `sign`), to 1e-9 of the derivative's scale."""
    rng = np.random.default_rng(5)
    ys = M.ystar_of(3)
    for sign in M.SIGNS:
        var = rng.uniform(0.5, 2.0, 40) * rng.choice([-1.0, 1.0], 40)
        mean = sign * rng.uniform(-30.0, 6.0, 40) * np.sqrt(np.abs(var))
        ref = M.reference_costs_mes(ys, sign, mean, var)
        hm, hv = LD(2.0 ** -26), np.abs(var).astype(LD) * LD(2.0 ** -26)
        Am = lambda m_, v_: M.reference_costs_mes(ys, sign, m_, v_, second=False)["A"]
        da = (Am(mean.astype(LD) + hm, var) - Am(mean.astype(LD) - hm, var)) / (2 * hm)
        db = (Am(mean, var.astype(LD) + hv) - Am(mean, var.astype(LD) - hv)) / (2 * hv)
        for name, got, want in (("a", ref["a"], da), ("b", ref["b"], db)):
            err = np.asarray(np.abs(got - want) / np.maximum(np.abs(want), LD(1e-3)), dtype=float)
            assert np.max(err) < 1e-9, (sign, name, float(np.max(err)))


def test_header_and_binding_census():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    dbg = open(os.path.join(ROOT, "include", "gpx_debug.h")).read()
    assert re.search(r"#define GPX_MES_MAX_K 1024\b", txt)
    assert re.search(r"enum gpx_acq_kind \{ GPX_ACQ_UCB = 0, GPX_ACQ_PI = 1, GPX_ACQ_EI = 2 \};", txt)          # unchanged
    for f in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % f, txt), f
    assert re.search(r"\bint gpx_dbg_acq_mes_epilogue\(", dbg)
    from gpexp_amd import _lib, device
    import gpexp_amd.experimentalDesign as impl
    import gpExp.experimentalDesign as shim
    assert set(NEW_ENTRIES) | {"gpx_dbg_acq_mes_epilogue"} <= set(_lib._SIGS)
    assert set(NEW_ENTRIES) | {"gpx_dbg_acq_mes_epilogue"} <= set(_lib.exported_symbols())
    assert device.MES_MAX_K == 1024
    for name in ("acq_mes", "acq_mes_grad", "acq_mes_batch", "dbg_acq_mes_epilogue"):
        assert callable(getattr(device, name)), name
    for name in ("acq_mes", "acq_mes_grad", "acq_mes_batch"):
        assert callable(getattr(device.VfeModel, name)), name
    assert "costFuncMES" in impl.__all__ and shim.costFuncMES is impl.costFuncMES


def test_class_layer_composition_is_the_reference_modules():
    """experimentalDesign.mesEntropyTerm (what costFuncMES.evaluate composes) gives terms_f64's h, special values included."""
    from gpexp_amd.experimentalDesign import mesEntropyTerm
    g = np.concatenate([M.g_grid_mes(), -M.g_grid_mes(), [np.inf, -np.inf, np.nan, 40.0, 41.0]])
    assert A.same_pattern(mesEntropyTerm(g), M.terms_f64(g)[0])


def test_gumbel_optima_against_brute_force_quantiles():
    """On a made-up (mu, s) vector: the three quartiles the sampler bisects are those of a brute-force tabulation of
    P(min_j f_j > y), the samples are the fitted Gumbel's inverse at the uniforms, monotone in them, and minimize=False mirrors."""
    from scipy.special import ndtr
    from gpexp_amd.experimentalDesign import gumbelOptima
    rng = np.random.default_rng(11)
    mu, s = rng.uniform(-1.0, 1.0, 60), rng.uniform(0.05, 0.6, 60)
    y = np.linspace(-6.0, 3.0, 900001)
    surv = np.ones_like(y)
    for m_, s_ in zip(mu, s):
        surv *= ndtr((m_ - y) / s_)                      # P(min f > y), decreasing in y
    # on z = -y the sampler's cdf of max(-f) is surv: its p-quantile in z is minus the y at which surv crosses p
    yq = {p: float(y[np.searchsorted(-surv, -p)]) for p in (0.25, 0.5, 0.75)}
    b = (-yq[0.25] + yq[0.75]) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    a = -yq[0.5] + b * np.log(np.log(2.0))
    r = np.array([0.03, 0.25, 0.5, 0.75, 0.9, 0.999])
    want = -(a - b * np.log(-np.log(r)))
    got = gumbelOptima(mu, s, r)
    print("quartiles of the minimum (brute force): %s; samples %s" % (yq, got))
    assert np.max(np.abs(got - want)) < 1e-4                               # (the table's step is 1e-5)
    # the fitted distribution reproduces the median and the interquartile range it was fitted to
    q1, q2, q3 = gumbelOptima(mu, s, [0.25, 0.5, 0.75])
    assert abs(q2 - yq[0.5]) < 1e-4 and abs((q1 - q3) - (yq[0.25] - yq[0.75])) < 1e-4
    assert np.all(np.diff(got) < 0)                                        # larger uniform: larger max(-f): smaller minimum
    assert np.array_equal(gumbelOptima(-mu, s, r, minimize=False), -got)
    for bad in ([0.0], [1.0], [np.nan]):
        with pytest.raises(ValueError):
            gumbelOptima(mu, s, bad)
    with pytest.raises(ValueError):
        gumbelOptima(mu, -s, r)
