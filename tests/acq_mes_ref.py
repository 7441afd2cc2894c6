"""Longdouble references, the float64 composition, the epilogue's own bound and mutants for max-value entropy search (MES), the
fourth Bayesian-optimisation cost of gpexp_amd/csrc/acq.hip (NumPy / SciPy only; data and references of tests/test_acq_mes_host.py
and tests/test_gpu_acq_mes.py, not product code).  Conventions, metrics and the bound rule are tests/acq_ref.py's.

THE COST.  mu the posterior mean, var the SIGNED variance, s = sqrt(|var|), sg = sgn(var), K sampled optima y*_k; sign = +1: sampled
minima, gamma_k = (mu - y*_k) / s; sign = -1: sampled maxima, gamma_k = (y*_k - mu) / s; lambda = phi / Phi:
    h(gamma)  = gamma lambda / 2 - log Phi(gamma)            h'(gamma) = -(lambda / 2) (1 + gamma (gamma + lambda))
    A = -(1/K) sum_k h(gamma_k)       a = dA/dmu = -(sign / (K s)) sum_k h'       b = dA/dvar = (sg / (2 K s^2)) sum_k h' gamma_k
summed in the order k = 0 .. K-1; a = b = NaN where var == 0 exactly.

THE FORMULATION (acq.hip, mes_h; restated in float64 by terms_f64).  With t = -gamma / sqrt 2 >= T0 the continued fraction
    1 / (sqrt(pi) erfcx t) = t + D,   D = (1/2) / (t + C2),   C2 = 1 / (t + (3/2) / (t + 2 / (t + ..)))      (partial numerators k / 2)
truncated after the numerator CF_TERMS / 2 gives lambda = sqrt 2 (t + D), h = log(2 sqrt(pi) (t + D)) - (1 - w) / 2 and
1 + gamma (gamma + lambda) = w = C2 / (t + C2): no cancellation, no exponential.  Elsewhere the composition through the tail Q =
erfc(|gamma| / sqrt 2) / 2, phi from an exactly formed gamma^2 / 2, log Q (gamma <= 0) or log1p(-Q) (gamma > 0); beyond gamma = 40
h = h' = 0.  T0 = 2 and CF_TERMS = 73: the fewest terms whose truncation of D and of C2 at t = T0 is below u / 8 (host test, against
mpmath); at T0 = 3, 41 terms serve, but the composition below it then loses 2 T0^2 = 18 times the library's error in h (measured
with SciPy: 123 u at gamma = -4.2 against 20 u at -2.8 for T0 = 2) and gamma^4 / 2 = 162 times in h'.

THE BOUND (epilogue_bound_mes): first-order rounding of that formulation, FIXED library constants: acq_ref's erfc 16 ulp and exp 3 ulp,
log 3 ulp and log1p 2 ulp (the OpenCL double-precision ceilings), one ulp <= 2 u, with kernel_reference.DENORMAL_STEP."""
import contextlib

import math

import numpy as np

import acq_ref as A

LD, U, DS = A.LD, A.U, A.DS
T0, CF_TERMS = 2.0, 73                         # acq.hip's MES_T0 / MES_CF_TERMS (pinned by the host test)
G_ZERO = 40.0                                  # beyond: h = h' = 0
LOG_ULP, LOG1P_ULP = 3.0, 2.0                  # FIXED, beside A.ERFC_ULP and A.EXP_ULP
_TWO_SQRT_PI = LD(2) * A._SQRT_PI
_T_CF_LD = LD(1) / LD(2)                       # the longdouble reference takes the fraction from t = 1/2 on (acq_ref's 1200 terms)
SIGNS = (1, -1)


# ---- h and h' in longdouble -------------------------------------------------------------------------------------------------------
def _cf_ld(t, terms=A._CF_TERMS):
    """(C2, t + C2) of the continued fraction, evaluated backward from the partial numerator terms / 2."""
    f = np.array(t, dtype=LD)
    for k in range(terms, 2, -1):
        f = t + (LD(k) / LD(2)) / f
    C2 = LD(1) / f
    return C2, t + C2


def terms_ld(g):
    """(h, h') in longdouble, a few 2^-64 relative for every finite gamma; h(+inf) = h'(+inf) = 0, h(-inf) = +inf with h' left NaN
    (the formulation's inf * 0), NaN for NaN."""
    g = np.asarray(g, dtype=LD)
    with np.errstate(all="ignore"):
        t = -g * A._SQRT_HALF
        cf = t >= _T_CF_LD
        tt = np.where(cf & np.isfinite(t), t, LD(1))
        C2, den = _cf_ld(tt)
        w, td = C2 / den, tt + (LD(1) / LD(2)) / den
        h_cf = np.log(_TWO_SQRT_PI * td) - (LD(1) - w) / LD(2)
        hp_cf = -(td * A._SQRT_HALF) * w
        gg = np.where(cf | ~np.isfinite(g), LD(0), g)
        phi, Q = A.phi_ld(gg), A._upper_tail(np.abs(gg))
        neg = gg <= 0
        lam = phi / np.where(neg, Q, LD(1) - Q)
        h_c = gg * lam / LD(2) - np.where(neg, np.log(np.where(neg, Q, LD(1))), np.log1p(-np.where(neg, LD(0), Q)))
        hp_c = -(lam / LD(2)) * (LD(1) + gg * (gg + lam))
        h, hp = np.where(cf, h_cf, h_c), np.where(cf, hp_cf, hp_c)
        pinf, ninf, nan = np.isposinf(g), np.isneginf(g), np.isnan(g)
        h = np.where(pinf, LD(0), np.where(ninf, LD(np.inf), np.where(nan, LD(np.nan), h)))
        hp = np.where(pinf, LD(0), np.where(ninf | nan, LD(np.nan), hp))
    return h, hp


def _second_ld(g):
    """h'' by central differences of h' (relative step 2^-20, absolute below |gamma| = 1): 1e-12 relative, for the SCALES only."""
    g = np.asarray(g, dtype=LD)
    with np.errstate(all="ignore"):
        step = np.maximum(np.abs(g), LD(1)) * LD(2.0 ** -20)
        return (terms_ld(g + step)[1] - terms_ld(g - step)[1]) / (LD(2) * step)


# ---- the reference values ----------------------------------------------------------------------------------------------------------
def gammas_ld(mu, var, ystar, sign):
    """(gamma (K, m), s, sg) in longdouble from float64 (or longdouble) mean and SIGNED variance."""
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    y = np.asarray(ystar, dtype=float).astype(LD).reshape(-1, 1)
    one = np.ones(np.broadcast(mu, var).shape, dtype=LD)
    with np.errstate(all="ignore"):
        s, sg = np.sqrt(np.abs(var)) * one, np.sign(var) * one
        d = (mu * one)[None, :] - y if sign > 0 else y - (mu * one)[None, :]
        return d / s[None, :], s, sg


def reference_costs_mes(ystar, sign, mu_ld, var_ld, second=True):
    """dict(A, a, b[, a_mu, a_var, b_mu, b_var], s, g, h, hp) in longdouble: acq_ref.reference_costs' keys for the MES cost.  The
    second derivatives (closed forms in h'', which comes from differences) serve the gradient's scale only."""
    g, s, sg = gammas_ld(mu_ld, var_ld, ystar, sign)
    K = LD(g.shape[0])
    var = np.asarray(var_ld, dtype=LD) * np.ones(s.shape, dtype=LD)
    with np.errstate(all="ignore"):
        h, hp = terms_ld(g)
        sh, shp, shg = np.sum(h, axis=0), np.sum(hp, axis=0), np.sum(hp * g, axis=0)
        out = dict(A=-sh / K, a=-(LD(sign) / (K * s)) * shp, b=(sg / (LD(2) * K * s * s)) * shg, s=s, g=g, h=h, hp=hp)
        if second:
            h2 = _second_ld(g)
            out["a_mu"] = -np.sum(h2, axis=0) / (K * s * s)
            out["a_var"] = LD(sign) * sg * np.sum(hp + g * h2, axis=0) / (LD(2) * K * s ** 3)
            out["b_mu"] = out["a_var"]
            out["b_var"] = -np.sum(LD(3) / LD(2) * hp * g + h2 * g * g / LD(2), axis=0) / (LD(2) * K * s ** 4)
        for k in ("a", "b"):
            out[k] = np.where(var == 0, LD(np.nan), out[k])
    return out


# ---- the float64 composition, with one defect when asked ------------------------------------------------------------------------
MES_MUTANTS = {
    "erfc-log": "h and h' composed from erfc, exp and log everywhere (no continued fraction)",
    "mean-ystar": "h of the mean y* instead of the mean of h",
    "no-half": "h = gamma lambda - log Phi",
    "flip-sign": "gamma with the opposite sign",
    "abs-b": "sgn(var) dropped from b",
}


def terms_f64(g, mutant=None):
    """(h, h') in float64: mes_h of acq.hip restated in NumPy, operation for operation but for the fused multiply-adds the device
    compiler may form; it also defines the special values."""
    g = np.asarray(g, dtype=float)
    half = 1.0 if mutant == "no-half" else 0.5
    with np.errstate(all="ignore"):
        t = -g * np.sqrt(0.5)
        cf = (t >= T0) & (mutant != "erfc-log")
        tt = np.where(cf, t, T0)
        f = tt.copy()
        for k in range(CF_TERMS, 2, -1):
            f = tt + (0.5 * k) / f
        C2 = 1.0 / f
        den = tt + C2
        w, td = C2 / den, tt + 0.5 / den
        h_cf = np.log(3.54490770181103205460 * td) - half * (1.0 - w)
        hp_cf = -(np.sqrt(0.5) * td) * w
        comp = ~cf & (g <= G_ZERO)
        gm = np.where(comp, g, 0.0)
        p, e = _two_prod_f64(gm)
        E = np.exp(-0.5 * p)
        phi = (E - 0.5 * e * E) * 0.39894228040143267794
        Q = 0.5 * _erfc(np.abs(gm) * np.sqrt(0.5))
        neg = gm <= 0.0
        lam = phi / np.where(neg, Q, 1.0 - Q)
        h_c = half * gm * lam - np.where(neg, np.log(Q), np.log1p(-Q))
        hp_c = -0.5 * lam * (1.0 + gm * (gm + lam))
        zero = np.where(g > G_ZERO, 0.0, np.nan)
        return np.where(cf, h_cf, np.where(comp, h_c, zero)), np.where(cf, hp_cf, np.where(comp, hp_c, zero))


_erfc = np.vectorize(math.erfc, otypes=[float])      # the C library's: SciPy's gives 0 beyond 26.6 (acq_ref.flushed_early), where
#                                                       erfc is a subnormal double up to 27.2


def _two_prod_f64(x):
    """(p, e) with x x = p + e exactly (Dekker's split; |x| <= 40 here)."""
    p = x * x
    c = 134217729.0 * x
    hi = c - (c - x)
    lo = x - hi
    return p, ((hi * hi - p) + 2.0 * hi * lo) + lo * lo


def costs_f64_mes(ystar, sign, mean, var, mutant=None):
    """(A, a, b) in float64: mes_cost of acq.hip restated (the sums in the order k = 0 .. K-1); `mutant`: one of MES_MUTANTS."""
    mean, var = np.asarray(mean, dtype=float), np.asarray(var, dtype=float)
    y = np.asarray(ystar, dtype=float).ravel()
    if mutant == "mean-ystar":
        y = np.array([np.mean(y)])
    sgn = -sign if mutant == "flip-sign" else sign
    K = float(y.size)
    with np.errstate(all="ignore"):
        s = np.sqrt(np.abs(var)) * np.ones_like(mean + var)
        sg = np.ones_like(s) if mutant == "abs-b" else np.sign(var) * np.ones_like(s)
        sh, shp, shg = np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)
        for yk in y:
            g = ((mean - yk) if sgn > 0 else (yk - mean)) / s
            h, hp = terms_f64(g, mutant)
            sh, shp, shg = sh + h, shp + hp, shg + hp * g
        a = -(sgn / (K * s)) * shp
        b = (sg / (2.0 * K * s * s)) * shg
        a, b = np.where(var == 0, np.nan, a), np.where(var == 0, np.nan, b)
        return -(sh / K), a, b


# ---- the epilogue's own bound --------------------------------------------------------------------------------------------------------
def epilogue_bound_mes(ystar, sign, mu, var):
    """dict(A, a, b): bounds on |device - exact| of mes_cost's three results at float64 inputs taken as exact -- first order in u,
    doubled for the second-order terms, with DENORMAL_STEP wherever a result or an intermediate may be subnormal (acq_ref.
    epilogue_bound's rules).  Each basic operation has relative error u; erfc 32 u, exp 6 u, log 6 u, log1p 4 u.  Per sample k:
        s = sqrt(|var|), g = (mu - y) / s                 dg <= 3 u |g|
      t = -g / sqrt 2 >= T0 (the continued fraction):     dt <= 5 u t                      (dg, the constant, the product)
        f (backward, a division and a sum per level)      own rounding <= 4 u f: the level k passes theta_k = (k / 2) / (f_k f_k+1) of
                                                          the error below it on, theta <= 1/2 for k <= 8 at t >= 2, so the 7 u a deep
                                                          level may carry arrive below u, beside 2 u of the top levels; and
                                                          0 < df/dt <= 1 with f >= t, so dt moves f by at most 5 u f
        C2 = 1 / f                                        dC2 <= 10 u C2
        den = t + C2                                      dden <= 11 u den
        w = C2 / den                                      dw <= 22 u w
        td = t + 0.5 / den                                dtd <= 13 u td
        h = log(c td) - 0.5 (1 - w)                       dh <= 15 u + 6 u |log| + 0.5 (dw + u) + u |h|
        h' = -(td / sqrt 2) w                             dh' <= 38 u |h'|
      else, g <= 40 (the composition):
        Q = 0.5 erfc(|g| / sqrt 2)                        dQ <= phi |g| 5 u + 33 u Q         (acq_ref's dPhi)
        phi = exp(-p / 2) (1 - e / 2) / sqrt(2 pi)        dphi <= phi (3 g^2 u + 9 u)        (g^2 = p + e exactly: only dg enters)
        P = Q or 1 - Q;  lam = phi / P                    dP <= dQ + u P;  dlam <= (dphi + lam dP) / P + u lam
        L = log Q or log1p(-Q)                            dL <= dQ / P + 6 u |L| or 4 u |L|
        h = 0.5 g lam - L                                 dh <= 0.5 (|g| dlam + lam dg) + u |g| lam + dL + u |h|
        z1 = g + lam, z2 = g z1, z3 = 1 + z2              dz1 <= dg + dlam + u |z1|, dz2 <= |g| dz1 + |z1| dg + u |z2|, dz3 <= dz2 + u |z3|
        h' = -0.5 lam z3                                  dh' <= 0.5 (lam dz3 + |z3| dlam) + 2 u |h'|
      else h = h' = 0 exactly (Q and phi are below half the smallest subnormal).
    The sums (K - 1 additions each) and the results:
        A = -(sum h) / K                                  dA <= (sum dh + (K - 1) u sum |h|) / K + 2 u |A|
        a = -(sign / (K s)) sum h'                        da <= (sum dh' + (K - 1) u sum |h'|) / (K s) + 4 u |a|
        b = (sg / (2 K s s)) sum h' g                     db <= (sum (|g| dh' + |h'| dg + u |h' g|) + (K - 1) u sum |h' g|) / (2 K s^2) + 6 u |b|"""
    ref = reference_costs_mes(ystar, sign, np.asarray(mu, dtype=float), np.asarray(var, dtype=float), second=False)
    K = float(np.asarray(ystar).size)
    with np.errstate(all="ignore"):
        f = lambda x: np.abs(np.asarray(x, dtype=float))
        g, h, hp, s = f(ref["g"]), f(ref["h"]), f(ref["hp"]), f(ref["s"])
        gs = np.asarray(ref["g"], dtype=float)
        dg = 3.0 * U * g + DS
        # the continued fraction
        t = g * np.sqrt(0.5)
        C2, den = (np.asarray(x, dtype=float) for x in _cf_ld(np.where(np.isfinite(t) & (t >= 0.5), t, 1.0).astype(LD), CF_TERMS))
        w = C2 / den
        dh_cf = 15.0 * U + 2.0 * LOG_ULP * U * (h + 0.5) + 0.5 * (22.0 * U * w + U) + U * h + DS
        dhp_cf = 38.0 * U * hp + DS
        # the composition
        phi = f(A.phi_ld(ref["g"]))
        Q = f(A._upper_tail(np.abs(ref["g"])))
        neg = gs <= 0
        P = np.where(neg, Q, 1.0 - Q)
        lam = phi / P
        dQ = phi * g * 5.0 * U + (2.0 * A.ERFC_ULP + 1.0) * U * Q + DS
        dphi = phi * (3.0 * g * g * U + (2.0 * A.EXP_ULP + 3.0) * U) + DS
        dP = dQ + U * P
        dlam = (dphi + lam * dP) / P + U * lam
        L = np.where(neg, f(np.log(Q)), f(np.log1p(-Q)))
        dL = dQ / P + np.where(neg, 2.0 * LOG_ULP, 2.0 * LOG1P_ULP) * U * L
        dh_c = 0.5 * (g * dlam + lam * dg) + U * g * lam + dL + U * h + DS
        z1 = f(gs + lam)
        z3 = f(1.0 + gs * (gs + lam))
        dz1 = dg + dlam + U * z1
        dz2 = g * dz1 + z1 * dg + U * g * z1
        dz3 = dz2 + U * z3
        dhp_c = 0.5 * (lam * dz3 + z3 * dlam) + 2.0 * U * hp + DS
        cf = (gs < 0) & (t >= T0 * (1.0 - 8.0 * U))                      # (at the seam the device may take either branch:
        comp_ok = ~((gs < 0) & (t >= T0 * (1.0 + 8.0 * U)))              #  the larger bound serves both)
        dh = np.where(cf & comp_ok, np.maximum(dh_cf, dh_c), np.where(cf, dh_cf, dh_c))
        dhp = np.where(cf & comp_ok, np.maximum(dhp_cf, dhp_c), np.where(cf, dhp_cf, dhp_c))
        far = gs > G_ZERO
        dh, dhp = np.where(far, DS, dh), np.where(far, DS, dhp)
        A_, a, b = f(ref["A"]), f(ref["a"]), f(ref["b"])
        dA = (np.sum(dh, axis=0) + (K - 1.0) * U * np.sum(h, axis=0)) / K + 2.0 * U * A_
        da = (np.sum(dhp, axis=0) + (K - 1.0) * U * np.sum(hp, axis=0)) / (K * s) + 4.0 * U * a
        db = (np.sum(g * dhp + hp * dg + U * hp * g, axis=0) + (K - 1.0) * U * np.sum(hp * g, axis=0)) / (2.0 * K * s * s) + 6.0 * U * b
        return dict(A=2.0 * dA + DS, a=2.0 * da + DS, b=2.0 * db + DS)


# ---- acq_ref's metrics for the MES cost -------------------------------------------------------------------------------------------
@contextlib.contextmanager
def acq_ref_for_mes(ystar, sign, mutant=None):
    """Inside the block acq_ref's three cost-specific functions (reference_costs, epilogue_bound, costs_f64; their `acq` and `param`
    arguments are then unused) are the MES ones on (ystar, sign): everything acq_ref builds on them -- cost_reference, omega_A, the
    comparators, grad_reference / route_grad, the batch replay and its comparators, the regret rule -- judges the MES cost without
    a second copy, and acq_ref.py stays as it is.  `mutant`: one defect of MES_MUTANTS in the float64 comparator.
    The stand-ins keep the originals' signatures (names and defaults, so a keyword call works too), and the block refuses to start
    unless every user inside acq_ref resolves the three names through acq_ref's own globals -- a `from acq_ref import costs_f64`
    elsewhere would keep the closed-form cost, and has to go through this module instead."""
    default = mutant
    users = (A.cost_reference, A.route_costs, A.route_grad, A.grad_reference, A.batch_reference, A.batch_refit_rows, A.batch_rank1_rows)
    assert all(f.__globals__ is vars(A) for f in users), "acq_ref's metrics no longer read their cost functions from acq_ref's globals"
    saved = A.reference_costs, A.epilogue_bound, A.costs_f64

    def reference_costs(acq, param, mu_ld, var_ld):
        return reference_costs_mes(ystar, sign, mu_ld, var_ld)

    def epilogue_bound(acq, param, mu, var):
        return epilogue_bound_mes(ystar, sign, mu, var)

    def costs_f64(acq, param, mean, var, mutant=None):
        return costs_f64_mes(ystar, sign, mean, var, mutant if mutant in MES_MUTANTS else default)

    A.reference_costs, A.epilogue_bound, A.costs_f64 = reference_costs, epilogue_bound, costs_f64
    try:
        yield A
    finally:
        A.reference_costs, A.epilogue_bound, A.costs_f64 = saved


MES = "mes"            # the `acq` handed to acq_ref's functions inside acq_ref_for_mes (never compared with UCB / PI / EI there)


# ---- made-to-order rows for the epilogue alone ----------------------------------------------------------------------------------
EPI_K = (1, 3, 17)


def ystar_of(K):
    """K sampled optima around 0: 0 first (so gamma_0 walks the grid), then fixed values in (-1, 1) on a 2^-10 grid."""
    rng = np.random.default_rng(4100 + K)
    return np.concatenate([[0.0], np.round(rng.uniform(-1.0, 1.0, K - 1) * 1024.0) / 1024.0])


def g_grid_mes():
    """acq_ref.g_grid (-38.6 .. 9) and the reaches of this cost: -1e150, -1e6, -1e3, -100, the seam -T0 sqrt 2 -+ 1e-9, 20, 37,
    38.5, 38.6."""
    seam = -T0 * np.sqrt(2.0)
    return np.unique(np.concatenate([A.g_grid(), [-1e150, -1e6, -1e3, -100.0, seam - 1e-9, seam + 1e-9, seam, 20.0, 37.0, 38.5, 38.6]]))


def epilogue_pool_mes(sign):
    """(mean, var): mean = sign g s over g_grid_mes for each var of acq_ref.EPI_VARS (gamma_0 = g with y*_0 = 0; the other y* put
    gamma_k at g -+ O(1) for var = 1 and at -+1e150 for var = 1e-300), then acq_ref's special rows."""
    g = g_grid_mes()
    mean = np.concatenate([sign * g * np.sqrt(v) for v in A.EPI_VARS])
    var = np.concatenate([np.full(g.size, v) for v in A.EPI_VARS])
    sm, sv = A.epilogue_pool()
    n = A.g_grid().size * len(A.EPI_VARS)
    return np.concatenate([mean, sm[n:]]), np.concatenate([var, sv[n:]])


def epilogue_rows_mes(m, sign):
    """The pool cut into rows of m candidates (the last row wraps round); m == 1: every seventh candidate and the special ones."""
    mean, var = epilogue_pool_mes(sign)
    n = mean.size
    if m == 1:
        idx = sorted(set(range(0, n, 7)) | set(range(n - 21, n)))
        return [(mean[i:i + 1], var[i:i + 1]) for i in idx]
    return [(np.take(mean, np.arange(r, r + m), mode="wrap"), np.take(var, np.arange(r, r + m), mode="wrap")) for r in range(0, n, m)]


def ystar_cases(y):
    """{name: y* (3,)} of a case, for sampled minima: at, below and above min y (by a tenth and a whole spread of y)."""
    lo, spread = float(np.min(y)), float(np.max(y) - np.min(y))
    return {"at min y": np.array([lo, lo - 0.1 * spread, lo + 0.1 * spread]),
            "below min y": np.array([lo - spread, lo - 0.5 * spread, lo - 0.1 * spread]),
            "above min y": np.array([lo + 0.1 * spread, lo + 0.3 * spread, lo + 0.5 * spread])}
