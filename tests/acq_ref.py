"""Per-candidate error metrics, longdouble references, float64 comparators and mutants for the Bayesian-optimisation costs UCB, PI and
EI of gpexp_amd/csrc/acq.hip (NumPy / SciPy only; data and references of tests/test_acq_host.py and tests/test_gpu_acq_bounds.py, not
product code).  Same conventions as tests/posterior_ref.py, whose cases, longdouble solves and comparators it carries through the
cost epilogue.

THE COSTS.  mu the posterior mean, var the SIGNED variance, s = sqrt(|var|), g = (param - mu) / s, Phi the normal distribution
function, phi its density:
    UCB  A = -(mu - kappa s)       a = dA/dmu = -1        b = dA/dvar = kappa sgn(var) / (2 s)
    PI   A = -Phi(g)               a = phi / s            b = phi g sgn(var) / (2 s^2)
    EI   A = -s (g Phi + phi)      a = Phi                b = -phi sgn(var) / (2 s)
a = b = NaN where var == 0 exactly (acq.hip's contract).  PI and EI are tails: at g = -38 they are 1e-300 of the vector's maximum,
and max|x - y| / max|y| gives them no digits.

THE EPILOGUE'S OWN BOUND R (epilogue_bound): first-order rounding of acq_cost alone, float64 inputs taken as exact; derivation in
its docstring.  The library constants are FIXED: erfc 16 ulp, exp 3 ulp (the OpenCL double-precision ceilings the ROCm device library
documents itself to); one ulp is at most 2 u.

THE END-TO-END METRIC.  With S_m, S_v of posterior_ref (the first-order effect on mean and variance of a relative perturbation u of
every input entry), per candidate j
    omega_A = max_j |got_j - ref_j| / (u S_A,j),        S_A,j = |a_j| S_m,j + |b_j| S_v,j + R_j / u
so a candidate whose EI is 1e-200 is judged to the digits its posterior and the epilogue determine.  From points the error counts in
excess of |a| A_m + |b| A_v (posterior_ref's allowances).  THE BOUND: device omega_A <= MARGIN (= 8) x the larger COMPARATOR on
the same arrays: posterior_ref.route_values("lapack" | "b128") followed by the float64 epilogue bo_compose.costs.  Never a device
result.  No candidate is left out: underflowed and saturated ones are judged with the DENORMAL_STEP term of R."""
import numpy as np
import scipy.special as sps

import bo_compose as BC
import design_replay_ref as DR           # (its import fails where np.longdouble is plain float64)
import kernel_reference as KR
import posterior_ref as P
from chol_stability_ref import MARGIN, U, check_bound   # noqa: F401  (re-exported)

LD = DR.LD
UCB, PI, EI = BC.UCB, BC.PI, BC.EI
ACQS = {"ucb": UCB, "pi": PI, "ei": EI}
KAPPA = 2.0
DS = KR.DENORMAL_STEP
ERFC_ULP, EXP_ULP = 16.0, 3.0            # FIXED (see epilogue_bound); one ulp <= 2 u
CASE_NAMES = ("se-well", "se-tiny-noise", "m52-tiny-noise", "m32-per-point")

_PI_LD = LD("3.14159265358979323846264338327950288419716939937510")
_SQRT_PI = np.sqrt(_PI_LD)
_SQRT_2PI = np.sqrt(LD(2) * _PI_LD)
_SQRT_HALF = np.sqrt(LD(1) / LD(2))
_X_SMALL = LD(1) / LD(2)       # |x| below: the series of erf; above: the continued fraction of erfc
_CF_TERMS = 1200               # backward terms of the continued fraction: at x = 1/2 the value no longer moves with more (host test)


# ---- Phi and phi in longdouble ------------------------------------------------------------------------------------------------
def _exp_neg_half_sq(g):
    """e^(-g^2 / 2) with g^2 formed exactly (hi + lo, Dekker): a rounded argument would cost g^2 2^-64 relative, 0.2 u at g = -38."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        gf = np.where(np.isfinite(g), g, LD(0))
        p, e = DR._two_prod(gf, gf)
        out = np.exp(-p / LD(2)) * (LD(1) - e / LD(2))
        return np.where(np.isinf(g), LD(0), np.where(np.isnan(g), LD(np.nan), out))


def _erf_series(x):
    """erf(x) = 2 / sqrt(pi) e^(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 .. (2n+1)): positive terms only, |x| <= 1/2."""
    x2 = x * x
    term = np.array(x, dtype=LD)
    acc = term.copy()
    for n in range(1, 80):
        term = term * (LD(2) * x2 / LD(2 * n + 1))
        acc = acc + term
    return LD(2) / _SQRT_PI * np.exp(-x2) * acc


def _erfcx_cf(x):
    """erfc(x) e^(x^2) = 1 / (sqrt(pi) (x + (1/2) / (x + 1 / (x + (3/2) / (x + ..))))), x >= 1/2, evaluated backward."""
    f = np.array(x, dtype=LD)
    for k in range(_CF_TERMS, 0, -1):
        f = x + (LD(k) / LD(2)) / f
    return LD(1) / (_SQRT_PI * f)


def _upper_tail(t):
    """Q(t) = 1 - Phi(t) for t >= 0 (longdouble), to a few 2^-64 relative."""
    t = np.asarray(t, dtype=LD)
    x = t * _SQRT_HALF
    small = x < _X_SMALL
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        lo = (LD(1) - _erf_series(np.where(small, x, LD(0)))) / LD(2)
        hi = _exp_neg_half_sq(t) * _erfcx_cf(np.where(small | ~np.isfinite(x), LD(1), x)) / LD(2)
    return np.where(small, lo, np.where(np.isinf(t), LD(0), hi))


def erfc_ld(x):
    """erfc in longdouble (series below |x| = 1/2, continued fraction above, x^2 formed exactly); exact 0 / 2 at +-inf, NaN for NaN."""
    x = np.asarray(x, dtype=LD)
    ax = np.abs(x)
    small = ax < _X_SMALL
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        p, e = DR._two_prod(np.where(np.isfinite(ax), ax, LD(0)), np.where(np.isfinite(ax), ax, LD(0)))
        hi = np.exp(-p) * (LD(1) - e) * _erfcx_cf(np.where(small | ~np.isfinite(ax), LD(1), ax))
        q = np.where(small, LD(1) - _erf_series(np.where(small, ax, LD(0))), np.where(np.isinf(ax), LD(0), hi))
    return np.where(np.isnan(x), LD(np.nan), np.where(x >= 0, q, LD(2) - q))


def Phi_ld(g):
    """The normal distribution function in longdouble: 0.5 erfc(-g / sqrt 2) with erfc written here, a few 2^-64 relative over
    -38.6 <= g <= 9 (tests/test_acq_host.py pins it against 50 digits); exactly 0 / 1 at -inf / +inf, NaN for NaN."""
    g = np.asarray(g, dtype=LD)
    q = _upper_tail(np.abs(g))
    return np.where(np.isnan(g), LD(np.nan), np.where(g <= 0, q, LD(1) - q))


def phi_ld(g):
    """The normal density in longdouble (the square formed exactly)."""
    return _exp_neg_half_sq(np.asarray(g, dtype=LD)) / _SQRT_2PI


# ---- the reference values -------------------------------------------------------------------------------------------------------
def reference_costs(acq, param, mu_ld, var_ld):
    """dict(A, a, b, a_mu, a_var, b_mu, b_var, g, s, Phi, phi) in longdouble from the mean and the SIGNED variance: the cost, its
    derivatives a = dA/dmu and b = dA/dvar (b carries sgn(var)), and their derivatives in closed form.  The edges are the float64
    composition's (bo_compose.costs): the formulas are evaluated as written, so EI at var == 0 and any NaN input give NaN; a = b =
    NaN where var == 0 exactly (acq.hip's contract)."""
    mu, var = np.asarray(mu_ld, dtype=LD), np.asarray(var_ld, dtype=LD)
    p = LD(param)
    one = np.ones(np.broadcast(mu, var).shape, dtype=LD)
    with np.errstate(all="ignore"):
        s = np.sqrt(np.abs(var)) * one
        sg = np.sign(var) * one
        if acq == UCB:
            out = dict(A=-(mu - p * s), a=-one, b=p * sg / (LD(2) * s), a_mu=0 * one, a_var=0 * one, b_mu=0 * one,
                       b_var=-p / (LD(4) * s ** 3), g=0 * one, Phi=0 * one, phi=0 * one)
        else:
            g = (p - mu) / s
            Phi, phi = Phi_ld(g), phi_ld(g)
            if acq == PI:
                out = dict(A=-Phi, a=phi / s, b=phi * g * sg / (LD(2) * s * s), a_mu=g * phi / (s * s),
                           a_var=phi * sg * (g * g - LD(1)) / (LD(2) * s ** 3), b_var=phi * g * (g * g - LD(3)) / (LD(4) * s ** 4))
            else:
                out = dict(A=-s * (g * Phi + phi), a=Phi, b=-phi * sg / (LD(2) * s), a_mu=-phi / s,
                           a_var=-phi * g * sg / (LD(2) * s * s), b_var=-phi * (g * g - LD(1)) / (LD(4) * s ** 3))
            out["b_mu"] = out["a_var"]
            out.update(g=g, Phi=Phi, phi=phi)
        zero = (var == 0) * (one == one)
        for k in ("a", "b"):
            out[k] = np.where(zero, LD(np.nan), out[k])
        out["s"] = s
    return out


# ---- the float64 epilogue, with one defect when asked ---------------------------------------------------------------------------
EPILOGUE_MUTANTS = {
    "erf-form": "Phi as 0.5 (1 + erf(g / sqrt 2))",
    "phi-f32": "phi through float32",
    "abs-b": "sgn(var) dropped from b",
    "ei-no-phi": "EI as -s g Phi",
}


def flushed_early(g):
    """Where scipy.stats.norm.cdf gives 0 although Phi is a (subnormal) double: SciPy's ndtr gives up where g^2 / 2 exceeds log(DBL_MAX)
    = 709.78, that is below g = -37.68; Phi reaches half the smallest subnormal at -38.49 only."""
    g = np.asarray(g, dtype=float)
    with np.errstate(all="ignore"):
        return np.isfinite(g) & (g < -37.6) & (BC.spstats.norm.cdf(g) == 0.0) & (np.asarray(Phi_ld(g), dtype=float) >= DS)


def cdf_f64(g):
    """scipy.stats.norm.cdf, bit for bit, except where it flushes early (flushed_early): there 0.5 erfc(-g / sqrt 2) of the C library,
    which serves the subnormal range.  A comparator that returns 0 for 1e-310 scores 1e9 in omega_A and would void the bound."""
    import math
    g = np.asarray(g, dtype=float)
    with np.errstate(all="ignore"):
        Phi = np.array(BC.spstats.norm.cdf(g), dtype=float)
        for i in zip(*np.nonzero(flushed_early(g))):
            Phi[i] = 0.5 * math.erfc(-g[i] * math.sqrt(0.5))
    return Phi


def costs_f64(acq, param, mean, var, mutant=None):
    """(A, a, b) in float64: bo_compose.costs (bit for bit without a mutant, but for cdf_f64's window) and the (a, b) of
    bo_compose.DenseModel.grad, NaN where var == 0 exactly; `mutant` names one defect of EPILOGUE_MUTANTS."""
    mean, var = np.asarray(mean, dtype=float), np.asarray(var, dtype=float)
    with np.errstate(all="ignore"):
        s = np.sqrt(np.abs(var))
        sg = np.ones_like(var) if mutant == "abs-b" else np.sign(var)
        if acq == UCB:
            A, a, b = -(mean - param * s), -np.ones_like(s + mean), param * sg / (2.0 * s)
        else:
            g = (param - mean) / s
            Phi = 0.5 * (1.0 + sps.erf(g * np.sqrt(0.5))) if mutant == "erf-form" else cdf_f64(g)
            phi = BC.spstats.norm.pdf(g)
            if mutant == "phi-f32":
                phi = (np.exp((-0.5 * g * g).astype(np.float32)) * np.float32(0.3989422804014327)).astype(float)
            if acq == PI:
                A, a, b = -Phi, phi / s, phi * g * sg / (2.0 * s * s)
            else:
                A, a, b = -s * (g * Phi + (0.0 if mutant == "ei-no-phi" else phi)), Phi, -phi * sg / (2.0 * s)
        a, b = np.where(var == 0, np.nan, a), np.where(var == 0, np.nan, b)
    return A, a, b


# ---- the epilogue's own bound ------------------------------------------------------------------------------------------------------
def epilogue_bound(acq, param, mu, var):
    """dict(A, a, b): bounds R on |device - exact| of acq_cost's three results at float64 inputs (mu, var) taken as exact -- first
    order in u = 2^-53, doubled for the second-order terms, every term with kernel_reference.DENORMAL_STEP for a result or an
    intermediate in the subnormal range.  A bound, so its own rounding is beside the point (float64).

    The device's operations (acq.hip, acq_cost), each basic one (+ - * / sqrt) with relative error u:
        s = sqrt(|var|)                               ds  <= u s
        g = (param - mu) / s                          dg  <= 3 u |g|                        (subtraction, s, division)
        x = -g * M_SQRT1_2                            dx  <= 5 u |x|                        (dg, the constant's rounding, the product)
        Phi = 0.5 erfc(x)      |dPhi/dg| = phi        dPhi <= phi |g| 5 u + (32 + 1) u Phi  (erfc: 16 ulp = 32 u; one u of slack for
                                                                                             the halving next to a subnormal)
        t = -0.5 g g                                  dt  <= |g| dg + u g^2 / 2 = 3.5 g^2 u
        phi = exp(t) * 0.3989..                       dphi <= phi (3.5 g^2 u + (6 + 2) u)   (exp: 3 ulp = 6 u; the constant, the product)
        UCB  A = -(mu - kappa s)                      dA  <= 2 u |kappa| s + u |A|
        PI   A = -Phi                                 dA  <= dPhi
        EI   A = -s (g Phi + phi)                     dA  <= s [|g| dPhi + Phi dg + dphi + 2 u (|g| Phi + phi)] + 2 u |A|
                                                           (the two roundings inside the bracket: u |g Phi| + u |g Phi + phi|;
                                                            outside it: ds and the product)
        UCB  a = -1, b = kappa sgn / (2 s)            da = 0,  db <= 2 u |b|
        PI   a = phi / s                              da  <= dphi / s + 2 u |a|
             b = phi g sgn / (2 s s)                  db  <= (|g| dphi + phi dg) / (2 s^2) + 5 u |b|
        EI   a = Phi                                  da  <= dPhi
             b = -phi sgn / (2 s)                     db  <= dphi / (2 s) + 2 u |b|
    EI cancels like 1 / g^2 in the tail (g Phi + phi ~ phi / g^2): the bound is absolute in phi, so the device may lose the digits
    the cancellation costs and no more.  The library constants are fixed, not measured: 16 ulp for erfc and 3 ulp for exp are the
    OpenCL double-precision ceilings the ROCm device library documents itself to."""
    ref = reference_costs(acq, param, np.asarray(mu, dtype=float), np.asarray(var, dtype=float))
    with np.errstate(all="ignore"):
        f = {k: np.abs(np.asarray(v, dtype=float)) for k, v in ref.items()}
        s, g, Phi, phi, A = f["s"], f["g"], f["Phi"], f["phi"], f["A"]
        if acq == UCB:
            dA = 2.0 * U * abs(param) * s + U * A
            da, db = np.zeros_like(s), 2.0 * U * f["b"]
        else:
            dg = 3.0 * U * g + DS
            dPhi = phi * g * 5.0 * U + (2.0 * ERFC_ULP + 1.0) * U * Phi + DS
            dphi = phi * (3.5 * g * g * U + (2.0 * EXP_ULP + 2.0) * U) + DS
            if acq == PI:
                dA = dPhi
                da = dphi / s + 2.0 * U * f["a"]
                db = (g * dphi + phi * dg) / (2.0 * s * s) + 5.0 * U * f["b"]
            else:
                dA = s * (g * dPhi + Phi * dg + dphi + 2.0 * U * (g * Phi + phi) + DS) + 2.0 * U * A
                da = dPhi
                db = dphi / (2.0 * s) + 2.0 * U * f["b"]
        return dict(A=2.0 * dA + DS, a=2.0 * da + DS, b=2.0 * db + DS)


def judged(ref_value, bound):
    """Where a result is held to its bound: the reference and the bound both finite.  Elsewhere the float64 composition's pattern
    (NaN, zero, infinity) is required exactly."""
    return np.isfinite(np.asarray(ref_value, dtype=float)) & np.isfinite(bound)


def bound_ratio(got, ref_value, bound, where):
    """max |got - ref| / bound over `where` (inf when a judged value is not finite)."""
    if not np.any(where):
        return 0.0
    with np.errstate(all="ignore"):
        q = np.asarray(np.abs(np.asarray(got, dtype=LD) - ref_value)[where] / np.asarray(bound, dtype=LD)[where], dtype=float)
    return float(np.max(q)) if np.all(np.isfinite(q)) else float("inf")


def same_pattern(got, want):
    """Bit-for-bit agreement of the special values: NaN where NaN, and equal (as numbers) elsewhere."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]))


# ---- made-to-order rows for the epilogue alone ----------------------------------------------------------------------------------
EPI_SIZES = (1, 127, 128, 129, 257)
EPI_VARS = (1.0, 1e-6, 1e-300, 4.0)        # sqrt(1e-300) = 1e-150: s, g and s s stay clear of the subnormal range


def g_grid():
    """g from -38.6 to 9: every 0.1 around -38 (Phi and phi enter the subnormal range at -37.5 / -38.5), dense around 0, 0.5 apart
    from -5 to 9, 14 points across the tail between."""
    return np.unique(np.concatenate([np.arange(-386, -375) / 10.0, np.linspace(-37.0, -6.0, 14), np.arange(-10, 19) / 2.0,
                                     [-0.1, -1e-3, -1e-8, 1e-8, 1e-3, 0.1]]))


def epilogue_pool():
    """(mean, var) of every made-to-order candidate, param = 0: mean = -g s over g_grid for each var of EPI_VARS, then the special
    rows (var < 0, var == +-0, var = inf, mean NaN / +-inf, param == mean, NaN variance)."""
    g = g_grid()
    mean = np.concatenate([-g * np.sqrt(v) for v in EPI_VARS])
    var = np.concatenate([np.full(g.size, v) for v in EPI_VARS])
    special = [(0.3, -1.0), (-2.0, -4.0), (-7e-3, -1e-6), (3.0, -1.0), (0.5, 0.0), (-0.5, 0.0), (0.5, -0.0), (-0.5, -0.0), (0.0, 0.0),
               (0.0, -0.0), (1.0, np.inf), (-1.0, np.inf), (0.0, np.inf), (np.nan, 1.0), (np.nan, 0.0), (1.0, np.nan), (np.inf, 1.0),
               (-np.inf, 1.0), (0.0, 1.0), (0.0, 1e-300), (np.inf, np.inf)]
    sm, sv = np.array(special).T
    return P._ro(np.concatenate([mean, sm])), P._ro(np.concatenate([var, sv]))


def epilogue_rows(m):
    """The pool cut into rows of m candidates (the last row wraps round); m == 1: every fifth candidate and all the special ones."""
    mean, var = epilogue_pool()
    n = mean.size
    if m == 1:
        idx = sorted(set(range(0, n, 5)) | set(range(n - 21, n)))
        return [(mean[i:i + 1], var[i:i + 1]) for i in idx]
    return [(np.take(mean, np.arange(r, r + m), mode="wrap"), np.take(var, np.arange(r, r + m), mode="wrap")) for r in range(0, n, m)]


def argmin_rows(m):
    """[(label, mean, var)] for the arg-min of a row of m candidates (UCB, kappa = 2, cost = 2 s - mean): the minimum repeated bit
    for bit at candidates 1, 127, 128 and m - 1 (those inside the row), NaN at candidate 0 and inside the second block, and a row
    of nothing but NaN."""
    rng = np.random.default_rng(900 + m)
    mean, var = rng.uniform(-1.0, 1.0, m), rng.uniform(0.5, 2.0, m)
    ties = sorted({i for i in (1, 127, 128, m - 1) if 0 <= i < m})
    mean[ties], var[ties] = 3.0, 0.25
    rows = [("ties at %s" % ties, mean.copy(), var.copy())]
    mean[0] = np.nan
    if m > 130:
        mean[130] = np.nan
    rows.append(("NaN at candidate 0 and in the second block", mean.copy(), var.copy()))
    if m > 1:
        late = mean.copy()
        late[ties[:-1]] = 0.0          # the minimum at the last candidate only
        rows.append(("the minimum at the last candidate", late, var.copy()))
    rows.append(("all NaN", np.full(m, np.nan), var.copy()))
    return rows


# ---- the end-to-end metric ---------------------------------------------------------------------------------------------------------
def params_of(y):
    """{name: param} of a case: fBest (PI, EI) as the largest, the median and the smallest observation."""
    return {"max y": float(np.max(y)), "median y": float(np.median(y)), "min y": float(np.min(y))}


def param_for(acq, p):
    return KAPPA if acq == UCB else p


def cost_reference(acq, param, ref):
    """The longdouble costs of a posterior_ref reference (its val["m"], val["v"], scale, and allow when built from points):
    dict(val = reference_costs(..), S = S_A per candidate (float64), allow = |a| A_m + |b| A_v or None, R)."""
    mu, var = ref["val"]["m"], ref["val"]["v"]
    val = reference_costs(acq, param, mu, var)
    R = epilogue_bound(acq, param, np.asarray(mu, dtype=float), np.asarray(var, dtype=float))
    a, b = np.abs(np.asarray(val["a"], dtype=float)), np.abs(np.asarray(val["b"], dtype=float))
    S = a * ref["scale"]["m"] + b * ref["scale"]["v"] + R["A"] / U
    allow = a * ref["allow"]["m"] + b * ref["allow"]["v"] if "allow" in ref else None
    return dict(val=val, S=S, allow=allow, R=R)


def omega_A(got, cref, allowance=True):
    """max_j |got_j - ref_j| / (u S_A,j) over ALL candidates, the error in excess of the allowance when the reference has one."""
    return P.omega(got, cref["val"]["A"], cref["S"], cref["allow"] if allowance else None)


ROUTE_MUTANTS = ("last-row", "tile-seam")      # posterior_ref's, carried through the epilogue
COST_MUTANTS = {                               # name -> the costs it is judged in
    "erf-form": (PI, EI), "phi-f32": (EI,), "ei-no-phi": (EI,), "last-row": (UCB, PI, EI), "tile-seam": (UCB, PI, EI),
}
REL_BLIND = ("erf-form", "phi-f32", "last-row", "tile-seam")    # pass max|x - y| / max|y| <= 1e-10 (asserted on the host)


def route_costs(route, acq, param, K, B, kd, alpha, mutant=None):
    """The float64 costs of a comparator: posterior_ref.route_values, then bo_compose.costs (as costs_f64 restates it); `mutant`: one defect, of the route
    (ROUTE_MUTANTS) or of the epilogue (EPILOGUE_MUTANTS)."""
    pv = P.route_values(route, K, B, kd, alpha=alpha, mutant=mutant if mutant in ROUTE_MUTANTS else None)
    return costs_f64(acq, param, pv["m"], pv["v"], mutant if mutant in EPILOGUE_MUTANTS else None)[0], pv


def comparator_omegas(acq, param, cref, K, B, kd, alpha):
    """{route: omega_A} of the comparators on the same arrays as the reference (never with an allowance: they start from the
    arrays the reference starts from, rounded once)."""
    return {route: omega_A(route_costs(route, acq, param, K, B, kd, alpha)[0], cref, allowance=False) for route in P.ROUTES}


def regret(cref, best, top):
    """(shortfall, allowed) of a pick: ref_cost[best] - min_j ref_cost_j, against 2 u MARGIN top S_A,best -- `top` the larger
    comparator omega_A: the device's pick is the reference's, or indistinguishable from it within the bound."""
    A = cref["val"]["A"]
    short = float(A[best] - np.min(A[~np.isnan(np.asarray(A, dtype=float))]))
    return short, 2.0 * U * MARGIN * top * float(cref["S"][best])


def check_regret(label, cref, best, top):
    short, allowed = regret(cref, best, top)
    print("  %-34s pick %d: reference cost above the reference's best by %.3e, allowed %.3e" % (label, best, short, allowed))
    assert 0 <= best < cref["S"].size, "%s: pick %d" % (label, best)
    assert short <= allowed, "%s: pick %d is worse than the reference's best by %.3e > %.3e" % (label, best, short, allowed)


# ---- the gradient --------------------------------------------------------------------------------------------------------------
# grad_jl = sum_i D_jil (a_j alpha_i - 2 b_j beta_ij),  D_jil = dk(z_j, x_i) / dz_jl.  Scale = the same first-order effect of a relative
# perturbation u of every input:
#     S_G,jl = sum_i |D_jil| c_ji (|a_j alpha_i| + 2 |b_j beta_ij|)             the terms, c = the derivative's own rounding constant
#            + |sum_i D_jil alpha_i| da_j / u + 2 |sum_i D_jil beta_ij| db_j / u   the coefficients: d a = |a_mu| u S_m + |a_var| u S_v + R_a
#            + 2 |b_j| sum_i |D_jil| S_beta,ij                                   the solve: S_beta,j = |K^-1| (|b_j| + |K| |beta_j|)
# c_ji = E_ji / (u |k_ji|) + 4: the assembly's per-entry bound of posterior_ref.assembly_bound in the difference form (the gradient
# kernel forms x_i - z_j first) relative to the entry, and four roundings for the coordinate difference, the constant and the products.
GRAD_MUTANTS = {                               # name -> the costs it is judged in (abs-b: where var < 0)
    "phi-f32": (PI,), "abs-b": (UCB, PI, EI), "last-row": (UCB, PI, EI), "tile-seam": (UCB, PI, EI), "alpha-shift": (UCB, PI, EI),
}


def dk_ld(spec, Z, X):
    """(D (m, n, d), k (m, n)) in longdouble from the points: D_jil = dk(z_j, x_i) / dz_jl (the true derivative, bo_compose.dkdz's)."""
    k = DR.cov_ld(spec, Z, X)
    diff = np.asarray(Z, dtype=float).astype(LD)[:, None, :] - np.asarray(X, dtype=float).astype(LD)[None, :, :]
    d = int(spec["d"])
    if spec["kind"] == "se":
        cl = np.broadcast_to(np.asarray(spec["cl"], dtype=float), (d,)).astype(LD)
        return -(diff / (cl * cl)) * k[:, :, None], k
    c2 = LD(3 if spec["kind"] == "matern32" else 5) / (LD(float(spec["rho"])) * LD(float(spec["rho"])))
    t = np.sqrt(c2 * np.sum(diff * diff, axis=2))
    if spec["kind"] == "matern32":                 # k = sig (1 + t) e^-t,  dk/dz = -sig c^2 e^-t (z - x)
        f = c2 * k / (LD(1) + t)
    else:                                          # k = sig (1 + t + t^2 / 3) e^-t,  dk/dz = -sig c^2 / 3 (1 + t) e^-t (z - x)
        f = c2 / LD(3) * k * (LD(1) + t) / (LD(1) + t + t * t / LD(3))
    return -f[:, :, None] * diff, k


def with_kd(ref, kd_old, kd_new):
    """The posterior reference of the same K and B with another prior variance per point (it enters the variance additively)."""
    out = dict(ref, val=dict(ref["val"]), scale=dict(ref["scale"]))
    out["val"]["v"] = ref["val"]["v"] + (np.asarray(kd_new, dtype=LD) - np.asarray(kd_old, dtype=LD))
    out["scale"]["v"] = ref["scale"]["v"] - np.abs(kd_old) + np.abs(kd_new)
    return out


def grad_reference(spec, X, Z, K, B, alpha, acq, param, ref):
    """dict(val (m, d) longdouble, S (m, d), cref): the gradient of the costs w.r.t. the candidates from the posterior reference `ref`
    of the arrays (K, B; its beta, mean and variance), alpha as given and the derivative from the points, with the scale S_G."""
    cref = cost_reference(acq, param, ref)
    v = cref["val"]
    D, k = dk_ld(spec, Z, X)
    al = np.asarray(alpha, dtype=LD)
    betaT = np.ascontiguousarray(ref["beta"].T)                              # (m, n)
    wgt = v["a"][:, None] * al[None, :] - LD(2) * v["b"][:, None] * betaT
    val = np.sum(D * wgt[:, :, None], axis=1)
    with np.errstate(all="ignore"):
        f = lambda x: np.abs(np.asarray(x, dtype=float))
        Dabs, kf = f(D), f(k)
        E = P.assembly_bound(spec, Z, X, k, "diff")
        c = np.where(kf > 0, E / (U * np.where(kf > 0, kf, 1.0)), 0.0) + 4.0
        a, b, bT = f(v["a"]), f(v["b"]), f(betaT)
        T1 = np.einsum("jil,ji->jl", Dabs, c * (a[:, None] * np.abs(alpha)[None, :] + 2.0 * b[:, None] * bT))
        da = f(v["a_mu"]) * ref["scale"]["m"] + f(v["a_var"]) * ref["scale"]["v"] + cref["R"]["a"] / U
        db = f(v["b_mu"]) * ref["scale"]["m"] + f(v["b_var"]) * ref["scale"]["v"] + cref["R"]["b"] / U
        T2 = f(np.sum(D * al[None, :, None], axis=1)) * da[:, None]
        T3 = 2.0 * f(np.sum(D * betaT[:, :, None], axis=1)) * db[:, None]
        Sb = np.abs(np.linalg.inv(K)) @ (np.abs(B) + np.abs(K) @ bT.T)      # (n, m)
        T4 = 2.0 * b[:, None] * np.einsum("jil,ij->jl", Dabs, Sb)
    return dict(val=val, S=T1 + T2 + T3 + T4 + DS / U, cref=cref)


def omega_G(got, gref, rows=None):
    """max_jl |got_jl - ref_jl| / (u S_G,jl) over every row with a finite reference (`rows`: a mask of the rows judged)."""
    ok = np.all(np.isfinite(np.asarray(gref["val"], dtype=float)), axis=1)
    if rows is not None:
        ok = ok & rows
    return P.omega(np.asarray(got)[ok], gref["val"][ok], gref["S"][ok])


def route_grad(route, spec, X, Z, K, B, kd, alpha, acq, param, mutant=None):
    """(grad (m, d), costs, posterior values) of a float64 route: bo_compose.DenseModel.grad restated on the given arrays -- the
    values and the backward solve by the route, (a, b) by the float64 epilogue, the derivative by bo_compose.dkdz."""
    import scipy.linalg as sl
    import chol_stability_ref as CR
    pv = P.route_values(route, K, B, kd, alpha=alpha, mutant=mutant if mutant in ROUTE_MUTANTS else None)
    A_, a, b = costs_f64(acq, param, pv["m"], pv["v"], mutant if mutant in EPILOGUE_MUTANTS else None)
    if route == "lapack":
        beta = sl.cho_solve(sl.cho_factor(K, lower=True, check_finite=False), B, check_finite=False)
    else:
        bs = int(route[1:])
        beta = CR.solve_block_inverse(CR.chol_block_inverse(K, bs), B, bs)
    al = np.roll(alpha, 1) if mutant == "alpha-shift" else np.asarray(alpha, dtype=float)
    rows = np.ones(K.shape[0], dtype=bool)
    if mutant == "last-row":
        rows[-1] = False
    if mutant == "tile-seam":
        beta = beta.copy()
        beta[:, 128] = beta[:, 127]
    out = np.empty(Z.shape)
    with np.errstate(all="ignore"):
        for j in range(Z.shape[0]):
            out[j] = BC.dkdz(spec, Z[j], X)[rows].T @ (a[j] * al[rows] - 2.0 * b[j] * beta[rows, j])
    return out, A_, pv


def grad_comparator_omegas(gref, spec, X, Z, K, B, kd, alpha, acq, param, rows=None):
    return {route: omega_G(route_grad(route, spec, X, Z, K, B, kd, alpha, acq, param)[0], gref, rows) for route in P.ROUTES}


def dims_case(kind, d, n=60, m=40, seed=0):
    """dict(spec, X, Z, y, nugget) in d dimensions: n training points, m candidates of which 5 are training points and 5 next to one
    (the DMAX classes beside the ones tests/test_gpu_grad_dims.py sweeps)."""
    rng = np.random.default_rng(7000 + 10 * d + seed)
    length = 0.05 if d == 1 else 0.5 * np.sqrt(d)        # (60 points: 0.03 apart on the line, 2 .. 3 apart in nine dimensions)
    spec = dict(kind="se", d=d, cl=list(np.linspace(0.8, 1.4, d) * length), signalSize=1.2) if kind == "se" else \
        dict(kind=kind, d=d, rho=1.5 * length, signalSize=1.1)
    X = rng.uniform(-1.0, 1.0, (n, d))
    Z = rng.uniform(-1.0, 1.0, (m, d))
    Z[:5] = X[[0, 1, n // 2, n - 2, n - 1]]
    Z[5:10] = X[10:15] + 1e-7 * rng.standard_normal((5, d))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return dict(spec=spec, X=P._ro(X), Z=P._ro(Z), y=P._ro(y), nugget=1e-2, n=n)      # (the noise of y: 0.1^2)


# ---- the q-batch picks -----------------------------------------------------------------------------------------------------------
BATCH_Q = 6
BATCH_NOISE = 1e-6
BATCH_CASES = ("m52-tiny-noise", "se-tiny-noise")


def batch_candidates(name):
    """257 candidates of a case: its 130, 20 duplicates of training points, 10 pairs 1e-7 apart, 87 more points of the cube."""
    c = P.case(name)
    rng = np.random.default_rng(8100 + P.CASES[name][3])
    dup = c["X"][rng.choice(c["n"], size=20, replace=False)]
    first = rng.uniform(-1.0, 1.0, (10, P.D))
    pairs = np.empty((20, P.D))
    pairs[0::2], pairs[1::2] = first, first + 1e-7 * rng.standard_normal((10, P.D))
    return P._ro(np.vstack([c["Z"], dup, pairs, rng.uniform(-1.0, 1.0, (257 - 170, P.D))]))


def batch_params(param, lies, track_best):
    """The cost's parameter at every pick: the caller's, raised to the largest believed value so far when track_best."""
    out, p = [], float(param)
    for t in range(len(lies)):
        out.append(p)
        if track_best:
            p = max(p, float(lies[t]))
    return out


class BatchBase:
    """The longdouble model on X alone that every replay on the same (spec, X, noise, C) starts from: from the points (cov_ld), or --
    `arrays` = (K with the noise on its diagonal, B = K(X, C), kd) -- from the device's own fills taken back (the tight rule of
    posterior_ref: the solve and the recurrence are judged alone; only the picks' own rows k(c_s, .) come from the points)."""

    def __init__(self, spec, X, noise, C, arrays=None):
        n = X.shape[0]
        if arrays is None:
            self.K = DR.cov_ld(spec, X)
            self.K[np.diag_indices(n)] += LD(float(noise))
            self.B = DR.cov_ld(spec, X, C)
            self.kd = DR.prior_ld(spec, C.shape[0])
        else:
            assert all(np.asarray(a).dtype == np.float64 for a in arrays)
            self.K, self.B, self.kd = (np.asarray(a, dtype=LD) for a in arrays)
        self.arrays = arrays
        self.L = DR.chol_ld(self.K)
        self.W = DR.solve_lower_ld(self.L, self.B)


def _base_f64(spec, X, noise, C, arrays):
    """(K, B, kd) in float64 for the comparators: the given arrays, or cov_f64 from the points."""
    if arrays is not None:
        return tuple(np.array(a, dtype=float) for a in arrays)
    K = DR.cov_f64(spec, X)
    K = 0.5 * (K + K.T)
    K[np.diag_indices_from(K)] += noise
    return K, DR.cov_f64(spec, X, C), np.full(C.shape[0], float(spec["signalSize"]))


def batch_reference(spec, X, y, noise, C, picks, lies, acq, param, track_best, base=None):
    """[dict(val, S, R, allow=None, masked)] per pick t (`base`: a BatchBase of the same problem, shared between replays; its arrays
    when it was built from some): the longdouble costs of ALL candidates on the model refitted on X + C[picks[:t]]
    with y + lies[:t] (the replay of the device's own picks and believed values, as design_replay_ref replays the selectors), the
    scale S_A on the grown system with the end-to-end mean scale S_M, and the mask of the candidates picked before.  The factor
    grows by one row per pick (its new row IS the pick's column of W)."""
    import scipy.linalg as sl
    base = base or BatchBase(spec, X, noise, C)
    K, L, B, W, kd = base.K, base.L, base.B, base.W, base.kd
    yt = np.asarray(y, dtype=float).astype(LD)
    z = DR.solve_lower_ld(L, yt)
    params = batch_params(param, lies, track_best)
    out = []
    for t in range(len(picks)):
        mean, var = np.dot(W.T, z), kd - np.sum(W * W, axis=0)
        Lf, Wf = np.asarray(L, dtype=float), np.asarray(W, dtype=float)
        beta = sl.solve_triangular(Lf, Wf, lower=True, trans="T", check_finite=False)
        alpha_hat = sl.solve_triangular(Lf, np.asarray(z, dtype=float), lower=True, trans="T", check_finite=False)
        scale = P._scales(np.abs(np.asarray(K, dtype=float)), np.abs(np.asarray(B, dtype=float)), np.asarray(kd, dtype=float), beta,
                          np.asarray(yt, dtype=float), None, alpha_hat, None)
        ref = dict(val={"m": mean, "v": var}, scale={"m": scale["M"], "v": scale["v"]})
        cref = cost_reference(acq, params[t], ref)
        masked = np.zeros(C.shape[0], dtype=bool)
        masked[np.asarray(picks[:t], dtype=int)] = True
        cref["masked"] = masked
        out.append(cref)
        if t + 1 == len(picks):
            break
        s = int(picks[t])
        l = W[:, s].copy()
        brow = DR.cov_ld(spec, C[s:s + 1], C)[0]
        diag = np.sqrt(brow[s] + LD(float(noise)) - np.dot(l, l))
        n = L.shape[0]
        L2 = np.zeros((n + 1, n + 1), dtype=LD)
        L2[:n, :n], L2[n, :n], L2[n, n] = L, l, diag
        K2 = np.zeros((n + 1, n + 1), dtype=LD)
        K2[:n, :n], K2[n, :n], K2[:n, n], K2[n, n] = K, B[:, s], B[:, s], brow[s] + LD(float(noise))
        W = np.vstack([W, ((brow - np.dot(l, W)) / diag)[None, :]])
        B = np.vstack([B, brow[None, :]])
        z = np.append(z, (LD(float(lies[t])) - np.dot(l, z)) / diag)
        yt = np.append(yt, LD(float(lies[t])))
        K, L = K2, L2
    return out


def batch_refit_rows(spec, X, y, noise, C, picks, lies, acq, param, track_best, arrays=None):
    """(q, M) float64 comparator: the refit loop through LAPACK on the device's picks and believed values (the base arrays as given or
    cov_f64 from the points, the picks' rows by cov_f64, cho_factor per pick, the float64 epilogue); NaN at the candidates picked
    before."""
    import scipy.linalg as sl
    K, Bx, kd = _base_f64(spec, np.asarray(X, dtype=float), noise, C, arrays)
    ya = np.array(y, dtype=float)
    params = batch_params(param, lies, track_best)
    rows = []
    for t in range(len(picks)):
        c = sl.cho_factor(K, lower=True, check_finite=False)
        Wx = sl.solve_triangular(np.tril(c[0]), Bx, lower=True, check_finite=False)
        row = costs_f64(acq, params[t], Bx.T @ sl.cho_solve(c, ya, check_finite=False), kd - np.sum(Wx * Wx, axis=0))[0]
        row[np.asarray(picks[:t], dtype=int)] = np.nan
        rows.append(row)
        s = int(picks[t])
        brow = DR.cov_f64(spec, C[s:s + 1], C)[0]
        n = K.shape[0]
        K2 = np.empty((n + 1, n + 1))
        K2[:n, :n], K2[n, :n], K2[:n, n], K2[n, n] = K, Bx[:, s], Bx[:, s], brow[s] + noise
        K, Bx, ya = K2, np.vstack([Bx, brow[None, :]]), np.append(ya, float(lies[t]))
    return np.array(rows)


def batch_rank1_rows(spec, X, y, noise, C, picks, lies, acq, param, track_best, arrays=None, route="lapack"):
    """(q, M) float64 comparator: the rank-one recurrence of include/gpx.h on the device's picks and believed values --
    delta = v_s + noise, u = (k(c_s, .) - W[:, s]^T W - sum_r U[r][s] U[r]) / sqrt(delta), mu += u (y_s - mu_s) / sqrt(delta),
    v -= u^2; a pivot with delta <= 1e-13 k(c_s, c_s) conditions nothing.  `route`: the factor and the two solves of the model on X
    by LAPACK, or "b128" by the explicit-inverse emulation of chol_stability_ref (posterior_ref's second comparator: the end-to-end
    mean through explicit 128-order inverses scores 2.4 where LAPACK scores 0.6 at noise 1e-6, and so does the device)."""
    import scipy.linalg as sl
    import chol_stability_ref as CR
    K, Bx, kd = _base_f64(spec, np.asarray(X, dtype=float), noise, C, arrays)
    if route == "lapack":
        c = sl.cho_factor(K, lower=True, check_finite=False)
        W = sl.solve_triangular(np.tril(c[0]), Bx, lower=True, check_finite=False)
        mu = Bx.T @ sl.cho_solve(c, np.asarray(y, dtype=float), check_finite=False)
    else:
        bs = int(route[1:])
        L = CR.chol_block_inverse(K, bs)
        W = CR.forward_block_inverse(L, Bx, bs)
        mu = Bx.T @ CR.solve_block_inverse(L, np.asarray(y, dtype=float), bs)
    v = kd - np.sum(W * W, axis=0)
    params = batch_params(param, lies, track_best)
    Um = np.zeros((len(picks), C.shape[0]))
    rows = []
    for t in range(len(picks)):
        row = costs_f64(acq, params[t], mu, v)[0]
        row[np.asarray(picks[:t], dtype=int)] = np.nan
        rows.append(row)
        s = int(picks[t])
        delta = v[s] + noise
        if delta > 1e-13 * kd[s]:
            u = (DR.cov_f64(spec, C[s:s + 1], C)[0] - W[:, s] @ W - Um[:t, s] @ Um[:t]) / np.sqrt(delta)
            Um[t] = u
            mu = mu + u * (float(lies[t]) - mu[s]) / np.sqrt(delta)
            v = v - u * u
    return np.array(rows)


def batch_rank1_b128_rows(*args, **kw):
    return batch_rank1_rows(*args, route="b128", **kw)


BATCH_COMPARATORS = {"refit": batch_refit_rows, "rank-one": batch_rank1_rows, "rank-one b128": batch_rank1_b128_rows}


def omega_A_row(got_row, cref):
    """omega_A over the candidates of a batch row that are not masked; the masked ones must be NaN exactly (inf otherwise)."""
    got_row = np.asarray(got_row, dtype=float)
    if not np.all(np.isnan(got_row[cref["masked"]])):
        return float("inf")
    ok = ~cref["masked"]
    return P.omega(got_row[ok], cref["val"]["A"][ok], cref["S"][ok])


def batch_regret(cref, pick, top):
    """regret() among the candidates that were still to be had."""
    A_ = cref["val"]["A"]
    ok = ~cref["masked"] & ~np.isnan(np.asarray(A_, dtype=float))
    return float(A_[pick] - np.min(A_[ok])), 2.0 * U * MARGIN * top * float(cref["S"][pick])
