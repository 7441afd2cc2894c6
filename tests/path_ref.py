"""Float64 / longdouble replays, bounds, comparators and mutants for pathwise posterior sampling (gpx_paths_*; NumPy only; data and
references of tests/test_path_host.py and tests/test_gpu_paths.py, not product code).  Conventions of tests/sample_ref.py:
u = 2^-53, replays in np.longdouble, the device compared with a replay from ITS OWN resident quantities (here the update weights V),
never with a solve made elsewhere.

    f~_s(z) = sum_j c_sj cos(omega_j . z + b_j),  c = fl(sqrt(2 sig / L)) w  (one float64 product, as the device forms it)
    V       = alpha - (K + noise I)^-1 (f~(X) + eps)
    f_s(z)  = f~_s(z) + sum_i v_si k(x_i, z)

Value bound, per element (s, m), unit constants:
    u [ (L + N + 4) T + sum_j |c_sj| (d + 2) (sum_l |omega_jl z_ml| + |b_j|) + sum_i |v_si| k_i (4 + (d + 2) e_i) ],
    T = sum_j |c_sj| + sum_i |v_si| k_i,   e_i = r^2 / 2 (squared exponential) or t (Matern): the size of the exponent.
First term: a sum of L + N products in any order, a cosine / exponential good to a unit or two, the stored result.  Second: the
argument of a cosine is a d-term inner product and one addition, its absolute error (d + 2) u (sum |omega z| + |b|) passes through
|d cos| <= 1.  Third: the exponent carries (d + 2) roundings relative, which the exponential multiplies by its size; 4 covers the
polynomial factor, signalSize and the square root.  The cap a device value is held to is MARGIN (= chol_stability_ref.MARGIN = 8)
times the bound.  The gradient bound has the same form with |omega_jl| on every feature term and the size of dk/dz_l on every
kernel term.
"""
import numpy as np

import chol_stability_ref as CR
import design_replay_ref as DR

LD, U, MARGIN = CR.LD, CR.U, CR.MARGIN
TWO_NU = {"matern32": 3.0, "matern52": 5.0}


# ---- spectral scaling ---------------------------------------------------------------------------------------------------------------
def frequencies(spec, g, u=None, mutant=None):
    """omega (L, d) in float64, as gpexp_amd.paths.spectralFrequencies: g / cl, or g / rho * sqrt(2 nu / u).
    mutant "matern_as_se": a Matern kernel's frequencies drawn as a squared exponential's of length rho."""
    g = np.asarray(g, dtype=float)
    if spec["kind"] == "se":
        cl = np.asarray(spec["cl"], dtype=float).ravel()
        return g / (np.tile(cl, g.shape[1]) if cl.size == 1 else cl)[None, :]
    if mutant == "matern_as_se":
        return g / float(spec["rho"])
    return g / float(spec["rho"]) * np.sqrt(TWO_NU[spec["kind"]] / np.asarray(u, dtype=float))[:, None]


def base_draws(spec, S, L, N, seed):
    """dict(g, u, phase, w, xi): the base draws of gpexp_amd.paths.PathBase.draw, seeded."""
    rng = np.random.default_rng(seed)
    d = int(spec["d"])
    g = rng.standard_normal((L, d))
    u = rng.chisquare(TWO_NU[spec["kind"]], L) if spec["kind"] in TWO_NU else None
    return dict(g=g, u=u, phase=rng.uniform(0.0, 2.0 * np.pi, L), w=rng.standard_normal((S, L)), xi=rng.standard_normal((S, N)))


def amplitude(spec, L, mutant=None):
    return np.sqrt((1.0 if mutant == "amplitude" else 2.0) * float(spec["signalSize"]) / L)


def feature_weights(spec, w, mutant=None):
    """c = amp * w in float64 (the one product the device's host side makes)."""
    w = np.asarray(w, dtype=float)
    return amplitude(spec, w.shape[1], mutant) * w


def hoeffding_t(n_entries, L, delta=1e-9):
    """|Phi Phi^T - K| / signalSize <= t for all n_entries entries with probability 1 - delta: every entry is a mean of L independent
    terms 2 cos(.) cos(.) of range 4 (Hoeffding), union bound over the entries."""
    return float(np.sqrt(8.0 * np.log(2.0 * n_entries / delta) / L))


def feature_gram_error(spec, omega, phase, Z):
    """max |Phi Phi^T - K| / signalSize over the points Z (float64)."""
    sig = float(spec["signalSize"])
    Phi = np.sqrt(2.0 * sig / omega.shape[0]) * np.cos(Z @ omega.T + phase[None, :])
    return float(np.max(np.abs(Phi @ Phi.T - DR.cov_f64(spec, Z)))) / sig


# ---- replays ------------------------------------------------------------------------------------------------------------------------
def _cov(spec, A, B, dtype):
    return DR.cov_ld(spec, A, B) if dtype is LD else DR.cov_f64(spec, A, B)


def cos_features(omega, phase, Z, dtype=LD, mutant=None):
    """(M, L): cos(omega_j . z_m + b_j).  mutant "phase": the phase dropped."""
    arg = np.asarray(Z, dtype=float).astype(dtype) @ np.asarray(omega, dtype=float).astype(dtype).T
    if mutant != "phase":
        arg = arg + np.asarray(phase, dtype=float).astype(dtype)[None, :]
    return np.cos(arg)


def prior_paths(c, omega, phase, Z, dtype=LD, mutant=None):
    """(S, M): f~_s(z_m)."""
    return np.asarray(c, dtype=float).astype(dtype) @ cos_features(omega, phase, Z, dtype, mutant).T


def update_weights(spec, X, alpha_or_y, noise, c, omega, phase, eps, dtype=float, mutant=None, from_y=True):
    """V (S, N) = coeff - (K + noise I)^-1 (f~(X) + eps) by a dense solve (the HOST's weights: the GPU tests replay from the device's
    own V instead).  mutants: "no_eps" (eps not subtracted), "plus" (+ instead of -)."""
    K = _cov(spec, X, None, dtype)
    K = K + dtype(noise) * np.eye(K.shape[0], dtype=dtype)
    R = prior_paths(c, omega, phase, X, dtype, mutant)
    if eps is not None and mutant != "no_eps":
        R = R + np.asarray(eps, dtype=float).astype(dtype)
    Kf = K.astype(float)
    sol = np.linalg.solve(Kf, R.T.astype(float)).T
    coeff = np.linalg.solve(Kf, np.asarray(alpha_or_y, dtype=float)) if from_y else np.asarray(alpha_or_y, dtype=float)
    return coeff[None, :] + sol if mutant == "plus" else coeff[None, :] - sol


def paths(spec, c, omega, phase, V, X, Z, dtype=LD, mutant=None):
    """(S, M): f_s(z_m) from the feature weights c and the update weights V (X None or V None: prior paths).
    mutant "next_path": point m reads the weights of path s + 1 (cyclically)."""
    c = np.asarray(c, dtype=float)
    if mutant == "next_path":
        c = np.roll(c, -1, axis=0)
    f = prior_paths(c, omega, phase, Z, dtype, mutant)
    if X is not None and V is not None and np.shape(V)[1] > 0:
        V = np.asarray(V, dtype=float)
        if mutant == "next_path":
            V = np.roll(V, -1, axis=0)
        f = f + V.astype(dtype) @ _cov(spec, X, Z, dtype)
    return f


def _scales(spec, dtype):
    sig, sc = DR._params_f64(spec)
    return dtype(sig), np.asarray(sc, dtype=float).astype(dtype)


def kernel_point_gradient(spec, X, Z, dtype=LD):
    """(N, P, d): d k(x_i, z_p) / d z_p[l], the true derivative (0 at z = x_i), from the float64 scales the device holds."""
    sig, sc = _scales(spec, dtype)
    diff = np.asarray(X, dtype=float).astype(dtype)[:, None, :] - np.asarray(Z, dtype=float).astype(dtype)[None, :, :]   # x - z
    r2 = np.sum((diff * sc) ** 2, axis=2)
    if spec["kind"] == "se":
        f = sig * np.exp(-r2 / 2)
    else:
        t = np.sqrt(r2)
        f = sig * np.exp(-t) if spec["kind"] == "matern32" else sig * (1 + t) * np.exp(-t) / 3
    return f[:, :, None] * diff * (sc * sc)[None, None, :]


def gradient(spec, c, omega, phase, V, X, Zp, path, dtype=LD, mutant=None):
    """(P, d): grad of path path[p] at Zp[p].  mutant "sine_sign": the sign of the sine term flipped."""
    path = np.asarray(path)
    om = np.asarray(omega, dtype=float).astype(dtype)
    arg = np.asarray(Zp, dtype=float).astype(dtype) @ om.T + np.asarray(phase, dtype=float).astype(dtype)[None, :]
    cw = np.asarray(c, dtype=float).astype(dtype)[path] * np.sin(arg)                     # (P, L)
    g = (cw if mutant == "sine_sign" else -cw) @ om
    if X is not None and V is not None and np.shape(V)[1] > 0:
        dk = kernel_point_gradient(spec, X, Zp, dtype)                                       # (N, P, d)
        g = g + np.einsum("pi,ipl->pl", np.asarray(V, dtype=float).astype(dtype)[path], dk)
    return g


# ---- bounds and comparators -----------------------------------------------------------------------------------------------------------
def _exponent_size(spec, X, Z):
    sig, sc = DR._params_f64(spec)
    r2 = np.sum(((np.asarray(X, dtype=float)[:, None, :] - np.asarray(Z, dtype=float)[None, :, :]) * sc) ** 2, axis=2)
    return 0.5 * r2 if spec["kind"] == "se" else np.sqrt(r2)


def value_bound(spec, c, omega, phase, V, X, Z):
    """(S, M): the per-element bound of the module docstring (without MARGIN)."""
    c, om, Z = np.abs(np.asarray(c, dtype=float)), np.abs(np.asarray(omega, dtype=float)), np.asarray(Z, dtype=float)
    L, d = om.shape
    argsize = np.abs(Z) @ om.T + np.abs(phase)[None, :]                                   # (M, L)
    T = np.sum(c, axis=1)[:, None] * np.ones((1, Z.shape[0]))
    rest = (d + 2) * (c @ argsize.T)
    n = 0
    if X is not None and V is not None and np.shape(V)[1] > 0:
        aV, k = np.abs(np.asarray(V, dtype=float)), np.abs(DR.cov_f64(spec, X, Z))
        n = aV.shape[1]
        T = T + aV @ k
        rest = rest + aV @ (k * (4.0 + (d + 2) * _exponent_size(spec, X, Z)))
    return U * ((L + n + 4) * T + rest)


def gradient_bound(spec, c, omega, phase, V, X, Zp, path):
    """(P, d): the same form for the gradient: |omega_jl| on every feature term, |dk/dz_l| on every kernel term."""
    path = np.asarray(path)
    c, om, Zp = np.abs(np.asarray(c, dtype=float))[path], np.abs(np.asarray(omega, dtype=float)), np.asarray(Zp, dtype=float)
    L, d = om.shape
    argsize = np.abs(Zp) @ om.T + np.abs(phase)[None, :]                                  # (P, L)
    T = c @ om                                                                             # (P, d)
    rest = (d + 2) * ((c * argsize) @ om)
    n = 0
    if X is not None and V is not None and np.shape(V)[1] > 0:
        aV = np.abs(np.asarray(V, dtype=float))[path]                                      # (P, N)
        dk = np.abs(kernel_point_gradient(spec, X, Zp, float))                             # (N, P, d)
        n = aV.shape[1]
        T = T + np.einsum("pi,ipl->pl", aV, dk)
        rest = rest + np.einsum("pi,ipl->pl", aV * (4.0 + (d + 2) * _exponent_size(spec, X, Zp).T), dk)
    return U * ((L + n + 4) * T + rest)


def check_within(got, ref, bound, label="", margin=MARGIN):
    """|got - ref| <= margin * bound elementwise; prints the largest ratio before it asserts and returns it."""
    err = np.abs(np.asarray(got, dtype=float).astype(LD) - ref).astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print("  %-48s max |got - replay| / bound = %.3f (cap %g)" % (label, worst, margin))
    assert np.all(np.isfinite(np.asarray(got, dtype=float))), "%s: non-finite values" % label
    assert worst <= margin, "%s: |got - replay| reaches %.3f x the bound (cap %g)" % (label, worst, margin)
    return worst


def first_argbest(rows, minimize=True):
    """Per row the FIRST index of the minimum (maximum) among the entries that are not NaN -- np.argmin / np.argmax on a row without
    NaN; a NaN never wins, and a row of nothing but NaN gives index 0 (np.argmin's answer there)."""
    rows = np.asarray(rows, dtype=float)
    nan = np.isnan(rows)
    key = np.where(nan, np.inf, rows if minimize else -rows)
    return np.argmax(~nan & (key == key.min(axis=1)[:, None]), axis=1)


def mutant_argbest_last(rows, minimize=True):
    rows = np.asarray(rows)
    rev = rows[:, ::-1]
    return rows.shape[1] - 1 - (np.argmin(rev, axis=1) if minimize else np.argmax(rev, axis=1))


def check_argbest(idx, val, rows, minimize=True, label=""):
    """Exact: the first arg-best of the device's own rows and the value there."""
    want = first_argbest(rows, minimize)
    assert np.array_equal(np.asarray(idx), want), "%s: arg-best %r, first arg-best of the rows %r" % (label, idx, want)
    assert np.array_equal(np.asarray(val), np.asarray(rows)[np.arange(len(want)), want]), "%s: arg-best values" % label


def solve_residual_bound(Ld, x, r, dV, r_err):
    """Normwise bound on |Khat x - r|_inf for x solved against the factor Ld (Khat = Ld Ld^T) by two triangular solves:
    (2 gamma_n + gamma_n^2 <= gamma_{3n+1}) (| |L||L^T| |_inf |x|_inf + |r|_inf)  -- Higham Thm 10.4 without the factorisation's own
    term -- times MARGIN for the explicit block inverses, plus what the test itself adds: x is recovered as alpha - V (one rounding
    of the device's subtraction, |dx| <= u |V|, passed through |Khat|: dV = | |Khat| |V| |_inf) and r is the longdouble replay of
    a right-hand side the device formed in float64 (r_err = the value cap of the prior path + u |r|)."""
    n = Ld.shape[0]
    aL = np.abs(Ld)
    return MARGIN * CR.gamma(3 * n + 1) * (float(np.max(np.sum(aL @ aL.T, axis=1))) * float(np.max(np.abs(x))) +
                                           float(np.max(np.abs(r)))) + U * dV + r_err


# ---- the closed-form distribution of the paths ----------------------------------------------------------------------------------------
def path_distribution(spec, X, y, noise, omega, phase, Z):
    """(mean (M,), cov (M, M)) of f(Z) over w ~ N(0, I), xi ~ N(0, I) at FIXED features: mean = G y, cov = A (Phi_J Phi_J^T) A^T + noise G G^T
    with G = K(Z, X) (K + noise I)^-1, A = [I, -G], Phi_J the scaled features at J = (Z; X)."""
    K = DR.cov_f64(spec, X)
    K[np.diag_indices_from(K)] += noise
    G = np.linalg.solve(K, DR.cov_f64(spec, X, Z)).T
    J = np.vstack([Z, X])
    Phi = amplitude(spec, omega.shape[0]) * cos_features(omega, phase, J, float)
    A = np.hstack([np.eye(Z.shape[0]), -G])
    return G @ y, A @ (Phi @ Phi.T) @ A.T + noise * (G @ G.T)


def distribution_z(samples, mean, cov):
    """(largest |sample mean - mean| and largest |sample cov - cov|, each in its own standard errors): se of mean_i =
    sqrt(C_ii / S), of cov_ij = sqrt((C_ii C_jj + C_ij^2) / S)."""
    S = samples.shape[0]
    dg = np.diag(cov)
    zm = np.abs(samples.mean(axis=0) - mean) / np.sqrt(dg / S)
    zc = np.abs(np.cov(samples.T, bias=True) - cov) / np.sqrt((np.outer(dg, dg) + cov ** 2) / S)
    return float(np.max(zm)), float(np.max(zc))
