"""Per-point error metrics, longdouble references, float64 comparators and mutants for the posterior mean, variance, covariance and
IVAR (NumPy / SciPy only; data and references of tests/test_posterior_host.py and tests/test_gpu_posterior_bounds.py, not product
code).  Same conventions as tests/chol_stability_ref.py.

THE METRIC.  With u = 2^-53, for every evaluation point j (b_j = K(X, z_j), beta_j = K^-1 b_j, alpha = K^-1 y):

    omega = max_j |got_j - ref_j| / (u S_j)

    variance            v_j = kd_j - |L^-1 b_j|^2          S_v,j  = kd_j + 2 |beta_j|^T |b_j| + |beta_j|^T |K| |beta_j|
    mean, given alpha   m_j = b_j^T alpha                  S_m,j  = |b_j|^T |alpha|
    mean, end to end    M_j = b_j^T K^-1 y                 S_M,j  = |b_j|^T |alpha| + |beta_j|^T |y| + |beta_j|^T |K| |alpha|
    covariance          C_jl = kzz_jl - w_j^T w_l          S_c,jl = |kzz_jl| + |beta_j|^T |b_l| + |beta_l|^T |b_j| + |beta_j|^T |K| |beta_l|
    IVAR                I = mean_j v_j                     S_I    = mean_j S_v,j

S is the first-order effect on the value of a relative perturbation u of EVERY input entry (d v = d kd - 2 beta^T d b + beta^T dK beta,
and so on), so a backward-stable route scores O(1 .. n) whatever cond(K), and a point whose variance is 1e-6 is judged to as many
digits as its inputs determine -- where max|a - b| / max|b| judges it to none.

THE BOUND.  device omega <= MARGIN (= 8, chol_stability_ref.MARGIN and its reasons) x the larger of the two COMPARATORS on the same
arrays: "lapack" (cho_factor / solve_triangular / NumPy sums) and "b128" (the explicit-inverse emulation of chol_stability_ref).
Never a device result.  omega_I is one number, so a comparator's own figure is a single draw; the comparators' omega_v / sqrt(m) stands
beside it (comparator_omegas).  From points (reference_from_points) the bound gains the assembly's own allowance, the per-entry bound E of
tests/kernel_reference.py propagated to first order:  A_v,j = E_kd + 2 |beta_j|^T E_B,j + |beta_j|^T E_K |beta_j|, and likewise for
the others; omega then counts only the error in excess of A."""
import functools

import numpy as np
import scipy.linalg as sl

import chol_stability_ref as CR
import design_replay_ref as DR           # (its import fails where np.longdouble is plain float64)
import kernel_reference as KR
from chol_stability_ref import MARGIN, U, check_bound   # noqa: F401  (re-exported: the GPU test's one import)

LD = DR.LD
M_EVAL = 130            # one full column tile plus a tile with two live columns
N_ON, N_NEAR = 20, 20   # Z[0:20] training points exactly, Z[20:40] training points + 1e-7 N(0, 1)
D = 3

SE3 = dict(kind="se", d=3, cl=[0.5, 0.6, 0.7], signalSize=1.2)
M52 = dict(kind="matern52", d=3, rho=0.7, signalSize=1.1)
M32 = dict(kind="matern32", d=3, rho=0.7, signalSize=1.1)
MEHLER = dict(kind="mehler", d=3, t=[0.2, 0.25, 0.3])
KIND_ID = {"se": 0, "matern32": 1, "matern52": 2, "mehler": 3}      # gpexp_amd.device.K_*

# name -> (spec, n, noise; None = a per-point nugget log-uniform in [1e-6, 1e-2], seed)
CASES = {
    "se-well": (SE3, 300, 0.05, 5101),
    "se-tiny-noise": (SE3, 300, 1e-6, 5102),
    "m52-tiny-noise": (M52, 300, 1e-6, 5103),
    "m32-per-point": (M32, 300, None, 5104),
    "mehler": (MEHLER, 300, 1e-4, 5105),
    "m52-oop": (M52, 2200, 1e-4, 5106),
}
SMALL = [c for c in CASES if CASES[c][1] <= 640]        # the cases with a full longdouble reference
FROM_POINTS = [c for c in SMALL if CASES[c][0]["kind"] != "mehler"]   # cov_ld has no Mehler
MOVED = 40              # training rows that ivar_update's case moves (the last ones)
N_SAMPLED = 16


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name, m=M_EVAL):
    """dict(spec, X (n, 3), Z (m, 3), nugget (float or (n,)), y (n,), X2) of a case, drawn once, read-only.  X2 = X with its last
    MOVED rows redrawn (ivar_update).  The last MOVED rows of X and X2 lie inside the bounding box of the rows before them, so
    that both sets have the same box (the fills centre on it)."""
    spec, n, noise, seed = CASES[name]
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, D))
    lo, hi = X[:n - MOVED].min(axis=0), X[:n - MOVED].max(axis=0)
    X[n - MOVED:] = np.clip(X[n - MOVED:], lo, hi)
    X2 = X.copy()
    X2[n - MOVED:] = np.clip(rng.uniform(-1.0, 1.0, (MOVED, D)), lo, hi)
    nugget = float(noise) if noise is not None else 10.0 ** rng.uniform(-6.0, -2.0, n)
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    fixed = [0, 127, 128, n - 1]
    others = rng.choice(np.setdiff1d(np.arange(n), fixed), size=N_ON - len(fixed), replace=False)
    near = rng.choice(n, size=N_NEAR, replace=False)
    Z = rng.uniform(-1.0, 1.0, (max(m, N_ON + N_NEAR), D))
    Z[:N_ON] = X[np.concatenate([fixed, others])]
    Z[N_ON:N_ON + N_NEAR] = X[near] + 1e-7 * rng.standard_normal((N_NEAR, D))
    return dict(spec=spec, X=_ro(X), X2=_ro(X2), Z=_ro(Z[:m].copy()), nugget=nugget if noise is not None else _ro(nugget),
                y=_ro(y), n=n)


def sampled_cols(m=M_EVAL):
    """N_SAMPLED columns: the on-point ones for rows 0, 127, 128, n - 1, four near-point ones, eight of the rest."""
    rest = np.random.default_rng(77).choice(np.arange(N_ON + N_NEAR, m), size=N_SAMPLED - 8, replace=False)
    return np.array(sorted([0, 1, 2, 3, N_ON, N_ON + 1, N_ON + 2, N_ON + 3] + [int(c) for c in rest]))


# ---- host stand-ins for the device fills (CPU tests) ---------------------------------------------------------------------------
def mehler_f64(spec, A, B):
    t = np.asarray(spec["t"], dtype=float)
    om = 1.0 - t * t
    c1, c2, sig = t * t / (2.0 * om), t / om, float(np.prod(om ** -0.5))
    x = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        x += c1[k] * (A[:, k][:, None] ** 2 + B[:, k][None, :] ** 2) - c2[k] * A[:, k][:, None] * B[:, k][None, :]
    return sig * np.exp(-x)


def host_arrays(name, m=M_EVAL, moved=False):
    """(K with the nugget, B = K(X, Z), kd, kzz) in float64 on the host: what the GPU tests take back from the device's fills."""
    c = case(name, m)
    X, Z = (c["X2"] if moved else c["X"]), c["Z"]
    f = (lambda A, B: mehler_f64(c["spec"], A, B)) if c["spec"]["kind"] == "mehler" else (lambda A, B: DR.cov_f64(c["spec"], A, B))
    K = f(X, X)
    K = 0.5 * (K + K.T)
    K[np.diag_indices_from(K)] += c["nugget"]
    kzz = f(Z, Z)
    return K, f(X, Z), np.diag(kzz).copy(), 0.5 * (kzz + kzz.T)


# ---- the longdouble reference -------------------------------------------------------------------------------------------------
def solve_upper_ld(L, B):
    """L^-T B in longdouble by back substitution (row i from the rows below it)."""
    B = np.array(B, dtype=LD)
    X = np.zeros_like(B)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        acc = B[i] - (np.dot(L[i + 1:, i], X[i + 1:]) if i + 1 < n else LD(0))
        X[i] = acc / L[i, i]
    return X


def _scales(Kabs, Babs, kd, beta, y, alpha, alpha_hat, kzz):
    """The S of every metric in float64 (they only scale an error)."""
    ab = np.abs(np.asarray(beta, dtype=float))
    KB = Kabs @ ab
    out = {"v": np.abs(kd) + 2.0 * np.sum(ab * Babs, axis=0) + np.sum(ab * KB, axis=0)}
    out["I"] = float(np.mean(out["v"]))
    if alpha is not None:
        out["m"] = Babs.T @ np.abs(alpha)
    if alpha_hat is not None:
        aa = np.abs(np.asarray(alpha_hat, dtype=float))
        out["M"] = Babs.T @ aa + ab.T @ np.abs(y) + KB.T @ aa
    if kzz is not None:
        cross = ab.T @ Babs
        out["c"] = np.abs(kzz) + cross + cross.T + ab.T @ KB
    return out


def _reference_ld(K, B, kd, y, alpha, kzz):
    """The reference from longdouble (or float64) arrays; everything in longdouble."""
    K, B, kd = np.asarray(K, dtype=LD), np.asarray(B, dtype=LD), np.asarray(kd, dtype=LD)
    L = DR.chol_ld(K)
    W = DR.solve_lower_ld(L, B)
    beta = solve_upper_ld(L, W)
    val = {"v": kd - np.sum(W * W, axis=0)}
    val["I"] = np.sum(val["v"]) / LD(val["v"].size)
    alpha_hat = None
    if alpha is not None:
        val["m"] = np.dot(B.T, np.asarray(alpha, dtype=LD))
    if y is not None:
        alpha_hat = solve_upper_ld(L, DR.solve_lower_ld(L, np.asarray(y, dtype=LD)[:, None]))[:, 0]
        val["M"] = np.dot(B.T, alpha_hat)
    if kzz is not None:
        val["c"] = np.asarray(kzz, dtype=LD) - np.dot(W.T, W)
    Kf, Bf = np.abs(np.asarray(K, dtype=float)), np.abs(np.asarray(B, dtype=float))
    scale = _scales(Kf, Bf, np.asarray(kd, dtype=float), beta, y, alpha, alpha_hat, None if kzz is None else np.asarray(kzz, dtype=float))
    return dict(val=val, scale=scale, beta=beta, alpha_hat=alpha_hat, W=W, L=L)


def reference(K, B, kd, y=None, alpha=None, kzz=None):
    """dict(val={v, I[, m][, M][, c]}, scale={same keys}, beta, alpha_hat, W, L) of GIVEN float64 arrays (K (n, n) with the nugget on its
    diagonal, B (n, m), kd (m,), kzz (m, m)), everything in longdouble: L = chol(K), w_j = L^-1 b_j, beta_j = L^-T w_j, alpha_hat = K^-1 y."""
    for a in (K, B, kd):
        assert np.asarray(a).dtype == np.float64
    return _reference_ld(K, B, kd, y, alpha, kzz)


_SLICE_BITS = 19        # two slices' product has <= 38 bits; 2^38 x n <= 2^53 up to n = 32768: float64 BLAS sums them exactly


def _slices(A, count, axis, late=None):
    """`count` float64 arrays whose sum is A (longdouble) up to 2^-(19 count) of the largest magnitude along `axis`: slice k holds an
    integer of at most 20 bits times 2^(e - 19 k), e the exponent of that largest magnitude.  `late` (a longdouble array far below
    A: the low part of a two-term value) joins the remainder before the fourth slice."""
    rem = np.array(A, dtype=LD)
    mx = np.max(np.abs(rem), axis=axis, keepdims=True).astype(float)
    e = np.where(mx > 0, np.ceil(np.log2(np.where(mx > 0, mx, 1.0))) + 1.0, 0.0).astype(int)
    out = []
    for k in range(1, count + 1):
        if k == 4 and late is not None:
            rem = rem + late
        q = np.ldexp(LD(1), e - _SLICE_BITS * k)
        s = np.rint(rem / q) * q
        rem = rem - s
        out.append(np.asarray(s, dtype=float))
    return out


def _residual(Ks, Bc, beta_h, beta_l):
    """b - K (beta_h + beta_l) per column, the products and their sums exact (sliced operands in float64 BLAS), the slices' products
    added to b by compensated summation in longdouble: the result carries a few 2^-64 of ITSELF, not of |K| |beta|."""
    bs = _slices(beta_h, 5, 0, late=beta_l)
    s, comp = Bc.astype(LD), np.zeros(Bc.shape, dtype=LD)
    for p, q in sorted(((p, q) for p in range(len(Ks)) for q in range(len(bs))), key=sum):
        s, err = DR._two_sum(s, -(Ks[p] @ bs[q]).astype(LD))
        comp = comp + err
    return s + comp


def reference_sampled(K, B, kd, cols, max_iter=8):
    """dict(val={v}, scale={v}, cols) for the sampled columns of a larger case: float64 cho_factor, then iterative refinement of beta_j,
    carried as a sum of two longdoubles, against the exact residual (_residual) until |b_j - K beta_j|_inf <= 2^-60 |b_j|_inf; then
    v_j = kd_j - b_j^T beta_j with error-free products.  (A residual formed by a longdouble matrix product stalls at 1 .. 3 x 2^-60
    |b|: its own rounding, n 2^-64 |K| |beta|.)"""
    cols = np.asarray(cols)
    Bc = np.ascontiguousarray(B[:, cols])
    c = sl.cho_factor(K, lower=True, check_finite=False)
    Ks = _slices(K, 4, 1)
    beta_h = sl.cho_solve(c, Bc, check_finite=False).astype(LD)
    beta_l = np.zeros_like(beta_h)
    bnorm = np.max(np.abs(Bc), axis=0)
    for _ in range(max_iter):
        r = _residual(Ks, Bc, beta_h, beta_l)
        if np.all(np.max(np.abs(r), axis=0).astype(float) <= 2.0 ** -60 * bnorm):
            break
        beta_h, e = DR._two_sum(beta_h, sl.cho_solve(c, r.astype(float), check_finite=False).astype(LD))
        beta_l = beta_l + e
    else:
        raise AssertionError("reference_sampled: the refinement did not reach 2^-60 |b| in %d steps" % max_iter)
    p, e = DR._two_prod(Bc.astype(LD), beta_h)
    v = np.asarray(kd, dtype=LD)[cols] - (np.sum(p, axis=0) + np.sum(e + Bc.astype(LD) * beta_l, axis=0))
    scale = _scales(np.abs(K), np.abs(Bc), np.asarray(kd, dtype=float)[cols], beta_h, None, None, None, None)
    return dict(val={"v": v}, scale={"v": scale["v"]}, cols=cols, beta=beta_h, residual=r)


# ---- from points ---------------------------------------------------------------------------------------------------------------
def assembly_bound(spec, A, B, k_true, form="diff", center=None):
    """The per-entry bound of kernel_reference.Reference.bound for all pairs (A_i, B_j), vectorised in float64 (it is a bound: its own
    rounding is beside the point; tests/test_posterior_host.py pins it against the Decimal original on sampled pairs).
    `k_true` = the true values (cov_ld)."""
    assert spec["kind"] in KR.STATIONARY
    kind, d = spec["kind"], int(spec["d"])
    sig, sc = DR._params_f64(spec)
    A, B = np.asarray(A, dtype=float), np.asarray(B, dtype=float)
    s = np.zeros((A.shape[0], B.shape[0]))
    for k in range(d):
        s += ((A[:, k][:, None] - B[:, k][None, :]) * sc[k]) ** 2
    k_abs = np.abs(np.asarray(k_true, dtype=float))
    if kind == "se":
        x, Dk = 0.5 * s, 0.5 * k_abs
    else:
        x = np.sqrt(s)
        Dk = sig * np.exp(-x) / 2.0 if kind == "matern32" else sig * (1.0 + x) * np.exp(-x) / 6.0
    if form == "diff":
        T = s
    else:
        a = np.abs((A - np.asarray(center)[None, :]) * sc[None, :])
        b = np.abs((B - np.asarray(center)[None, :]) * sc[None, :])
        T = np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :] + 2.0 * (a @ b.T)
    return (8.0 + 0.2 * np.abs(x)) * 2.0 * U * k_abs + Dk * (2.0 * d + 16.0) * U * T + KR.DENORMAL_STEP


def reference_from_points(spec, X, Z, nugget, y=None, alpha=None, want_cov=False, forms=("diff", "diff", "diff"), centers=(None, None, None)):
    """The same reference with K, B, kd, kzz from cov_ld on the points, plus `allow` = {metric: A}: the assembly's allowance to first
    order.  forms / centers = the distance form and the centre of the device's three fills (K(X, X), K(X, Z), K(Z, Z);
    device.kfill_plan) -- nothing else comes from the device.  Also `f64` = the arrays rounded to float64 (the comparators' input)."""
    X, Z = np.asarray(X, dtype=float), np.asarray(Z, dtype=float)
    n = X.shape[0]
    nug = np.broadcast_to(np.asarray(nugget, dtype=float), (n,))
    K = DR.cov_ld(spec, X)
    EK = assembly_bound(spec, X, X, K, forms[0], centers[0])
    K[np.diag_indices(n)] += nug.astype(LD)
    EK[np.diag_indices(n)] += U * np.abs(np.diag(K).astype(float))      # the one rounding of k + nugget (kernel_reference.errors)
    B = DR.cov_ld(spec, X, Z)
    EB = assembly_bound(spec, X, Z, B, forms[1], centers[1])
    kd = DR.prior_ld(spec, Z.shape[0])
    Ekd = 16.0 * U * np.asarray(kd, dtype=float)                        # the bound at x = 0, T = 0
    kzz = DR.cov_ld(spec, Z) if want_cov else None
    ref = _reference_ld(K, B, kd, y, alpha, kzz)
    ab = np.abs(np.asarray(ref["beta"], dtype=float))
    EKb = EK @ ab
    allow = {"v": Ekd + 2.0 * np.sum(ab * EB, axis=0) + np.sum(ab * EKb, axis=0)}
    allow["I"] = float(np.mean(allow["v"]))
    if alpha is not None:
        allow["m"] = EB.T @ np.abs(alpha)
    if y is not None:
        aa = np.abs(np.asarray(ref["alpha_hat"], dtype=float))
        allow["M"] = EB.T @ aa + EKb.T @ aa
    if want_cov:
        cross = ab.T @ EB
        allow["c"] = assembly_bound(spec, Z, Z, kzz, forms[2], centers[2]) + cross + cross.T + ab.T @ EKb
    ref["allow"] = allow
    ref["f64"] = dict(K=np.asarray(K, dtype=float), B=np.asarray(B, dtype=float), kd=np.asarray(kd, dtype=float),
                      kzz=None if kzz is None else np.asarray(kzz, dtype=float))
    return ref


# ---- the metric ----------------------------------------------------------------------------------------------------------------
def omega(got, ref_val, scale, allow=None, where=None):
    """max |got - ref| / (u S) over the entries (`where`: an index of them), the error counted in excess of `allow` when given."""
    err = np.abs(np.asarray(got, dtype=LD) - ref_val)
    if allow is not None:
        err = np.maximum(err - np.asarray(allow, dtype=LD), LD(0))
    q = np.asarray(err / (LD(U) * np.asarray(scale, dtype=LD)), dtype=float)
    if where is not None:
        q = q[where]
    return float(np.max(q)) if np.all(np.isfinite(q)) else float("inf")


def omegas(got, ref, where=None, allowance=True):
    """{metric: omega} for the metrics present in both `got` ({v, m, M, c, I}) and the reference; a from-points reference's allowance
    is taken off the error unless allowance=False (the comparators, which start from the true arrays rounded once)."""
    allow = ref.get("allow") if allowance else None
    return {k: omega(got[k], ref["val"][k], ref["scale"][k], None if allow is None else allow[k], None if k in ("I", "c") else where)
            for k in ref["val"] if k in got}


def rel(a, b):
    """The metric of the existing posterior tests: max |a - b| / max |b|."""
    return float(np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))) / np.max(np.abs(np.asarray(b, dtype=float))))


# ---- comparators and mutants -----------------------------------------------------------------------------------------------------
ROUTES = ("lapack", "b128")
# name -> the metrics it is judged in
MUTANTS = {
    "last-row": ("v", "m"),       # the last training row missing from the column sums and the dot
    "row-chunk": ("v", "m"),      # one row chunk's partial dropped (rows 32 .. 47)
    "tile-seam": ("v", "m"),      # column 128 reading column 127's solve
    "scale-B": ("v",),            # every entry of B scaled by 1 + 3e-13
    "nugget": ("v",),             # the variance taken as kd - nugget - ssq
    "alpha-shift": ("m",),        # alpha shifted by one entry
}
REL_BLIND = ("last-row", "row-chunk", "tile-seam", "scale-B")


def route_values(route, K, B, kd, y=None, alpha=None, kzz=None, cols=None, mutant=None, nugget=None):
    """{v, I[, m][, M][, c]} of a float64 route on the given arrays (`cols`: those columns only; then no I), with one defect when
    `mutant` names one (MUTANTS; "nugget" needs the nugget)."""
    if cols is not None:
        B, kd = np.ascontiguousarray(B[:, cols]), kd[cols]
    if mutant == "scale-B":
        B = B * (1.0 + 3e-13)
    if route == "lapack":
        c = sl.cho_factor(K, lower=True, check_finite=False)
        L = np.tril(c[0])
        W = sl.solve_triangular(L, B, lower=True, check_finite=False)
        alpha_c = sl.cho_solve(c, y, check_finite=False) if y is not None else None
    else:
        b = int(route[1:])
        L = CR.chol_block_inverse(K, b)
        W = CR.forward_block_inverse(L, B, b)
        alpha_c = CR.solve_block_inverse(L, y, b) if y is not None else None
    Bm = B
    if mutant == "tile-seam":
        W, Bm = W.copy(), B.copy()
        W[:, 128], Bm[:, 128] = W[:, 127], B[:, 127]
    rows = np.ones(K.shape[0], dtype=bool)
    if mutant == "last-row":
        rows[-1] = False
    if mutant == "row-chunk":
        rows[32:48] = False
    if mutant == "alpha-shift":
        alpha = np.roll(alpha, 1)
    out = {"v": kd - np.sum(W[rows] * W[rows], axis=0)}
    if mutant == "nugget":
        out["v"] = kd - np.mean(np.broadcast_to(nugget, (K.shape[0],))) - np.sum(W * W, axis=0)
    if cols is None:
        out["I"] = float(np.mean(out["v"]))
    if alpha is not None:
        out["m"] = Bm[rows].T @ alpha[rows]
    if alpha_c is not None:
        out["M"] = B.T @ alpha_c
    if kzz is not None:
        out["c"] = kzz - W.T @ W
    return out


def comparator_omegas(ref, K, B, kd, y=None, alpha=None, kzz=None, cols=None):
    """{metric: {route: omega}} of the comparators on the same arrays as the reference."""
    out = {}
    for route in ROUTES:
        for k, v in omegas(route_values(route, K, B, kd, y, alpha, kzz, cols), ref, allowance=False).items():
            out.setdefault(k, {})[route] = v
    if "I" in out:
        # omega_I is ONE number, the mean of m per-point errors in units of the mean scale: a comparator's own figure is a single
        # draw anywhere between 0 and omega_v / sqrt(m) (independent per-point errors of either sign; measured 2e-4 .. 0.15), and 8 x
        # a lucky draw is no bound.  The figure a route with the comparators' per-point accuracy is expected to reach joins them.
        out["I"]["v/sqrt(m)"] = max(out["v"].values()) / np.sqrt(float(B.shape[1]))
    return out


def reference_mean(B, alpha):
    """dict(val={m}, scale={m}) of the mean from a given alpha alone (no solve: any size)."""
    return dict(val={"m": np.asarray(CR._ld_matmul(np.ascontiguousarray(B.T), np.asarray(alpha, dtype=float)[:, None]))[:, 0]},
                scale={"m": np.abs(B).T @ np.abs(alpha)})


def check_all(label, got, cmp_):
    """check_bound for every metric of `got` ({metric: device omega}) against `cmp_` ({metric: {route: omega}}): every figure is printed
    before the first failure surfaces; returns the failures' messages."""
    failures = []
    for k, value in got.items():
        try:
            check_bound("%s omega_%s" % (label, k), value, cmp_[k])
        except AssertionError as e:
            failures.append(str(e))
    return failures


@functools.lru_cache(maxsize=None)
def host_alpha(name):
    """A float64 alpha for the mean's own metric: LAPACK's solve on the host stand-in of K (any fixed vector of that size serves)."""
    K = host_arrays(name)[0] if CASES[name][1] <= 640 else None
    c = case(name)
    if K is None:
        return _ro(np.random.default_rng(5).standard_normal(c["n"]) * 10.0)
    return _ro(sl.cho_solve(sl.cho_factor(K, lower=True), c["y"]))


def pairwise_mean(v):
    """api.hip's pairwise_mean restated: h = ceil(m / 2), v[i] += v[i + h], m <- h; then one division.  Additions only, so NumPy
    reproduces the device's bits."""
    v = np.array(v, dtype=float)
    count = m = v.size
    while m > 1:
        h = (m + 1) // 2
        v[:m - h] += v[h:m]
        m = h
    return v[0] / float(count)
