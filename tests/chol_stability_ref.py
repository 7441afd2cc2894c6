"""Backward-error metrics and float64 emulations of the explicit-inverse Cholesky scheme (NumPy only; data and references of
tests/test_chol_stability_host.py and tests/test_gpu_chol_stability.py, not product code).

What is judged is always a BACKWARD error -- how far the computed factor / solution / inverse is from solving a nearby
problem exactly -- because on K with cond(K) ~ 1e10 two correct factorisations differ by cond * u in the forward sense.  Every
residual is formed in np.longdouble (64-bit significand here, asserted below), so that the residual's own rounding (2^-64 per
operation) stays three orders below the smallest value that is measured (LAPACK's ~ 20 * 2^-53).

The emulations restate, in float64 NumPy, the scheme of gpexp_amd/csrc/chol.hip at the level where its rounding behaviour is
decided: every triangular solve is a PRODUCT with an explicit inverse (16-order T_p inside the leaf, 128-order leaf inverses,
1024-order block inverses), and larger inverses are built from the inverses of their halves."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "chol_stability_ref: np.longdouble has eps = %g > 2^-63 on this platform; the residuals of the stability metrics need an "
    "extended-precision type (x87 80-bit or wider) and cannot be trusted in plain float64" % float(np.finfo(LD).eps))

U = 2.0 ** -53          # unit round-off of float64
MARGIN = 8.0            # device value <= MARGIN * max(LAPACK, emulations): MFMA accumulation order, inverses by recursive
                        # products instead of dtrtri, the leaf's reciprocal.  A margin over the REFERENCE's number.

K_SE, K_MATERN32, K_MATERN52 = 0, 1, 2   # gpexp_amd.device.K_*


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def gamma_chol(n):
    """Componentwise bound on |K - L L^T| / (|L| |L^T|) of a Cholesky factorisation by ANY ordering of the inner products
    (Higham, Accuracy and Stability, Thm 10.3): gamma_{n+1}."""
    return gamma(n + 1)


# ---- matrix families -------------------------------------------------------------------------------------------------
# name -> (kind, hyper-parameters as the C ABI takes them, nugget); d = 3, X uniform in [-1, 1]^3
FAMILIES = {
    "S8": (K_SE, [0.8, 0.88, 0.72, 1.0], 1e-8),
    "S6s": (K_SE, [0.8, 0.88, 0.72, 1e-6], 1e-14),
    "M10": (K_MATERN52, [3.0, 1.0], 1e-10),
    "W": (K_MATERN32, [0.5, 1.0], 0.1),
}
ILL = ("S8", "S6s", "M10")
D = 3


def family_points(name, n, extra=0):
    """(X (n, 3), Z (extra, 3)) of a family at size n: seeded by the family's position and n."""
    rng = np.random.default_rng(1000 * sorted(FAMILIES).index(name) + n)
    X = rng.uniform(-1.0, 1.0, (n, D))
    Z = rng.uniform(-1.0, 1.0, (extra, D))
    return X, Z


def host_cov(name, X, nugget=None):
    """K(X, X) + diag(nugget) of a family in float64 on the host (the CPU tests' stand-in for the device fill, which the GPU
    tests take back with to_host())."""
    kind, hyp, nug = FAMILIES[name]
    X = np.asarray(X, dtype=float)
    S = X / np.asarray(hyp[:D]) if kind == K_SE else X
    r2 = np.zeros((X.shape[0], X.shape[0]))
    for k in range(D):      # from coordinate differences: exactly 0 between identical points (the planted rows)
        r2 += (S[:, k][:, None] - S[:, k][None, :]) ** 2
    if kind == K_SE:
        K = hyp[D] * np.exp(-0.5 * r2)
    elif kind == K_MATERN32:
        t = np.sqrt(3.0 * r2) / hyp[0]
        K = hyp[1] * (1.0 + t) * np.exp(-t)
    else:
        t = np.sqrt(5.0 * r2) / hyp[0]
        K = hyp[1] * (1.0 + t + t * t / 3.0) * np.exp(-t)
    K = 0.5 * (K + K.T)
    K[np.diag_indices_from(K)] += nug if nugget is None else nugget
    return K


def graded_block(n=128):
    """D A D with D = diag(10^(-4 i / (n-1))) and A the leading n points of family W: an SPD block whose pivots span eight
    decades although A itself is well conditioned."""
    X, _ = family_points("W", n)
    dg = 10.0 ** (-4.0 * np.arange(n) / (n - 1.0))
    return host_cov("W", X) * dg[:, None] * dg[None, :]


# ---- extended-precision products -------------------------------------------------------------------------------------
_POOL = ThreadPoolExecutor(max_workers=8)   # NumPy's longdouble loops release the GIL


def _ld_matmul(A, B, chunk=512):
    """A @ B with every product and sum in np.longdouble (A: m x k, B: k x p, float64 in); k in chunks over a thread pool."""
    A = np.asarray(A)
    B = np.asarray(B)
    k = A.shape[1]

    def part(k0):
        return np.dot(A[:, k0:k0 + chunk].astype(LD), B[k0:k0 + chunk].astype(LD))

    out = None
    for p in _POOL.map(part, range(0, k, chunk)):
        out = p if out is None else out + p
    return out


def sample_rows(n, seed=0):
    """48 seeded rows plus the first, the middle and the last one (sorted, unique); all rows when n is small."""
    if n <= 51:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    r = set(int(i) for i in rng.choice(n, size=48, replace=False))
    r.update((0, n // 2, n - 1))
    return np.array(sorted(r))


def _llt_rows(L, rows, chunk=512):
    """(L L^T)[rows, :] in np.longdouble for a LOWER triangular L: column chunk [k0, k1) only meets the rows >= k0 on both sides."""
    n = L.shape[0]
    rows = np.asarray(rows)

    def part(k0):
        sel = rows >= k0
        out = np.zeros((rows.size, n), dtype=LD)
        if sel.any():
            Lq = L[k0:, k0:k0 + chunk].astype(LD)
            out[sel, k0:] = np.dot(Lq[rows[sel] - k0], Lq.T)
        return out

    acc = np.zeros((rows.size, n), dtype=LD)
    for p in _POOL.map(part, range(0, n, chunk)):
        acc += p
    return acc


# ---- metrics ---------------------------------------------------------------------------------------------------------
def _factor_residual(K, L, rows):
    n = K.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    L = np.tril(np.asarray(L, dtype=float))
    R = np.abs(K[rows].astype(LD) - _llt_rows(L, rows))
    return rows, L, R


def eta(K, L, rows=None):
    """(eta_cw, eta_s) from one residual K - L L^T over the given rows (all when None):
    eta_cw = max_ij |K - L L^T|_ij / (|L| |L^T|)_ij, the componentwise backward error of the factor (Higham Thm 10.3 bounds it
    by gamma_{n+1} for a Cholesky factorisation); eta_s = max_ij |K - L L^T|_ij / sqrt(K_ii K_jj)."""
    rows, L, R = _factor_residual(K, L, rows)
    aL = np.abs(L)
    den = aL[rows] @ aL.T
    dg = np.sqrt(np.diag(K))
    return float(np.max(R / den)), float(np.max(R / (dg[rows][:, None] * dg[None, :])))


def eta_cw(K, L, rows=None):
    return eta(K, L, rows)[0]


def eta_s(K, L, rows=None):
    return eta(K, L, rows)[1]


def omega(K, a, y):
    """Oettli-Prager componentwise backward error of a as a solution of K a = y: max_i |K a - y|_i / (|K| |a| + |y|)_i."""
    a = np.asarray(a, dtype=float).reshape(K.shape[0], -1)
    y = np.asarray(y, dtype=float).reshape(K.shape[0], -1)
    r = np.abs(_ld_matmul(K, a) - y.astype(LD))
    den = np.abs(K) @ np.abs(a) + np.abs(y)
    return float(np.max(r / den))


def omega_tri(L, W, B, rows=None):
    """The same for L W = B with a lower triangular L, per column, then maximised; on the given rows (all when None)."""
    n = L.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    L = np.tril(np.asarray(L, dtype=float))
    W = np.asarray(W, dtype=float).reshape(n, -1)
    B = np.asarray(B, dtype=float).reshape(n, -1)
    r = np.abs(_ld_matmul(L[rows], W) - B[rows].astype(LD))
    den = np.abs(L[rows]) @ np.abs(W) + np.abs(B[rows])
    return float(np.max(np.max(r / den, axis=0)))


def rho_inv(K, P, cols=None):
    """max_ij |P K - I|_ij / (|P| |K|)_ij on the given columns (all when None): the left residual of P as an inverse of K."""
    n = K.shape[0]
    cols = np.arange(n) if cols is None else np.asarray(cols)
    Kc = np.ascontiguousarray(K[:, cols])
    R = _ld_matmul(P, Kc)
    R[cols, np.arange(cols.size)] -= 1
    den = np.abs(P) @ np.abs(Kc)
    return float(np.max(np.abs(R) / den))


# ---- emulations ------------------------------------------------------------------------------------------------------
def _chol_unblocked(A):
    """Column-by-column Cholesky of a small block (the 16 x 16 step of the leaf)."""
    A = np.array(A, dtype=float)
    n = A.shape[0]
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def _inv_substitution(L):
    """Inverse of a small lower triangular block by forward substitution, row by row (T_p of the leaf)."""
    n = L.shape[0]
    T = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        T[i] = (e - L[i, :i] @ T[:i]) / L[i, i]
    return T


def tri_inverse(L, base=16):
    """L^-1 from the inverses of the two halves, [A 0; C B]^-1 = [A^-1 0; -B^-1 (C A^-1)  B^-1], split on multiples of `base`,
    forward substitution at order <= base (chol.hip: binv_build_rec / chol_trtri above the leaf, the leaf's own block columns
    below)."""
    n = L.shape[0]
    if n <= base:
        return _inv_substitution(L)
    s = (n // base // 2) * base
    if s == 0:
        s = base
    Ai = tri_inverse(L[:s, :s], base)
    Bi = tri_inverse(L[s:, s:], base)
    T = np.zeros((n, n))
    T[:s, :s] = Ai
    T[s:, s:] = Bi
    T[s:, :s] = -(Bi @ (L[s:, :s] @ Ai))
    return T


_INNER = {16: 0, 128: 16, 1024: 128}


def _factor_diag(Dm, inner):
    if inner == 0 or Dm.shape[0] <= 16:
        return _chol_unblocked(Dm)
    if Dm.shape[0] <= inner:           # a ragged last block no larger than the next scheme's own block
        return _factor_diag(Dm, _INNER[inner])
    return chol_block_inverse(Dm, inner)


def chol_block_inverse(K, b, panel_dtype=np.float64):
    """Right-looking Cholesky in float64 whose panel solve is A21 <- A21 inv(L11)^T with an explicit inverse of the b-order
    diagonal factor (b = 16, 128, 1024).  The diagonal block itself is factored by the next scheme down: 1024 by 128, 128 by
    16 (the leaf), 16 unblocked.  `panel_dtype=np.float32` rounds the panel product's operands: a factor the metrics must
    reject (the host tests feed it to them)."""
    inner = _INNER[b]
    A = np.array(K, dtype=float)
    n = A.shape[0]
    for j in range(0, n, b):
        w = min(b, n - j)
        D11 = A[j:j + w, j:j + w]
        L11 = _factor_diag(D11, inner)
        A[j:j + w, j:j + w] = L11
        if j + w < n:
            T = tri_inverse(L11)
            P = (A[j + w:, j:j + w].astype(panel_dtype) @ T.T.astype(panel_dtype)).astype(np.float64)
            A[j + w:, j:j + w] = P
            for c0 in range(0, n - j - w, 1024):      # lower block columns of the trailing update only
                c1 = min(c0 + 1024, n - j - w)
                A[j + w + c0:, j + w + c0:j + w + c1] -= P[c0:] @ P[c0:c1].T
    return np.tril(A)


def forward_block_inverse(L, B, b):
    """W = L^-1 B by block forward substitution, every diagonal solve a product with the explicit b-order inverse (vector or
    matrix right-hand side; b >= n: one product with the whole inverse)."""
    n = L.shape[0]
    R = np.array(B, dtype=float).reshape(n, -1)
    W = np.zeros_like(R)
    for j in range(0, n, b):
        w = min(b, n - j)
        W[j:j + w] = tri_inverse(L[j:j + w, j:j + w]) @ (R[j:j + w] - L[j:j + w, :j] @ W[:j])
    return W.reshape(np.shape(B))


def backward_block_inverse(L, B, b):
    """Z = L^-T B, the transposed sweep of forward_block_inverse (same block boundaries)."""
    n = L.shape[0]
    R = np.array(B, dtype=float).reshape(n, -1)
    Z = np.zeros_like(R)
    starts = list(range(0, n, b))
    for j in reversed(starts):
        w = min(b, n - j)
        Z[j:j + w] = tri_inverse(L[j:j + w, j:j + w]).T @ (R[j:j + w] - L[j + w:, j:j + w].T @ Z[j + w:])
    return Z.reshape(np.shape(B))


def solve_block_inverse(L, y, b):
    """K^-1 y through forward and backward substitution with explicit b-order inverses (gpx_potrs)."""
    return backward_block_inverse(L, forward_block_inverse(L, y, b), b)


def inverse_by_halving(L):
    """(L^-1, P = L^-T L^-1): the inverse of the factor from products of the halves' inverses, then the product (gpx_potri)."""
    Li = tri_inverse(np.tril(L))
    return Li, Li.T @ Li


def reference_values(K, lapack, y=None, Kxz=None, rows=None, inverse=False, bs=(128, 1024)):
    """{metric: {"lapack" | "b<order>": value}} on one matrix K.  `lapack` = dict(L=, alpha=, W=, P=) of LAPACK's results
    (dpotrf, dpotrs of y, dtrtrs of Kxz, the inverse; the entries a metric needs).  The emulated solves run on the emulated
    factor of the same block order (one emulated factor alive at a time)."""
    out = {"eta_cw": {}, "eta_s": {}}
    if y is not None:
        out["omega"] = {"lapack": omega(K, lapack["alpha"], y)}
    if Kxz is not None:
        out["omega_tri"] = {"lapack": omega_tri(lapack["L"], lapack["W"], Kxz, rows)}
    if inverse:
        out["rho_inv"] = {"lapack": rho_inv(K, lapack["P"], rows)}
    for nm in ["lapack"] + ["b%d" % b for b in bs]:
        b = int(nm[1:]) if nm != "lapack" else 0
        L = np.tril(lapack["L"]) if b == 0 else chol_block_inverse(K, b)
        out["eta_cw"][nm], out["eta_s"][nm] = eta(K, L, rows)
        if b and y is not None:
            out["omega"][nm] = omega(K, solve_block_inverse(L, y, b), y)
        if b and Kxz is not None:
            out["omega_tri"][nm] = omega_tri(L, forward_block_inverse(L, Kxz, b), Kxz, rows)
        if b and inverse:
            out["rho_inv"][nm] = rho_inv(K, inverse_by_halving(L)[1], rows)
        del L
    return out


# ---- the bound -------------------------------------------------------------------------------------------------------
def check_bound(label, device, refs, cap=None, margin=MARGIN):
    """device <= margin * max(refs) -- refs: {name: value} of LAPACK and the emulations on the SAME matrix -- and, when `cap` is
    given (family W: the gamma bound of a backward-stable method), device <= cap as well.  Prints every figure before it
    asserts; returns the ratio device / max(refs)."""
    top = max(refs.values())
    ratio = device / top
    print("  %-34s device %.3e | %s | ratio %.2f of %g%s"
          % (label, device, "  ".join("%s %.3e" % kv for kv in refs.items()), ratio, margin,
             "" if cap is None else " | cap %.3e" % cap))
    assert np.isfinite(device), "%s: device value is not finite" % label
    assert device <= margin * top, "%s: device %.3e > %g x %.3e (largest reference value)" % (label, device, margin, top)
    if cap is not None:
        assert device <= cap, "%s: device %.3e above the backward-stable bound %.3e on a well-conditioned matrix" % (label, device, cap)
    return ratio


# ---- planted pivots --------------------------------------------------------------------------------------------------
# size -> [(q, p)]: planted row p and its partner q < p (distinct, below 1000, never a planted row themselves).  p sits on the last /
# first column of a 16-block, a leaf, a 1024 block, the recursion's split (split(4608) = 2304), a 4096 panel (4096 = the first
# pivot of the diagonal block the look-ahead factors on the side stream; 8192 = the first of the ragged last panel) and on the
# last row (1408, 4608, 8320 padded: the padding must never be counted).
PLANTS = {
    1300: [(0, 1), (3, 15), (5, 16), (60, 127), (100, 128), (500, 1023), (7, 1024), (900, 1299)],
    4500: [(11, 2047), (22, 2048), (33, 2303), (44, 2304)],
    8300: [(11, 4095), (22, 4096), (33, 4097), (44, 8191), (55, 8192), (66, 8299)],
}
PLANTS_TWO = [[(11, 1000), (22, 5000)], [(11, 4100), (22, 4090)]]   # n = 8300: two panels at once; one leaf apart, larger first
PIV_MIN = 1e-13 * 1.1      # GP._factor: 1e-13 * (signalSize + max nugget) on family W


def planted(name, n, pairs, base_nugget=None):
    """(X, per-point nugget) of a family with X[p] = X[q] and nugget 0 at p and q for every (q, p) in pairs: row p of K then
    equals row q exactly, and pivot p of the factorisation is zero up to rounding."""
    X, _ = family_points(name, n)
    nug = np.full(n, FAMILIES[name][2] if base_nugget is None else base_nugget)
    for q, p in pairs:
        assert q < p
        X[p] = X[q]
        nug[p] = nug[q] = 0.0
    return X, nug


def ldlt_pivots(K, piv_min=PIV_MIN):
    """Pivots d of the unblocked L D L^T of K without pivoting (right-looking, float64).  A pivot of at most `piv_min` in
    magnitude eliminates nothing, as the device's drop policy has it (its column is zero up to rounding)."""
    A = np.array(K, dtype=float)
    n = A.shape[0]
    d = np.empty(n)
    for j in range(n):
        d[j] = A[j, j]
        if j + 1 < n and abs(d[j]) > piv_min:
            c = A[j + 1:, j].copy()
            A[j + 1:, j + 1:] -= np.outer(c / d[j], c)
    return d


def check_pivot_report(reported, planted_rows):
    """The non-positive-definite report must name the FIRST planted row, 1-based."""
    want = min(planted_rows) + 1
    assert reported == want, "reported pivot %r, the first planted row is %d (1-based %d)" % (reported, want - 1, want)


def check_drop(dropped, alpha, planted_rows, alpha_reduced, tol=1e-10):
    """Drop policy: exactly len(planted_rows) points dropped, alpha exactly 0.0 there, and the other components those of the
    solve with the planted rows and columns deleted (relative max-norm <= tol)."""
    ps = sorted(planted_rows)
    assert dropped == len(ps), "dropped %r points, planted %d" % (dropped, len(ps))
    alpha = np.asarray(alpha)
    assert np.all(alpha[ps] == 0.0), alpha[ps]
    keep = np.setdiff1d(np.arange(alpha.size), ps)
    err = np.max(np.abs(alpha[keep] - alpha_reduced)) / np.max(np.abs(alpha_reduced))
    assert err <= tol, err
    return err
