"""Per-entry error metrics, longdouble references, float64 comparators and mutants for the point gradients of the posterior variance
and of IVAR (NumPy / SciPy only; data and yardsticks of tests/test_pointgrad_host.py and tests/test_gpu_pointgrad_bounds.py, not
product code).  Same conventions as tests/posterior_ref.py, whose cases, evaluation sets and longdouble solves are reused.

THE QUANTITIES (gpexp_amd/csrc/grad.hip's header).  beta = K^-1 B, B = K(X, Z);  Dz_l[j, m] = dk(z_m, x_j)[l],  Dx_l[j, i] =
dk(x_j, x_i)[l] in grad.hip's conventions (squared exponential: the reference's, with the signal size twice; Matern and the 1-D Mehler
kernel: the true derivative);  nd[j, l] = d noise(x_j) / d x_jl (optional), mask[j, i] = [|x_i - x_j| < 1e-10],
A_l = Dx_l + mask * nd[:, l] (row j carries nd[j, l]):

    G[j, l, m] = beta_jm ( 2 Dz_l[j, m] + 2 (A_l beta)[j, m] - A_l[j, j] beta_jm )         gpx_var_grad          (n, d, M)
    N[m, l]    = -2 sum_j Dz_l[j, m] beta_jm                                               gpx_var_grad_newpt    (M, d)
    I[j, l]    = mean_m G[j, l, m]                                                         gpx_ivar_grad[_w|_rows]  (n, d)

Without nd, A_l = Dx_l has a zero diagonal and G = 2 beta (Dz_l + Dx_l beta).  Everything in np.longdouble.

THE METRIC.  omega = max over ENTRIES of |got - ref| / (u S), u = 2^-53, S the first-order effect on that entry of a relative
perturbation u of every input entry (K, B, Dz, Dx, nd) -- posterior_ref's convention.  With R = |K^-1| (|B| + |K| |beta|) (n x M, the
bound on d beta; K^-1 from the inverse of the longdouble factor), Ab = |Dx_l| + mask |nd_l| and a = diag(A_l):

    S_G[j, l, m] = R_jm |2 Dz_l + 2 A_l beta - a_j beta|_jm
                   + |beta_jm| ( 2 |Dz_l|_jm + 2 (Ab |beta|)_jm + 2 (Ab R)_jm + |a_j| (|beta_jm| + R_jm) )
    S_N[m, l]    = 2 ( |Dz_l[:, m]|^T |beta_m| + |gamma|^T |b_m| + |gamma|^T |K| |beta_m| ),   gamma = K^-1 Dz_l[:, m]
    S_I          = mean_m S_G

(d G = d beta (2 Dz + 2 A beta - a beta) + beta (2 dDz + 2 dA beta + 2 A d beta - da beta - a d beta), every term in absolute value;
without nd, a = 0 and S_G = 2 R |Dz_l + Dx_l beta| + 2 |beta| (|Dz_l| + |Dx_l| |beta| + |Dx_l| R).  N = -2 gamma^T b, so
d N = -2 (dDz^T beta + gamma^T d b - gamma^T dK beta): the adjoint form needs no |K^-1|.)  No entry is left out of the maximum; where
S = 0 (n = 1: one training point, evaluated on itself) `got` must equal the reference exactly.

INPUTS AND ALLOWANCE.  K and B are GIVEN float64 arrays (the device's own fills taken back; the CPU tests' stand-ins).  Dz and Dx are
formed inside the gradient kernels from the points and cannot be taken back, so the reference forms them from the points in longdouble
(plain longdouble: a few 2^-64 (1 + x) relative, pinned against 50 digits) and every metric subtracts an ALLOWANCE: the per-entry
bound E_D of the device's Dz / Dx propagated to first order, A_G = 2 |beta_jm| (E_Dz + (E_Dx |beta|))_jm, A_N = 2 sum_j E_Dz |beta|,
A_I = mean_m A_G; omega counts only the excess (posterior_ref.reference_from_points' rule).

    radial kinds   D_l = c_l f(s) (u_l - p_l), s = sum_k ((u_k - p_k) scale_k)^2, t = sqrt s
                     SE  f = sig e^(-s/2), c_l = -sig scale_l^2;  Matern-3/2  f = e^-t, c = -sig scale^2;  Matern-5/2  f = (1 + t) e^-t,
                     c = -sig scale^2 / 3
                   E_f = (8 + 0.2 x) 2u |f| + |df/ds| s (2d + 16) u + 2^-1073      kernel_reference's constants, its "diff" form,
                     x = s/2 (SE) or t;  |df/ds| s = f s / 2, t e^-t / 2, s e^-t / 2  (finite as t -> 0)
                   E_D = |c_l| |u_l - p_l| E_f + NR u |D_l|,  NR = 9 (11 for Matern-5/2) roundings counted from radial_pair /
                     radial_finish / dkpair: the difference (1); scale_l stored rounded -- 1 / cl one rounding, sqrt(3 | 5) / rho
                     two -- and entering squared (4); sig * scale * scale (2); the product with the radial factor and the one with
                     the difference (2); Matern-5/2: the constant 1/3 and its product (2).
    Mehler, d = 1  D = -q k(u, p), q = 2 c1 u - c2 p;  E_D = |q| E_k + u |k| (5 (|2 c1 u| + |c2 p|) + 2 |q|): E_k kernel_reference's
                     Mehler bound; c1 = t^2 / (2 (1 - t^2)) and c2 = t / (1 - t^2) from the host (4 roundings at most) and their
                     product with the coordinate (1) on either term, the subtraction and the product with k (2).

The roundings of the sums, of the products with beta and of the solves are NOT in the allowance: they are what omega measures.

THE BOUND.  device omega <= MARGIN (= 8) x the larger of the two COMPARATORS on the same arrays -- "lapack" (cho_factor / cho_solve,
NumPy sums) and "b128" (chol_stability_ref's block-inverse emulation, forward then backward) -- never a device value.  Where that
maximum is below 1 it counts as 1 ("one" in the printed figures): at n = 1 both comparators are exactly 0, and less than one rounding
cannot be asked of any route.  omega_I is a mean of M errors of either sign; as in posterior_ref.comparator_omegas the comparators'
omega_G / sqrt(M) joins them."""
import functools
import decimal
from decimal import Decimal

import numpy as np
import scipy.linalg as sl

import chol_stability_ref as CR
import design_replay_ref as DR
import kernel_reference as KR
import posterior_ref as P
from chol_stability_ref import MARGIN, U, check_bound   # noqa: F401  (re-exported: the tests' one import)
from helpers import NoiseFunc

LD = P.LD
CASES = ("se-well", "se-tiny-noise", "m52-tiny-noise", "m32-per-point")      # posterior_ref's, n = 300, M = 130, d = 3
MEHLER1 = dict(kind="mehler", d=1, t=[0.6])
DRAWN = {      # name -> (spec, n, noise, seed): cases drawn here with posterior_ref's layout of the evaluation set
    "mehler-1d": (MEHLER1, 150, 1e-4, 6101),
    "m52-large": (P.M52, 4100, 1e-4, 6102),     # 4224 padded: the smallest n whose solves take the block inverses
}
EDGES = ((1, 1), (2, 1), (3, 2), (127, 127), (128, 128), (129, 129), (257, 130))
EDGE_KINDS = {"se": "se-tiny-noise", "matern32": "m32-per-point", "matern52": "m52-tiny-noise"}
DUP_ROWS = (3, 17, 140)     # the heteroscedastic case: rows 17 and 140 duplicate row 3
N_ON, N_NEAR = P.N_ON, P.N_NEAR


@functools.lru_cache(maxsize=None)
def _drawn(name):
    spec, n, noise, seed = DRAWN[name]
    d = int(spec["d"])
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, d))
    fixed = [0, 127, 128, n - 1]
    others = rng.choice(np.setdiff1d(np.arange(n), fixed), size=N_ON - len(fixed), replace=False)
    near = rng.choice(n, size=N_NEAR, replace=False)
    Z = rng.uniform(-1.0, 1.0, (P.M_EVAL, d))
    Z[:N_ON] = X[np.concatenate([fixed, others])]
    Z[N_ON:N_ON + N_NEAR] = X[near] + 1e-7 * rng.standard_normal((N_NEAR, d))
    return dict(spec=spec, X=P._ro(X), Z=P._ro(Z), nugget=float(noise), n=n)


def problem(name, n=None, m=None, hetero=False):
    """dict(spec, X (n, d), Z (m, d), nugget (float or (n,)), nd (None or (n, d))): the leading n rows / m columns of a case (all by
    default).  hetero: rows 17 and 140 become copies of row 3 and nd = helpers.NoiseFunc(d).deriv(X)."""
    c = _drawn(name) if name in DRAWN else P.case(name, max(P.M_EVAL, int(m or 0)))     # (M > 130: posterior_ref draws that many)
    n = c["n"] if n is None else int(n)
    m = c["Z"].shape[0] if m is None else int(m)
    X, Z, nug = np.array(c["X"][:n]), np.array(c["Z"][:m]), c["nugget"]
    nug = nug if np.ndim(nug) == 0 else np.array(nug[:n])
    nd = None
    if hetero:
        for r in DUP_ROWS[1:]:
            if r < n:
                X[r] = X[DUP_ROWS[0]]
        nd = np.asarray(NoiseFunc(X.shape[1]).deriv(X), dtype=float)
    return dict(spec=c["spec"], X=X, Z=Z, nugget=nug, nd=nd)


def host_fills(p):
    """(K with the nugget, B = K(X, Z)) in float64 on the host: the CPU tests' stand-ins for the device's fills."""
    spec, X, Z = p["spec"], p["X"], p["Z"]
    f = (lambda A, B: P.mehler_f64(spec, A, B)) if spec["kind"] == "mehler" else (lambda A, B: DR.cov_f64(spec, A, B))
    K = f(X, X)
    K = 0.5 * (K + K.T)
    K[np.diag_indices_from(K)] += p["nugget"]
    return K, f(X, Z)


# ---- the kernels and their point derivatives from the points -----------------------------------------------------------------------
def _consts_ld(spec):
    """(sig, scale[d], c1[d], c2[d]) in longdouble from the double hyper-parameters (kernel_reference._params at 50 digits)."""
    sig, sc, c1, c2 = KR._params(spec)
    cv = lambda v: None if v is None else [DR._ld_of_decimal(x) for x in v]     # noqa: E731
    return DR._ld_of_decimal(sig), cv(sc), cv(c1), cv(c2)


def kernel_ld(spec, Up, Pp):
    """k(u_a, p_b) in plain longdouble (the central-difference test's kernel; the references take K and B as given)."""
    return _pairs_ld(spec, Up, Pp)[0]


def _pairs_ld(spec, Up, Pp):
    """(k, [D_l], aux) for all pairs (u_a, p_b) in longdouble; aux = the float64 pieces the bound E_D is built from."""
    kind, d = spec["kind"], int(spec["d"])
    sig, sc, c1, c2 = _consts_ld(spec)
    Up, Pp = np.asarray(Up, dtype=LD), np.asarray(Pp, dtype=LD)
    if kind == "mehler":
        assert d == 1, "point derivatives exist for the 1-D Mehler kernel only"
        u, p = Up[:, 0][:, None], Pp[:, 0][None, :]
        x = c1[0] * (u * u + p * p) - c2[0] * u * p
        k = sig * np.exp(-x)
        q = LD(2) * c1[0] * u - c2[0] * p
        aux = dict(k=k, x=x, T=c1[0] * (u * u + p * p) + np.abs(c2[0] * u * p), q=q, t1=np.abs(LD(2) * c1[0] * u) + 0 * p,
                   t2=np.abs(c2[0] * p) + 0 * u)
        return k, [-q * k], aux
    diff = [Up[:, l][:, None] - Pp[:, l][None, :] for l in range(d)]
    s = sum((diff[l] * sc[l]) ** 2 for l in range(d))
    if kind == "se":
        f = sig * np.exp(-s / LD(2))
        k, x, dfs = f, s / LD(2), f * s / LD(2)
        cl = [-sig * sc[l] * sc[l] for l in range(d)]
    else:
        t = np.sqrt(s)
        e = np.exp(-t)
        if kind == "matern32":
            f, k, dfs = e, sig * (LD(1) + t) * e, t * e / LD(2)
            cl = [-sig * sc[l] * sc[l] for l in range(d)]
        else:
            f, k, dfs = (LD(1) + t) * e, sig * (LD(1) + t + s / LD(3)) * e, s * e / LD(2)
            cl = [-sig * sc[l] * sc[l] / LD(3) for l in range(d)]
        x = t
    return k, [cl[l] * f * diff[l] for l in range(d)], dict(f=f, x=x, dfs=dfs, cl=cl, diff=diff)


NR = {"se": 9.0, "matern32": 9.0, "matern52": 11.0}      # the roundings of c_l f diff_l besides the radial factor's own (docstring)


def deriv_pairs(spec, Up, Pp):
    """([D_l] longdouble, [E_D,l] float64), each (len(Up), len(Pp)): D_l[a, b] = dk(u_a, p_b)[l] and the bound on the device's error in
    it (module docstring)."""
    kind, d = spec["kind"], int(spec["d"])
    _, D, aux = _pairs_ld(spec, Up, Pp)
    fl = lambda a: np.abs(np.asarray(a, dtype=float))     # noqa: E731
    if kind == "mehler":
        k, x = fl(aux["k"]), fl(aux["x"])
        Ek = (8.0 + 3.0 * d + 0.2 * x) * 2.0 * U * k + k * (2.0 * d + 16.0) * U * fl(aux["T"]) + KR.DENORMAL_STEP
        q = fl(aux["q"])
        return D, [q * Ek + U * k * (5.0 * (fl(aux["t1"]) + fl(aux["t2"])) + 2.0 * q)]
    Ef = (8.0 + 0.2 * fl(aux["x"])) * 2.0 * U * fl(aux["f"]) + fl(aux["dfs"]) * (2.0 * d + 16.0) * U + KR.DENORMAL_STEP
    return D, [abs(float(aux["cl"][l])) * fl(aux["diff"][l]) * Ef + NR[kind] * U * fl(D[l]) for l in range(d)]


def deriv_f64(spec, Up, Pp):
    """[D_l] in float64 in the order of radial_pair / radial_finish (Mehler: of kpair / dk): what E_D is pinned on, on the host."""
    kind, d = spec["kind"], int(spec["d"])
    Up, Pp = np.asarray(Up, dtype=float), np.asarray(Pp, dtype=float)
    if kind == "mehler":
        t = float(spec["t"][0])
        om = 1.0 - t * t
        c1, c2, sig = t * t / (2.0 * om), t / om, om ** -0.5
        u, p = Up[:, 0][:, None], Pp[:, 0][None, :]
        kv = sig * np.exp(-(c1 * u * u + c1 * p * p - c2 * u * p))
        return [-(2.0 * c1 * u - c2 * p) * kv]
    sig, sc = DR._params_f64(spec)
    diff = [Up[:, l][:, None] - Pp[:, l][None, :] for l in range(d)]
    r2 = np.zeros(diff[0].shape)
    for l in range(d):
        r2 += (diff[l] * sc[l]) ** 2
    t = np.sqrt(r2)
    f = sig * np.exp(-0.5 * r2) if kind == "se" else np.exp(-t) if kind == "matern32" else (1.0 + t) * np.exp(-t)
    out = []
    for l in range(d):
        c = -sig * sc[l] * sc[l]
        out.append((c * (1.0 / 3.0) if kind == "matern52" else c) * (f * diff[l]))
    return out


_CTX = decimal.Context(prec=50)


def deriv_decimal(spec, u, p):
    """[D_l] of ONE pair of points at 50 digits."""
    kind, d = spec["kind"], int(spec["d"])
    sig, sc, c1, c2 = KR._params(spec)
    with decimal.localcontext(_CTX):
        u, p = [Decimal(float(v)) for v in u], [Decimal(float(v)) for v in p]
        if kind == "mehler":
            x = c1[0] * (u[0] * u[0] + p[0] * p[0]) - c2[0] * u[0] * p[0]
            return [-(2 * c1[0] * u[0] - c2[0] * p[0]) * sig * (-x).exp()]
        s = sum(((u[l] - p[l]) * sc[l]) ** 2 for l in range(d))
        t = s.sqrt()
        if kind == "se":
            return [-sig * sc[l] * sc[l] * sig * (-s / 2).exp() * (u[l] - p[l]) for l in range(d)]
        f = (-t).exp() if kind == "matern32" else (1 + t) * (-t).exp() / 3
        return [-sig * sc[l] * sc[l] * f * (u[l] - p[l]) for l in range(d)]


def coincidence_mask(X):
    """mask[j, i] = |x_i - x_j| < 1e-10 (gp.py:308; grad.hip's same_point), from coordinate differences in float64."""
    X = np.asarray(X, dtype=float)
    s = np.zeros((X.shape[0], X.shape[0]))
    for l in range(X.shape[1]):
        s += (X[:, l][:, None] - X[:, l][None, :]) ** 2
    return np.sqrt(s) < 1e-10


# ---- the longdouble reference ------------------------------------------------------------------------------------------------------
def _ld_dot(A, B):
    return np.dot(np.asarray(A, dtype=LD), np.asarray(B, dtype=LD))


def _assemble(spec, X, Z, nd, beta, Kabs, Babs, Kinv, cols=None, perturb=None):
    """val / scale / allow / f64 from beta (n, M') in longdouble, |K|, |B| and K^-1 (float64: they only scale).  perturb = a function
    applied to every Dz_l, Dx_l and to nd (the perturbation test of S)."""
    n, d = X.shape
    Zc = Z if cols is None else Z[cols]
    m = Zc.shape[0]
    Dz, EDz = deriv_pairs(spec, Zc, X)
    Dz, EDz = [a.T for a in Dz], [a.T for a in EDz]                 # (n, M'): Dz_l[j, m] = dk(z_m, x_j)[l]
    if perturb is not None:
        Dz = [perturb(a) for a in Dz]
        nd = None if nd is None else perturb(np.asarray(nd, dtype=LD))
    ab = np.abs(np.asarray(beta, dtype=float))
    R = np.abs(Kinv) @ (Babs + Kabs @ ab)
    mask = coincidence_mask(X) if nd is not None else None
    G, N = np.zeros((n, d, m), dtype=LD), np.zeros((m, d), dtype=LD)
    SG, SN, AG, AN = np.zeros((n, d, m)), np.zeros((m, d)), np.zeros((n, d, m)), np.zeros((m, d))
    f64 = dict(Dz=[], Dx=[], mask=mask, nd=None if nd is None else np.asarray(nd, dtype=float), kinv=Kinv)
    Dx, EDx = _dx(spec, X)
    for l in range(d):
        Dxl, EDxl = Dx[l], EDx[l]
        if perturb is not None:
            Dxl = perturb(Dxl)
        A, Aabs = Dxl, np.abs(np.asarray(Dxl, dtype=float))
        if nd is not None:
            A = Dxl + mask * nd[:, l][:, None].astype(LD)
            Aabs = Aabs + mask * np.abs(np.asarray(nd[:, l], dtype=float))[:, None]
        a = np.diag(A).copy()
        Ab = _ld_matmul(A, beta)
        inner = LD(2) * Dz[l] + LD(2) * Ab - a[:, None] * beta
        G[:, l, :] = beta * inner
        N[:, l] = -LD(2) * np.sum(Dz[l] * beta, axis=0)
        aDz, af = np.abs(np.asarray(Dz[l], dtype=float)), np.abs(np.asarray(a, dtype=float))[:, None]
        SG[:, l, :] = R * np.abs(np.asarray(inner, dtype=float)) + ab * (2.0 * aDz + 2.0 * (Aabs @ ab) + 2.0 * (Aabs @ R) + af * (ab + R))
        gam = np.abs(Kinv @ np.asarray(Dz[l], dtype=float))
        SN[:, l] = 2.0 * (np.sum(aDz * ab, axis=0) + np.sum(gam * Babs, axis=0) + np.sum(gam * (Kabs @ ab), axis=0))
        AG[:, l, :] = 2.0 * ab * (EDz[l] + EDxl @ ab)
        AN[:, l] = 2.0 * np.sum(EDz[l] * ab, axis=0)
        f64["Dz"].append(np.asarray(Dz[l], dtype=float))
        f64["Dx"].append(np.asarray(Dxl, dtype=float))
    val, scale, allow = {"G": G, "N": N}, {"G": SG, "N": SN}, {"G": AG, "N": AN}
    if cols is None:
        val["I"], scale["I"], allow["I"] = np.sum(G, axis=2) / LD(m), np.mean(SG, axis=2), np.mean(AG, axis=2)
    return dict(val=val, scale=scale, allow=allow, beta=beta, f64=f64, R=R, cols=cols)


def _dx(spec, X):
    """([Dx_l] longdouble, [E_Dx,l] float64), n x n each, every pair evaluated once; in row blocks over the thread pool when n is
    large (n = 4100: 16.8e6 pairs)."""
    n = X.shape[0]
    if n <= 1024:
        return deriv_pairs(spec, X, X)
    d = 1 if spec["kind"] == "mehler" else int(spec["d"])
    D, E = [np.empty((n, n), dtype=LD) for _ in range(d)], [np.empty((n, n)) for _ in range(d)]

    def block(r0):
        Db, Eb = deriv_pairs(spec, X[r0:r0 + 128], X)
        for l in range(d):
            D[l][r0:r0 + 128], E[l][r0:r0 + 128] = Db[l], Eb[l]
    list(CR._POOL.map(block, range(0, n, 128)))
    return D, E


def _ld_matmul(A, B):
    """A @ B in longdouble; row blocks over the thread pool when A is large."""
    if A.shape[0] <= 1024:
        return _ld_dot(A, B)
    B = np.asarray(B, dtype=LD)
    out = np.empty((A.shape[0], B.shape[1]), dtype=LD)

    def block(r0):
        out[r0:r0 + 128] = np.dot(np.asarray(A[r0:r0 + 128], dtype=LD), B)
    list(CR._POOL.map(block, range(0, A.shape[0], 128)))
    return out


def reference(K, B, p, perturb=None):
    """dict(val={G, N, I}, scale=, allow=, beta, f64={Dz, Dx, mask, nd}, R) of GIVEN arrays K (n, n; with the nugget), B (n, M) --
    float64, or longdouble for the central-difference test -- and the problem p (spec, X, Z, nd): L = chol(K), beta = L^-T L^-1 B,
    K^-1 from L^-1, all in longdouble."""
    Kl, Bl = np.asarray(K, dtype=LD), np.asarray(B, dtype=LD)
    L = DR.chol_ld(Kl)
    beta = P.solve_upper_ld(L, DR.solve_lower_ld(L, Bl))
    Li = DR.solve_lower_ld(L, np.eye(L.shape[0], dtype=LD))
    Kinv = np.asarray(_ld_dot(Li.T, Li), dtype=float)
    return _assemble(p["spec"], p["X"], p["Z"], p["nd"], beta, np.abs(np.asarray(K, dtype=float)), np.abs(np.asarray(B, dtype=float)), Kinv,
                     perturb=perturb)


def reference_sampled(K, B, p, cols):
    """The same for G and N on the sampled columns `cols` of a large case: beta from posterior_ref.reference_sampled (float64 factor,
    refinement against the exact residual), S from a float64 inverse (it only scales)."""
    cols = np.asarray(cols)
    rs = P.reference_sampled(K, B, np.zeros(B.shape[1]), cols)
    Kinv = sl.lapack.dpotri(sl.lapack.dpotrf(K, lower=1)[0], lower=1)[0]
    Kinv = np.tril(Kinv) + np.tril(Kinv, -1).T
    return _assemble(p["spec"], p["X"], p["Z"], p["nd"], rs["beta"], np.abs(K), np.abs(B[:, cols]), Kinv, cols=cols)


# ---- the metric --------------------------------------------------------------------------------------------------------------------
def omega(got, ref_val, scale, allow=None, where=None):
    """max |got - ref| / (u S) over the entries (`where`: an index of the LAST axis of G, the first of N), the error counted in excess
    of `allow`; an entry with S = 0 scores 0 when got equals the reference exactly and inf otherwise."""
    got = np.asarray(got, dtype=LD).reshape(ref_val.shape)
    err = np.abs(got - ref_val)
    exact = err == 0
    if allow is not None:
        err = np.maximum(err - np.asarray(allow, dtype=LD), LD(0))
    S = np.asarray(scale, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(np.where(S > 0, err / (LD(U) * S), np.where(exact, LD(0), LD(np.inf))), dtype=float)
    if where is not None:
        q = q[..., where] if q.ndim == 3 else q[where]
    return float(np.max(q)) if np.all(np.isfinite(q)) else float("inf")


def omegas(got, ref, where=None, allowance=True):
    """{metric: omega} for the metrics present in both `got` ({G, N, I}) and the reference.  allowance=False: the comparators, which
    start from the reference's own Dz / Dx rounded once."""
    return {k: omega(got[k], ref["val"][k], ref["scale"][k], ref["allow"][k] if allowance else None, None if k == "I" else where)
            for k in ref["val"] if k in got}


# ---- comparators and mutants -------------------------------------------------------------------------------------------------------
ROUTES = ("lapack", "b128")
# name -> (the metrics it is judged in, needs nd)
MUTANTS = {
    "radial-1e-11": (("N", "I"), False),      # Dz scaled by 1 + 1e-11
    "last-row": (("G", "I"), False),          # the G rows of the last training point scaled by 1 + 3e-10
    "last-coord": (("G", "I"), False),        # coordinate d - 1 of G scaled by 1 + 3e-10
    "diag-twice": (("I",), True),             # the diagonal entry of S = beta beta^T counted twice in I
    "tile-seam": (("G", "N"), False),         # evaluation column 128 reads column 127's beta
    "row-chunk": (("G", "N", "I"), False),    # training rows 32 .. 47 missing from the sums over j / i
    "dup-mask": (("G", "I"), True),           # the coincidence mask reduced to i == j
}
REL_BLIND = ("radial-1e-11", "last-row", "last-coord")      # pass posterior_ref.rel <= 1e-9, the older tests' assertion


def route_beta(route, K, B):
    if route == "lapack":
        return sl.cho_solve(sl.cho_factor(K, lower=True, check_finite=False), B, check_finite=False)
    b = int(route[1:])
    L = CR.chol_block_inverse(K, b)
    return CR.backward_block_inverse(L, CR.forward_block_inverse(L, B, b), b)


def route_values(route, K, B, ref, mutant=None):
    """{G, N[, I]} of a float64 route on the given arrays and the reference's Dz / Dx rounded to float64 (on the reference's sampled
    columns when it has them; then no I), with one defect when `mutant` names one (MUTANTS)."""
    f, cols = ref["f64"], ref["cols"]
    beta = route_beta(route, K, B if cols is None else np.ascontiguousarray(B[:, cols]))
    n, m = beta.shape
    d = len(f["Dz"])
    if mutant == "tile-seam":
        beta = beta.copy()
        beta[:, 128] = beta[:, 127]
    rows = np.ones(n, dtype=bool)
    if mutant == "row-chunk":
        rows[32:48] = False
    G, N, extra = np.zeros((n, d, m)), np.zeros((m, d)), np.zeros((n, d))
    for l in range(d):
        Dz, A = f["Dz"][l], f["Dx"][l]
        if mutant == "radial-1e-11":
            Dz = Dz * (1.0 + 1e-11)
        if f["nd"] is not None:
            A = A + (np.eye(n, dtype=bool) if mutant == "dup-mask" else f["mask"]) * f["nd"][:, l][:, None]
        a = np.diag(A)[:, None]
        G[:, l, :] = beta * (2.0 * Dz + 2.0 * (A[:, rows] @ beta[rows]) - a * beta)
        N[:, l] = -2.0 * np.sum(Dz[rows] * beta[rows], axis=0)
        extra[:, l] = np.mean(a * beta * beta, axis=1)
    if mutant == "last-row":
        G[-1] *= 1.0 + 3e-10
    if mutant == "last-coord":
        G[:, d - 1] *= 1.0 + 3e-10
    out = {"G": G, "N": N}
    if cols is None:
        out["I"] = np.mean(G, axis=2) + (extra if mutant == "diag-twice" else 0.0)
    return out


def comparator_omegas(ref, K, B):
    """{metric: {route: omega, ..., "one": 1}} of the comparators on the same arrays as the reference (module docstring, THE BOUND)."""
    out = {}
    for route in ROUTES:
        for k, v in omegas(route_values(route, K, B, ref), ref, allowance=False).items():
            out.setdefault(k, {})[route] = v
    if "I" in out:
        out["I"]["G/sqrt(M)"] = max(out["G"].values()) / np.sqrt(float(ref["val"]["G"].shape[2]))
    for k in out:
        out[k]["one"] = 1.0
    return out


def device_values(var_grad=None, newpt=None, ivar_grad=None):
    """The device's flat results in the reference's shapes: (n d, M) -> G, (M d,) -> N, (n d,) -> I (reshaped by omega)."""
    out = {}
    if var_grad is not None:
        out["G"] = var_grad
    if newpt is not None:
        out["N"] = newpt
    if ivar_grad is not None:
        out["I"] = ivar_grad
    return out


def check_all(label, got, cmp_):
    """check_bound for every metric of `got` ({metric: device omega}; "G(on point)" is judged by cmp_["G"]): every figure is printed
    before the first failure surfaces; returns the failures' messages."""
    failures = []
    for k, value in got.items():
        try:
            check_bound("%s omega_%s" % (label, k), value, cmp_[k.split("(")[0]])
        except AssertionError as e:
            failures.append(str(e))
    return failures
