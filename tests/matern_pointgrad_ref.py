"""Yardstick of the Matern point gradients (data, not product code): the gradients of the posterior variance w.r.t. point
locations as dense NumPy algebra, with the TRUE point derivative of the isotropic Matern kernels.  `oracle.kernel_derivative`
raises for Matern (the reference's KernelIsoMatern has no `derivative`), so the closed form lives here; it is validated
against central differences of the oracle's posterior variance in tests/test_matern_pointgrad_host.py.

    dk(u, p)[l] = g(r) (u_l - p_l),   t = sqrt(2 nu) |u - p| / rho
    nu = 3/2:  k = sig (1 + t) e^-t            g = -sig (3 / rho^2) e^-t
    nu = 5/2:  k = sig (1 + t + t^2/3) e^-t    g = -sig (5 / (3 rho^2)) (1 + t) e^-t

With beta = P K(X, Z), P = (K + nugget)^-1 (or the precision handed in: FITC), nd[j][l] = d noise(x_j) / d x_jl and
A_l[j][i] = dk(x_j, x_i)[l] + [|x_i - x_j| < 1e-10] nd[j][l]   (the coincidence mask of gp.py:308-317):

    full[j d + l, m] = beta[j, m] ( 2 dk(z_m, x_j)[l] + 2 (A_l beta)[j, m] - A_l[j, j] beta[j, m] )
    newpt[m, l]      = -2 sum_j dk(z_m, x_j)[l] beta[j, m]
    ivar             = mean of `full` over m

and, when the WHOLE evaluation set lies within 1e-10 of training point j (gp.py:318-320), noise(x_j) is added to row j of
K(X, Z) before the solve and nd[j][l] to dk(z_m, x_j)[l] in the first term.
"""
import numpy as np


def spec_of(kind, rho, sig, d):
    """The oracle's dict for the kernel."""
    return dict(kind=kind, rho=float(rho), signalSize=float(sig), d=int(d))


def _t(kind, rho, A, B):
    """t[i, j] = sqrt(2 nu) |a_i - b_j| / rho, from coordinate differences (one coordinate at a time: nothing 3-D)."""
    assert kind in ("matern32", "matern52")
    r2 = np.zeros((len(A), len(B)))
    for l in range(A.shape[1]):
        e = A[:, l][:, None] - B[:, l][None, :]
        r2 += e * e
    return np.sqrt(3.0 if kind == "matern32" else 5.0) * np.sqrt(r2) / rho


def kgmat(kind, rho, sig, A, B):
    """(k(a_i, b_j), g(|a_i - b_j|)): the kernel and the radial factor of its derivative, dk(a_i, b_j)[l] = g[i, j] (a_il - b_jl)."""
    t = _t(kind, rho, A, B)
    e = np.exp(-t)
    if kind == "matern32":
        return sig * (1.0 + t) * e, -sig * (3.0 / rho ** 2) * e
    return sig * (1.0 + t + t * t / 3.0) * e, -sig * (5.0 / (3.0 * rho ** 2)) * (1.0 + t) * e


def kmat(kind, rho, sig, A, B):
    """k(a_i, b_j), (len(A), len(B))."""
    return kgmat(kind, rho, sig, A, B)[0]


def gmat(kind, rho, sig, A, B):
    return kgmat(kind, rho, sig, A, B)[1]


def dkmat(kind, rho, sig, U, P):
    """out[i, j, l] = d k(u_i, p_j) / d u_il (small sets only)."""
    return gmat(kind, rho, sig, U, P)[:, :, None] * (U[:, None, :] - P[None, :, :])


def gradients(kind, rho, sig, X, Z, nugget, noise_func=None, prec=None, full_cols=None):
    """(full (N d, M'), newpt (M d,), ivar (N d,)) for the model on X with nugget (float or (N,)) -- or with the precision
    matrix `prec` (N, N) instead.  `noise_func`: callable with .deriv (tests/helpers.NoiseFunc).  `full` covers the first
    M' = full_cols evaluation points (default: all); `ivar` is the mean over ALL of them, summed without forming `full`
    (S = beta beta^T), so that N = 4100, M = 8200 stays a few N x M arrays."""
    X, Z = np.asarray(X, dtype=float), np.asarray(Z, dtype=float)
    n, d = X.shape
    m = len(Z)
    mf = m if full_cols is None else min(int(full_cols), m)
    Kxz, Gxz = kgmat(kind, rho, sig, X, Z)                   # dk(z_m, x_j)[l] = Gxz[j, m] (z_ml - x_jl)
    Kxx, Gxx = kgmat(kind, rho, sig, X, X)                   # dk(x_j, x_i)[l] = Gxx[j, i] (x_jl - x_il)
    if prec is None:
        Kn = Kxx + np.diag(np.broadcast_to(np.asarray(nugget, dtype=float), (n,)))
        solve = lambda B: np.linalg.solve(Kn, B)             # noqa: E731
    else:
        solve = lambda B: prec @ B                           # noqa: E731
    beta0 = solve(Kxz)                                       # the gradient w.r.t. the evaluation points never sees the bias
    Q0 = Gxz * beta0
    newpt = -2.0 * (Z * Q0.sum(axis=0)[:, None] - Q0.T @ X)
    nd, hit, beta = None, np.zeros(n, dtype=bool), beta0
    if noise_func is not None:
        nd = np.asarray(noise_func.deriv(X), dtype=float).reshape(n, d)
        # gp.py:318-320: a norm over ALL evaluation points -- only a set that is one point (repeated) can pass it
        if np.ptp(Z, axis=0).max() < 2e-10:
            hit = np.array([np.linalg.norm(X[j:j + 1] - Z) < 1e-10 for j in range(n)])
        if hit.any():
            beta = solve(Kxz + np.where(hit, np.asarray(noise_func(X), dtype=float), 0.0)[:, None])
        same = _t(kind, 1.0, X, X) < 1e-10 * np.sqrt(3.0 if kind == "matern32" else 5.0)     # |x_i - x_j| < 1e-10
    Q = Gxz * beta
    S = beta @ beta.T
    full = np.zeros((n, d, mf))
    ivar = np.zeros((n, d))
    b = beta[:, :mf]
    for l in range(d):
        A = Gxx * (X[:, l][:, None] - X[:, l][None, :])
        bias = np.zeros(n)
        if nd is not None:
            A = A + same * nd[:, l][:, None]
            bias = np.where(hit, nd[:, l], 0.0)
        first = Gxz[:, :mf] * (Z[:mf, l][None, :] - X[:, l][:, None]) + bias[:, None]
        full[:, l, :] = b * (2.0 * first + 2.0 * (A @ b) - np.diag(A)[:, None] * b)
        ivar[:, l] = (2.0 * (Q @ Z[:, l] - X[:, l] * Q.sum(axis=1)) + 2.0 * bias * beta.sum(axis=1)
                      + 2.0 * np.sum(A * S, axis=1) - np.diag(A) * np.diag(S)) / float(m)
    return full.reshape(n * d, mf), newpt.reshape(m * d), ivar.reshape(n * d)
