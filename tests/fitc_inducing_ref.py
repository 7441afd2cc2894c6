"""NumPy restatement of the gradient of the FITC log marginal likelihood w.r.t. the inducing-point LOCATIONS, for the tests: data,
not product code.  Built on fitc_grad_ref._model (same notation).

Moving s_u changes row u of Kuf = K(S,X) and row and column u of K(S,S); the diagonals k(s_u,s_u), k(x_i,x_i) and the nugget
inside Quu do not depend on S.  With R = B (M - diag m) (nu x N) and T = R B^T (nu x nu) of the hyper-parameter gradient,
    dL/ds_u[l] = sum_i R[u][i] dk(s_u, x_i)/ds_u[l] - sum_v 1/2 (T[u][v] + T[v][u]) dk(s_u, s_v)/ds_u[l]
and the TRUE point derivatives dk(u, p)/du_l = -c_l f(r) (u_l - p_l):
    se        f = k(u, p)          c_l = 1 / cl_l^2
    matern32  f = e^-t             c   = s 3 / rho^2           t = sqrt(3) |u - p| / rho
    matern52  f = (1 + t) e^-t     c   = s 5 / (3 rho^2)       t = sqrt(5) |u - p| / rho
(zero and smooth at u = p, so S a subset of X needs no special case, and the v = u term vanishes).
"""
import numpy as np

import fitc_grad_ref as ref


def perturbed(S, scale=0.05, seed=101):
    """S moved off the training points: S + scale N(0,1), fixed seed."""
    return S + scale * np.random.default_rng(seed).standard_normal(S.shape)


def point_derivs(spec, A, Bp):
    """[dk(a_u, b_c)/da_u[l] for l < d], each (len(A), len(Bp)); differences first, then scaled."""
    hyp = ref.hyp_of(spec)
    d, s, kind = spec["d"], float(hyp[-1]), spec["kind"]
    if kind == "se":
        scale = 1.0 / hyp[:d]
    else:
        scale = np.full(d, (np.sqrt(3.0) if kind == "matern32" else np.sqrt(5.0)) / hyp[0])
    diff = [A[:, None, k] - Bp[None, :, k] for k in range(d)]     # one dimension at a time: no (nu, N, d) array
    acc = sum((v * scale[k]) ** 2 for k, v in enumerate(diff))
    if kind == "se":
        f, c = s * np.exp(-0.5 * acc), scale ** 2
    elif kind == "matern32":
        t = np.sqrt(acc)
        f, c = np.exp(-t), s * scale ** 2
    else:
        t = np.sqrt(acc)
        f, c = (1.0 + t) * np.exp(-t), s * scale ** 2 / 3.0
    return [-c[k] * f * diff[k] for k in range(d)]


def _assemble(spec, X, S, R, T):
    duf = point_derivs(spec, S, X)
    duu = point_derivs(spec, S, S)
    Ts = 0.5 * (T + T.T)
    return np.stack([np.sum(R * a, axis=1) - np.sum(Ts * b, axis=1) for a, b in zip(duf, duu)], axis=1)


def weights(spec, X, S, y, noise):
    """(R, T) through nu x N matrices only, as fitc_grad_ref.fitc_value_grad forms them."""
    m = ref._model(spec, X, S, y, noise)
    al, Bm, Y = m["alpha"], m["B"], m["Y"]
    mi = al * al - m["Gi"] + np.sum(Y * Y, axis=0)
    R = np.outer(Bm @ al, al) - Bm * m["Gi"] + ((Bm @ Y.T) @ Y) - Bm * mi
    return R, R @ Bm.T


def grad_S(spec, X, S, y, noise):
    """dL/dS (nu, d) through nu x N matrices only."""
    R, T = weights(spec, X, S, y, noise)
    return _assemble(spec, X, S, R, T)


def grad_S_dense(spec, X, S, y, noise):
    """The same with M = alpha alpha^T - P formed explicitly (N x N), P from the Cholesky factor of Q + G (fitc_grad_dense)."""
    m = ref._model(spec, X, S, y, noise)
    Bm = m["B"]
    C = m["Kuf"].T @ Bm
    C = 0.5 * (C + C.T) + np.diag(m["g"])
    Li = np.linalg.solve(np.linalg.cholesky(C), np.eye(len(y)))
    P = Li.T @ Li
    al = P @ y
    M = np.outer(al, al) - P
    R = Bm @ (M - np.diag(np.diag(M)))
    return _assemble(spec, X, S, R, R @ Bm.T)


def value(spec, X, S, y, noise):
    return ref._model(spec, X, S, y, noise)["value"]
