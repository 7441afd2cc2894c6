"""NumPy restatement of leave-one-out cross-validation for FITC models and its hyper-parameter gradient for the tests: data, not
product code.  Built on fitc_grad_ref (its cases, `_model` and `_assemble`).

The model's prior covariance of the observations is Kt = Q + G (Q = Kfu Quu^-1 Kuf, G = diag(k(x_i,x_i) + noise - Q_ii)), the
matrix whose likelihood GP.loglikeParams scores on a FITC model; P = Kt^-1 is the Woodbury precision, alpha = P y.  Leave-one-out
is taken UNDER THAT MODEL: p(y_i | y_-i) is the Gaussian conditional of N(0, Kt),
    p_i = P_ii = ginv_i - ssq_i,   mean_i = y_i - alpha_i / p_i,   var_i = 1 / p_i,     ssq_i = |Y[:, i]|^2, Y = La^-1 Ks
    L = sum_i [ 1/2 log p_i - alpha_i^2 / (2 p_i) ] - N/2 log 2 pi
and dL = 1/2 tr(M dKt) with the symmetric
    r = alpha / p,  b = P r,  c_i = (1 + alpha_i^2 / p_i) / p_i,  C = diag(c),     M = alpha b^T + b alpha^T - P C P,  m = diag M
    R = B (M - diag m)  (nu x N),   T = R B^T  (nu x nu)            and fitc_grad_ref._assemble's last line.
Three forms: through nu x N matrices only (`loo`), with P and M explicit (`loo_dense`), and by deleting row and column i of Kt
(`delete_one`).  Gradients in the order of the C ABI, [lengths..., signalSize, noise]; `noise` is the noise VARIANCE.
"""
import numpy as np

import fitc_grad_ref as ref

CASES, IDS, BLOCKED, case = ref.CASES, ref.IDS, ref.BLOCKED, ref.case


def _terms(al, p, y):
    value = float(np.sum(0.5 * np.log(p) - 0.5 * al * al / p) - 0.5 * len(y) * ref.LOG2PI)
    return value, y - al / p, 1.0 / p


def loo(spec, X, S, y, noise):
    """dict(value, mean, var, grad) through nu x N and nu x nu matrices only (P = Gi - Y^T Y is never formed)."""
    m = ref._model(spec, X, S, y, noise)
    al, Bm, Y, Gi = m["alpha"], m["B"], m["Y"], m["Gi"]
    ssq = np.sum(Y * Y, axis=0)
    p = Gi - ssq
    value, mean, var = _terms(al, p, y)
    r = al / p
    c = (1.0 + al * al / p) / p
    b = Gi * r - Y.T @ (Y @ r)
    C1 = Bm @ Y.T
    H = (Y * c) @ Y.T
    C2 = (Bm * (Gi * c)) @ Y.T - C1 @ H
    mi = 2.0 * al * b - (Gi * Gi * c - 2.0 * Gi * c * ssq + np.sum(Y * (H @ Y), axis=0))
    BPCP = Bm * (Gi * Gi * c) - (C1 @ Y) * (c * Gi) - C2 @ Y
    R = np.outer(Bm @ al, b) + np.outer(Bm @ b, al) - BPCP - Bm * mi
    T = R @ Bm.T
    return dict(value=value, mean=mean, var=var, grad=ref._assemble(spec, m, R, T, float(np.sum(mi))))


def _dense_cov(m):
    C = m["Kuf"].T @ m["B"]
    return 0.5 * (C + C.T) + np.diag(m["g"])


def loo_dense(spec, X, S, y, noise):
    """The same with P (from the Cholesky factor of Q + G) and M formed explicitly (N x N)."""
    m = ref._model(spec, X, S, y, noise)
    Bm = m["B"]
    Li = np.linalg.solve(np.linalg.cholesky(_dense_cov(m)), np.eye(len(y)))
    P = Li.T @ Li
    al = P @ y
    p = np.diag(P).copy()
    value, mean, var = _terms(al, p, y)
    b = P @ (al / p)
    c = (1.0 + al * al / p) / p
    M = np.outer(al, b) + np.outer(b, al) - (P * c) @ P
    mi = np.diag(M).copy()
    R = Bm @ (M - np.diag(mi))
    T = R @ Bm.T
    return dict(value=value, mean=mean, var=var, grad=ref._assemble(spec, m, R, T, float(np.sum(mi))))


def dense_value(spec, X, S, y, noise):
    return loo_dense(spec, X, S, y, noise)["value"]


def delete_one(spec, X, S, y, noise, i):
    """(mean_i, var_i) of y_i given y_-i under N(0, Q + G): row and column i removed, one solve."""
    Kt = _dense_cov(ref._model(spec, X, S, y, noise))
    keep = np.arange(len(y)) != i
    k = Kt[keep, i]
    sol = np.linalg.solve(Kt[np.ix_(keep, keep)], np.column_stack([y[keep], k]))
    return float(k @ sol[:, 0]), float(Kt[i, i] - k @ sol[:, 1])
