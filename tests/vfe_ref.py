"""NumPy restatement of the VFE objective (Titsias' variational free energy), its gradients and its predictor, for the tests:
data, not product code.  Built on fitc_grad_ref's helpers (same notation) and bo_compose.dkdz.

Conventions are the library's: Quu = K(S,S) + noise I (the nugget stays inside, i.e. inducing variables u = f(S) + eps), Kuf = K(S,X),
B = Quu^-1 Kuf, Q = Kfu B, Kt = Q + noise I, P = Kt^-1 = I / noise - Y^T Y with Ks = -Kuf / noise, A = Quu + Kuf Kfu / noise,
Y = chol(A)^-1 Ks, alpha = P y:
    F = -1/2 y^T alpha - 1/2 (N log noise + log|A| - log|Quu|) - N/2 log 2 pi - (1 / (2 noise)) sum_i (k(x_i,x_i) - Q_ii)
With M = alpha alpha^T - P (never formed), R = B (M + I / noise) = (B alpha) alpha^T + (B Y^T) Y, T = R B^T:
    dF/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) - (N / noise) dk(x,x)/d theta ]
    dF/d noise = 1/2 [ tr M - tr T ] + sum_i (k_ii - Q_ii) / (2 noise^2),   tr M = sum_i (alpha_i^2 - 1 / noise + |Y[:, i]|^2)
    dF/ds_u    = sum_i R[u][i] dk(s_u,x_i)/ds_u - sum_v 1/2 (T[u][v] + T[v][u]) dk(s_u,s_v)/ds_u
Predictor at z (k_u = K(S, z)):  mean = k_u^T B alpha,  var = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2.
Gradients come in the order of the C ABI, [lengths..., signalSize, noise]; `noise` is the noise VARIANCE.
"""
import numpy as np

import bo_compose
import fitc_grad_ref as ref

LOG2PI = ref.LOG2PI


def _model(spec, X, S, y, noise):
    s = float(ref.hyp_of(spec)[-1])
    Kuu, dKuu = ref.kparts(spec, S, S)
    Kuf, dKuf = ref.kparts(spec, S, X)
    n, nu = X.shape[0], S.shape[0]
    Quu = Kuu + noise * np.eye(nu)
    Lu = np.linalg.cholesky(Quu)
    W = np.linalg.solve(Lu, Kuf)
    q = np.sum(W * W, axis=0)
    trres = float(np.sum(s - q))
    Ks = -Kuf / noise
    La = np.linalg.cholesky(Quu - Ks @ Kuf.T)
    Y = np.linalg.solve(La, Ks)
    alpha = y / noise - Y.T @ (Y @ y)
    logdet = n * np.log(noise) + 2.0 * np.sum(np.log(np.diag(La))) - 2.0 * np.sum(np.log(np.diag(Lu)))
    value = -0.5 * y @ alpha - 0.5 * logdet - 0.5 * n * LOG2PI - 0.5 * trres / noise
    Bm = np.linalg.solve(Lu.T, W)
    return dict(s=s, Kuu=Kuu, dKuu=dKuu, Kuf=Kuf, dKuf=dKuf, Quu=Quu, Lu=Lu, La=La, Y=Y, alpha=alpha, B=Bm, q=q, trres=trres,
                value=float(value))


def value(spec, X, S, y, noise):
    return _model(spec, X, S, y, noise)["value"]


def weights(m):
    """(R, T) through nu x N matrices only."""
    al, Bm, Y = m["alpha"], m["B"], m["Y"]
    R = np.outer(Bm @ al, al) + (Bm @ Y.T) @ Y
    return R, R @ Bm.T


def value_grad(spec, X, S, y, noise):
    """(F, gradient [lengths..., signalSize, noise]) through nu x N matrices only."""
    m = _model(spec, X, S, y, noise)
    n = X.shape[0]
    hyp = ref.hyp_of(spec)
    R, T = weights(m)
    out = [0.5 * (2.0 * np.sum(R * dk) - np.sum(T * du)) / hyp[k] for k, (dk, du) in enumerate(zip(m["dKuf"], m["dKuu"]))]
    out.append(0.5 * ((2.0 * np.sum(R * m["Kuf"]) - np.sum(T * m["Kuu"])) / m["s"] - n / noise))
    trM = float(np.sum(m["alpha"] ** 2 - 1.0 / noise + np.sum(m["Y"] ** 2, axis=0)))
    out.append(0.5 * (trM - np.trace(T)) + 0.5 * m["trres"] / noise ** 2)
    return m["value"], np.array(out)


def grad_S(spec, X, S, y, noise):
    """dF/dS (nu, d) through nu x N matrices only; the point derivatives row by row from bo_compose.dkdz ((n, d) per s_u)."""
    R, T = weights(_model(spec, X, S, y, noise))
    Ts = 0.5 * (T + T.T)
    return np.stack([R[u] @ bo_compose.dkdz(spec, S[u], X) - Ts[u] @ bo_compose.dkdz(spec, S[u], S) for u in range(S.shape[0])])


def dense_value(spec, X, S, y, noise):
    """F through the dense N x N form: Cholesky of the symmetrised Q + noise I, trace(Q) explicit."""
    m = _model(spec, X, S, y, noise)
    n = X.shape[0]
    Q = m["Kuf"].T @ m["B"]
    Q = 0.5 * (Q + Q.T)
    Lc = np.linalg.cholesky(Q + noise * np.eye(n))
    z = np.linalg.solve(Lc, y)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(Lc))) - 0.5 * n * LOG2PI - 0.5 * (n * m["s"] - np.trace(Q)) / noise)


def exact_loglike(spec, X, y, noise):
    """The exact dense log marginal likelihood of the same data, K(X,X) + noise I."""
    n = X.shape[0]
    Lc = np.linalg.cholesky(ref.kparts(spec, X, X)[0] + noise * np.eye(n))
    z = np.linalg.solve(Lc, y)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(Lc))) - 0.5 * n * LOG2PI)


def predict(spec, X, S, y, noise, Z):
    """(mean, var) of the latent f at Z: k_u^T B alpha and k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2."""
    m = _model(spec, X, S, y, noise)
    Ku = ref.kparts(spec, S, Z)[0]
    a = np.linalg.solve(m["Lu"], Ku)
    b = np.linalg.solve(m["La"], Ku)
    return Ku.T @ (m["B"] @ m["alpha"]), m["s"] - np.sum(a * a, axis=0) + np.sum(b * b, axis=0)


def predict_dense(spec, X, S, y, noise, Z):
    """The same predictor in its other forms: mean = k_u^T A^-1 Kuf y / noise; var = k - Q_zz + (Q_zz - Q_zf Kt^-1 Q_fz) with
    Q_zf = k_u^T B and Kt = Q + noise I formed N x N."""
    m = _model(spec, X, S, y, noise)
    n = X.shape[0]
    Ku = ref.kparts(spec, S, Z)[0]
    A = m["La"] @ m["La"].T
    mean = Ku.T @ np.linalg.solve(A, m["Kuf"] @ y) / noise
    Qzz = np.sum(Ku * np.linalg.solve(m["Quu"], Ku), axis=0)
    Qzf = Ku.T @ m["B"]
    Q = m["Kuf"].T @ m["B"]
    Kt = 0.5 * (Q + Q.T) + noise * np.eye(n)
    var = m["s"] - Qzz + (Qzz - np.sum(Qzf * np.linalg.solve(Kt, Qzf.T).T, axis=1))
    return mean, var
