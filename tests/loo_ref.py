"""NumPy restatement of leave-one-out cross-validation (Rasmussen & Williams 5.4.2) for the tests: data, not product code.

Zero prior mean; K includes the nugget D = diag(noise).  With P = K^-1, alpha = P y, p_i = P_ii:
    mu_i = y_i - alpha_i / p_i,  var_i = 1 / p_i,  L_LOO = sum_i [-1/2 log var_i - (y_i - mu_i)^2 / (2 var_i) - 1/2 log 2 pi]
    dL_LOO / d theta = sum_i (alpha_i a_i - 1/2 (1 + alpha_i^2 / p_i) q_i) / p_i,  W = P dK,  a = W alpha,  q_i = sum_l W_il P_il

Kernels are flat specs (kind, d, hyp) in the order of the C ABI: 'se' hyp = [cl_0..cl_{d-1}, signalSize]; 'm32' / 'm52'
hyp = [rho, signalSize].  Gradients come in the order [lengths..., signalSize, noise]; `noise` is a common additive shift of
every nugget entry, so its derivative is taken with respect to the noise VARIANCE.
"""
import numpy as np

LOG2PI = np.log(2.0 * np.pi)


def nlen(kind, d):
    return d if kind == "se" else 1


def _scaled_diffs(kind, d, hyp, X):
    """e[i, j, k] = (x_ik - x_jk) * scale_k: differences first, then scaled."""
    hyp = np.asarray(hyp, dtype=float)
    if kind == "se":
        scale = 1.0 / hyp[:d]
    else:
        scale = np.full(d, (np.sqrt(3.0) if kind == "m32" else np.sqrt(5.0)) / hyp[0])
    return (X[:, None, :] - X[None, :, :]) * scale[None, None, :]


def cov0(kind, d, hyp, X):
    """K0: the covariance without the nugget."""
    e = _scaled_diffs(kind, d, hyp, X)
    acc = np.sum(e * e, axis=2)
    s = float(hyp[-1])
    if kind == "se":
        return s * np.exp(-0.5 * acc)
    t = np.sqrt(acc)
    if kind == "m32":
        return s * (1.0 + t) * np.exp(-t)
    return s * (1.0 + t + acc / 3.0) * np.exp(-t)


def cov0_mehler(t, X):
    """Mehler kernel, k = prod_k (1 - t_k^2)^-1/2 exp(-(t_k^2 (a_k^2 + b_k^2) - 2 t_k a_k b_k) / (2 (1 - t_k^2))) (value only: the
    leave-one-out predictions need nothing else of a kernel)."""
    t = np.asarray(t, dtype=float)
    om = 1.0 - t * t
    a, b = X[:, None, :], X[None, :, :]
    expo = np.sum((t * t * (a * a + b * b) - 2.0 * t * a * b) / (2.0 * om), axis=2)
    return np.prod(om ** -0.5) * np.exp(-expo)


def nugget_vector(nugget, n):
    return np.broadcast_to(np.asarray(nugget, dtype=float), (n,)).copy()


def cov(kind, d, hyp, X, nugget):
    return cov0(kind, d, hyp, X) + np.diag(nugget_vector(nugget, X.shape[0]))


def dcov(kind, d, hyp, X):
    """[dK/d length_0, ..., dK/d signalSize, dK/d noise]."""
    hyp = np.asarray(hyp, dtype=float)
    e = _scaled_diffs(kind, d, hyp, X)
    acc = np.sum(e * e, axis=2)
    s = float(hyp[-1])
    K0 = cov0(kind, d, hyp, X)
    out = []
    if kind == "se":
        for k in range(d):
            out.append(K0 * e[:, :, k] ** 2 / hyp[k])
    else:
        t = np.sqrt(acc)
        rho_dk = s * acc * np.exp(-t) if kind == "m32" else s * acc * (1.0 + t) * np.exp(-t) / 3.0
        out.append(rho_dk / hyp[0])
    out.append(K0 / s)
    out.append(np.eye(X.shape[0]))
    return out


def loo_closed(K, y):
    """(mean, var, L_LOO) from the closed form through np.linalg.inv."""
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    alpha = P @ y
    p = np.diag(P)
    mean = y - alpha / p
    var = 1.0 / p
    logp = np.sum(-0.5 * np.log(var) - (y - mean) ** 2 / (2.0 * var) - 0.5 * LOG2PI)
    return mean, var, float(logp)


def loo_brute(K, y):
    """The same by N actual refits: Cholesky of K with point i left out, prediction of the observation y_i."""
    n = K.shape[0]
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        Lc = np.linalg.cholesky(K[np.ix_(keep, keep)])
        k = K[keep, i]
        w = np.linalg.solve(Lc, k)
        z = np.linalg.solve(Lc, y[keep])
        mean[i] = w @ z
        var[i] = K[i, i] - w @ w
    logp = np.sum(-0.5 * np.log(var) - (y - mean) ** 2 / (2.0 * var) - 0.5 * LOG2PI)
    return mean, var, float(logp)


def _row_sum(alpha, p, a, q):
    return float(np.sum((alpha * a - 0.5 * (1.0 + alpha ** 2 / p) * q) / p))


def loo_grad_closed(K, dKs, y):
    """dL_LOO / d theta for every dK in dKs, generic form (one product W = P dK each)."""
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    alpha = P @ y
    p = np.diag(P)
    out = []
    for dK in dKs:
        W = P @ dK
        out.append(_row_sum(alpha, p, W @ alpha, np.sum(W * P, axis=1)))
    return np.array(out)


def loo_grad_shortcuts(K, D, s, y):
    """[d/d signalSize, d/d noise] WITHOUT a product, from row reductions over P (P K0 = I - P D)."""
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    alpha = P @ y
    p = np.diag(P)
    g_sig = _row_sum(alpha, p, (alpha - P @ (D * alpha)) / s, (p - (P * P) @ D) / s)
    g_noise = _row_sum(alpha, p, P @ alpha, np.sum(P * P, axis=1))
    return np.array([g_sig, g_noise])


def loo_all(kind, d, hyp, X, nugget, y):
    """(mean, var, L_LOO, gradient [lengths..., signalSize, noise]) of the closed form."""
    K = cov(kind, d, hyp, X, nugget)
    mean, var, logp = loo_closed(K, y)
    return mean, var, logp, loo_grad_closed(K, dcov(kind, d, hyp, X), y)


def loo_value(kind, d, theta, X, nugget, y):
    """L_LOO as a function of theta = [hyp..., noise shift]: what central differences are taken of."""
    theta = np.asarray(theta, dtype=float)
    K = cov(kind, d, theta[:-1], X, nugget_vector(nugget, X.shape[0]) + theta[-1])
    return loo_closed(K, y)[2]


def loo_grad_fd(kind, d, hyp, X, nugget, y, h=1e-5):
    theta = np.concatenate([np.asarray(hyp, dtype=float), [0.0]])
    g = np.empty(theta.size)
    for k in range(theta.size):
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        g[k] = (loo_value(kind, d, tp, X, nugget, y) - loo_value(kind, d, tm, X, nugget, y)) / (2.0 * h)
    return g


def case(kind, d, n, noise, seed, per_point=False):
    """Test problem: points in [-1, 1]^d, a smooth function plus noise; (hyp, X, nugget, y)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, d))
    nugget = noise * (0.5 + rng.uniform(0.0, 1.0, n)) if per_point else float(noise)
    y = np.sin(2.0 * np.pi * X.sum(1) / d) + np.sqrt(nugget_vector(nugget, n)) * rng.standard_normal(n)
    if kind == "se":
        hyp = list(0.6 + 0.1 * np.arange(d)) + [1.3]
    else:
        hyp = [0.9, 1.3]
    return np.array(hyp), X, nugget, y
