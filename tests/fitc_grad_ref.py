"""NumPy restatement of the FITC log marginal likelihood and its hyper-parameter gradient for the tests: data, not product code.

Inducing points S (nu), nodes X (N), zero prior mean.  Quu = K(S,S) + noise I (the nugget is inside), Kuf = K(S,X),
B = Quu^-1 Kuf, Q = Kfu B, g_i = k(x_i,x_i) + noise - Q_ii, Gi = diag(1/g), Ks = -Kuf Gi, A = Quu + Kuf Gi Kfu,
P = Gi - Ks^T A^-1 Ks, alpha = P y:
    L = -1/2 y^T alpha - 1/2 (sum log g + log|A| - log|Quu|) - N/2 log 2 pi
With M = alpha alpha^T - P (never formed), m = diag M, R = B (M - diag m) (nu x N), T = R B^T (nu x nu):
    dL/d theta  = 1/2 [ 2 sum R o dKuf/d theta - sum T o dK(S,S)/d theta + sum_i m_i dk(x_i,x_i)/d theta ]
    dL/d noise  = 1/2 [ sum m - tr T ]
(the 1e-12 guard the library adds to g before inverting is ignored: g >= 0.02 in every case here).

Kernel specs are the oracle's dicts ({"kind": "se" | "matern32" | "matern52", ...}).  Gradients come in the order of the C ABI,
[lengths..., signalSize, noise]: the d correlation lengths of 'se' or the one rho of a Matern; `noise` is the noise VARIANCE.
"""
import numpy as np

LOG2PI = np.log(2.0 * np.pi)
KIND_ID = {"se": 0, "matern32": 1, "matern52": 2}

# (kind, d, lengths, signalSize, N, nu, noise, seed)
CASES = [("se", 3, [0.3, 0.45, 0.6], 1.7, 257, 129, 0.1, 11),
         ("matern32", 2, [0.5], 1.4, 300, 130, 0.1, 12),
         ("matern52", 8, [1.5], 1.2, 260, 129, 0.05, 13),
         ("se", 8, [1.0, 1.2, 0.8, 1.5, 0.9, 1.1, 1.3, 0.7], 1.0, 260, 129, 0.05, 14),
         ("matern32", 8, [1.2], 0.8, 385, 257, 0.02, 15),
         ("se", 1, [0.1], 1.0, 150, 40, 0.1, 16)]
IDS = ["se-d3", "m32-d2", "m52-d8", "se-d8", "m32-d8-nu257", "se-d1-nu40"]
# Lu and La cross the 1024-order block inverses of the device solves
BLOCKED = ("matern52", 8, [1.5], 1.2, 2304, 1152, 0.05, 17)


def make_spec(kind, d, lengths, s):
    if kind == "se":
        return {"kind": "se", "cl": [float(v) for v in lengths], "signalSize": float(s), "d": int(d)}
    return {"kind": kind, "rho": float(lengths[0]), "signalSize": float(s), "d": int(d)}


def case(c):
    """(spec, X, S, y, noise): X ~ U(-1,1)^d, y = sin(3 x_0) + 0.1 N(0,1), S a random subset of X."""
    kind, d, lengths, s, n, nu, noise, seed = c
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, d))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n)
    S = X[rng.permutation(n)[:nu]].copy()
    return make_spec(kind, d, lengths, s), X, S, y, float(noise)


def hyp_of(spec):
    """Flat hyper-parameters in the order of the C ABI: [lengths..., signalSize]."""
    if spec["kind"] == "se":
        cl = np.asarray(spec["cl"], dtype=float)
        if cl.size == 1:
            cl = np.tile(cl, spec["d"])
        return np.concatenate([cl, [spec["signalSize"]]])
    return np.array([spec["rho"], spec["signalSize"]], dtype=float)


def spec_with(spec, hyp):
    """The same kernel with other hyper-parameters."""
    hyp = np.asarray(hyp, dtype=float)
    return make_spec(spec["kind"], spec["d"], hyp[:-1], hyp[-1])


def kparts(spec, A, Bp):
    """(K0, [length-type derivative WITHOUT its 1 / length, ...]) between the point sets A and Bp; differences first, then
    scaled.  SE: K0 e_k^2 per dimension; Matern: rho dk/d rho."""
    hyp = hyp_of(spec)
    d, s, kind = spec["d"], float(hyp[-1]), spec["kind"]
    if kind == "se":
        scale = 1.0 / hyp[:d]
    else:
        scale = np.full(d, (np.sqrt(3.0) if kind == "matern32" else np.sqrt(5.0)) / hyp[0])
    e2 = [((A[:, None, k] - Bp[None, :, k]) * scale[k]) ** 2 for k in range(d)]   # one dimension at a time: no (nu, N, d) array
    acc = sum(e2)
    if kind == "se":
        K0 = s * np.exp(-0.5 * acc)
        return K0, [K0 * v for v in e2]
    t = np.sqrt(acc)
    if kind == "matern32":
        return s * (1.0 + t) * np.exp(-t), [s * acc * np.exp(-t)]
    return s * (1.0 + t + acc / 3.0) * np.exp(-t), [s * acc * (1.0 + t) * np.exp(-t) / 3.0]


def _model(spec, X, S, y, noise):
    s = float(hyp_of(spec)[-1])
    Kuu, dKuu = kparts(spec, S, S)
    Kuf, dKuf = kparts(spec, S, X)
    Quu = Kuu + noise * np.eye(S.shape[0])
    Lu = np.linalg.cholesky(Quu)
    W = np.linalg.solve(Lu, Kuf)
    g = s + noise - np.sum(W * W, axis=0)
    Gi = 1.0 / g
    Ks = -Kuf * Gi
    La = np.linalg.cholesky(Quu - Ks @ Kuf.T)
    Y = np.linalg.solve(La, Ks)
    alpha = Gi * y - Y.T @ (Y @ y)
    value = -0.5 * y @ alpha - 0.5 * (np.sum(np.log(g)) + 2.0 * np.sum(np.log(np.diag(La))) - 2.0 * np.sum(np.log(np.diag(Lu)))) \
        - 0.5 * len(y) * LOG2PI
    Bm = np.linalg.solve(Lu.T, W)
    return dict(s=s, Kuu=Kuu, dKuu=dKuu, Kuf=Kuf, dKuf=dKuf, Quu=Quu, g=g, Gi=Gi, Ks=Ks, Y=Y, alpha=alpha, B=Bm, value=float(value))


def _assemble(spec, m, R, T, msum):
    hyp = hyp_of(spec)
    out = [0.5 * (2.0 * np.sum(R * dk) - np.sum(T * du)) / hyp[k] for k, (dk, du) in enumerate(zip(m["dKuf"], m["dKuu"]))]
    out.append(0.5 * ((2.0 * np.sum(R * m["Kuf"]) - np.sum(T * m["Kuu"])) / m["s"] + msum))
    out.append(0.5 * (msum - np.trace(T)))
    return np.array(out)


def fitc_value_grad(spec, X, S, y, noise):
    """(L, gradient [lengths..., signalSize, noise]) through nu x N matrices only."""
    m = _model(spec, X, S, y, noise)
    al, Bm, Y = m["alpha"], m["B"], m["Y"]
    mi = al * al - m["Gi"] + np.sum(Y * Y, axis=0)
    R = np.outer(Bm @ al, al) - Bm * m["Gi"] + ((Bm @ Y.T) @ Y) - Bm * mi
    T = R @ Bm.T
    return m["value"], _assemble(spec, m, R, T, float(np.sum(mi)))


def fitc_grad_dense(spec, X, S, y, noise):
    """The same gradient with M = alpha alpha^T - P formed explicitly (N x N), P from the Cholesky factor of Q + G."""
    m = _model(spec, X, S, y, noise)
    Bm = m["B"]
    C = m["Kuf"].T @ Bm
    C = 0.5 * (C + C.T) + np.diag(m["g"])
    Lc = np.linalg.cholesky(C)
    Li = np.linalg.solve(Lc, np.eye(len(y)))
    P = Li.T @ Li
    al = P @ y
    M = np.outer(al, al) - P
    mi = np.diag(M).copy()
    R = Bm @ (M - np.diag(mi))
    T = R @ Bm.T
    return _assemble(spec, m, R, T, float(np.sum(mi)))


def cond_quu(spec, S, noise):
    return float(np.linalg.cond(kparts(spec, S, S)[0] + noise * np.eye(S.shape[0])))
