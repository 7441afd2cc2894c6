"""NumPy restatements of the Bayesian-optimisation costs (experimentalDesign.py:889-1003) and of their gradient w.r.t. the
candidate -- test infrastructure, not product code.

`costs` is the composition a user would write today: posterior mean and variance, then abs, sqrt and scipy.stats.norm, exactly
as the reference's `evaluate` does per point.  `grad_closed_form` is the analytic gradient, with a dense Cholesky solve on the
host:  grad_z A = sum_j dk(z, x_j)/dz (a alpha_j - 2 b beta_j),  beta = K^-1 k(X, z),  a = dA/dmu,  b = dA/dvar."""
import numpy as np
import scipy.stats as spstats

UCB, PI, EI = 0, 1, 2


def costs(acq, param, mean, var):
    """Costs from the posterior mean and the variance (signed or abs: GP.evaluate's abs is applied here)."""
    mean = np.asarray(mean, dtype=float)
    s = np.sqrt(np.abs(np.asarray(var, dtype=float)))
    if acq == UCB:
        return -(mean - param * s)
    g = (param - mean) / s
    if acq == PI:
        return -spstats.norm.cdf(g)
    return -s * (g * spstats.norm.cdf(g) + spstats.norm.pdf(g))


def _sqdist(A, B, w):
    """sum_l w_l (A_il - B_jl)^2, coordinate by coordinate (no N x M x d temporary)."""
    out = np.zeros((A.shape[0], B.shape[0]))
    for l in range(A.shape[1]):
        diff = A[:, l:l + 1] - B[None, :, l]
        out += w[l] * diff * diff
    return out


def kmat(spec, A, B):
    """k(A_i, B_j) for the stationary kernels of the oracle's spec dicts."""
    d = spec["d"]
    if spec["kind"] == "se":
        cl = np.broadcast_to(np.asarray(spec["cl"], dtype=float), (d,))
        return spec["signalSize"] * np.exp(-0.5 * _sqdist(A, B, cl ** -2.0))
    c = (np.sqrt(3.0) if spec["kind"] == "matern32" else np.sqrt(5.0)) / spec["rho"]
    t = c * np.sqrt(_sqdist(A, B, np.ones(d)))
    if spec["kind"] == "matern32":
        return spec["signalSize"] * (1.0 + t) * np.exp(-t)
    return spec["signalSize"] * (1.0 + t + t * t / 3.0) * np.exp(-t)


def dkdz(spec, z, X):
    """(n, d): d k(z, x_j) / d z, true derivative (no doubled signalSize)."""
    d = spec["d"]
    diff = z[None, :] - X                       # z - x_j
    if spec["kind"] == "se":
        cl = np.broadcast_to(np.asarray(spec["cl"], dtype=float), (d,))
        k = kmat(spec, z[None, :], X)[0]
        return -diff / cl[None, :] ** 2 * k[:, None]
    c = (np.sqrt(3.0) if spec["kind"] == "matern32" else np.sqrt(5.0)) / spec["rho"]
    t = c * np.sqrt(np.sum(diff * diff, axis=1))
    if spec["kind"] == "matern32":
        f = spec["signalSize"] * c * c * np.exp(-t)
    else:
        f = spec["signalSize"] * c * c / 3.0 * (1.0 + t) * np.exp(-t)
    return -f[:, None] * diff


class DenseModel(object):
    """Host GP (Cholesky of K + noise I) for the closed forms."""

    def __init__(self, spec, X, y, noise):
        self.spec, self.X = spec, np.asarray(X, dtype=float)
        K = kmat(spec, self.X, self.X) + noise * np.eye(len(self.X))
        self.L = np.linalg.cholesky(K)
        self.alpha = self.solve(np.asarray(y, dtype=float))

    def solve(self, b):
        import scipy.linalg as sla
        return sla.cho_solve((self.L, True), b)

    def posterior(self, Z):
        Kx = kmat(self.spec, self.X, Z)                 # n x M
        W = np.linalg.solve(self.L, Kx)
        prior = kmat(self.spec, Z[:1], Z[:1])[0, 0]     # stationary: k(z, z) is a constant
        return Kx.T @ self.alpha, prior - np.sum(W * W, axis=0)

    def grad(self, acq, param, Z):
        """(M, d) closed-form gradients of the costs at the rows of Z."""
        Z = np.asarray(Z, dtype=float)
        mean, var = self.posterior(Z)
        s = np.sqrt(np.abs(var))
        sg = np.sign(var)
        if acq == UCB:
            a = -np.ones_like(s)
            b = param * sg / (2.0 * s)
        else:
            g = (param - mean) / s
            Phi, phi = spstats.norm.cdf(g), spstats.norm.pdf(g)
            if acq == PI:
                a, b = phi / s, phi * g * sg / (2.0 * s * s)
            else:
                a, b = Phi, -phi * sg / (2.0 * s)
        beta = self.solve(kmat(self.spec, self.X, Z))    # n x M
        out = np.empty(Z.shape)
        for m in range(Z.shape[0]):
            out[m] = dkdz(self.spec, Z[m], self.X).T @ (a[m] * self.alpha - 2.0 * b[m] * beta[:, m])
        return out
