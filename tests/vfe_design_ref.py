"""NumPy restatement of IVAR design on a VFE model (gpx_vfe_design_*, gpx_vfe_var_grad*) for the tests: data, not product code.
Float64, no device.  Built on fitc_grad_ref.kparts / case, vfe_ref and bo_compose.dkdz (the TRUE point derivative).

Notation of vfe_ref: S the nu inducing points, k_u(.) = K(S, .), Quu = K(S,S) + noise I = Lu Lu^T, and for design points X
    A = Quu + K(S,X) K(X,S) / noise = La La^T,       var(z) = k(z,z) - |Lu^-1 k_u(z)|^2 + |La^-1 k_u(z)|^2
No observations enter.  With the MC points Z (M of them), C = A^-1 K(S,Z):
    cost      = mean_j var(z_j)                                              `cost`: the DIRECT form, per point, no Gram matrix
    gradient  d cost / dx_i[l] = -(2 / noise) sum_u H[u][i] dk(x_i,s_u)/dx_i[l],   H = (C C^T / M) K(S,X)                    `grad`
    d var(z_j) / dx_k[l] = -(2 / noise) (K(X,S) C)[k][j] ((dK(X,S)/dx[l]) C)[k][j]                                       `var_grad`
    d var(z_j) / dz_j[l] = -2 sum_u dk(z_j,s_u)/dz_j[l] gamma_u,   gamma = Quu^-1 k_u(z_j) - A^-1 k_u(z_j)          `var_grad_newpt`
`gram_path` is the device's own sequence (Gz = K(S,Z) K(Z,S) / M, the two-sided solves and their traces, the pinned split)."""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import bo_compose
import fitc_grad_ref as ref
import vfe_ref as vref


def _quu(spec, S, noise):
    return ref.kparts(spec, S, S)[0] + noise * np.eye(S.shape[0])


def _a(spec, X, S, noise):
    P = ref.kparts(spec, S, X)[0]
    return _quu(spec, S, noise) + P @ P.T / noise, P


def cost(spec, X, S, noise, Z):
    """Signed mean of the per-point variational variances at Z of the model with nodes X: vfe_ref.predict's variance (through
    Lu^-1 K(S,Z) and La^-1 K(S,Z)); the observations do not enter it."""
    return float(np.mean(vref.predict(spec, X, S, np.zeros(X.shape[0]), noise, Z)[1]))


def _c(spec, X, S, noise, Z):
    A, P = _a(spec, X, S, noise)
    return cho_solve((np.linalg.cholesky(A), True), ref.kparts(spec, S, Z)[0]), P


def _rows(spec, X, S, H):
    """out[i][l] = sum_u H[u][i] dk(x_i, s_u)/dx_i[l]"""
    return np.stack([H[:, i] @ bo_compose.dkdz(spec, X[i], S) for i in range(X.shape[0])])


def grad(spec, X, S, noise, Z):
    """(N, d): the closed form in the inducing space, through C C^T / M."""
    C, P = _c(spec, X, S, noise, Z)
    return -(2.0 / noise) * _rows(spec, X, S, (C @ C.T / Z.shape[0]) @ P)


def var_grad(spec, X, S, noise, Z):
    """The literal (N d, M) matrix, row k d + l = d var(z_.) / dx_k[l]."""
    C, P = _c(spec, X, S, noise, Z)
    E = P.T @ C
    d = X.shape[1]
    out = np.empty((X.shape[0] * d, Z.shape[0]))
    for k in range(X.shape[0]):
        out[k * d:(k + 1) * d] = -(2.0 / noise) * E[k][None, :] * (bo_compose.dkdz(spec, X[k], S).T @ C)
    return out


def var_grad_newpt(spec, X, S, noise, Z):
    """(M d,): d var(z_j) / dz_j, flattened."""
    C, _ = _c(spec, X, S, noise, Z)
    Ku = ref.kparts(spec, S, Z)[0]
    gamma = cho_solve((np.linalg.cholesky(_quu(spec, S, noise)), True), Ku) - C
    return np.concatenate([-2.0 * (gamma[:, j] @ bo_compose.dkdz(spec, Z[j], S)) for j in range(Z.shape[0])])


def gram_path(spec, Xp, Xf, S, noise, Z):
    """(cost, gradient (b, d) w.r.t. the free points Xf) by the device's own sequence: create (Lu, Gz, kbar, c0), pin (A0), eval."""
    two_sided = lambda L, G: solve_triangular(L, solve_triangular(L, G, lower=True).T, lower=True).T   # L^-1 G L^-T
    Quu = _quu(spec, S, noise)
    Lu = np.linalg.cholesky(Quu)
    Ku = ref.kparts(spec, S, Z)[0]
    Gz = Ku @ Ku.T / Z.shape[0]
    kbar = float(spec["signalSize"])
    c0 = np.trace(two_sided(Lu, Gz))
    A0 = Quu
    if Xp is not None and len(Xp) > 0:
        Pp = ref.kparts(spec, S, Xp)[0]
        A0 = Quu + Pp @ Pp.T / noise
    P = ref.kparts(spec, S, Xf)[0]
    La = np.linalg.cholesky(A0 + P @ P.T / noise)
    Y1 = two_sided(La, Gz)
    V = solve_triangular(La, P, lower=True)
    H = solve_triangular(La.T, Y1 @ V, lower=False)
    return float(kbar - c0 + np.trace(Y1)), -(2.0 / noise) * _rows(spec, Xf, S, H)


def directional_fd(f, X, V, h):
    """Central difference of the scalar function f along the direction V: (f(X + h V) - f(X - h V)) / (2 h)."""
    return (f(X + h * V) - f(X - h * V)) / (2.0 * h)


def spec_of(ks):
    """The oracle's dict of a device KernelSpec (kind 0 / 1 / 2 = se / matern32 / matern52)."""
    hyp = np.asarray(ks.hyp, dtype=float)
    kind = {v: k for k, v in ref.KIND_ID.items()}[ks.kind]
    return ref.make_spec(kind, ks.d, hyp[:-1], hyp[-1])


class HostPoints(object):
    """What device.points returns, on the host."""

    def __init__(self, a):
        self.a = np.array(a, dtype=float)
        self.shape = self.a.shape


class NumpyVfeDesign(object):
    """A double of device.VfeDesign on `gram_path`, counting its calls (class attribute `calls`), for host tests of the class."""
    calls = {"create": 0, "pin": 0, "eval": 0}

    def __init__(self, ctx, spec, S, noise, Z):
        self.spec, self.S, self.noise, self.Z, self.Xp = spec_of(spec), S.a, float(noise), Z.a, None
        self.calls["create"] += 1

    def pin(self, Xp):
        self.Xp = None if Xp is None or Xp.shape[0] == 0 else Xp.a
        self.calls["pin"] += 1

    def eval(self, Xf, want_grad=True):
        self.calls["eval"] += 1
        c, g = gram_path(self.spec, self.Xp, Xf.a, self.S, self.noise, self.Z)
        return c, (g if want_grad else None)

    def shape(self):
        return self.S.shape[0], self.Z.shape[0], 0 if self.Xp is None else self.Xp.shape[0]
