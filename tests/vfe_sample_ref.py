"""Longdouble / float64 restatements of posterior sampling on a VFE model (gpx_vfe_paths_create, gpx_vfe_posterior_cov,
gpx_vfe_psampler_create; NumPy only; data and references of tests/test_vfe_sample_host.py and tests/test_gpu_vfe_sample.py, not
product code).  Built on design_replay_ref (cov_ld, chol_ld, solve_lower_ld), posterior_ref.solve_upper_ld, path_ref (the paths
themselves, with X := S) and the conventions of vfe_ref: Quu = K(S,S) + noise I = Lu Lu^T (inducing variables u = f(S) + eps),
Kuf = K(S,X), A = Quu + Kuf Kfu / noise = La La^T, beta_u = Quu^-1 Kuf alpha = A^-1 Kuf y / noise, k_u(z) = K(S, z).

    V      = 1 beta_u^T - (F~_S + sqrt(noise) Xi1) Quu^-1 + Xi2 La^-1           (P x nu; F~_S[s][u] = f~_s(s_u))
    f_s(z) = sum_j c_sj cos(omega_j . z + b_j) + sum_u v_su k(s_u, z)             (path_ref.paths with X := S)
    exact covariance         k(z,z') - k_u^T Quu^-1 k_u' + k_u^T A^-1 k_u'
    finite-feature covariance  A_J (Phi_J Phi_J^T) A_J^T + noise G_u G_u^T + K_zu A^-1 K_uz,  G_u = K_zu Quu^-1, A_J = [I, -G_u], J = (Z; S)
With K(J, J) in place of Phi_J Phi_J^T the second is the first.  The paths are linear in the base draws (w, Xi1, Xi2): with J_map
the map's matrix (columns: the paths of the unit base draws minus the zero-draw path, which is the mean), J_map J_map^T is the
finite-feature covariance.  That identity sees every change of V's distribution; exchanging Xi1 and Xi2 is none (both are standard
normal), so the mutant "swap" is seen by the comparison of V itself under one base only.

Mutants of `weights`: "la_side" (Xi2 La^-T: the wrong side), "no_xi1" (Xi1 dropped), "plus" (+ before the Quu solve), "quu_no_nugget"
(the Quu of that solve without its nugget), "swap" (Xi1 and Xi2 exchanged).

A Mehler kernel has no longdouble covariance here (design_replay_ref.cov_ld): its entries are formed in float64 (sample_ref.cov_f64)
and the algebra after them runs in the asked precision.
"""
import numpy as np

import chol_stability_ref as CR
import design_replay_ref as DR
import path_ref as PR
import posterior_ref as P
import sample_ref as SR

LD = DR.LD
MUTANTS = ("la_side", "no_xi1", "plus", "quu_no_nugget", "swap")


# ---- linear algebra in either precision --------------------------------------------------------------------------------------------
def cov(spec, A, B=None, dtype=LD):
    if spec["kind"] == "mehler":
        return SR.cov_f64(spec, A, B).astype(dtype)
    if dtype is not LD:
        return DR.cov_f64(spec, A, B)
    if B is None or A.shape[0] * B.shape[0] < 1 << 18:
        return DR.cov_ld(spec, A, B)
    step = -(-A.shape[0] // 8)                   # a large cross block: its rows dealt to the thread pool
    return np.concatenate(list(CR._POOL.map(lambda r0: DR.cov_ld(spec, A[r0:r0 + step], B), range(0, A.shape[0], step))))


def mm(A, B, dtype=LD):
    """A @ B; in longdouble the rows of A are dealt to chol_stability_ref's thread pool (NumPy's longdouble loops release the GIL)."""
    if dtype is not LD:
        return np.asarray(A, dtype=float) @ np.asarray(B, dtype=float)
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    if A.shape[0] * A.shape[1] * (B.shape[1] if B.ndim == 2 else 1) < 1 << 22:
        return np.dot(A, B)
    step = -(-A.shape[0] // 8)
    return np.concatenate(list(CR._POOL.map(lambda r0: np.dot(A[r0:r0 + step], B), range(0, A.shape[0], step))))


def chol(A, dtype=LD, nb=128):
    """Lower Cholesky factor.  Longdouble: design_replay_ref.chol_ld, above order 2 nb blocked around it (left-looking panels of nb
    columns: the same arithmetic, the trailing products through `mm`)."""
    if dtype is not LD:
        return np.linalg.cholesky(np.asarray(A, dtype=float))
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    if n <= 2 * nb:
        return DR.chol_ld(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(0, n, nb):
        e = min(j + nb, n)
        col = A[j:, j:e] - (mm(L[j:, :j], L[j:e, :j].T) if j else LD(0))
        L[j:e, j:e] = DR.chol_ld(col[:e - j])
        if e < n:
            L[e:, j:e] = DR.solve_lower_ld(L[j:e, j:e], col[e - j:].T).T
    return L


def fwd(L, B, dtype=LD):
    """L^-1 B."""
    if dtype is LD:
        return DR.solve_lower_ld(L, B)
    return np.linalg.solve(np.asarray(L, dtype=float), np.asarray(B, dtype=float))


def bwd(L, B, dtype=LD):
    """L^-T B."""
    if dtype is LD:
        B = np.asarray(B, dtype=LD)
        return P.solve_upper_ld(L, B[:, None])[:, 0] if B.ndim == 1 else P.solve_upper_ld(L, B)
    return np.linalg.solve(np.asarray(L, dtype=float).T, np.asarray(B, dtype=float))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def model(spec, X, S, y, noise, dtype=LD):
    """dict(Quu, Lu, La, beta_u[, Kuu]) in `dtype`; y None: no beta_u (the covariances need none)."""
    nu = S.shape[0]
    Kuu = cov(spec, S, S if nu > 512 else None, dtype)      # (large: as a cross block, which is threaded; the same entries)
    Quu = Kuu + dtype(noise) * np.eye(nu, dtype=dtype)
    Kuf = cov(spec, S, X, dtype)
    A = Quu + mm(Kuf, Kuf.T, dtype) / dtype(noise)
    m = dict(Kuu=Kuu, Quu=Quu, Lu=chol(Quu, dtype), La=chol(A, dtype), beta_u=None)
    if y is not None:
        r = mm(Kuf, np.asarray(y, dtype=float).astype(dtype), dtype) / dtype(noise)
        m["beta_u"] = bwd(m["La"], fwd(m["La"], r, dtype), dtype)
    return m


def weights(spec, S, noise, m, c, omega, phase, xi1, xi2, dtype=LD, mutant=None):
    """V (P, nu) from the model dict `m` and the base draws (c = path_ref.feature_weights(w); xi1, xi2: (P, nu) unit draws)."""
    xi1, xi2 = np.asarray(xi1, dtype=float).astype(dtype), np.asarray(xi2, dtype=float).astype(dtype)
    if mutant == "swap":
        xi1, xi2 = xi2, xi1
    return weights_eps(spec, S, m, c, omega, phase, np.sqrt(dtype(noise)) * xi1, xi2, dtype, mutant)


def weights_eps(spec, S, m, c, omega, phase, eps_u, xi_q, dtype=LD, mutant=None):
    """V from the arguments of the C ABI: eps_u = sqrt(noise) Xi1 and xi_q = Xi2, each (P, nu) or None (zeros)."""
    R = PR.prior_paths(c, omega, phase, S, dtype)
    xi2 = np.zeros(R.shape, dtype=dtype) if xi_q is None else np.asarray(xi_q).astype(dtype)
    if mutant != "no_xi1" and eps_u is not None:
        R = R + np.asarray(eps_u).astype(dtype)
    Lu = chol(m["Kuu"], dtype) if mutant == "quu_no_nugget" else m["Lu"]
    sol = bwd(Lu, fwd(Lu, R.T, dtype), dtype).T                                   # (F~_S + eps_u) Quu^-1
    q = fwd(m["La"], xi2.T, dtype).T if mutant == "la_side" else bwd(m["La"], xi2.T, dtype).T      # row s: (La^-T xi2_s)^T
    b = np.asarray(m["beta_u"], dtype=dtype)[None, :]
    return (b + sol if mutant == "plus" else b - sol) + q


def paths(spec, c, omega, phase, V, S, Z, dtype=LD):
    return PR.paths(spec, c, omega, phase, V, S, Z, dtype)


def gradient(spec, c, omega, phase, V, S, Zp, path, dtype=LD):
    return PR.gradient(spec, c, omega, phase, V, S, Zp, path, dtype)


def mean(spec, S, m, Z, dtype=LD):
    return mm(cov(spec, S, Z, dtype).T, m["beta_u"], dtype)


def exact_cov(spec, S, m, Z, dtype=LD):
    """k(z,z') - k_u^T Quu^-1 k_u' + k_u^T A^-1 k_u' = K(Z,Z) - Wu^T Wu + Wa^T Wa."""
    Ku = cov(spec, S, Z, dtype)
    Wu, Wa = fwd(m["Lu"], Ku, dtype), fwd(m["La"], Ku, dtype)
    return cov(spec, Z, None, dtype) - mm(Wu.T, Wu, dtype) + mm(Wa.T, Wa, dtype)


def feature_cov(spec, S, noise, m, omega, phase, Z, dtype=LD, prior="features"):
    """A_J (Phi_J Phi_J^T) A_J^T + noise G_u G_u^T + K_zu A^-1 K_uz; prior="exact": K(J, J) in place of Phi_J Phi_J^T."""
    Ku = cov(spec, S, Z, dtype)
    G = bwd(m["Lu"], fwd(m["Lu"], Ku, dtype), dtype).T                            # K_zu Quu^-1
    J = np.vstack([Z, S])
    if prior == "exact":
        PP = cov(spec, J, None, dtype)
    else:
        Phi = dtype(PR.amplitude(spec, omega.shape[0])) * PR.cos_features(omega, phase, J, dtype)
        PP = mm(Phi, Phi.T, dtype)
    AJ = np.hstack([np.eye(Z.shape[0], dtype=dtype), -G])
    Wa = fwd(m["La"], Ku, dtype)
    return mm(mm(AJ, PP, dtype), AJ.T, dtype) + dtype(noise) * mm(G, G.T, dtype) + mm(Wa.T, Wa, dtype)


# ---- the linear map of the base draws ------------------------------------------------------------------------------------------------
def unit_draws(L, nu):
    """(w, xi1, xi2) of the L + 2 nu + 1 paths whose base draws are the unit vectors of (w, Xi1, Xi2), then one all-zero path."""
    n = L + 2 * nu
    E = np.vstack([np.eye(n), np.zeros((1, n))])
    return E[:, :L].copy(), E[:, L:L + nu].copy(), E[:, L + nu:].copy()


def linear_map(f):
    """(mean (M,), J_map (M, L + 2 nu)) from the (L + 2 nu + 1, M) values of the unit_draws paths."""
    f = np.asarray(f)
    return f[-1], (f[:-1] - f[-1][None, :]).T


def unit_paths(spec, S, noise, m, omega, phase, Z, dtype=LD, mutant=None):
    """The values of the unit_draws paths by the definition."""
    w, xi1, xi2 = unit_draws(omega.shape[0], S.shape[0])
    c = PR.feature_weights(spec, w)
    return paths(spec, c, omega, phase, weights(spec, S, noise, m, c, omega, phase, xi1, xi2, dtype, mutant), S, Z, dtype)


def rel(a, b):
    """max |a - b| / max |b|."""
    b = np.asarray(b)
    return float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))
