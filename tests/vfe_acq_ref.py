"""NumPy restatements of the Bayesian-optimisation costs on a VFE model -- their gradient w.r.t. the candidate and the q-point
batch recurrence -- for the tests: data, not product code.  Built on vfe_ref (the model and its predictor), bo_compose (the cost
formulas, dk/dz) and bo_batch_compose (the refit loop).

Notation of vfe_ref: S the nu inducing points, Quu = K(S,S) + noise I = Lu Lu^T, A = Quu + Kuf Kfu / noise = La La^T,
beta_u = Quu^-1 Kuf alpha = B alpha, k_u(z) = K(S, z);  mean = k_u^T beta_u,  var = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2.

Gradient.  With a = dA/dmu, b = dA/dvar of bo_compose.DenseModel.grad's table and k(z,z) constant:
    gamma(z) = Quu^-1 k_u - A^-1 k_u,     grad_z A = sum_u dk(z, s_u)/dz (a beta_u[u] - 2 b gamma(z)[u])

Batch.  The loop "cost on the grown data; first minimum; append the pick with its believed value", every refit with the SAME S and
hyper-parameters: one more observation at c_s changes A to A + k_u(c_s) k_u(c_s)^T / noise and nothing else, so with
Wa = La^-1 K(S, C), r_j = k(c_j,c_j) - |Lu^-1 k_u(c_j)|^2 (fixed) and t_j = |Wa[:, j]|^2, per pick
    v_j = r_j + t_j;   delta = noise + t_s  (NOT v_s + noise);   y_s = mu_s (believer) or the constant
    u_j = (Wa[:, s]^T Wa[:, j] - sum_{r<t} U[r][s] U[r][j]) / sqrt(delta);   U[t] = u
    mu_j += u_j (y_s - mu_s) / sqrt(delta);   t_j -= u_j^2;   param = max(param, y_s) under the "best" rule
`refit_path` is that loop taken literally: vfe_ref.predict on X + picks per pick."""
import numpy as np
import scipy.stats as spstats

import bo_batch_compose as bb
import bo_compose as bc
import fitc_grad_ref as ref
import vfe_ref as vref


def coefficients(acq, param, mean, var):
    """(a, b) = (dA/dmu, dA/dvar) at the posterior (mean, signed variance)."""
    s = np.sqrt(np.abs(var))
    sg = np.sign(var)
    if acq == bc.UCB:
        return -np.ones_like(s), param * sg / (2.0 * s)
    g = (param - mean) / s
    Phi, phi = spstats.norm.cdf(g), spstats.norm.pdf(g)
    if acq == bc.PI:
        return phi / s, phi * g * sg / (2.0 * s * s)
    return Phi, -phi * sg / (2.0 * s)


def grad_setup(spec, X, S, y, noise, Z, reordered=False):
    """What the gradients of every cost at the rows of Z share: the posterior, beta_u, gamma (nu x M) and dk/dz per candidate.
    reordered=True: gamma from one solve with Quu and one with A = La La^T formed, instead of the two backward sweeps."""
    Z = np.asarray(Z, dtype=float)
    m = vref._model(spec, X, S, y, noise)
    Ku = ref.kparts(spec, S, Z)[0]
    wu = np.linalg.solve(m["Lu"], Ku)
    wa = np.linalg.solve(m["La"], Ku)
    beta_u = m["B"] @ m["alpha"]
    if reordered:
        gamma = np.linalg.solve(m["Quu"], Ku) - np.linalg.solve(m["La"] @ m["La"].T, Ku)
    else:
        gamma = np.linalg.solve(m["Lu"].T, wu) - np.linalg.solve(m["La"].T, wa)
    return dict(mean=Ku.T @ beta_u, var=m["s"] - np.sum(wu * wu, axis=0) + np.sum(wa * wa, axis=0), beta_u=beta_u, gamma=gamma,
                dk=[bc.dkdz(spec, z, S) for z in Z], reordered=reordered)


def grad_of(setup, acq, param):
    """(M, d) closed-form gradients of one cost from grad_setup's parts (reordered: the weighted sum taken back to front,
    coordinate by coordinate)."""
    a, b = coefficients(acq, param, setup["mean"], setup["var"])
    out = []
    for j, dk in enumerate(setup["dk"]):
        w = a[j] * setup["beta_u"] - 2.0 * b[j] * setup["gamma"][:, j]
        out.append([np.sum(dk[::-1, l] * w[::-1]) for l in range(dk.shape[1])] if setup["reordered"] else dk.T @ w)
    return np.array(out)


def grad(spec, X, S, y, noise, acq, param, Z, reordered=False):
    """(M, d) closed-form gradients of the costs at the rows of Z.  reordered=True: the same quantity summed in another order,
    for the round-off figure the tolerances quote."""
    return grad_of(grad_setup(spec, X, S, y, noise, Z, reordered), acq, param)


def posterior_of(spec, S, noise):
    """The `posterior_of` of bo_batch_compose.refit_path for a VFE model with the inducing points S kept."""
    return lambda Xa, ya: lambda C: vref.predict(spec, Xa, S, ya, noise, C)


def refit_path(spec, X, S, y, noise, C, acq, param_rule, lie, q, forced=None):
    return bb.refit_path(spec, X, y, noise, C, acq, param_rule, lie, q, forced=forced, posterior_of=posterior_of(spec, S, noise))


def rank1_path(spec, X, S, y, noise, C, acq, param_rule, lie, q):
    """(picks, rows (q x M, NaN at the picks made before), believed values (q,)) by the recurrence."""
    assert param_rule == "best" or not isinstance(param_rule, str)
    m = vref._model(spec, X, S, y, noise)
    Ku = ref.kparts(spec, S, C)[0]
    wu = np.linalg.solve(m["Lu"], Ku)
    Wa = np.linalg.solve(m["La"], Ku)
    mu = Ku.T @ (m["B"] @ m["alpha"])
    r = m["s"] - np.sum(wu * wu, axis=0)
    t = np.sum(Wa * Wa, axis=0)
    U = np.zeros((q, len(C)))
    picks, rows, lies = [], [], []
    param = bb._param(param_rule, y)
    for k in range(q):
        c = bc.costs(acq, param, mu, r + t)
        c[picks] = np.nan
        s = bb.first_min(c)
        delta = noise + t[s]
        believed = float(mu[s]) if lie == "believer" else float(lie)
        rows.append(c)
        picks.append(s)
        lies.append(believed)
        u = (Wa[:, s] @ Wa - U[:k, s] @ U[:k]) / np.sqrt(delta)
        U[k] = u
        mu = mu + u * (believed - mu[s]) / np.sqrt(delta)
        t = t - u * u
        if isinstance(param_rule, str):
            param = max(param, believed)
    return picks, np.array(rows), np.array(lies)


def grad_inputs(spec, X, y):
    """The 24 candidates of the gradient tests: uniform in [-1, 1]^d from default_rng(77), the first next to a training point, eleven
    around the best observation (where PI / EI with fBest = max y are not saturated)."""
    d = spec["d"]
    rng = np.random.default_rng(77)
    Z = rng.uniform(-1.0, 1.0, (24, d))
    Z[0] = X[3] + 1e-7
    Z[1:12] = X[np.argmax(y)] + 0.05 * rng.standard_normal((11, d))
    return Z


def central_differences(costs_of, Z, h=1e-5):
    """(M, d) central differences of costs_of (points -> costs), every perturbed point in ONE call."""
    M, d = Z.shape
    P = np.repeat(Z[:, None, :], 2 * d, axis=1)
    for l in range(d):
        P[:, 2 * l, l] += h
        P[:, 2 * l + 1, l] -= h
    c = np.asarray(costs_of(P.reshape(-1, d))).reshape(M, 2 * d)
    return (c[:, 0::2] - c[:, 1::2]) / (2 * h)


ACQ_PARAMS = {"ucb": (bc.UCB, lambda y: 2.0), "pi": (bc.PI, lambda y: float(np.max(y))), "ei": (bc.EI, lambda y: float(np.max(y)))}
