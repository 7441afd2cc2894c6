"""NumPy restatements of q-point batch acquisition (Kriging believer / constant liar) -- test infrastructure, not product code.

`refit_path` is the loop a user writes without `selectBatch`: per pick a NEW model on the data grown by the earlier picks and their
believed values, the posterior at every candidate, the cost, the mask, the first minimum.  It is built only from
`bo_compose.DenseModel` / `bo_compose.costs`, which `test_bo_host.py` pins against the reference fixture: the yardstick.
`rank1_path` is the recurrence gpx_acq_batch implements (include/gpx.h): one model, rank-one conditioning per pick.

`param_rule`: a float = the cost's parameter at every pick (kappa; a given fBest); "best" = max of the observations AND the values
believed so far (what constructing the cost anew on the grown data gives).  `lie`: "believer" or a float.
`posterior_of(X, y)` (optional) returns a function Z -> (mean, signed variance) in place of `DenseModel(...).posterior`, for
kernels `bo_compose.kmat` does not have.
Both return (picks, rows (q x M, NaN at the picks made before), believed values (q,))."""
import numpy as np

import bo_compose as bc


def first_min(c):
    ok = np.flatnonzero(~np.isnan(c))
    return -1 if ok.size == 0 else int(ok[np.argmin(c[ok])])


def _param(param_rule, ys):
    return float(np.max(ys)) if isinstance(param_rule, str) else float(param_rule)


def refit_path(spec, X, y, noise, C, acq, param_rule, lie, q, forced=None, posterior_of=None):
    assert param_rule == "best" or not isinstance(param_rule, str)
    Xa, ya, picks, rows, lies = np.array(X, dtype=float), np.array(y, dtype=float), [], [], []
    for t in range(q):
        if posterior_of is None:
            mean, var = bc.DenseModel(spec, Xa, ya, noise).posterior(C)
        else:
            mean, var = posterior_of(Xa, ya)(C)
        c = bc.costs(acq, _param(param_rule, ya), mean, var)
        c[picks] = np.nan
        s = first_min(c) if forced is None else int(forced[t])
        believed = float(mean[s]) if lie == "believer" else float(lie)
        rows.append(c)
        picks.append(s)
        lies.append(believed)
        Xa, ya = np.vstack((Xa, C[s:s + 1])), np.append(ya, believed)
    return picks, np.array(rows), np.array(lies)


def rank1_path(spec, X, y, noise, C, acq, param_rule, lie, q):
    assert param_rule == "best" or not isinstance(param_rule, str)
    m = bc.DenseModel(spec, X, y, noise)
    Kx = bc.kmat(spec, X, C)
    W = np.linalg.solve(m.L, Kx)
    mu = Kx.T @ m.alpha
    v = bc.kmat(spec, C[:1], C[:1])[0, 0] - np.sum(W * W, axis=0)
    U = np.zeros((q, len(C)))
    picks, rows, lies = [], [], []
    param = _param(param_rule, y)
    for t in range(q):
        c = bc.costs(acq, param, mu, v)
        c[picks] = np.nan
        s = first_min(c)
        delta = v[s] + noise
        believed = float(mu[s]) if lie == "believer" else float(lie)
        rows.append(c)
        picks.append(s)
        lies.append(believed)
        u = (bc.kmat(spec, C[s:s + 1], C)[0] - W[:, s] @ W - U[:t, s] @ U[:t]) / np.sqrt(delta)
        U[t] = u
        mu = mu + u * (believed - mu[s]) / np.sqrt(delta)
        v = v - u * u
        if isinstance(param_rule, str):
            param = max(param, believed)
    return picks, np.array(rows), np.array(lies)


# the configurations of the batch tests: name -> (spec, n, M, noise, seed)
CONFIGS = {
    "se3": (dict(kind="se", cl=[0.5, 0.7, 0.9], signalSize=1.3, d=3), 120, 500, 1e-3, 11),
    "m52": (dict(kind="matern52", rho=0.8, signalSize=1.1, d=4), 200, 700, 1e-2, 12),
    "m32": (dict(kind="matern32", rho=0.5, signalSize=1.3, d=2), 80, 400, 1e-3, 13),
    "big": (dict(kind="matern52", rho=1.5, signalSize=1.0, d=8), 4100, 9000, 1e-2, 4100),
}


def problem(name):
    """(spec, X, y, C, noise): X, then C uniform on [-1, 1]^d, then the noise draw of y."""
    spec, n, M, noise, seed = CONFIGS[name]
    rng = np.random.default_rng(seed)
    d = spec["d"]
    X = rng.uniform(-1, 1, (n, d))
    C = rng.uniform(-1, 1, (M, d))
    y = np.sin(3 * X[:, 0]) + 0.5 * np.cos(2 * X.sum(axis=1)) + np.sqrt(noise) * rng.standard_normal(n)
    return spec, X, y, C, noise


def row_err(got, want):
    """max-norm of a cost row's error relative to the row's largest magnitude; the NaN patterns must coincide."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok])) / np.max(np.abs(want[ok])))
