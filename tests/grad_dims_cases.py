"""One recipe for every case of the gradient sweep over the dimension classes up to 32 (tests/test_grad_dims_host.py,
tests/test_gpu_grad_dims.py): data and NumPy references, not product code.

Dimensions: the smallest and the full case of each register-array size of GPX_SE_DISPATCH that no dense gradient test reaches
(9 and 16 for the arrays of 16 coordinates, 17 and 32 for those of 32), and d = 2 (the array of 2, which grad.hip never ran).
N = 300 is one full stride of the 256-thread loops plus a ragged tail, ragged against the 64 and the 128 tiles; 70 evaluation
points / candidates / inducing points are one ragged 64 tile, below one 128 tile.

    X ~ U(-1, 1)^d from default_rng(700 + d);   y = sin(3 X + arange(d)).sum(1) / sqrt(d) + 0.1 N(0, 1)
    Z, C ~ U(-1, 1)^d, 70 each; the last 35 candidates are X[argmax y] + 0.05 N(0, 1)   (PI / EI not saturated)
    S = the first 70 rows of a permutation of X;   noise variance 0.05
    se        cl_l = sqrt(d) (0.6 + 0.8 ((7 l) mod d) / d), signalSize 1.3     (distinct, not monotone in l)
    matern32  rho = 1.2 sqrt(d), signalSize 1.1
    matern52  rho = 1.5 sqrt(d), signalSize 1.1

Every reference is one of the NumPy forms the suite already has (oracle/gpexp_oracle.py, loo_ref, fitc_grad_ref, fitc_loo_ref,
fitc_inducing_ref, vfe_ref, vfe_acq_ref, matern_pointgrad_ref, bo_compose), computed once per case, shared and read-only.  The
second forms (`*_other`) are what a bound is re-derived from when the first form's own error is not small against it."""
import functools
from types import SimpleNamespace

import numpy as np

import bo_compose as bc
import fitc_grad_ref as fref
import fitc_inducing_ref as iref
import fitc_loo_ref as flref
import loo_ref
import matern_pointgrad_ref as mref
import vfe_acq_ref as aref
import vfe_ref as vref
from oracle import gpexp_oracle as orc

DIMS = (2, 9, 16, 17, 32)
KINDS = ("se", "matern32", "matern52")
N, M, NU, NOISE = 300, 70, 70, 0.05
LOO_KIND = {"se": "se", "matern32": "m32", "matern52": "m52"}
# register arrays of GPX_SE_DISPATCH (gpx_internal.h) a dimension takes
DMAX = {2: 2, 8: 8, 9: 16, 16: 16, 17: 32, 32: 32}
# UCB (kappa = 2), PI and EI with fBest = max y -- and PI, EI with fBest = median y: y carries noise of deviation 0.1, so max y lies
# several posterior deviations above the posterior mean where the model is well determined (g = (fBest - mean) / s >= 4 at every
# candidate of half the cases); PI's gradient is then of order 1e-3 .. 1e-9, still compared entry by entry on the device, but too
# small for central differences of the cost to resolve.  With the median both costs are of order one at every d.
ACQ = {"ucb": (bc.UCB, lambda y: 2.0), "pi": (bc.PI, lambda y: float(np.max(y))), "ei": (bc.EI, lambda y: float(np.max(y))),
       "pi_median": (bc.PI, lambda y: float(np.median(y))), "ei_median": (bc.EI, lambda y: float(np.median(y)))}
ACQS = tuple(ACQ)
PARAMS = [(kind, d) for kind in KINDS for d in DIMS]
IDS = ["%s-d%d" % p for p in PARAMS]
# the 6 evaluation points / candidates whose gradients the host test differentiates numerically: three of the uniform ones and
# three of those around the best observation
FD_POINTS = (0, 17, 34, 35, 52, 69)


def se_lengths(d):
    return np.sqrt(d) * (0.6 + 0.8 * ((7 * np.arange(d)) % d) / d)


def make_spec(kind, d, lengths=None):
    """The oracle's dict for the kernel of the recipe (or with other correlation lengths)."""
    if kind == "se":
        cl = se_lengths(d) if lengths is None else np.asarray(lengths, dtype=float)
        return dict(kind="se", cl=[float(v) for v in cl], signalSize=1.3, d=int(d))
    return dict(kind=kind, rho=float((1.2 if kind == "matern32" else 1.5) * np.sqrt(d)), signalSize=1.1, d=int(d))


def hyp_of(spec):
    """[lengths..., signalSize], the order of the C ABI."""
    return fref.hyp_of(spec)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(kind, d):
    """SimpleNamespace(kind, d, spec, X, y, Z, C, S, noise): drawn once, read-only."""
    rng = np.random.default_rng(700 + d)
    X = rng.uniform(-1.0, 1.0, (N, d))
    y = np.sin(3.0 * X + np.arange(d)).sum(1) / np.sqrt(d) + 0.1 * rng.standard_normal(N)
    Z = rng.uniform(-1.0, 1.0, (M, d))
    C = rng.uniform(-1.0, 1.0, (M, d))
    C[M // 2:] = X[np.argmax(y)] + 0.05 * rng.standard_normal((M - M // 2, d))
    S = X[rng.permutation(N)[:NU]].copy()
    frozen(X, y, Z, C, S)
    return SimpleNamespace(kind=kind, d=d, spec=make_spec(kind, d), X=X, y=y, Z=Z, C=C, S=S, noise=NOISE)


def swapped(c):
    """The SE case with the last two correlation lengths exchanged."""
    cl = se_lengths(c.d)
    cl[[c.d - 2, c.d - 1]] = cl[[c.d - 1, c.d - 2]]
    return SimpleNamespace(**dict(vars(c), spec=make_spec("se", c.d, cl)))


def zeroed(P):
    """The point set with its last coordinate set to zero."""
    Q = np.array(P)
    Q[:, -1] = 0.0
    return Q


def embedded(c, value=0.3):
    """The same model in d + 1 coordinates: one more coordinate, the same constant for every point; length 1 for SE."""
    def grow(P):
        return np.ascontiguousarray(np.hstack([P, np.full((len(P), 1), value)]))
    spec = dict(c.spec, d=c.d + 1)
    if c.kind == "se":
        spec["cl"] = list(c.spec["cl"]) + [1.0]
    return SimpleNamespace(kind=c.kind, d=c.d + 1, spec=spec, X=grow(c.X), y=c.y, Z=grow(c.Z), C=grow(c.C), S=grow(c.S), noise=c.noise)


# ---- metrics: those of the existing parity tests -------------------------------------------------------------------------------
def entry_relerr(a, b):
    """max_i |a_i - b_i| / |b_i| (tests/test_gpu_fitc_grad.py, tests/test_gpu_golden_r6.py)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def max_relerr(a, b):
    """max |a - b| / max |b| (tests/test_gpu_fitc_inducing.py; helpers.rel and test_gpu_bo.vrel are the same figure)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# (metric, bound) of every comparison of tests/test_gpu_grad_dims.py: those of the existing parity test of the same entry point
#   entry: entry_relerr, every component against its own size;  max: max_relerr, against the largest entry of the reference
TOL = {
    "lml": ("entry", 1e-9),            # tests/test_gpu_api.py, tests/test_gpu_golden_r6.py
    "loo": ("max", 1e-9),              # tests/test_gpu_loo.py (helpers.rel)
    "point": ("max", 1e-9),            # tests/test_gpu_f1.py, tests/test_gpu_matern_pointgrad.py (helpers.rel)
    "fitc_point": ("max", 1e-8),       # tests/test_gpu_matern_pointgrad.py::test_fitc_model, tests/test_gpu_f1.py (FITC)
    "acq": ("max", 1e-9),              # tests/test_gpu_bo.py (vrel)
    "vfe_acq": ("max", 1e-8),          # tests/test_gpu_vfe_acq.py (vrel)
    "fitc_lml": ("entry", 1e-8),       # tests/test_gpu_fitc_grad.py
    "fitc_loo": ("entry", 1e-8),       # tests/test_gpu_fitc_loo.py
    "fitc_inducing": ("max", 1e-8),    # tests/test_gpu_fitc_inducing.py
    "vfe": ("entry", 1e-8),            # tests/test_gpu_vfe.py, the hyper-parameter gradient
    "vfe_inducing": ("max", 1e-8),     # tests/test_gpu_vfe.py, dF/dS
}


def err(what, a, b):
    """The error of `a` against the reference `b` in the metric of TOL[what]."""
    return entry_relerr(a, b) if TOL[what][0] == "entry" else max_relerr(a, b)


# ---- references ----------------------------------------------------------------------------------------------------------------
def acq_param(name, y):
    return ACQ[name][1](y)


ACQ_ID = {name: v[0] for name, v in ACQ.items()}


def lml(c):
    """(value, gradient [lengths..., signalSize, noise VARIANCE]) of the dense log marginal likelihood: oracle.loglike_grad with its
    'noise' entry taken back from the reference's 2 * noise scaling (gp.py:463-464) to what the device entry points return."""
    val, g = orc.loglike_grad(c.spec, c.X, c.y, c.noise)
    out = np.array([g[k] for k in orc.hyp_keys(c.spec)])
    out[-1] /= 2.0 * c.noise
    return float(val), out


def lml_other(c):
    """The same gradient from a Cholesky factor instead of the oracle's pinv, and from kparts' derivative matrices."""
    K0, dK = fref.kparts(c.spec, c.X, c.X)
    hyp = hyp_of(c.spec)
    Li = np.linalg.solve(np.linalg.cholesky(K0 + c.noise * np.eye(N)), np.eye(N))
    P = Li.T @ Li
    a = P @ c.y
    T = np.outer(a, a) - P
    return np.array([0.5 * np.sum(T * m) / hyp[k] for k, m in enumerate(dK)] + [0.5 * np.sum(T * K0) / hyp[-1], 0.5 * np.trace(T)])


def loo(c):
    """(mean, var, L_LOO, gradient) of the dense leave-one-out closed form (loo_ref.loo_all)."""
    return loo_ref.loo_all(LOO_KIND[c.kind], c.d, hyp_of(c.spec), c.X, c.noise, c.y)


def point_grads(c, Z=None, prec=None):
    """(full (N d, M), newpt (M d,), ivar (N d,)) of the posterior variance: the oracle's reference-convention forms for the
    squared exponential, matern_pointgrad_ref.gradients for the Materns; with the precision `prec` instead of the dense one."""
    Z = c.Z if Z is None else Z
    if c.kind != "se":
        return mref.gradients(c.kind, c.spec["rho"], c.spec["signalSize"], c.X, Z, c.noise, prec=prec)
    model = dict(X=np.array(c.X), P=prec) if prec is not None else orc.fit(c.spec, c.X, None, c.noise)
    full = orc.variance_derivative(c.spec, model, Z)
    return full, orc.variance_deriv_wrt_newpt(c.spec, model, Z), full.sum(axis=1) / float(len(Z))   # (the sum: oracle.ivar_grad)


def se_point_grads_dense(c, Z=None, prec=None):
    """The squared exponential's three gradients in the reference's convention as dense algebra (the derivative is linear in the
    coordinate difference): the second form beside the oracle's loops."""
    Z = c.Z if Z is None else Z
    cl, sig = np.asarray(c.spec["cl"]), c.spec["signalSize"]
    K0, Kxz = bc.kmat(c.spec, c.X, c.X), bc.kmat(c.spec, c.X, Z)
    beta = prec @ Kxz if prec is not None else np.linalg.solve(K0 + c.noise * np.eye(N), Kxz)
    cc = -sig / cl ** 2
    Q = beta * Kxz
    R = K0 * (beta @ beta.T)
    ivar = 2.0 * cc * ((Q @ Z - c.X * Q.sum(axis=1, keepdims=True)) + (c.X * R.sum(axis=1, keepdims=True) - R @ c.X)) / len(Z)
    newpt = -2.0 * cc * (Z * Q.sum(axis=0)[:, None] - Q.T @ c.X)
    K0b = K0 @ beta
    full = np.zeros((N, c.d, len(Z)))
    for l in range(c.d):
        t1 = cc[l] * (Z[None, :, l] - c.X[:, None, l]) * Kxz
        t2 = cc[l] * (c.X[:, None, l] * K0b - K0 @ (c.X[:, None, l] * beta))
        full[:, l, :] = beta * (2.0 * t1 + 2.0 * t2)
    return full.reshape(N * c.d, len(Z)), newpt.reshape(-1), ivar.reshape(-1)


class FitcSolve(object):
    """(Q + G)^-1 of the FITC model on (X, S) as an operator: `P @ B` and `A @ P` are Cholesky solves with the dense N x N
    covariance Q + G (condition ~1e4: an error of ~1e-12), so that it goes wherever the references take a precision MATRIX.  A
    product with the explicit precision loses cond(Q + G) times the error of its entries, because P K(X, Z) is that much smaller
    than |P| |K(X, Z)|: `fitc_point_gap` measures what that costs the gradients."""
    __array_ufunc__ = None      # ndarray @ FitcSolve goes to __rmatmul__

    def __init__(self, c):
        m = fref._model(c.spec, c.X, c.S, c.y, c.noise)
        self.L = np.linalg.cholesky(flref._dense_cov(m))
        self.woodbury = np.diag(m["Gi"]) - m["Y"].T @ m["Y"]       # the explicit matrix, from the two factors of the model

    def __matmul__(self, B):
        return np.linalg.solve(self.L.T, np.linalg.solve(self.L, B))

    def __rmatmul__(self, A):
        return (self @ np.asarray(A).T).T


def fitc_prec(c):
    return FitcSolve(c)


def fitc_point_gap(c):
    """The FITC point gradients from the explicit Woodbury precision and from oracle.fitc_matrices' (pinv(Quu), an explicit inverse
    of Quu + Kuf G^-1 Kfu) against the reference from Cholesky solves, in the parity test's metric: (woodbury, oracle), each the
    worst of the three gradients.  The first is the two-forms figure of this reference (seen <= 1.5e-10: the bound of the parity test
    stands); the second is why the oracle's matrix is not the yardstick here (seen up to 2.1e-6, two hundred bounds)."""
    ref = reference(c.kind, c.d, "fitc_point")
    forms = se_point_grads_dense if c.kind == "se" else point_grads
    return tuple(max(err("fitc_point", a, b) for a, b in zip(forms(c, prec=P), ref))
                 for P in (FitcSolve(c).woodbury, orc.fitc_matrices(c.spec, c.X, c.noise, c.S)[1]))


def variance(c, X, Z):
    """The oracle's posterior variance at Z of the model refitted on X."""
    return orc.posterior(c.spec, orc.fit(c.spec, X, None, c.noise), Z, compvar=1)[1]


def variance_dense(c, X, Z):
    """The same variance from bo_compose.kmat and a Cholesky factor: what the central differences over many refits are taken of
    (tests/test_grad_dims_host.py holds it to the oracle's first)."""
    Kxz = bc.kmat(c.spec, X, Z)
    W = np.linalg.solve(np.linalg.cholesky(bc.kmat(c.spec, X, X) + c.noise * np.eye(len(X))), Kxz)
    return c.spec["signalSize"] - np.sum(W * W, axis=0)


def acq_grads(c, C=None):
    """{name: (M, d)} closed-form gradients of the costs of ACQ on the dense model (bo_compose.DenseModel.grad)."""
    C = c.C if C is None else C
    model = bc.DenseModel(c.spec, c.X, c.y, c.noise)
    return {name: model.grad(ACQ_ID[name], acq_param(name, c.y), C) for name in ACQS}


def acq_costs(c, name, P):
    mean, var = bc.DenseModel(c.spec, c.X, c.y, c.noise).posterior(P)
    return bc.costs(ACQ_ID[name], acq_param(name, c.y), mean, var)


def vfe_acq_grads(c, C=None, reordered=False):
    """{name: (M, d)} closed-form gradients of the costs of ACQ on the VFE model (vfe_acq_ref)."""
    setup = aref.grad_setup(c.spec, c.X, c.S, c.y, c.noise, c.C if C is None else C, reordered)
    return {name: aref.grad_of(setup, ACQ_ID[name], acq_param(name, c.y)) for name in ACQS}


def vfe_acq_costs(c, name, P):
    return bc.costs(ACQ_ID[name], acq_param(name, c.y), *vref.predict(c.spec, c.X, c.S, c.y, c.noise, P))


def fitc_lml(c):
    return fref.fitc_value_grad(c.spec, c.X, c.S, c.y, c.noise)


def fitc_loo(c):
    return flref.loo(c.spec, c.X, c.S, c.y, c.noise)


def fitc_inducing(c):
    return iref.grad_S(c.spec, c.X, c.S, c.y, c.noise)


def vfe(c):
    """(F, hyper gradient, dF/dS)"""
    return vref.value_grad(c.spec, c.X, c.S, c.y, c.noise) + (vref.grad_S(c.spec, c.X, c.S, c.y, c.noise),)


@functools.lru_cache(maxsize=None)
def reference(kind, d, what):
    """The reference `what` of the case, computed once per process and read-only."""
    c = case(kind, d)
    out = {"lml": lml, "loo": loo, "point": point_grads, "fitc_point": lambda cc: point_grads(cc, prec=fitc_prec(cc)),
           "acq": acq_grads, "vfe_acq": vfe_acq_grads, "fitc_lml": fitc_lml, "fitc_loo": fitc_loo, "fitc_inducing": fitc_inducing,
           "vfe": vfe}[what](c)
    for a in (out.values() if isinstance(out, dict) else out if isinstance(out, tuple) else (out,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
