"""Gaussian-process model with the reference's interface (gpExp/gp.py, class GP), computed on the GPU.

What changes underneath: the reference builds K row by row in Python, inverts it with
`numpy.linalg.pinv` (SVD) and evaluates every posterior variance as a separate `k^T P k` matvec.  Here K is
assembled by one HIP kernel, factored once (K = L L^T, blocked fp64-MFMA Cholesky), and every later quantity is a
triangular solve or a column reduction against L:

    coeff = K^-1 y                     gpx_potrs        (gp.py:101)
    log det K = 2 sum log L_ii         gpx_logdet       (gp.py:434)
    mean = K(Z,X) coeff                gpx_posterior    (gp.py:137)
    var_j = k(z_j,z_j) - |L^-1 k_j|^2  gpx_posterior    (gp.py:142-144, 253-255)

`covarianceMatrix` and `precisionMatrix` remain available as attributes (external code reads them,
experimentalDesign.py:241-242) but are materialised lazily, on first access, from the device.

Rank-deficient K (e.g. noise 0.0 with coincident points): pinv truncates silently, Cholesky cannot.  Policy: a pivot
at round-off level (<= 1e-13 * largest diagonal entry) fails the factorisation, which is then repeated with those
points DROPPED (gpx_potrf_policy: unit pivot, zero column, zero row of the inverse -- every solve returns 0 in that
component, as if the point were not in the training set) and a RuntimeWarning says how many.  For an exactly duplicated
point with equal function values that is the pinv answer (posterior mean and variance to 1e-8, reference fixture
`rankdef`); `coeff` differs in how it is split between the duplicates (pinv: equal halves; here: all on the first).

FITC (gp.py:182-210, 401-426): `GP(kernel, noise, FITC=fraction)` draws the inducing points with
`np.random.permutation` exactly as the reference does (seed it the same way and the same points come out) and keeps
chol(Quu), Kuf, G and chol(Quu + Kuf G^-1 Kfu) on the device (gpx_fitc_*); predictions use the Woodbury form, the
N x N `covarianceMatrix` / `precisionMatrix` are only built when read.  The reference compares `self.fitcnodes == None`,
which raises for an ndarray, so there a GP instance survives only ONE FITC operation; here refits simply reuse
`fitcnodes`.  `generateSamples` stays out of scope.

VFE (none in the reference): `GP(kernel, noise, FITC=fraction, sparse="vfe")` keeps the same inducing points but scores and predicts
with Titsias' variational free energy (gpx_vfe_*): `loglikeParams` / `computeLogLike` return the lower bound F, with its
gradients, `evaluate` / `evaluateVariance` the optimal variational posterior of the latent function -- not FITC's convention of
the true k(z, X) against the Woodbury precision.  Quu keeps the noise nugget, as in the FITC model.
"""
import copy
import warnings

import numpy as np

from . import device as _dev
from . import dist as _dist
from ._lib import NotPositiveDefinite, hdot as _hdot
from .gp_kernel_utilities import calculateCovarianceMatrix, _check_nugget  # noqa: F401  (re-export like the reference)
from .paths import PathBase, spectralFrequencies as _spectralFrequencies

try:  # the reference prefers nlopt and falls back to SciPy (gp.py:28-41); only the SciPy branch is provided
    from scipy.optimize import fmin_l_bfgs_b as bfgs
except ImportError:  # pragma: no cover
    bfgs = None
NLOPT = False


def drawBaseSamples(baseSamples, nSamples, width, what):
    """The standard-normal base samples of a sampling call as a C-contiguous float64 array (S, width).  None draws
    np.random.standard_normal((nSamples, width)) -- the device makes no random numbers -- except under an attached multi-process
    session, where the calls run replicated and every rank would draw its own: ValueError.  A given array brings its own sample
    count S (nSamples is not consulted) and is checked for its shape (S >= 1, width) and finiteness (ValueError)."""
    width = int(width)
    if baseSamples is None:
        if int(nSamples) < 1:
            raise ValueError("%s: needs at least one sample, not %r" % (what, nSamples))
        if _dist.session() is not None:
            raise ValueError("%s: under a multi-process session baseSamples must be given (the call runs replicated and every "
                             "rank would draw its own)" % what)
        return np.ascontiguousarray(np.random.standard_normal((int(nSamples), width)), dtype=np.float64)
    xi = np.ascontiguousarray(baseSamples, dtype=np.float64)
    if xi.ndim != 2 or xi.shape[0] < 1 or xi.shape[1] != width:
        raise ValueError("%s: baseSamples must have shape (nSamples >= 1, %d), not %r" % (what, width, xi.shape))
    if not np.all(np.isfinite(xi)):
        raise ValueError("%s: baseSamples must be finite" % what)
    return xi


class JointSampler(object):
    """What GP.posteriorSampler returns: a device-resident joint sampler at M points (device.PosteriorSampler) behind the
    base-sample rules of drawBaseSamples."""

    def __init__(self, state, m):
        self._state, self.nPoints = state, int(m)

    def _live(self):
        if self._state is None:
            raise ValueError("the sampler is closed")
        return self._state

    def draw(self, nSamples=1, baseSamples=None):
        """(nSamples, M): row s = mean + F baseSamples[s]."""
        st = self._live()
        return st.draw(drawBaseSamples(baseSamples, nSamples, self.nPoints, "draw"))

    def argbest(self, nSamples=1, baseSamples=None, minimize=True, returnSamples=False):
        """(indices (nSamples,) int64, values (nSamples,)[, samples (nSamples, M)]): per draw the FIRST index of its minimum
        (minimize=False: maximum) and the value there, reduced on the device."""
        st = self._live()
        return st.argbest(drawBaseSamples(baseSamples, nSamples, self.nPoints, "argbest"), minimize=bool(minimize),
                          want_samples=bool(returnSamples))

    def close(self):
        if self._state is not None:
            self._state.close()
        self._state = None


class PathSampler(object):
    """What GP.pathSampler / GP.priorPathSampler return: S device-resident posterior (prior) PATHS (device.PathSampler), functions
    that can be evaluated at any number of points, in chunks, and differentiated.  `base` is the PathBase they were made from."""

    def __init__(self, state, base, d):
        self._state, self.base, self.nPaths, self._d = state, base, base.nPaths, int(d)

    def _points(self, pts):
        if self._state is None:
            raise ValueError("the sampler is closed")
        pts = np.asarray(pts, dtype=float)
        assert pts.ndim == 2 and pts.shape[1] == self._d, "evaluation points for GP is incorrect shape"
        return _dev.points(_dev.context(), pts)

    def evaluate(self, newpt):
        """(S, M): row s = path s at the rows of `newpt`."""
        Z = self._points(newpt)
        return self._state.evaluate(Z)

    def argbest(self, newpt, minimize=True, returnValues=False):
        """(indices (S,) int64, values (S,)[, values (S, M)]): per path the FIRST index of its minimum (minimize=False: maximum)
        over the rows of `newpt` and the value there, reduced on the device; without returnValues only these reach the host."""
        Z = self._points(newpt)
        return self._state.argbest(Z, minimize=bool(minimize), want_values=bool(returnValues))

    def gradient(self, points, pathIndex, returnValues=False):
        """(P, d): row p = the gradient of path pathIndex[p] at points[p] [, the values (P,) there]."""
        Z = self._points(points)
        return self._state.gradient(Z, np.asarray(pathIndex, dtype=np.int64).ravel(), want_values=bool(returnValues))

    def close(self):
        if self._state is not None:
            self._state.close()
        self._state = None


class GP:
    """Zero-prior-mean GP regression model."""

    coeff = None
    noise = None
    pts = None
    FITC = None
    fitcnodes = None
    sparse = "fitc"   # which sparse model FITC=fraction builds: "fitc" or "vfe"

    def __init__(self, kernel_in, noiseIn, **kwargs):
        sparse = kwargs.get('sparse', 'fitc')
        if sparse not in ('fitc', 'vfe'):
            raise ValueError("GP: sparse must be 'fitc' or 'vfe', not %r" % (sparse,))
        if sparse == 'vfe' and kwargs.get('FITC') is None:
            raise ValueError("GP: sparse='vfe' needs FITC=fraction (the share of the nodes drawn as inducing points)")
        self.sparse = sparse
        try:
            self.kernel = copy.deepcopy(kernel_in)
        except Exception:
            print("warning ")
            self.kernel = copy.copy(kernel_in)
        self.noise = noiseIn  # added to the diagonal as a VARIANCE (gp.py:68, 178)
        if 'FITC' in kwargs:
            self.FITC = kwargs['FITC']  # fraction of the nodes used as inducing points (gp.py:69-70, 187)
        self._fitc = None    # device FITC model (gpx_fitc_*)
        self._X = None       # device point set
        self._Lc = None      # distributed-factor mode (dist.CyclicFactor): the factor lives block-cyclic on the ranks ...
        self._Ld = None      # ... and a dense factor is assembled only when something asks for `_L`
        self._L = None       # device Cholesky factor of K(pts) + nugget
        self._nugget = None  # nugget that went into _L
        self._K_host = None
        self._P_host = None
        self.jitter = 0.0    # kept for compatibility: the rank-deficient policy no longer perturbs the diagonal
        self.dropped = 0     # points dropped by the rank-deficient policy in the last factorisation
        # f2: the last factorisation, kept so that a refit whose leading points (and hyper-parameters) did
        # not change -- the design loop pins earlier points by bounds, experimentalDesign.py:722-724 -- only assembles and
        # factors the trailing rows.  (host copy of the points, nugget, hyper-parameter key, device factor)
        self._fcache = None
        self.reuseFactor = True

    # shallow copies (costFunctionGP_IVAR does copy.copy(gp), experimentalDesign.py:64) share device state,
    # which is immutable once built: a refit replaces the handles instead of mutating them.

    # ---- lazy dense attributes -------------------------------------------------------------------------
    @property
    def covarianceMatrix(self):
        if self._K_host is None and self._fitc is not None:
            self._K_host = self._fitc.dense(cov=True, prec=False)[0]
        elif self._K_host is None and self.pts is not None:
            self._K_host = calculateCovarianceMatrix(self.kernel, self.pts, self._nugget)
        return self._K_host

    @covarianceMatrix.setter
    def covarianceMatrix(self, value):
        self._K_host = value

    @property
    def precisionMatrix(self):
        if self._P_host is None and self._fitc is not None:
            self._P_host = self._fitc.dense(cov=False, prec=True)[1]
        elif self._P_host is None and self._has_factor():
            self._P_host = _dev.potri(_dev.context(), self._L).to_host(tri=2)   # lower triangle valid: mirrored
        return self._P_host

    @precisionMatrix.setter
    def precisionMatrix(self, value):
        self._P_host = value

    # the dense device factor.  Under a multi-process launch in the distributed-factor mode (dist.Session.use_cyclic) the fit
    # leaves a CyclicFactor instead: train / evaluate / evaluateVariance / the likelihood / the IVAR cost work on that, and a
    # dense replica is assembled the first time anything else reads `_L`.
    @property
    def _L(self):
        if self._Ld is None and self._Lc is not None:
            self._Ld = self._Lc.dense()
        return self._Ld

    @_L.setter
    def _L(self, value):
        if getattr(value, "is_cyclic", False):
            self._Lc, self._Ld = value, None
        else:
            self._Lc, self._Ld = None, value

    def _has_factor(self):
        return self._Lc is not None or self._Ld is not None

    # ---- helpers --------------------------------------------------------------------------------------------
    def gpPriorMean(self, pts):
        return np.zeros((pts.shape[0]))

    def _factor(self, nodes, nugget, remember=True):
        """Assemble K(nodes)+diag(nugget) and factor it in place on the device -> (X, L, 0.0).  `remember=False`
        (likelihood evaluations: every call has new hyper-parameters) neither consults nor replaces the kept factor."""
        _check_nugget(nugget)
        nodes = np.asarray(nodes, dtype=float)
        assert nodes.ndim == 2 and nodes.shape[1] == self.kernel.dimension, \
            (" Incorrect dimension of input points fed to kernel ", nodes.shape)
        ctx = _dev.context()
        spec = self.kernel._spec()
        X = _dev.points(ctx, nodes)
        # Rank-deficient policy (module docstring): pivots at round-off level count as failed, and the retry DROPS those
        # points, which is what the reference's pinv does with an exactly duplicated point (gp.py:181).
        diag = float(spec.hyp[-1]) if spec.kind != _dev.K_MEHLER else float(np.max(_dev.kdiag(ctx, spec, X)))
        tau = 1e-13 * (diag + float(np.max(np.asarray(nugget, dtype=float))))
        self.dropped = 0
        prev_policy = getattr(ctx, "_potrf_policy", (0.0, False))   # a policy the user set on the shared context survives
        try:
            _dev.potrf_policy(ctx, tau, False)
            self._last_refit = None    # (factor the last fit started from, rows it kept): costFunctionGP_IVAR updates its kept solve
            hit = self._cached_factor(nodes, nugget, spec)
            if hit is not None:
                return X, hit, 0.0
            keep = self._reusable_rows(nodes, nugget, spec) if remember else 0
            if keep > 0:
                try:
                    old = self._fcache[3]
                    L = _dev.refit_rows(ctx, spec, X, nugget, old, keep)
                    self._remember(nodes, nugget, spec, L)
                    self._last_refit = (old, keep)
                    return X, L, 0.0
                except NotPositiveDefinite:
                    pass  # fall through to the full path and its rank-deficient policy
            sess = _dist.session()
            if sess is not None and sess.use_fit(nodes.shape[0]):
                # multi-process launch: 2-D block-cyclic distributed fit, every rank keeps a replica of the factor
                # (dist.Session.factor).  A non-PD result is agreed by all ranks; they then all take the replicated
                # single-GPU path below with its rank-deficient policy.
                try:
                    Xd, L = sess.factor(spec, nodes, nugget, keep=remember)
                    if remember and not getattr(L, "is_cyclic", False):   # (rows are reused from a DENSE previous factor only)
                        self._remember(nodes, nugget, spec, L)
                    return Xd, L, 0.0
                except NotPositiveDefinite:
                    pass
            K = _dev.kfill(ctx, spec, X, nugget=nugget)
            try:
                L = _dev.potrf(ctx, K)
                if remember:
                    self._remember(nodes, nugget, spec, L)
                return X, L, 0.0
            except NotPositiveDefinite as first:
                if remember:
                    self._fcache = None
                _dev.kfill_into(ctx, spec, X, K, nugget=nugget)
                _dev.potrf_policy(ctx, tau, True)
                _dev.potrf(ctx, K)
                self.dropped = _dev.potrf_dropped(ctx)
                # once per (GP object, remember-mode): an optimiser loop over near-singular hyper-parameters would otherwise
                # raise it on every likelihood evaluation
                if not getattr(self, "_warned_dropped", {}).get(remember):
                    warnings.warn("covariance matrix not positive definite (pivot %d <= %.1e): %d point(s) whose "
                                  "conditional variance is at round-off level were dropped from the factor (the "
                                  "reference's pinv truncates the same directions)%s" %
                                  (first.pivot, tau, self.dropped,
                                   "" if remember else "; the log-likelihood returned is that of the REDUCED model -- the "
                                   "reference's value there is -0.5 y^T pinv(K) y - 0.5 slogdet(K) with slogdet -> -inf "
                                   "(gp.py:431-435), which no optimiser can use"), RuntimeWarning)
                    seen = dict(getattr(self, "_warned_dropped", {}))
                    seen[remember] = True
                    self._warned_dropped = seen
                return X, K, 0.0
        finally:
            _dev.potrf_policy(ctx, *prev_policy)

    @staticmethod
    def _spec_key(spec):
        return (spec.kind, spec.d, tuple(spec.hyp.tolist()))

    def _remember(self, nodes, nugget, spec, L):
        if self.reuseFactor and nodes.shape[0] >= 256:
            nug = None if np.ndim(nugget) == 0 else np.array(nugget, dtype=float, copy=True)
            self._fcache = (nodes.copy(), float(nugget) if nug is None else nug, self._spec_key(spec), L)
        else:
            self._fcache = None

    def _cached_factor(self, nodes, nugget, spec):
        """The kept factor itself when it IS the fit asked for: same kernel and hyper-parameters, bit-identical points, same
        nugget.  Read-only, so likelihood evaluations consult it too (computeLogLike right after train on the same points
        re-assembled and re-factored K: 2.4 of config C2's 6.3 ms)."""
        c = self._fcache
        if not self.reuseFactor or c is None or c[2] != self._spec_key(spec) or c[0].shape != nodes.shape:
            return None
        if np.ndim(nugget) == 0 and np.ndim(c[1]) == 0:
            if float(nugget) != c[1]:
                return None
        elif not np.array_equal(np.broadcast_to(np.asarray(nugget, dtype=float), (nodes.shape[0],)),
                                np.broadcast_to(np.asarray(c[1], dtype=float), (nodes.shape[0],))):
            return None
        return c[3] if np.array_equal(c[0], nodes) else None

    def _reusable_rows(self, nodes, nugget, spec):
        """Leading rows (multiple of 128) whose factor can be taken from the previous fit: same kernel and
        hyper-parameters, same nugget on those rows, bit-identical points.  0 = factor from scratch."""
        c = self._fcache
        if not self.reuseFactor or c is None or c[2] != self._spec_key(spec):
            return 0
        old, onug = c[0], c[1]
        m = min(old.shape[0], nodes.shape[0])
        if m < 128:
            return 0
        same = np.all(old[:m] == nodes[:m], axis=1)
        if np.ndim(nugget) == 0 and np.ndim(onug) == 0:
            if float(nugget) != onug:
                return 0
        else:
            a = np.broadcast_to(np.asarray(nugget, dtype=float), (nodes.shape[0],))[:m]
            b = np.broadcast_to(np.asarray(onug, dtype=float), (old.shape[0],))[:m]
            same = same & (a == b)
        p = m if same.all() else int(np.argmin(same))
        keep = (p // 128) * 128
        return keep if keep * 4 >= nodes.shape[0] else 0  # below a quarter of the rows the copy buys nothing

    # ---- training ---------------------------------------------------------------------------------------------
    def _fitc_model(self, nodes):
        """FITC branch of addNodesAndComputeCovariance / loglikeParams (gp.py:182-206, 401-426): inducing points are a
        random subset of the nodes, drawn once with np.random.permutation and then kept in `fitcnodes`."""
        nodes = np.asarray(nodes, dtype=float)
        assert nodes.ndim == 2 and nodes.shape[1] == self.kernel.dimension, \
            (" Incorrect dimension of input points fed to kernel ", nodes.shape)
        self._draw_fitcnodes(nodes)
        ctx = _dev.context()
        X = _dev.points(ctx, nodes)
        Model = _dev.VfeModel if self._vfe() else _dev.FitcModel
        return X, Model(ctx, self.kernel._spec(), X, _dev.points(ctx, self.fitcnodes), float(self.noise))

    def _vfe(self):
        return self.FITC is not None and self.sparse == 'vfe'

    def _not_on_vfe(self, what):
        if self._vfe():
            raise NotImplementedError("%s is not offered on a VFE model (GP(..., sparse='vfe')): its objective is "
                                      "loglikeParams (the variational bound), its predictor evaluate(compvar=0/1) / "
                                      "evaluateVariance; the point derivatives of its variance are vfeVarianceGradient / "
                                      "vfeVarianceGradientWRTnewpt, IVAR design on it costFunctionVFE_IVAR" % what)

    def _draw_fitcnodes(self, nodes):
        """The inducing points, unless set already: a random subset of the nodes (gp.py:186-189)."""
        if self.fitcnodes is None:
            nNodes = len(nodes)
            nu = int(np.floor(nNodes * self.FITC))
            indu = np.random.permutation(nNodes)[0:nu]
            self.fitcnodes = np.array(nodes[indu], dtype=float)

    def addNodesAndComputeCovariance(self, nodes, noiseIn=None):
        """Set the training locations and factor their covariance (no function values needed)."""
        if self.FITC is not None:
            if noiseIn is not None:
                print("NOT IMPLEMENTED YET")  # gp.py:208-209: per-point noise with FITC leaves the old state in place
            else:
                self._X, self._fitc = self._fitc_model(nodes)
                self._L = None
                self._nugget = self.noise
                self._K_host = None
                self._P_host = None
            self.pts = np.array(nodes, dtype=float, copy=True)
            return
        nugget = self.noise if noiseIn is None else noiseIn
        self._X, self._L, self.jitter = self._factor(nodes, nugget)
        self._nugget = nugget
        self._K_host = None
        self._P_host = None
        self.pts = np.array(nodes, dtype=float, copy=True)

    def train(self, pts, evalsIn, noiseIn=None):
        """Compute the GP coefficients K^-1 (y - prior mean); stored in `coeff`."""
        assert len(evalsIn.shape) == 1, "evaluations must be an (N,) array for training GP"
        evals = evalsIn - self.gpPriorMean(pts)
        self.addNodesAndComputeCovariance(pts, noiseIn)
        self.fVals = evals.copy()
        if self._fitc is not None:
            self.coeff = self._fitc.solve(evals)[0]
            return
        if self._Lc is not None:
            self.coeff = self._Lc.solve(evals)[0]          # distributed substitution on the block-cyclic factor
        else:
            self.coeff = _dev.potrs(_dev.context(), self._L, evals)

    # ---- prediction ---------------------------------------------------------------------------------------------
    def evaluate(self, newpt, compvar=0):
        """Posterior mean at `newpt`; compvar=1 also |variance| (gp.py:145), compvar=2 the full covariance."""
        assert newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        if compvar == 2:
            self._not_on_vfe("evaluate(compvar=2), the full posterior covariance,")
        ctx = _dev.context()
        spec = self.kernel._spec()
        Z = _dev.points(ctx, newpt)
        if self._fitc is not None:
            mean, var = self._fitc.posterior(self.coeff, Z, want_mean=True, want_var=(compvar == 1))
            out = mean + self.gpPriorMean(newpt)
            if compvar == 1:
                return out, np.abs(var)
            elif compvar == 2:  # dense by definition (gp.py:146-152); built from the materialised precision
                kv = _dev.kfill(ctx, spec, Z, Z=self._X).to_host()
                return out, _dev.kfill(ctx, spec, Z, Z=Z).to_host() - kv @ (self.precisionMatrix @ kv.T)
            return out
        sess = _dist.session()
        if sess is not None and (self._Lc is not None or sess.use_eval(newpt.shape[0])):
            # evaluation points sharded over the ranks, mean and variance gathered on every rank (the role of
            # parallelizeMcForLoop, parallel_utilities.py:26-80)
            mean, var = sess.posterior(spec, self._Lc or self._L, self._X, self.coeff, newpt, want_mean=True,
                                       want_var=(compvar == 1))
        else:
            mean, var = _dev.posterior(ctx, spec, self._L, self._X, self.coeff, Z, want_mean=True,
                                       want_var=(compvar == 1))
        out = mean + self.gpPriorMean(newpt)
        if compvar == 1:
            return out, np.abs(var)
        elif compvar == 2:
            return out, _dev.posterior_cov(ctx, spec, self._L, self._X, Z)
        return out

    def evaluateVariance(self, newpt, parallel=1):
        """Signed posterior variance at `newpt` (gp.py:213-259).  `parallel` is accepted and ignored: the
        reference forks CPU processes above 500001 points (gp.py:244-258); here the parallel branch is the multi-process
        launch itself -- one process per GPU, evaluation points sharded, the variance vector gathered on every rank."""
        assert self.pts is not None
        assert newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        ctx = _dev.context()
        if self._fitc is not None:
            return self._fitc.posterior(None, _dev.points(ctx, newpt), want_mean=False, want_var=True)[1]
        sess = _dist.session()
        if sess is not None and (self._Lc is not None or sess.use_eval(newpt.shape[0])):   # gp.py:244-258: the reference's parallel branch
            return sess.posterior(self.kernel._spec(), self._Lc or self._L, self._X, None, newpt, want_mean=False,
                                  want_var=True)[1]
        _, var = _dev.posterior(ctx, self.kernel._spec(), self._L, self._X, None, _dev.points(ctx, newpt),
                                want_mean=False, want_var=True)
        return var

    # ---- variance gradients w.r.t. point locations, on the device ---------------------------------------
    def _point_derivative_ready(self, newpt, referenceOnly=True):
        """Shape checks and the kernel gate of the point-derivative routines.  `referenceOnly` (the reference-named methods):
        only the kernels whose `derivative` the reference defines; False (varianceGradient / varianceGradientWRTnewpt, the
        IVAR gradient): also the kernels with a `pointDerivative` -- the isotropic Matern kernels."""
        self._not_on_vfe("the point derivative of the posterior variance (evaluateVarianceDerivative, evaluateVarianceDerivWRTnewpt, "
                         "varianceGradient*, costFunctionGP_IVAR.derivative)")
        assert self.pts is not None, "must specify training points before running this"
        assert newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        if not self._has_factor() and self._fitc is None:
            raise NotImplementedError("variance derivatives need a fitted model")
        if not referenceOnly and hasattr(self.kernel, "pointDerivative"):
            return
        if not hasattr(self.kernel, "derivative") or (self.kernel._spec().kind == _dev.K_MEHLER
                                                      and self.kernel.dimension != 1):
            # the reference defines Kernel.derivative for the squared exponential and the 1-D Mehler kernel only
            raise AttributeError("derivative of %s not implemented" % type(self.kernel).__name__)

    def evaluateVarianceDerivWRTnewpt(self, newpt):
        """d var(newpt_i) / d newpt_i, flattened (gp.py:261-280): gpx_var_grad_newpt."""
        self._point_derivative_ready(newpt)
        return self._var_grad_newpt(newpt)

    def _var_grad_newpt(self, newpt):
        ctx = _dev.context()
        if self._fitc is not None:    # the reference reads `precisionMatrix`: for FITC the Woodbury precision (gp.py:204-206)
            return self._fitc.var_grad_newpt(self.kernel._spec(), _dev.points(ctx, newpt))
        return _dev.var_grad_newpt(ctx, self.kernel._spec(), self._L, self._X, _dev.points(ctx, newpt))

    def evaluateVarianceDerivative(self, newpt, noiseFunc=None):
        """out[k*d+l, j] = d var(newpt_j) / d pts[k, l]  (gp.py:282-341): gpx_var_grad -- beta = K^-1 K(X,Z) by two
        triangular solves, one MFMA GEMM per coordinate, fused finish; the (N*d, M) result is the only thing that
        crosses to the host.  `noiseFunc` (callable with .deriv, demo2.py:45-58) adds its terms at coincident training
        points (gp.py:314-317) and, when the WHOLE evaluation set coincides with a training point, the terms of
        gp.py:318-320 (the reference tests `np.linalg.norm(p - newpt)`, a norm over all evaluation points)."""
        self._point_derivative_ready(newpt)
        return self._var_grad(newpt, noiseFunc)

    def _var_grad(self, newpt, noiseFunc):
        ctx = _dev.context()
        nd = eb = db = None
        if noiseFunc is not None:
            nd = np.asarray(noiseFunc.deriv(self.pts), dtype=float).reshape(self.pts.shape)
            spread = newpt - newpt[:1]
            if np.linalg.norm(spread) < 2e-10:       # otherwise no training point can be within 1e-10 of all of them
                hit = np.array([np.linalg.norm(self.pts[zz:zz + 1] - newpt) < 1e-10 for zz in range(len(self.pts))])
                if hit.any():
                    eb = np.where(hit, np.asarray(noiseFunc(self.pts), dtype=float), 0.0)
                    db = np.where(hit[:, None], nd, 0.0)
        if self._fitc is not None:
            return self._fitc.var_grad(self.kernel._spec(), _dev.points(ctx, newpt), nd, eb, db)
        return _dev.var_grad(ctx, self.kernel._spec(), self._L, self._X, _dev.points(ctx, newpt), nd, eb, db)

    def varianceGradient(self, newpt, noiseFunc=None):
        """out[k*d+l, j] = d var(newpt_j) / d pts[k, l], (N*d, M): evaluateVarianceDerivative -- same layout, same handling of
        `noiseFunc`, dense and FITC models -- for every kernel with a point derivative.  Squared exponential and 1-D Mehler:
        exactly what evaluateVarianceDerivative returns, i.e. the REFERENCE's convention, including the squared
        exponential's doubled signalSize (kernels.py:177).  Isotropic Matern (nu = 3/2, 5/2; KernelIsoMatern.pointDerivative),
        which the reference does not differentiate: the true gradient.  KernelMehlerND with d > 1 raises AttributeError."""
        self._point_derivative_ready(newpt, referenceOnly=False)
        return self._var_grad(newpt, noiseFunc)

    def varianceGradientWRTnewpt(self, newpt):
        """d var(newpt_i) / d newpt_i, flattened (M*d,): evaluateVarianceDerivWRTnewpt for every kernel with a point derivative,
        with the conventions of varianceGradient (reference's for squared exponential / 1-D Mehler, true for Matern)."""
        self._point_derivative_ready(newpt, referenceOnly=False)
        return self._var_grad_newpt(newpt)

    # ---- the same two derivatives on a VFE model: of the variational variance, inducing points held fixed ------------------------
    def _vfe_point_derivative_ready(self, name, newpt):
        if not self._vfe():
            raise ValueError("%s is the point derivative of the variational variance of VFE models (GP(..., FITC=fraction, "
                             "sparse='vfe')); on a dense or FITC model use varianceGradient / varianceGradientWRTnewpt" % name)
        if self.kernel._spec().kind == _dev.K_MEHLER:
            raise NotImplementedError("%s: %s has no point derivative here (squared exponential and isotropic Matern only)"
                                      % (name, type(self.kernel).__name__))
        if self.pts is None or self._fitc is None:
            raise NotImplementedError("%s needs a fitted model: set the nodes first (addNodesAndComputeCovariance / train)" % name)
        assert newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"

    def vfeVarianceGradient(self, newpt):
        """out[k*d+l, j] = d var(newpt_j) / d pts[k, l], (N*d, M) in evaluateVarianceDerivative's layout, of the variational
        posterior variance `evaluateVariance` returns on a VFE model (gpx_vfe_var_grad).  TRUE derivatives for every kernel -- no
        doubled signalSize for the squared exponential -- with `fitcnodes` held fixed, also where a node coincides with one.
        ValueError on a dense or FITC model, NotImplementedError for a Mehler kernel or before any nodes are set."""
        self._vfe_point_derivative_ready("vfeVarianceGradient", newpt)
        ctx = _dev.context()
        return self._fitc.design_var_grad(self.kernel._spec(), self._fitc.X, self._fitc.S, _dev.points(ctx, newpt))

    def vfeVarianceGradientWRTnewpt(self, newpt):
        """d var(newpt_i) / d newpt_i, flattened (M*d,), of the variational posterior variance (gpx_vfe_var_grad_newpt): TRUE
        derivatives, `fitcnodes` held fixed.  Errors as vfeVarianceGradient."""
        self._vfe_point_derivative_ready("vfeVarianceGradientWRTnewpt", newpt)
        ctx = _dev.context()
        return self._fitc.design_var_grad_newpt(self._fitc.S, _dev.points(ctx, newpt))

    def generateSamples(self, x, noise=1e-10):
        raise NotImplementedError("generateSamples (SVD sampling, gp.py:343-371) is outside the GPU hot path")

    # ---- joint samples (none of these touches generateSamples) ---------------------------------------------------------------
    def _sampling_ready(self, name, fitted=True):
        if self.FITC is not None:
            raise NotImplementedError("%s needs the dense Cholesky factor: there is no sampler for FITC / VFE models" % name)
        if fitted and (not self._has_factor() or self.coeff is None):
            raise NotImplementedError("%s needs a trained model: call train first" % name)

    def _jitter(self, ctx, spec, Z, jitter, name):
        """The nugget of a sampler: `jitter`, or 1e-10 * max k(z, z) over the evaluation points (gpx_kdiag)."""
        if jitter is None:
            return 1e-10 * float(np.max(_dev.kdiag(ctx, spec, Z)))
        jitter = float(jitter)
        if not (jitter >= 0.0 and np.isfinite(jitter)):
            raise ValueError("%s: jitter must be a finite number >= 0, not %r" % (name, jitter))
        return jitter

    def posteriorSampler(self, newpt, jitter=None, addNoise=False):
        """A sampler of the JOINT posterior of the latent function at the M rows of `newpt` (gpx_psampler_*): the posterior mean
        and F = chol(C + nugget I) stay on the device, C the full posterior covariance (evaluate(compvar=2)).  nugget = `jitter`,
        by default 1e-10 * max k(z, z); `addNoise` adds the model's scalar noise to it: samples of OBSERVATIONS.  No pivot is
        dropped: NotPositiveDefinite names the point when the nugget is too small (exact duplicates with jitter=0).  Returns an
        object with
            draw(nSamples=1, baseSamples=None)                        (S, M): row s = mean + F baseSamples[s]
            argbest(nSamples=1, baseSamples=None, minimize=True, returnSamples=False)
                                                                      (indices (S,) int64, values (S,)[, samples (S, M)]): per
                                                                      draw the first index of its minimum / maximum
            close()
        The device makes no random numbers: `baseSamples` (S, M) are the standard-normal base samples, drawn with
        np.random.standard_normal when None -- the same base samples give the same bits.  Dense models only (a VFE model has
        vfePosteriorSampler); under a multi-process
        session the calls run replicated, and baseSamples=None raises ValueError there (every rank would draw its own)."""
        self._sampling_ready("posteriorSampler")
        newpt = np.asarray(newpt, dtype=float)
        assert newpt.ndim == 2 and newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        ctx = _dev.context()
        spec = self.kernel._spec()
        Z = _dev.points(ctx, newpt)
        nugget = self._jitter(ctx, spec, Z, jitter, "posteriorSampler")
        if addNoise:
            if np.ndim(self.noise) != 0:
                raise NotImplementedError("posteriorSampler(addNoise=True) needs a scalar noise")
            nugget += float(self.noise)
        return JointSampler(_dev.PosteriorSampler(ctx, spec, self._L, self._X, self.coeff, Z, nugget), newpt.shape[0])

    def samplePosterior(self, newpt, nSamples=1, baseSamples=None, jitter=None):
        """(nSamples, M) joint posterior samples at `newpt`: posteriorSampler(newpt, jitter).draw(nSamples, baseSamples)."""
        smp = self.posteriorSampler(newpt, jitter=jitter)
        try:
            return smp.draw(nSamples, baseSamples)
        finally:
            smp.close()

    def samplePrior(self, x, nSamples=1, noise=1e-10, baseSamples=None):
        """(nSamples, M) joint samples of the PRIOR at the rows of `x` -- what the reference's generateSamples(x, noise) draws
        (gp.py:343-371), with no training set: a zero-mean normal vector of covariance K(x, x) + noise I.  The reference adds two
        independent terms, sqrt(K) z1 by an SVD and sqrt(noise) z2; here the noise is the nugget of one factorisation,
        chol(K + noise I): the same distribution from ONE base vector per sample (`baseSamples`, (nSamples, M))."""
        self._sampling_ready("samplePrior", fitted=False)
        x = np.asarray(x, dtype=float)
        assert x.ndim == 2 and x.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        ctx = _dev.context()
        spec = self.kernel._spec()
        Z = _dev.points(ctx, x)
        nugget = self._jitter(ctx, spec, Z, 0.0 if noise is None else noise, "samplePrior")
        smp = JointSampler(_dev.PosteriorSampler(ctx, spec, None, None, None, Z, nugget), x.shape[0])
        try:
            return smp.draw(nSamples, baseSamples)
        finally:
            smp.close()

    # ---- pathwise samples (Matheron's rule) ---------------------------------------------------------------------------------------
    def _pathBase(self, name, nPaths, nFeatures, base, nTrain):
        spec = self.kernel._spec()
        if spec.kind == _dev.K_MEHLER:
            raise NotImplementedError("%s: %s has no spectral density here (squared exponential and isotropic Matern only)"
                                      % (name, type(self.kernel).__name__))
        d = self.kernel.dimension
        if base is None:
            if _dist.session() is not None:
                raise ValueError("%s: under a multi-process session base must be given (the call runs replicated and every rank "
                                 "would draw its own)" % name)
            return PathBase.draw(nPaths, nFeatures, nTrain, d, spec)
        if not isinstance(base, PathBase):
            raise ValueError("%s: base must be a PathBase (PathBase.draw), not %r" % (name, type(base).__name__))
        if base.dimension != d or base.nTrain != nTrain or (base.u is None) != (spec.kind == _dev.K_SE):
            raise ValueError("%s: base was drawn for d = %d, %d training points and a %s kernel; the model has d = %d, %d points"
                             % (name, base.dimension, base.nTrain, "squared-exponential" if base.u is None else "Matern", d, nTrain))
        return base

    def pathSampler(self, nPaths=1, nFeatures=1024, base=None):
        """`nPaths` PATHS of the posterior of the latent function (gpx_paths_*; Matheron's rule, Wilson et al. 2020): each draw is
        a function, a random-Fourier-feature draw of the prior (`nFeatures` features) plus a kernel-basis update solved once
        against the resident factor, so it can be evaluated at ANY number of points afterwards (chunked under GPX_CROSS_BYTES; no
        M x M factor) and differentiated.  Returns an object with
            evaluate(newpt)                                          (S, M)
            argbest(newpt, minimize=True, returnValues=False)        (indices (S,) int64, values (S,)[, values (S, M)])
            gradient(points, pathIndex)                              (P, d): row p = gradient of path pathIndex[p] at points[p]
            base                                                     the PathBase used
            close()
        The device makes no random numbers: `base` (PathBase.draw(nPaths, nFeatures, N, d, kernel, rng)) holds every draw, made
        with NumPy when None -- the same base gives the same bits.  These are NOT exact posterior samples: with finitely many
        features the prior part has covariance Phi Phi^T instead of K (the mean is exact, the covariance tends to the posterior's as
        nFeatures grows); posteriorSampler stays the exact one.  Stationary kernels, dense models and scalar noise only
        (NotImplementedError; a VFE model has vfePathSampler); under a multi-process session the calls run replicated, and base=None raises ValueError there."""
        self._sampling_ready("pathSampler")
        if np.ndim(self.noise) != 0:
            raise NotImplementedError("pathSampler needs a scalar noise: there is no pathwise sampler for per-point noise")
        n = self.pts.shape[0]
        base = self._pathBase("pathSampler", nPaths, nFeatures, base, n)
        ctx = _dev.context()
        spec = self.kernel._spec()
        eps = np.sqrt(float(self.noise)) * base.xi
        state = _dev.PathSampler(ctx, spec, self._L, self._X, self.coeff, _spectralFrequencies(spec, base.g, base.u), base.phase,
                                 base.w, eps)
        return PathSampler(state, base, self.kernel.dimension)

    def samplePaths(self, newpt, nPaths=1, nFeatures=1024, base=None):
        """(nPaths, M) pathwise posterior samples at `newpt`: pathSampler(nPaths, nFeatures, base).evaluate(newpt)."""
        smp = self.pathSampler(nPaths, nFeatures, base)
        try:
            return smp.evaluate(newpt)
        finally:
            smp.close()

    def priorPathSampler(self, nPaths=1, nFeatures=1024, base=None):
        """Paths of the PRIOR (no training set, no update: V = 0) -- the pathwise counterpart of samplePrior, same object as
        pathSampler returns.  `base`: PathBase.draw(nPaths, nFeatures, 0, d, kernel, rng)."""
        self._sampling_ready("priorPathSampler", fitted=False)
        base = self._pathBase("priorPathSampler", nPaths, nFeatures, base, 0)
        ctx = _dev.context()
        spec = self.kernel._spec()
        state = _dev.PathSampler(ctx, spec, None, None, None, _spectralFrequencies(spec, base.g, base.u), base.phase, base.w, None)
        return PathSampler(state, base, self.kernel.dimension)

    # ---- the same samplers on a VFE model: of the optimal variational posterior, in the inducing space -----------------------------
    def _vfe_sampling_ready(self, name, denseName):
        if not self._vfe():
            raise ValueError("%s samples the variational posterior of VFE models (GP(..., FITC=fraction, sparse='vfe')); on a dense "
                             "model use %s; there is no sampler for FITC models" % (name, denseName))
        if self.pts is None or self._fitc is None or self.coeff is None:
            raise ValueError("%s needs a trained model: call train first" % name)

    def vfePathSampler(self, nPaths=1, nFeatures=1024, base=None):
        """pathSampler on a VFE model (gpx_vfe_paths_create; decoupled sampling, Wilson et al. 2020): `nPaths` paths of the optimal
        variational posterior, f_s(z) = sum_j c_sj cos(omega_j . z + b_j) + sum_u v_su k(s_u, z) over the nu inducing points with
            V = 1 beta_u^T - (f~(S) + sqrt(noise) Xi1) Quu^-1 + Xi2 La^-1,
        Xi1 the nugget draw of the inducing variables u = f(S) + eps and Xi2 the draw of q(u).  A path costs O(nFeatures + nu) per
        point, whatever the training-set size, and the build two nu-order solves for all paths at once.  Returns the object
        pathSampler returns (evaluate, argbest, gradient, base, close).  `base`: a PathBase drawn with nTrain = 2 nu
        (PathBase.draw(nPaths, nFeatures, 2 * nu, d, kernel, rng)): xi[:, :nu] is Xi1 and xi[:, nu:] is Xi2; drawn with NumPy when
        None -- the same base gives the same bits.  Zero draws give evaluate's mean; as nFeatures grows the covariance tends to
        vfePosteriorCovariance's (vfePosteriorSampler is the exact sampler).  ValueError on a dense or FITC model and before train;
        NotImplementedError for a Mehler kernel; under a multi-process session the calls run replicated, and base=None raises
        ValueError there."""
        self._vfe_sampling_ready("vfePathSampler", "pathSampler")
        nu = self.fitcnodes.shape[0]
        base = self._pathBase("vfePathSampler", nPaths, nFeatures, base, 2 * nu)
        spec = self.kernel._spec()
        state = self._fitc.path_sampler(self._fitc.S, self.coeff, _spectralFrequencies(spec, base.g, base.u), base.phase, base.w,
                                        np.sqrt(float(self.noise)) * base.xi[:, :nu], base.xi[:, nu:])
        return PathSampler(state, base, self.kernel.dimension)

    def vfeSamplePaths(self, newpt, nPaths=1, nFeatures=1024, base=None):
        """(nPaths, M) pathwise samples of the variational posterior at `newpt`: vfePathSampler(...).evaluate(newpt)."""
        smp = self.vfePathSampler(nPaths, nFeatures, base)
        try:
            return smp.evaluate(newpt)
        finally:
            smp.close()

    def _vfe_points(self, newpt):
        newpt = np.asarray(newpt, dtype=float)
        assert newpt.ndim == 2 and newpt.shape[1] == self.kernel.dimension, "evaluation points for GP is incorrect shape"
        return newpt, _dev.points(_dev.context(), newpt)

    def vfePosteriorCovariance(self, newpt):
        """(M, M): the full covariance of the variational posterior of the latent function at `newpt` (gpx_vfe_posterior_cov),
        k(z,z') - k_u^T Quu^-1 k_u' + k_u^T A^-1 k_u' -- what evaluate(compvar=2) is on a dense model; its diagonal is
        evaluateVariance.  Every kernel.  ValueError on a dense or FITC model and before train."""
        self._vfe_sampling_ready("vfePosteriorCovariance", "evaluate(compvar=2)")
        return self._fitc.posterior_cov(self._vfe_points(newpt)[1])

    def vfePosteriorSampler(self, newpt, jitter=None, addNoise=False):
        """posteriorSampler on a VFE model (gpx_vfe_psampler_create): the EXACT joint sampler of the variational posterior at the M
        rows of `newpt` -- evaluate's mean and F = chol(vfePosteriorCovariance + nugget I) stay on the device.  The nugget, its
        default (1e-10 * max k(z, z)), `addNoise`, NotPositiveDefinite and the object returned (draw, argbest, close) are
        posteriorSampler's.  Every kernel.  ValueError on a dense or FITC model and before train."""
        self._vfe_sampling_ready("vfePosteriorSampler", "posteriorSampler")
        newpt, Z = self._vfe_points(newpt)
        nugget = self._jitter(_dev.context(), self.kernel._spec(), Z, jitter, "vfePosteriorSampler")
        if addNoise:
            nugget += float(self.noise)
        return JointSampler(self._fitc.posterior_sampler(self.coeff, Z, nugget), newpt.shape[0])

    def vfeSamplePosterior(self, newpt, nSamples=1, baseSamples=None, jitter=None):
        """(nSamples, M) joint samples of the variational posterior at `newpt`: vfePosteriorSampler(newpt, jitter).draw(...)."""
        smp = self.vfePosteriorSampler(newpt, jitter=jitter)
        try:
            return smp.draw(nSamples, baseSamples)
        finally:
            smp.close()

    # ---- marginal likelihood -------------------------------------------------------------------------------------
    def computeLogLike(self, pts, evals):
        """Log marginal likelihood of (pts, evals) under the current hyper-parameters."""
        return self.loglikeParams(pts, evals)

    def loglikeParams(self, pts, evals, returnDeriv=0, noiseIn=None, inducingDeriv=False):
        """-1/2 y^T K^-1 y - 1/2 log det K - N/2 log 2 pi  [, {key: d/d key}] (gp.py:394-468).

        Does not touch the trained state.  `noiseIn` (per-point nugget) works here; in the reference that branch
        passes an unknown keyword and raises TypeError (gp.py:429-430).

        `inducingDeriv=True` (FITC models, with returnDeriv=1): the dict gains the key 'fitcnodes' after 'noise', the (nu, d)
        TRUE derivative of the value w.r.t. the inducing-point locations `self.fitcnodes` (gpx_fitc_lml_grad_inducing, the same
        call that gives the other entries).  ValueError on a dense model, with a per-point `noiseIn` or with returnDeriv=0.

        On a VFE model (sparse="vfe") the value is Titsias' lower bound F on the log marginal likelihood (gpx_vfe_bound) and the
        dict, with the same keys and conventions, its derivatives (gpx_vfe_grad); `noiseIn` raises NotImplementedError."""
        evals = np.asarray(evals, dtype=float)
        if inducingDeriv and (self.FITC is None or noiseIn is not None or returnDeriv != 1):
            raise ValueError("loglikeParams: inducingDeriv=True needs a FITC model without noiseIn (the dense likelihood has no "
                             "inducing points) and returnDeriv=1")
        if noiseIn is not None:
            self._not_on_vfe("per-point noise (noiseIn)")
        if self.FITC is not None and noiseIn is None:
            spec = self.kernel._spec()
            if returnDeriv == 1 and spec.kind == _dev.K_MEHLER:
                raise NotImplementedError("no hyper-parameter gradient of the %s for %s (squared exponential "
                                          "and isotropic Matern kernels only)"
                                          % ("VFE bound" if self._vfe() else "FITC likelihood", type(self.kernel).__name__))
            _, model = self._fitc_model(pts)
            if self._vfe():
                # gpx_vfe_bound / gpx_vfe_grad: the variational lower bound F and its TRUE derivatives, 'noise' scaled as below
                if returnDeriv != 1:
                    return model.bound(evals)
                keys = list(self.kernel.hyperParam.keys()) + ['noise']
                res = model.grad(spec, evals, want_inducing=bool(inducingDeriv))
                outD = dict(zip(keys, res[1]))
                outD['noise'] *= self.noise * 2.0
                if inducingDeriv:
                    outD['fitcnodes'] = res[2]
                return res[0], outD
            quad = model.solve(evals)[1]
            out = -0.5 * quad - 0.5 * model.logdet() - len(evals) / 2.0 * np.log(2.0 * np.pi)
            if returnDeriv == 1:
                # gpx_fitc_lml_grad: a few nu x nu x N products on the fitted model, no N x N matrix; its entries are true
                # derivatives, 'noise' w.r.t. the noise variance -- scaled as in the dense branch below (gp.py:463-464)
                keys = list(self.kernel.hyperParam.keys()) + ['noise']
                res = model.lml_grad(spec, evals, want_value=False, want_inducing=bool(inducingDeriv))
                outD = dict(zip(keys, res[1]))   # the value: `out`, as without the gradient
                outD['noise'] *= self.noise * 2.0
                if inducingDeriv:
                    outD['fitcnodes'] = res[2]
                return out, outD
            return out
        nugget = self.noise if noiseIn is None else noiseIn
        X, L, _ = self._factor(pts, nugget, remember=False)
        ctx = _dev.context()
        if getattr(L, "is_cyclic", False):
            alpha, logdet = L.solve(evals)                 # distributed substitution; a dense factor only for the gradient
            if returnDeriv == 1:
                L = L.dense()
        else:
            alpha = _dev.potrs(ctx, L, evals)
            logdet = _dev.logdet(ctx, L)
        out = -0.5 * _hdot(evals, alpha) - 0.5 * logdet - len(evals) / 2.0 * np.log(2.0 * np.pi)
        if returnDeriv == 1:
            keys = list(self.kernel.hyperParam.keys()) + ['noise']
            sess = _dist.session()
            if sess is not None and sess.use_fit(len(evals)):     # traces sharded by row slabs of K^-1 (dist_lml_grad)
                grad = sess.lml_grad(self.kernel._spec(), L, X, alpha)
            else:
                grad = _dev.lml_grad(ctx, self.kernel._spec(), L, X, alpha)
            outD = dict(zip(keys, grad))
            outD['noise'] *= self.noise * 2.0  # gp.py:463-464
            return out, outD
        return out

    # ---- leave-one-out cross-validation (Rasmussen & Williams 5.4.2; absent in the reference) --------------------------
    def _loo_factor(self, pts, noiseIn):
        """Factor of K(pts) + nugget under the current hyper-parameters for the leave-one-out calls -> (X, L, nugget).  As
        loglikeParams: the trained state is not touched, and right after `train` on the same points the kept factor is
        reused.  Under a multi-process session every rank runs the same single-GPU call (a block-cyclic factor is made dense
        first)."""
        self._not_on_vfe("looPredict / looLogLike (leave-one-out)")
        if self.FITC is not None:
            raise NotImplementedError("looPredict / looLogLike need the dense factor; on a FITC model call fitcLooPredict / "
                                      "fitcLooLogLike (leave-one-out under the model's own covariance Q + G)")
        nugget = self.noise if noiseIn is None else noiseIn
        X, L, _ = self._factor(pts, nugget, remember=False)
        if self.dropped > 0:
            raise ValueError("leave-one-out cross-validation is undefined here: the factorisation dropped %d point(s) whose "
                             "conditional variance is at round-off level (duplicated points at zero noise)" % self.dropped)
        if getattr(L, "is_cyclic", False):
            L = L.dense()
        return X, L, nugget

    def looPredict(self, pts, evals, noiseIn=None):
        """Leave-one-out predictions under the current hyper-parameters, without refits: (mean (N,), var (N,)) with
        mean_i, var_i the predictive distribution of the OBSERVATION evals_i given all the other points (the noise of point i is
        included): mean_i = y_i - alpha_i / P_ii, var_i = 1 / P_ii, P = K^-1, alpha = P y (gpx_loo).  Standardised residuals
        (evals - mean) / sqrt(var) check a fit before a design trusts it.  Every kernel; does not touch the trained state."""
        evals = np.asarray(evals, dtype=float)
        assert len(evals.shape) == 1, "evaluations must be an (N,) array"
        _, L, _ = self._loo_factor(pts, noiseIn)
        y = evals - self.gpPriorMean(pts)
        mean, var, _ = _dev.loo(_dev.context(), L, y)
        return mean + self.gpPriorMean(pts), var

    def looLogLike(self, pts, evals, returnDeriv=0, noiseIn=None):
        """Leave-one-out log predictive probability sum_i log p(y_i | y_-i)  [, {key: d/d key}] -- a model-selection objective
        beside the marginal likelihood, more robust when the kernel family is wrong.

        The dict has the keys of loglikeParams (`kernel.hyperParam` keys + 'noise'); its entries are the TRUE derivatives.
        In particular 'noise' is the derivative with respect to the noise VARIANCE (a common shift of every nugget), WITHOUT
        the reference's factor 2 * noise that loglikeParams carries (gp.py:463-464).  Gradient: squared exponential and
        isotropic Matern kernels (gpx_loo_grad).  Does not touch the trained state."""
        evals = np.asarray(evals, dtype=float)
        assert len(evals.shape) == 1, "evaluations must be an (N,) array"
        X, L, nugget = self._loo_factor(pts, noiseIn)
        y = evals - self.gpPriorMean(pts)
        ctx = _dev.context()
        if returnDeriv == 1:
            out, grad = _dev.loo_grad(ctx, self.kernel._spec(), L, X, nugget, y)
            keys = list(self.kernel.hyperParam.keys()) + ['noise']
            return out, dict(zip(keys, grad))
        return _dev.loo(ctx, L, y, want_pred=False)[2]

    # ---- leave-one-out for FITC models: under the model's own covariance Q + G, through nu x N matrices only -----------------
    def _fitc_loo_ready(self, name, dense_name):
        self._not_on_vfe("%s (leave-one-out)" % name)
        if self.FITC is None:
            raise ValueError("%s is the leave-one-out call of FITC models (GP(..., FITC=fraction)); on a dense model use %s"
                             % (name, dense_name))

    def fitcLooPredict(self, pts, evals):
        """Leave-one-out predictions of a FITC model under the current hyper-parameters, without refits: (mean (N,), var (N,)).

        The model's prior covariance of the observations is Kt = Q + G -- the matrix `loglikeParams` scores on a FITC model --
        and leave-one-out is taken UNDER THAT MODEL: mean_i, var_i are the Gaussian conditional of N(0, Kt) for the OBSERVATION
        evals_i given all the others, mean_i = y_i - alpha_i / P_ii, var_i = 1 / P_ii with the Woodbury precision P and
        alpha = P y (gpx_fitc_loo).  That equals refitting FITC on the points without x_i, with the same inducing points, and
        predicting y_i through the model's own cross-covariance Q.  It is NOT what `evaluate` returns at x_i after training
        without x_i: `evaluate` keeps the reference's convention, the true k(z, X) against P.

        Inducing points as in `loglikeParams`: drawn once, then kept in `fitcnodes`.  Every kernel; no `noiseIn` (per-point
        noise with FITC is not offered); does not touch the trained state.  O(nu^2 N), nothing N x N.  Under a multi-process
        session every rank runs the same single-GPU call, like the rest of FITC."""
        self._fitc_loo_ready("fitcLooPredict", "looPredict")
        evals = np.asarray(evals, dtype=float)
        assert len(evals.shape) == 1, "evaluations must be an (N,) array"
        _, model = self._fitc_model(pts)
        mean, var, _ = model.loo(evals - self.gpPriorMean(pts))
        return mean + self.gpPriorMean(pts), var

    def fitcLooLogLike(self, pts, evals, returnDeriv=0):
        """Leave-one-out log predictive probability sum_i log p(y_i | y_-i) of a FITC model  [, {key: d/d key}], with
        p(y_i | y_-i) as in `fitcLooPredict` (under the model's own covariance Q + G, not `evaluate`'s convention).

        The dict has the keys of loglikeParams (`kernel.hyperParam` keys + 'noise'); every entry is a TRUE derivative, 'noise'
        with respect to the noise VARIANCE, exactly as looLogLike's (no factor 2 * noise).  Gradient: squared exponential and
        isotropic Matern kernels (gpx_fitc_loo_grad: about twice the cost of the FITC likelihood gradient, O(nu^2 N), nothing
        N x N).  Inducing points as in `loglikeParams`; no `noiseIn`; does not touch the trained state."""
        self._fitc_loo_ready("fitcLooLogLike", "looLogLike")
        spec = self.kernel._spec()
        if returnDeriv == 1 and spec.kind == _dev.K_MEHLER:
            raise NotImplementedError("no hyper-parameter gradient of the FITC leave-one-out objective for %s (squared "
                                      "exponential and isotropic Matern kernels only)" % type(self.kernel).__name__)
        evals = np.asarray(evals, dtype=float)
        assert len(evals.shape) == 1, "evaluations must be an (N,) array"
        _, model = self._fitc_model(pts)
        y = evals - self.gpPriorMean(pts)
        if returnDeriv == 1:
            out, grad = model.loo_grad(spec, y)
            keys = list(self.kernel.hyperParam.keys()) + ['noise']
            return out, dict(zip(keys, grad))
        return model.loo(y, want_pred=False)[2]

    def getHypParamNames(self):
        return self.kernel.hyperParam.keys()

    def updateKernelParams(self, paramsIn):
        """Set new hyper-parameters; a 'noise' entry goes to `self.noise`, the rest to the kernel."""
        params = copy.copy(paramsIn)
        if 'noise' in params.keys():
            self.noise = copy.copy(params['noise'])
            del params['noise']
        self.kernel.updateHyperParameters(params)

    # ---- hyper-parameter fit: host driver around loglikeParams -----------------------------------
    def findOptParamsLogLike(self, pts, evals, paramsStart=None, paramLowerBounds=None, paramUpperBounds=None,
                             useNoise=None, maxiter=40, useLastParams=True, analyticGradient=False, objective="lml",
                             optimizeInducing=False, inducingBounds=None):
        """Maximise the marginal likelihood over the kernel hyper-parameters (+ noise unless `useNoise` is given);
        bounds default to [max(v/10, 1e-3), min(10 v, 10)], noise to [1e-12, 1] from 1e-5 (gp.py:498-590).

        `objective="loo"` maximises the leave-one-out log predictive probability instead (looLogLike; on a FITC model
        fitcLooLogLike, leave-one-out under the model's own covariance); with `analyticGradient=True` L-BFGS-B gets its
        gradient from gpx_loo_grad (FITC: gpx_fitc_loo_grad), whose 'noise' entry already is the derivative w.r.t. the noise
        variance.  Any other string raises ValueError.

        `analyticGradient=True` (opt-in; squared-exponential and isotropic Matern kernels) hands L-BFGS-B the
        gradient from gpx_lml_grad -- on a FITC model from gpx_fitc_lml_grad -- instead of letting it difference the objective
        (gp.py:635, approx_grad=True): one factorisation (one FITC fit) per iterate instead of nparams+1.  The default
        reproduces the reference's numerical-gradient search.

        `optimizeInducing=True` (FITC models; needs analyticGradient=True and objective="lml") fits the inducing-point
        LOCATIONS with the hyper-parameters, as Snelson & Ghahramani's pseudo-inputs: L-BFGS-B searches [hyper-parameters...,
        noise (unless useNoise), vec(S)] jointly, one gpx_fitc_fit and one gpx_fitc_lml_grad_inducing per iterate.  S starts
        at `self.fitcnodes` (drawn as usual if None) and stays inside `inducingBounds` = (lower (d,), upper (d,)), default the
        bounding box of `pts`.  On return `self.fitcnodes` holds the optimised points; the returned dict has no entry for
        them.

        On a VFE model (sparse="vfe") the objective is the variational bound, the one to trust with `optimizeInducing=True`: it
        never rewards piled-up inducing points or a collapsing noise.  objective="loo" raises NotImplementedError there."""
        if objective not in ("lml", "loo"):
            raise ValueError("findOptParamsLogLike: objective must be 'lml' or 'loo', not %r" % (objective,))
        if objective == "loo":
            self._not_on_vfe("objective='loo'")
        if optimizeInducing:
            if self.FITC is None:
                raise ValueError("findOptParamsLogLike: optimizeInducing=True needs a FITC model (GP(..., FITC=fraction))")
            if not analyticGradient:
                raise ValueError("findOptParamsLogLike: optimizeInducing=True needs analyticGradient=True (nu * d numerical "
                                 "differences per iterate are not offered)")
            if objective != "lml":
                raise ValueError("findOptParamsLogLike: optimizeInducing=True needs objective='lml' (the leave-one-out "
                                 "objective has no gradient w.r.t. the inducing-point locations yet)")
        if paramsStart is None:
            paramsStart = copy.deepcopy(self.kernel.hyperParam)
        if paramLowerBounds is None:
            paramLowerBounds = dict((k, np.max([v / 10.0, 1e-3])) for k, v in paramsStart.items())
        if paramUpperBounds is None:
            paramUpperBounds = dict((k, np.min([v * 10.0, 10.0])) for k, v in paramsStart.items())
        keys = list(paramsStart.keys())
        vals = [paramsStart[k] for k in keys]
        lbs = [paramLowerBounds[k] for k in keys]
        ubs = [paramUpperBounds[k] for k in keys]
        if useNoise is None:  # last key is the noise
            keys.append('noise')
            lbs.append(1e-12)
            ubs.append(1e0)
            vals.append(1e-5)
        nhyp = len(keys)
        if optimizeInducing:
            ptsArr = np.asarray(pts, dtype=float)
            self._draw_fitcnodes(ptsArr)          # the subset the first likelihood call would draw
            shapeS = np.shape(self.fitcnodes)
            if inducingBounds is None:
                inducingBounds = (ptsArr.min(axis=0), ptsArr.max(axis=0))
            lo, hi = (np.broadcast_to(np.asarray(b, dtype=float), shapeS[1:]) for b in inducingBounds)
            vals = list(vals) + list(np.clip(np.asarray(self.fitcnodes, dtype=float), lo, hi).ravel())
            lbs = list(lbs) + list(np.tile(lo, shapeS[0]))
            ubs = list(ubs) + list(np.tile(hi, shapeS[0]))

        def objFunc(in0, gradIn):
            self.updateKernelParams(dict(zip(keys, in0[:nhyp])))
            if optimizeInducing:
                self.fitcnodes = np.array(in0[nhyp:], dtype=float).reshape(shapeS)
                if gradIn.size > 0:
                    margLogLike, derivs = self.loglikeParams(pts, evals, returnDeriv=1, inducingDeriv=True)
                    if 'noise' in keys:
                        derivs['noise'] /= 2.0 * self.noise     # as below: the search variable is the noise VARIANCE
                    gradIn[:nhyp] = -np.array([derivs[k] for k in keys])
                    gradIn[nhyp:] = -derivs['fitcnodes'].ravel()
                else:
                    margLogLike = self.loglikeParams(pts, evals, returnDeriv=0)
            elif objective == "loo":
                looLogLike = self.fitcLooLogLike if self.FITC is not None else self.looLogLike
                if gradIn.size > 0:
                    margLogLike, derivs = looLogLike(pts, evals, returnDeriv=1)
                    gradIn[:] = -np.array([derivs[k] for k in keys])
                else:
                    margLogLike = looLogLike(pts, evals, returnDeriv=0)
            elif gradIn.size > 0:
                margLogLike, derivs = self.loglikeParams(pts, evals, returnDeriv=1)
                if analyticGradient and 'noise' in derivs and 'noise' in keys:
                    # loglikeParams scales the noise entry by 2*noise (gp.py:463-464, a derivative w.r.t. sqrt(noise));
                    # the search variable is the noise VARIANCE, so the optimiser gets the unscaled trace term
                    derivs['noise'] /= 2.0 * self.noise
                gradIn[:] = -np.array([derivs[k] for k in keys])
            else:
                margLogLike = self.loglikeParams(pts, evals, returnDeriv=0)
            objFunc.last_x_value = in0.copy()
            objFunc.last_f_value = -margLogLike
            return -margLogLike

        paramsOut, optValue = self.chooseParams(lbs, ubs, vals, objFunc, maxiter=maxiter, useLastParams=useLastParams,
                                                analyticGradient=analyticGradient)
        params = dict(zip(keys, paramsOut[:nhyp]))
        self.updateKernelParams(params)
        if optimizeInducing:
            self.fitcnodes = np.array(paramsOut[nhyp:], dtype=float).reshape(shapeS)
        return params, optValue

    def chooseParams(self, paramLowerBounds, paramUpperBounds, startValues, costFunction, maxiter=40,
                     useLastParams=True, analyticGradient=False):
        """SciPy L-BFGS-B, factr=1e10, maxfun=maxiter (gp.py:615-639): numerical gradients as in the reference, or the
        cost function's own gradient when `analyticGradient` is set."""
        bounds = list(zip(paramLowerBounds, paramUpperBounds))

        def objFunc(x):
            return costFunction(x, np.empty(0))

        def objFuncWithGrad(x):
            g = np.empty(len(x))
            f = costFunction(x, g)
            return f, g

        if analyticGradient:
            sol = bfgs(objFuncWithGrad, np.array(startValues), bounds=bounds, factr=1e10, maxfun=maxiter)[0]
        else:
            sol = bfgs(objFunc, np.array(startValues), bounds=bounds, approx_grad=True, factr=1e10, maxfun=maxiter)[0]
        return sol, objFunc(sol)
