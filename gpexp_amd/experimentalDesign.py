"""Experimental-design cost functions and greedy designs with the reference's interface
(gpExp/experimentalDesign.py), evaluated on the GPU.

Hot-path pieces:
  costFunctionGP_IVAR.evaluate        refit on the design + mean posterior variance over the MC points
                                      (experimentalDesign.py:79-117)            -> gpx_potrf + gpx_ivar
  performGreedyVarExperimentalDesign  greedy maximum posterior variance (:787-845) -> gpx_greedy_var
  costFunctionGP_MI / performGreedyMIExperimentalDesign (:223-285, :753-785)       -> gpx_mi_greedy
  greedyIVARStep                      discrete one-step-lookahead IVAR (the composition SURVEY.md 8c pins;
                                      the reference has no such function)        -> gpx_greedy_ivar_step

Host drivers kept because demo.py needs them: ExperimentalDesign.boundsFunction,
ExperimentalDesignDerivative.begin / beginWithVarGreedy (SciPy SLSQP branch).  The Mercer-basis "version 0" of
IVAR is dead code in the reference (no kernel defines `eigenvalues`, :122,129,193) and is not provided; the
COBYLA / greedy-continuation drivers (:500-751) and the space-filling / Bayesian-optimisation helpers (:852-1003)
are outside the hot path.
"""
import copy
import itertools
import sys

import numpy as np

try:
    from scipy.optimize import fmin_slsqp as slsqp
except ImportError:  # pragma: no cover
    slsqp = None
import scipy.optimize as optimize
import scipy.stats as spstats
from scipy.optimize import fmin_l_bfgs_b as _bfgs

from . import device as _dev
from . import dist as _dist
from . import gp_kernel_utilities  # noqa: F401  (the reference module exposes it)
from .gp import GP as _GP, drawBaseSamples as _drawBaseSamples

NLOPT = False

__all__ = ["costFunctionBase", "costFunctionGP_IVAR", "costFunctionGP_MI", "ExperimentalDesign",
           "ExperimentalDesignDerivative", "performGreedyVarExperimentalDesign",
           "performGreedyMIExperimentalDesign", "greedyIVARStep", "performGreedyIVARExperimentalDesign", "costFuncGPUCbound",
           "costFuncPI", "costFuncEI", "optimizeAcquisition", "costFunctionVFE_IVAR", "costFuncMES", "np"]


class costFunctionBase(object):

    def __init__(self, nInputs, space):
        self.numInputs = nInputs
        self.space = space


class costFunctionGP_IVAR(costFunctionBase):
    """Integrated posterior variance of a GP trained at the design points, estimated over MC points."""

    def __init__(self, gaussianProcess, nInputs, space, version=1, **kwargs):
        super(costFunctionGP_IVAR, self).__init__(nInputs, space)
        self.gaussianProcess = copy.copy(gaussianProcess)
        self.version = version
        if self.version != 1:
            raise NotImplementedError("IVAR version 0 needs a Mercer eigen-basis that no kernel class provides "
                                      "(dead code in the reference, experimentalDesign.py:119-146)")
        self._mc_dev = None  # MC points stay resident in HBM across optimiser evaluations
        if 'mcPoints' in kwargs:
            self.mcPoints = kwargs['mcPoints']
        else:
            self.mcPoints = space.sample((10000, space.dimension))

    # `mcPoints` is an attribute users reassign (the reference's drivers do): everything derived from the set -- its device copy, the
    # forward solve W kept for the gradient (N x M doubles: 2 GB at N = 8192, M = 32768) and the cost that goes with it -- is
    # dropped with it (the kept cost / gradient would otherwise belong to the previous set).
    @property
    def mcPoints(self):
        return self._mcPoints

    @mcPoints.setter
    def mcPoints(self, pts):
        self._mcPoints = pts
        self.nMC = len(pts)
        self.reset()

    def reset(self):
        """Drop the device state kept across optimiser iterations (MC points, forward solve, cost); the batch driver calls it
        when a batch ends."""
        self._mc_dev = None
        self._w_kept = None

    def _mc(self):
        if self._mc_dev is None:
            self._mc_dev = _dev.points(_dev.context(), self._mcPoints)
        return self._mc_dev

    def evaluate(self, inputPoints):
        """|mean_z var(z | design = inputPoints)| (experimentalDesign.py:100-117)."""
        assert inputPoints.shape == (self.numInputs, self.space.dimension), \
            ("inputPoints are the wrong size: ", inputPoints.shape)
        gp = self.gaussianProcess
        if self.space.noiseFunc is None:
            gp.addNodesAndComputeCovariance(inputPoints)
        else:
            gp.addNodesAndComputeCovariance(inputPoints, self.space.noiseFunc(inputPoints))
        if not gp._has_factor():   # FITC model: the same mean through the Woodbury precision (gp.py:246-255), as the reference
            return np.abs(np.mean(gp.evaluateVariance(self.mcPoints)))
        sess = _dist.session()
        if sess is not None and (gp._Lc is not None or sess.use_eval(self.nMC)):   # MC points sharded over the ranks, partial sums in rank order
            return np.abs(sess.ivar(gp.kernel._spec(), gp._Lc or gp._L, gp._X, self.mcPoints, cache=self))
        # An optimiser asks for the cost and then for its gradient at the same design (SLSQP: experimentalDesign.py:471-489):
        # from 1024 design points on the forward solve W = L^-1 K(X, Z) stays on the device for that gradient -- a third of
        # its work (design state across optimiser iterations).  Keyed on the factor OBJECT: the same design
        # gets the kept factor back from GP._cached_factor; one W at a time, (factor, W, signed cost).
        # ... and a batch loop moves the last points only (experimentalDesign.py:694-751): when the refit kept the leading rows of
        # the factor W belongs to, W keeps them too and only its trailing rows are solved again (gpx_ivar_update).
        prev, self._w_kept = getattr(self, "_w_kept", None), None
        if inputPoints.shape[0] >= 1024 and gp.reuseFactor and self.space.noiseFunc is None:
            ctx, spec = _dev.context(), gp.kernel._spec()
            lr = getattr(gp, "_last_refit", None)
            if prev is not None and prev[0] is gp._L:                  # the very fit W and the cost belong to
                self._w_kept = prev
                return np.abs(prev[2])
            if prev is not None and lr is not None and lr[0] is prev[0] and prev[1].shape[0] == inputPoints.shape[0]:
                cost = _dev.ivar_update(ctx, spec, gp._L, gp._X, self._mc(), prev[1], lr[1])
                self._w_kept = (gp._L, prev[1], cost)
                return np.abs(cost)
            del prev                                                   # (its W goes back to the pool before the next one is made)
            cost, W = _dev.ivar(ctx, spec, gp._L, gp._X, self._mc(), keep=True)
            if W is not None:
                self._w_kept = (gp._L, W, cost)
        else:
            cost = _dev.ivar(_dev.context(), gp.kernel._spec(), gp._L, gp._X, self._mc())
        return np.abs(cost)

    def derivative(self, inputPoints):
        """d IVAR / d design coordinates, flattened (experimentalDesign.py:168-179): gpx_ivar_grad --
        two triangular solves, one MFMA GEMM and a fused row reduction instead of the reference's (N*d x M) matrix --
        for the kernels the reference differentiates (squared exponential, 1-D Mehler: its convention, GP.varianceGradient) and
        the isotropic Matern kernels (the true gradient), with the heteroscedastic terms of `space.noiseFunc` when there is one.  With `pinnedPoints` set (the batch driver: the leading points are fixed by equal
        bounds) the entries of the pinned points are returned as ZEROS -- not the full gradient."""
        gp = self.gaussianProcess
        nd = None
        if self.space.noiseFunc is None:
            gp.addNodesAndComputeCovariance(inputPoints)
        else:
            gp.addNodesAndComputeCovariance(inputPoints, noiseIn=self.space.noiseFunc(inputPoints))
            nd = np.asarray(self.space.noiseFunc.deriv(inputPoints), dtype=float).reshape(inputPoints.shape)
        gp._point_derivative_ready(self.mcPoints, referenceOnly=False)
        if gp._fitc is not None:
            # FITC model: the reference sums evaluateVarianceDerivative over the MC points (experimentalDesign.py:171-177), which
            # reads the Woodbury precision (gp.py:322); gpx_fitc_var_grad, then the same mean over the MC points
            dv = gp._fitc.var_grad(gp.kernel._spec(), self._mc(), nd)
            return np.sum(dv, axis=1) / float(len(self.mcPoints))
        kept = getattr(self, "_w_kept", None)
        W = kept[1] if (kept is not None and nd is None and kept[0] is gp._L) else None    # (read only: it stays for the next cost)
        # `pinnedPoints` (set by the batch driver, experimentalDesign.py:719-724: the leading points are fixed by equal bounds, so
        # the optimiser never uses their entries): the gradient of the free points alone from the kept solve -- gpx_ivar_grad_rows,
        # 2 (N - r0) N M flops instead of 2 N^2 M; the pinned entries are returned as zeros
        r0 = (int(getattr(self, "pinnedPoints", 0)) // 128) * 128
        if W is not None and r0 > 0 and gp.kernel._spec().kind != _dev.K_MEHLER:
            g = np.zeros(inputPoints.shape[0] * self.space.dimension)
            g[r0 * self.space.dimension:] = _dev.ivar_grad_rows(_dev.context(), gp.kernel._spec(), gp._L, gp._X, self._mc(), W, r0)
            return g
        return _dev.ivar_grad(_dev.context(), gp.kernel._spec(), gp._L, gp._X, self._mc(), nd, W=W)


class costFunctionVFE_IVAR(costFunctionGP_IVAR):
    """costFunctionGP_IVAR on a VFE model (GP(..., FITC=fraction, sparse="vfe")), computed in the inducing space (gpx_vfe_design_*):
    the design enters the variational variance through a nu x nu matrix only and the MC points through one nu x nu Gram matrix,
    so a cost / gradient evaluation is O(nu^3 + nu^2 b) for b free points -- independent of the number of MC points and, with
    `pinnedPoints` (the batch driver), of the pinned count.  The gradient is the TRUE derivative of the signed cost, with the
    inducing points `gaussianProcess.fitcnodes` held fixed (squared exponential and isotropic Matern; Mehler: the cost only).

    The inducing points must be set before the cost is built: a design loop must not draw them from its own first iterate, and the
    batch driver rebuilds the cost every batch.  The class does NOT refit or touch its GP copy -- there is no
    addNodesAndComputeCovariance per iterate; the copy only supplies the kernel, the noise and the inducing points.  The device state
    (gpx_vfe_design_create: built lazily) is rebuilt when `mcPoints`, `fitcnodes`, the kernel's hyper-parameters or `noise` change
    (compared by value), and `reset()` drops it.  One entry of (cost, gradient) is kept, keyed on the bytes of the design: an
    optimiser's cost / gradient pair at the same design is one device call.  Per-point noise (`space.noiseFunc`) is not offered."""

    def __init__(self, gaussianProcess, nInputs, space, version=1, **kwargs):
        if not (isinstance(gaussianProcess, _GP) and gaussianProcess._vfe()):
            raise ValueError("costFunctionVFE_IVAR needs a VFE model (GP(..., FITC=fraction, sparse='vfe')); on a dense or FITC "
                             "model use costFunctionGP_IVAR")
        if gaussianProcess.fitcnodes is None:
            raise ValueError("costFunctionVFE_IVAR: set gaussianProcess.fitcnodes (the inducing points) first -- a design loop "
                             "must not draw them from its own first iterate")
        super(costFunctionVFE_IVAR, self).__init__(gaussianProcess, nInputs, space, version, **kwargs)
        self.pinnedPoints = 0

    def reset(self):
        """Drop the device state (and the parent's); the next evaluation rebuilds it."""
        super(costFunctionVFE_IVAR, self).reset()
        self._state = None     # (VfeDesign, pinned block or None)
        self._state_key = None
        self._last = None      # (bytes of the design, signed cost, flat gradient or None)

    def _design(self):
        gp = self.gaussianProcess
        spec = gp.kernel._spec()
        S = np.ascontiguousarray(gp.fitcnodes, dtype=float)
        Z = np.ascontiguousarray(self._mcPoints, dtype=float)
        key = self._state_key
        same = (self._state is not None and key[0] == spec.kind and np.array_equal(key[1], spec.hyp) and key[2] == float(gp.noise)
                and np.array_equal(key[3], S) and np.array_equal(key[4], Z))
        if not same:
            self._state = self._last = None    # (the old state goes back to the pool before the new one is made)
            ctx = _dev.context()
            self._state = [_dev.VfeDesign(ctx, spec, _dev.points(ctx, S), float(gp.noise), _dev.points(ctx, Z)), None]
            self._state_key = (spec.kind, spec.hyp.copy(), float(gp.noise), S.copy(), Z.copy())
        return self._state

    def _eval(self, inputPoints, want_grad):
        assert inputPoints.shape == (self.numInputs, self.space.dimension), \
            ("inputPoints are the wrong size: ", inputPoints.shape)
        if self.space.noiseFunc is not None:
            raise NotImplementedError("costFunctionVFE_IVAR: per-point noise (space.noiseFunc) is not offered -- a VFE model has "
                                      "one noise variance")
        X = np.ascontiguousarray(inputPoints, dtype=float)
        state = self._design()
        r0 = int(self.pinnedPoints)
        if not 0 <= r0 < X.shape[0]:
            raise ValueError("costFunctionVFE_IVAR: pinnedPoints = %d leaves no free point among %d" % (r0, X.shape[0]))
        key = (r0, X.tobytes())
        if self._last is not None and self._last[0] == key and (self._last[2] is not None or not want_grad):
            return self._last[1], self._last[2]
        ctx = _dev.context()
        pinned = X[:r0].copy()
        if state[1] is None or not np.array_equal(state[1], pinned):
            state[0].pin(_dev.points(ctx, pinned) if r0 > 0 else None)
            state[1] = pinned
        cost, g = state[0].eval(_dev.points(ctx, X[r0:]), want_grad=want_grad)
        grad = None
        if want_grad:
            grad = np.zeros(X.size)
            grad[r0 * X.shape[1]:] = np.asarray(g, dtype=float).ravel()
        self._last = (key, cost, grad)
        return cost, grad

    def _has_gradient(self):
        return self.gaussianProcess.kernel._spec().kind != _dev.K_MEHLER

    def evaluate(self, inputPoints):
        """|IVAR(design = inputPoints)|.  The gradient is computed in the same device call (where the kernel has one) and kept for
        a `derivative` at the same design."""
        return np.abs(self._eval(inputPoints, self._has_gradient())[0])

    def derivative(self, inputPoints):
        """d (signed IVAR) / d design coordinates, flattened (N*d,); the entries of the `pinnedPoints` leading points are ZEROS (the
        parent's contract for pinned points)."""
        if not self._has_gradient():
            raise NotImplementedError("costFunctionVFE_IVAR.derivative: %s has no point derivative here (squared exponential and "
                                      "isotropic Matern only)" % type(self.gaussianProcess.kernel).__name__)
        return self._eval(inputPoints, True)[1].copy()

    def evaluateWithDerivative(self, inputPoints):
        """(|IVAR|, gradient of the signed IVAR) from one device call."""
        g = self.derivative(inputPoints)
        return np.abs(self._last[1]), g


class costFunctionGP_MI(costFunctionBase):
    """Mutual-information ratio var(c | A) / var(c | all \\ A \\ c) among a fixed candidate set."""

    def __init__(self, gaussianProcess, nInputs, space, nmc=None, mcpoints=None, square=False):
        super(costFunctionGP_MI, self).__init__(nInputs, space)
        self.gaussianProcess = gaussianProcess  # NOT copied: the reference mutates the caller's GP (:227,240)
        if nmc is not None:
            self.nMC = nmc
            self.mcPoints = np.copy(mcpoints)
        elif space.dimension == 2 and square is True:
            x = np.linspace(-1, 1, 10)
            self.nMC = len(x) * len(x)
            self.mcPoints = np.array(list(itertools.product(x, x)))
        else:
            self.nMC = 200
            self.mcPoints = space.sample((self.nMC, space.dimension))
        self.gaussianProcess.addNodesAndComputeCovariance(self.mcPoints)

    def add_candidates(self, nCandidates, candidates):
        self.nMC = nCandidates
        self.mcPoints = copy.deepcopy(candidates)
        self.gaussianProcess.addNodesAndComputeCovariance(self.mcPoints)

    # the reference caches dense copies that evaluate() never uses (:241-242); kept as lazy views
    @property
    def cov(self):
        return self.gaussianProcess.covarianceMatrix

    @property
    def invcov(self):
        return self.gaussianProcess.precisionMatrix

    def _cond_var(self, rows, point):
        """var(f(point) | noisy observations at mcPoints[rows]) through a fresh factorisation."""
        gp = self.gaussianProcess
        ctx = _dev.context()
        spec = gp.kernel._spec()
        if len(rows) == 0:
            return _dev.kernel_eval(ctx, spec, point, point)[0]
        X, L, _ = gp._factor(self.mcPoints[rows, :], gp.noise)
        _, var = _dev.posterior(ctx, spec, L, X, None, _dev.points(ctx, point), want_mean=False)
        return var[0]

    def evaluate(self, index, indexAdded):
        """Ratio for candidate `index` given the already selected `indexAdded` (experimentalDesign.py:249-285)."""
        point = self.mcPoints[index, :].reshape((1, self.space.dimension))
        added = list(indexAdded)
        left = np.setdiff1d(np.setdiff1d(np.arange(self.nMC), added), [index])
        return self._cond_var(added, point) / self._cond_var(list(left), point)


class ExperimentalDesign(object):
    """Base class of the continuous design optimisers."""
    nMCpoints = 10000

    def __init__(self, costFunction, nPoints, nDims, **kwargs):
        self.costFunction = costFunction
        self.nPoints = nPoints
        self.nDims = nDims
        super(ExperimentalDesign, self).__init__()

    def boundsFunction(self, optPoints):
        """+1 if every point has non-zero probability density, else -1 (experimentalDesign.py:312-343)."""
        if len(np.shape(optPoints)) == 1:
            optPoints = np.reshape(optPoints, (int(len(optPoints) / self.nDims), self.nDims))
        out = np.array(self.costFunction.space.probDensity(optPoints), dtype=float)
        out[out == 0.0] = -1e0
        return -1e0 if np.min(out) < 0.0 else 1e0


class ExperimentalDesignDerivative(ExperimentalDesign):
    """Gradient-based continuous design (SciPy SLSQP; the nlopt branch of the reference is not provided)."""

    def __init__(self, costFunction, nPoints, nDims):
        self.addObj = lambda x: 0
        self.addGrad = lambda x: 0
        super(ExperimentalDesignDerivative, self).__init__(costFunction, nPoints, nDims)

    def addPenaltyToObjective(self, addObj, addGrad):
        self.addObj = addObj
        self.addGrad = addGrad

    def objFunc(self, in1, gradIn):
        in0 = np.reshape(in1, (int(len(in1) / self.nDims), self.nDims))
        if gradIn.size > 0:
            gradIn[:] = self.costFunction.derivative(in0)
        out = self.costFunction.evaluate(in0) - 10.0 * np.min(np.array([self.boundsFunction(in0), 0.0]))
        sys.stdout.write("\r Optimization (Cost = %s, ||g||= %s) OK\n" % (str(out), str(None)))
        sys.stdout.flush()
        return out

    def constraint(self, in0, gradIn):
        if gradIn.size > 0:
            gradIn[:] = -optimize.approx_fprime(in0, self.boundsFunction, 1e-8)
        return -self.boundsFunction(in0)

    def beginWithVarGreedy(self, nodesKeep=None, lbounds=[], rbounds=[]):
        """Start SLSQP from a greedy maximum-variance design; `nodesKeep` are pinned in front (:379-409)."""
        kTemp = copy.copy(self.costFunction.gaussianProcess.kernel)
        if nodesKeep is not None:
            mcPoints = np.concatenate((nodesKeep, self.costFunction.mcPoints), axis=0)
            indKeep = np.arange(len(nodesKeep)).tolist()
        else:
            try:
                mcPoints = self.costFunction.mcPoints[:]
            except AttributeError:
                mcPoints = self.costFunction.space.sample((1000, self.costFunction.space.dimension))
            indKeep = []
        startVals = performGreedyVarExperimentalDesign(kTemp, mcPoints, self.nPoints, self.nDims,
                                                       indKeepStart=indKeep)
        return self.begin([startVals], lbounds, rbounds)

    def begin(self, startValues, lbounds=[], rbounds=[]):
        """Minimise the cost from every start with SLSQP (acc=1e-6) and return the best design (:463-497)."""

        def func(xIn, *args):
            in0 = np.reshape(xIn, (int(len(xIn) / self.nDims), self.nDims))
            return self.costFunction.evaluate(in0) - 10.0 * np.min(np.array([self.boundsFunction(in0), 0.0]))

        def grad(xIn, *args):
            in0 = np.reshape(xIn, (int(len(xIn) / self.nDims), self.nDims))
            return self.costFunction.derivative(in0)

        nvar = len(startValues[0]) * self.nDims
        if len(lbounds) == 0:
            bounds = list(zip(-100.0 * np.ones(nvar), 100.0 * np.ones(nvar)))
        else:
            bounds = list(zip(lbounds, rbounds))
        # `freeVariablesOnly` (opt-in; the reference hands SLSQP every coordinate, the pinned ones with equal bounds,
        # experimentalDesign.py:719-724): the leading points whose bounds coincide are taken out of the optimiser's variable
        # vector -- the same problem, but SLSQP's dense algebra is O(variables^3) per iteration and a batch of 64 new points on
        # top of 4000 pinned ones is 64 d variables, not 4064 d.  Cost and gradient still see the whole design.
        free0 = 0
        if getattr(self, "freeVariablesOnly", False) and len(lbounds) > 0:
            fixed = np.asarray(lbounds, dtype=float) == np.asarray(rbounds, dtype=float)
            k = int(np.argmin(fixed)) if not fixed.all() else nvar
            free0 = (k // self.nDims) * self.nDims
        sol = []
        obj = np.zeros((len(startValues)))
        for ii in range(len(startValues)):
            x0 = startValues[ii].reshape((nvar))
            if free0 > 0:
                head = np.asarray(lbounds, dtype=float)[:free0]
                tail = slsqp(lambda xf, *a: func(np.concatenate((head, xf))), x0[free0:],
                             fprime=lambda xf, *a: grad(np.concatenate((head, xf)))[free0:], bounds=bounds[free0:], acc=1e-6)
                pts = np.concatenate((head, np.atleast_1d(tail)))
            else:
                pts = slsqp(func, x0, fprime=grad, bounds=bounds, acc=1e-6)
            sol.append(pts)
            obj[ii] = func(pts)
        best = sol[int(np.argmin(obj))]
        return np.reshape(best, (int(len(best) / self.nDims), self.nDims))


class ExperimentalDesignGreedyWithDerivatives(ExperimentalDesignDerivative):
    """Batch-greedy continuous design (experimentalDesign.py:694-751, the branch without continuation): points are added
    `nPointsBatch` at a time; every batch is an SLSQP run over ALL points so far in which the earlier ones are pinned by
    equal lower/upper bounds (:719-724) and the new ones start from a greedy maximum-variance pick.

    SURVEY.md 8 f2: because the pinned points lead every trial design, each cost/gradient evaluation of a batch re-uses
    the factor of their covariance block (gpx_refit_rows, O(N^2 b) instead of O(N^3/3)) -- GP._factor does that
    transparently for the GP copy the cost function owns."""

    def __init__(self, costFunction, nPoints, nPointsBatch, nDims, **kwargs):
        super(ExperimentalDesignGreedyWithDerivatives, self).__init__(costFunction, nPoints, nDims)
        self.nPointsBatch = nPointsBatch
        if kwargs.get('useCont', 0) != 0:
            raise NotImplementedError("hyper-parameter continuation (experimentalDesign.py:500-692) is outside the GPU "
                                      "hot path")

    def begin(self, startValues=np.array([])):
        nPointsAdded = len(startValues)
        points = startValues.copy() if len(startValues) > 0 else np.zeros((0, self.nDims))
        tol = 1e-16
        err = 10000
        cf = self.costFunction
        while (nPointsAdded < self.nPoints) and (err > tol):
            print("Number of points so far ", nPointsAdded)
            nPointsAdded = nPointsAdded + self.nPointsBatch
            lbounds = -100.0 * np.ones((nPointsAdded * self.nDims))
            rbounds = 100.0 * np.ones((nPointsAdded * self.nDims))
            nPointsPrev = nPointsAdded - self.nPointsBatch
            lbounds[0:nPointsPrev * self.nDims] = points.reshape((nPointsPrev * self.nDims))
            rbounds[0:nPointsPrev * self.nDims] = points.reshape((nPointsPrev * self.nDims))
            currCost = type(cf)(cf.gaussianProcess, nPointsAdded, cf.space, cf.version, mcPoints=cf.mcPoints)
            currCost.pinnedPoints = nPointsPrev          # (large designs: cost and gradient touch the new batch's rows only)
            expCurr = ExperimentalDesignDerivative(currCost, nPointsAdded, self.nDims)
            expCurr.freeVariablesOnly = getattr(self, "freeVariablesOnly", False)
            points = expCurr.beginWithVarGreedy(nodesKeep=points, lbounds=lbounds, rbounds=rbounds)
            err = currCost.evaluate(points)
            print("Current Error ", err)
            currCost.reset()                             # the batch is over: its forward solve (N x M doubles) leaves the device
        return points


def performGreedyMIExperimentalDesign(costFuncMI, nPoints, start=0):
    """Greedy mutual-information design among costFuncMI.mcPoints, seeded with [start] (:753-785).

    The reference evaluates two fresh pinv's per remaining candidate per step; gpx_mi_greedy carries the
    numerator as an incremental Cholesky row and the denominator as diag((K_SS+noise I)^-1) with rank-one
    down-dates of the inverse, so a step costs O(M^2)."""
    gp = costFuncMI.gaussianProcess
    sess = _dist.session()
    if sess is not None and sess.use_fit(len(costFuncMI.mcPoints)):   # scoring sharded by rows of the inverse (dist_mi_greedy)
        idx, _ = sess.mi_greedy(gp.kernel._spec(), costFuncMI.mcPoints, float(gp.noise), int(nPoints), int(start))
        return costFuncMI.mcPoints[list(idx), :]
    ctx = _dev.context()
    C = _dev.points(ctx, costFuncMI.mcPoints)
    idx, _ = _dev.mi_greedy(ctx, gp.kernel._spec(), C, float(gp.noise), int(nPoints), int(start))
    return costFuncMI.mcPoints[list(idx), :]


def performGreedyVarExperimentalDesign(kernel, mcPoints, nPoints, dimension, weights=None, indKeepStart=[]):
    """Greedy maximum-posterior-variance ("entropy") design among mcPoints (:787-845).

    As in the reference the caller's `indKeepStart` list is extended in place -- that aliasing is how callers
    get the indices back (:808) -- and mcPoints[indices] is returned.  First pick from an empty start is the
    arg-max of the (weighted) prior variance; ties go to the lowest index (np.argmax)."""
    if indKeepStart == []:
        indKeep = []
    else:
        indKeep = indKeepStart
    have = len(indKeep)
    if have % 10 == 0 and have < nPoints:
        print("Number of points we have ", have)
    if have < nPoints:
        ctx = _dev.context()
        C = _dev.points(ctx, np.asarray(mcPoints, dtype=float))
        idx = _dev.greedy_var(ctx, kernel._spec(), C, int(nPoints), keep=indKeep, weights=weights)
        for j in idx[have:]:
            indKeep.append(int(j))
    return mcPoints[indKeep, :]


def greedyIVARStep(gaussianProcess, candidates, mcPoints):
    """One step of discrete greedy IVAR for a GP whose training set is already factored
    (gp.addNodesAndComputeCovariance / train): returns (best_index, costs) where
    costs[j] = costFunctionGP_IVAR(gp, n+1, space, mcPoints=mcPoints).evaluate(vstack(gp.pts, candidates[j]))."""
    gp = gaussianProcess
    if not gp._has_factor():
        raise NotImplementedError("greedyIVARStep needs the dense Cholesky factor (GP built with FITC=... has none)")
    sess = _dist.session()
    if sess is not None and sess.use_eval(len(candidates)):      # candidates sharded, first-minimum merge, costs gathered
        return sess.greedy_ivar_step(gp.kernel._spec(), gp._L, gp._X, candidates, mcPoints, float(gp.noise))
    ctx = _dev.context()
    return _dev.greedy_ivar_step(ctx, gp.kernel._spec(), gp._L, gp._X, _dev.points(ctx, candidates),
                                 _dev.points(ctx, mcPoints), float(gp.noise))


def performGreedyIVARExperimentalDesign(gaussianProcess, candidates, mcPoints, nPoints, returnCosts=False):
    """`nPoints` picks of discrete greedy IVAR for a GP whose training set is already factored: at every pick the candidate whose
    addition minimises costFunctionGP_IVAR.evaluate (experimentalDesign.py:79-117) is appended to the design -- the loop
    `for k: best, _ = greedyIVARStep(gp, candidates, mcPoints); gp.addNodesAndComputeCovariance(vstack(gp.pts, candidates[best]))`
    (the reference has no such function) -- WITHOUT refitting: gpx_greedy_ivar keeps L^-1 K(X, C) and
    cov(Z, C | design) resident and conditions them on each pick by a rank-one update.  The GP itself is not modified.
    Returns candidates[indices] (as the reference's greedy designs do) or (indices, costs) with returnCosts=True."""
    gp = gaussianProcess
    if not gp._has_factor():
        raise NotImplementedError("performGreedyIVARExperimentalDesign needs the dense Cholesky factor (GP built with FITC=... has none)")
    candidates = np.asarray(candidates, dtype=float)
    sess = _dist.session()
    if sess is not None and sess.use_eval(len(candidates)):
        idx, costs = sess.greedy_ivar(gp.kernel._spec(), gp._L, gp._X, candidates, mcPoints, float(gp.noise), int(nPoints))
    else:
        ctx = _dev.context()
        n, m, nmc = gp.pts.shape[0], len(candidates), len(mcPoints)
        resident = 8.0 * (m + 128) * (n + nmc + int(nPoints) + 512)       # W_C, cov(Z, C), the picks' rows (+ padding)
        if not hasattr(ctx, "_hbm_bytes"):
            ctx._hbm_bytes = ctx.info()["hbm_bytes"]
        if resident + 16.0 * (n + 128) * (nmc + 128) + 8.0 * n * n > 0.8 * ctx._hbm_bytes:
            # the resident state does not fit beside the factor: the refit loop it replaces (chunked over the candidates)
            idx, costs, X = [], [], np.array(gp.pts, dtype=float, copy=True)
            g2 = copy.copy(gp)
            for _ in range(int(nPoints)):
                g2.addNodesAndComputeCovariance(X)
                best, c = greedyIVARStep(g2, candidates, mcPoints)
                idx.append(int(best))
                costs.append(float(c[best]))
                X = np.vstack((X, candidates[best:best + 1]))
            idx, costs = np.array(idx, dtype=np.int64), np.array(costs)
        else:
            idx, costs = _dev.greedy_ivar(ctx, gp.kernel._spec(), gp._L, gp._X, _dev.points(ctx, candidates),
                                          _dev.points(ctx, np.asarray(mcPoints, dtype=float)), float(gp.noise), int(nPoints))
    if returnCosts:
        return idx, costs
    return candidates[list(idx), :]


##########################################################
# Bayesian-optimisation cost functions (experimentalDesign.py:886-1003)
##########################################################
def firstMinIndex(costs):
    """Selection rule of bestCandidate (and of gpx_acq): the FIRST index of the minimum among the non-NaN costs, -1 when every
    cost is NaN."""
    c = np.asarray(costs, dtype=float).ravel()
    ok = np.flatnonzero(~np.isnan(c))
    if ok.size == 0:
        return -1
    return int(ok[np.argmin(c[ok])])


class _AcqCalls(object):
    """The three batched device calls on the trained model of a GP, the model's own arguments bound -- the one place that tells
    the model kinds apart:
      dense  gpx_acq / gpx_acq_grad / gpx_acq_batch on the Cholesky factor, the training points and the coefficients;
      VFE    VfeModel.acq / acq_grad / acq_batch on the device model (its inducing points are the model's) and the coefficients;
      FITC   none: `_costFuncBO._dense` raises NotImplementedError before one is asked for."""

    def __init__(self, ctx, gp):
        self.ctx, self.gp = ctx, gp
        sparse = getattr(gp, "_fitc", None)
        self.vfe = sparse if sparse is not None and gp._vfe() else None

    def acq(self, Z, kind, param, want_costs=True):
        gp = self.gp
        if kind == _dev.ACQ_MES:          # param = (yStar, sign): gpx_acq_mes / gpx_vfe_acq_mes
            if self.vfe is not None:
                return self.vfe.acq_mes(gp.coeff, Z, param[0], param[1], want_costs=want_costs)
            return _dev.acq_mes(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, Z, param[0], param[1], want_costs=want_costs)
        if self.vfe is not None:
            return self.vfe.acq(gp.coeff, Z, kind, param, want_costs=want_costs)
        return _dev.acq(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, Z, kind, param, want_costs=want_costs)

    def acq_grad(self, Z, kind, param):
        gp = self.gp
        if kind == _dev.ACQ_MES:
            if self.vfe is not None:
                return self.vfe.acq_mes_grad(gp.coeff, Z, param[0], param[1])
            return _dev.acq_mes_grad(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, Z, param[0], param[1])
        if self.vfe is not None:
            return self.vfe.acq_grad(gp.coeff, Z, kind, param)
        return _dev.acq_grad(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, Z, kind, param)

    def acq_batch(self, C, kind, param, track, lie, lieValue, q, want_all=False):
        gp = self.gp
        if kind == _dev.ACQ_MES:          # (no track_best: the sampled optima stay fixed from pick to pick)
            if self.vfe is not None:
                return self.vfe.acq_mes_batch(gp.coeff, C, param[0], param[1], lie, lieValue, q, want_all=want_all)
            return _dev.acq_mes_batch(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, C, float(gp.noise), param[0], param[1],
                                      lie, lieValue, q, want_all=want_all)
        if self.vfe is not None:
            return self.vfe.acq_batch(gp.coeff, C, kind, param, track, lie, lieValue, q, want_all=want_all)
        return _dev.acq_batch(self.ctx, gp.kernel._spec(), gp._L, gp._X, gp.coeff, C, float(gp.noise), kind, param, track, lie,
                              lieValue, q, want_all=want_all)


class _costFuncBO(costFunctionBase):
    """Shared part of the three Bayesian-optimisation costs.

    Reference semantics (experimentalDesign.py:889-1003): the constructor takes a SHALLOW copy of the GP (`copy.copy`) and trains it
    on (xTrain, yTrain) -- the caller's GP is left untouched (the copy's refit replaces its handles, gp.py) -- and `evaluate` scores
    the LAST row of its argument only, through a single-row GP.evaluate(compvar=1) and scipy.stats.

    Batched forms on the device (the new capability; dense models and VFE models, GP(..., FITC=fraction, sparse="vfe") -- a GP built
    with FITC=... alone raises NotImplementedError):
      evaluateBatch(candidates)    (M,) costs                                gpx_acq / gpx_vfe_acq
      bestCandidate(candidates)    (first arg-min among the non-NaN costs or -1, its cost)   gpx_acq / gpx_vfe_acq
      derivativeBatch(candidates)  (M, d): row m = d cost_m / d candidate_m   gpx_acq_grad / gpx_vfe_acq_grad
      derivative(trainPoints)      (d,): the gradient for the last row
    Under a multi-process launch these run replicated: every rank makes the same deterministic single-GPU call on the factor."""

    _acq = None

    def __init__(self, gaussianProcess, xTrain, yTrain, nInputs, space):
        super(_costFuncBO, self).__init__(nInputs, space)
        self.xTrain = xTrain
        self.yTrain = yTrain
        self.gaussianProcess = copy.copy(gaussianProcess)
        self.gaussianProcess.train(xTrain, yTrain)

    def _fBest(self):
        return np.max(self.yTrain)

    def _param(self):
        return self._fBest()

    def _posterior(self, trainPoints):
        newPoint = np.reshape(trainPoints[-1, :], (1, self.space.dimension))
        predMean, predvar = self.gaussianProcess.evaluate(newPoint, compvar=1)
        return predMean, np.sqrt(predvar)

    def _dense(self, candidates):
        gp = self.gaussianProcess
        if (gp._fitc is not None and not gp._vfe()) or (gp._fitc is None and not gp._has_factor()):
            raise NotImplementedError("batched acquisition costs need the dense Cholesky factor (GP built with FITC=... has none) "
                                      "or a VFE model (GP(..., FITC=fraction, sparse='vfe'))")
        # the device forms mean = K(Z, X) coeff: the zero prior mean of the base class (gp.py:73)
        assert type(gp).gpPriorMean is _GP.gpPriorMean and "gpPriorMean" not in vars(gp), \
            "batched acquisition costs assume the base class's zero gpPriorMean"
        candidates = np.asarray(candidates, dtype=float)
        assert candidates.ndim == 2 and candidates.shape[1] == self.space.dimension, \
            ("candidates are the wrong size: ", candidates.shape)
        ctx = _dev.context()
        return ctx, gp, _dev.points(ctx, candidates)

    def evaluateBatch(self, candidates):
        """(M,) costs of the candidates (rows), one device call."""
        ctx, gp, Z = self._dense(candidates)
        return _AcqCalls(ctx, gp).acq(Z, self._acq, self._param())[2]

    def bestCandidate(self, candidates):
        """(index, cost): the first index of the minimum among the non-NaN costs (-1 and NaN when every cost is NaN)."""
        ctx, gp, Z = self._dense(candidates)
        best, cost, _ = _AcqCalls(ctx, gp).acq(Z, self._acq, self._param(), want_costs=False)
        return best, cost

    def evaluateBatchWithDerivative(self, candidates):
        """((M,) costs, (M, d) gradients), one device call."""
        ctx, gp, Z = self._dense(candidates)
        return _AcqCalls(ctx, gp).acq_grad(Z, self._acq, self._param())

    def derivativeBatch(self, candidates):
        """(M, d): row m = d cost_m / d candidate_m -- the true derivative of evaluateBatch (squared exponential, Matern 3/2 and
        5/2; the Mehler kernel raises)."""
        return self.evaluateBatchWithDerivative(candidates)[1]

    def derivative(self, trainPoints):
        """(d,): the gradient of the cost of the last row."""
        return self.derivativeBatch(np.reshape(trainPoints[-1, :], (1, self.space.dimension)))[0]

    def _trackBest(self):
        """Whether a batch's believed values raise fBest from pick to pick -- what constructing the cost anew on the grown data
        would do (`_fBest` is max(yTrain))."""
        return True

    def _lie(self, lie):
        """(device lie kind, value) of selectBatch's `lie` argument."""
        if isinstance(lie, str):
            if lie == "believer":
                return _dev.LIE_BELIEVER, 0.0
            reducers = {"min": np.min, "max": np.max, "mean": np.mean}
            if lie not in reducers:
                raise ValueError("lie must be 'believer', 'min', 'max', 'mean' or a number, not %r" % (lie,))
            return _dev.LIE_CONSTANT, float(reducers[lie](self.yTrain))
        return _dev.LIE_CONSTANT, float(lie)

    def selectBatch(self, candidates, nPoints, lie="believer", returnAllCosts=False):
        """The next `nPoints` candidates to evaluate TOGETHER: the loop

            for t in range(nPoints):
                j, c = type(self)(gp, X_t, y_t, ...).bestCandidate(candidates)     # candidates picked before are skipped
                X_t, y_t = vstack(X_t, candidates[j]), append(y_t, believed value at candidates[j])

        without refitting (gpx_acq_batch: L^-1 K(X, candidates) stays on the device and every pick conditions the candidates' means
        and variances by a rank-one update; the GP's scalar noise is used at the picked points).  `lie` is the value believed at a
        pick: "believer" = the current posterior mean there (Kriging believer: means frozen, variances shrink), "min" / "max" /
        "mean" of yTrain or a number (constant liar).  For PI, and for EI unless the constructor was given fBest=, fBest rises to
        the largest believed value from pick to pick; kappa / a given fBest stay.

        Returns (indices (nPoints,) int64, costs (nPoints,)): costs[t] is the winner's cost at pick t; with returnAllCosts=True also
        allCosts (nPoints, M), row t = the costs pick t was chosen from (NaN at the candidates picked before).  The cost object and
        its GP are not modified.  Dense models and VFE models; on a VFE model (gpx_vfe_acq_batch) every refit of the loop keeps the
        inducing points and hyper-parameters, so a pick enters through the inducing variables only (delta = noise + |La^-1 k_u(c_s)|^2)
        -- the refit with fixed inducing points, not conditioning the predictor with v_s + noise.  Under a multi-process launch the call runs replicated: every rank makes the same
        deterministic single-GPU call on the factor."""
        kindLie, lieValue = self._lie(lie)
        q = int(nPoints)
        ctx, gp, C = self._dense(candidates)
        n, m = gp.pts.shape[0], C.shape[0]
        if q > m:
            raise ValueError("selectBatch: %d points asked of %d candidates" % (q, m))
        calls, param, track = _AcqCalls(ctx, gp), self._param(), self._trackBest()
        if not hasattr(ctx, "_hbm_bytes"):
            ctx._hbm_bytes = ctx.info()["hbm_bytes"]
        if calls.vfe is not None:
            nup = -(-gp.fitcnodes.shape[0] // 128) * 128
            resident = 8.0 * (m + 128) * (nup + q)              # Wa = La^-1 K(S, C), the picks' rows
            transient = 8.0 * (m + 128) * nup                   # set-up: the chunk the Lu solve consumes
            fits = resident + transient <= 0.8 * ctx._hbm_bytes
        else:
            resident = 8.0 * (m + 128) * (n + q + 512)              # W_C, the picks' rows (+ padding)
            transient = 8.0 * (m + 128) * (n + 512) if n >= 1920 else 0.0   # set-up: the cross matrix the out-of-place solve consumes
            fits = resident + transient + 8.0 * n * n <= 0.8 * ctx._hbm_bytes
        if not fits:
            return self._selectBatchRefit(candidates, q, kindLie, lieValue, param, track, returnAllCosts)
        out = calls.acq_batch(C, self._acq, param, track, kindLie, lieValue, q, want_all=returnAllCosts)
        idx, costs, allc = out[0], out[1], (out[3] if returnAllCosts else None)
        return (idx, costs, allc) if returnAllCosts else (idx, costs)

    def thompsonBatch(self, candidates, nPoints, baseSamples=None, jitter=None, minimize=True):
        """Thompson sampling over a candidate set: `nPoints` independent JOINT draws of the posterior at the candidates
        (GP.posteriorSampler -> gpx_psampler_argbest), one pick each -- the first index of the draw's minimum (minimize=False:
        maximum).  Returns (indices (nPoints,) int64, values (nPoints,)); independent draws may pick the same candidate.  Only the
        picks reach the host.  `baseSamples` (nPoints, M): the standard-normal base samples (np.random.standard_normal when None);
        `jitter`: the sampler's nugget (default 1e-10 * max k(c, c)).  Dense models only (NotImplementedError on FITC / VFE)."""
        gp = self.gaussianProcess
        gp._sampling_ready("thompsonBatch")
        return self._thompsonBatch(gp.posteriorSampler, candidates, nPoints, baseSamples, jitter, minimize)

    def vfeThompsonBatch(self, candidates, nPoints, baseSamples=None, jitter=None, minimize=True):
        """thompsonBatch on a VFE model: the same picks from EXACT joint draws of the variational posterior at the candidates
        (GP.vfePosteriorSampler -> gpx_vfe_psampler_create).  ValueError on a dense or FITC model."""
        return self._thompsonBatch(self.gaussianProcess.vfePosteriorSampler, candidates, nPoints, baseSamples, jitter, minimize)

    def _thompsonCandidates(self, candidates):
        candidates = np.asarray(candidates, dtype=float)
        assert candidates.ndim == 2 and candidates.shape[1] == self.space.dimension, \
            ("candidates are the wrong size: ", candidates.shape)
        return candidates

    def _thompsonBatch(self, posteriorSampler, candidates, nPoints, baseSamples, jitter, minimize):
        """The body of thompsonBatch / vfeThompsonBatch; `posteriorSampler`: the GP's constructor of the joint sampler."""
        smp = posteriorSampler(self._thompsonCandidates(candidates), jitter=jitter)
        try:
            idx, val = smp.argbest(int(nPoints), baseSamples, minimize=minimize)
        finally:
            smp.close()
        return idx, val

    def thompsonPaths(self, candidates, nPoints, nFeatures=1024, base=None, minimize=True, polish=False, lbounds=None,
                      rbounds=None, maxiter=50):
        """Thompson sampling with PATHS (GP.pathSampler -> gpx_paths_eval): `nPoints` posterior paths with `nFeatures` random
        features, ONE arg-best pass over the candidates -- any number of them, chunked under GPX_CROSS_BYTES, no M x M factor --
        one pick each: the first index of the path's minimum (minimize=False: maximum).  Returns (points (q, d), values (q,),
        indices (q,) int64); independent paths may pick the same candidate.  `base`: the PathBase of the draws (PathBase.draw with
        NumPy when None; the same base gives the same result).
        polish=True: a path is a differentiable function, so SciPy L-BFGS-B then runs from every path's discrete winner at once,
        the way optimizeAcquisition drives its starts -- the objective is the SUM of the paths' values over the stacked q x d
        vector (separable), one gpx_paths_grad call per iteration -- inside the box [lbounds, rbounds] (default: the candidates'
        bounding box).  A polished point replaces the discrete winner only where its value is better, so no value is worse than
        the discrete one; `indices` stays the discrete index.  Pathwise samples are approximate draws (GP.pathSampler);
        thompsonBatch draws exactly.  Stationary kernels and dense models only (NotImplementedError otherwise)."""
        return self._thompsonPaths(self.gaussianProcess.pathSampler, candidates, nPoints, nFeatures, base, minimize, polish, lbounds,
                                   rbounds, maxiter)

    def vfeThompsonPaths(self, candidates, nPoints, nFeatures=1024, base=None, minimize=True, polish=False, lbounds=None,
                         rbounds=None, maxiter=50):
        """thompsonPaths on a VFE model, with decoupled paths of the variational posterior (GP.vfePathSampler ->
        gpx_vfe_paths_create): a pick costs O(nFeatures + nu) per candidate whatever the training-set size.  `base`: a PathBase
        drawn with nTrain = 2 nu.  Everything else, `polish` included, as thompsonPaths.  ValueError on a dense or FITC model,
        NotImplementedError for a Mehler kernel."""
        return self._thompsonPaths(self.gaussianProcess.vfePathSampler, candidates, nPoints, nFeatures, base, minimize, polish,
                                   lbounds, rbounds, maxiter)

    def _thompsonPaths(self, pathSampler, candidates, nPoints, nFeatures, base, minimize, polish, lbounds, rbounds, maxiter):
        """The body of thompsonPaths / vfeThompsonPaths; `pathSampler`: the GP's constructor of the paths."""
        candidates = self._thompsonCandidates(candidates)
        q, d = int(nPoints), candidates.shape[1]
        inside = None
        if polish:
            lb = np.min(candidates, axis=0) if lbounds is None else np.broadcast_to(np.asarray(lbounds, dtype=float), (d,))
            ub = np.max(candidates, axis=0) if rbounds is None else np.broadcast_to(np.asarray(rbounds, dtype=float), (d,))
            # candidates outside the box take no part (`indices` still counts rows of `candidates`)
            inside = np.flatnonzero(np.all((candidates >= lb) & (candidates <= ub), axis=1))
            if len(inside) == 0:
                raise ValueError("thompsonPaths: no candidate lies inside the bounds")
        smp = pathSampler(q, nFeatures, base)
        try:
            q = smp.nPaths
            if inside is None or len(inside) == len(candidates):
                idx, val = smp.argbest(candidates, minimize=minimize)
            else:
                idx, val = smp.argbest(candidates[inside], minimize=minimize)
                idx = inside[idx]
            pts = candidates[idx].copy()
            if polish:
                sgn, paths = (1.0 if minimize else -1.0), np.arange(q, dtype=np.int64)

                def objective(x):
                    g, v = smp.gradient(np.ascontiguousarray(np.reshape(x, (q, d))), paths, returnValues=True)
                    if not np.all(np.isfinite(v)) or not np.all(np.isfinite(g)):
                        return 1e300, np.zeros(q * d)
                    return sgn * float(np.sum(v)), sgn * g.ravel()

                x = _bfgs(objective, np.clip(pts, lb, ub).ravel(), bounds=list(zip(np.tile(lb, q), np.tile(ub, q))),
                          maxiter=int(maxiter))[0]
                P = np.clip(np.reshape(x, (q, d)), lb, ub)
                pv = smp.gradient(P, paths, returnValues=True)[1]
                better = (pv < val) if minimize else (pv > val)
                pts[better], val = P[better], np.where(better, pv, val)
        finally:
            smp.close()
        return pts, val, idx

    def _selectBatchRefit(self, candidates, q, kindLie, lieValue, param, track, returnAllCosts):
        """selectBatch when the resident state does not fit beside the factor: the refit loop it replaces, with the existing calls
        (gpx_acq / gpx_vfe_acq chunk the candidates).  On a VFE model every refit keeps the inducing points (`fitcnodes` is set)."""
        candidates = np.asarray(candidates, dtype=float)
        ctx = _dev.context()
        g2 = copy.copy(self.gaussianProcess)
        X, y = np.array(self.xTrain, dtype=float, copy=True), np.array(self.yTrain, dtype=float, copy=True).ravel()
        idx, costs, rows = [], [], []
        for t in range(q):
            if t > 0:
                g2.train(X, y)
            c = _AcqCalls(ctx, g2).acq(_dev.points(ctx, candidates), self._acq, param)[2]
            c[idx] = np.nan
            j = firstMinIndex(c)
            if j < 0:
                raise _dev._lib.GpxError("selectBatch: pick %d of %d: no candidate has a non-NaN cost" % (t + 1, q))
            believed = lieValue
            if kindLie == _dev.LIE_BELIEVER:
                believed = float(g2.evaluate(candidates[j:j + 1], compvar=0)[0])
            idx.append(j)
            costs.append(float(c[j]))
            rows.append(c)
            X, y = np.vstack((X, candidates[j:j + 1])), np.append(y, believed)
            if track:
                param = max(param, believed)
        out = (np.array(idx, dtype=np.int64), np.array(costs))
        return out + (np.array(rows),) if returnAllCosts else out


class costFuncGPUCbound(_costFuncBO):
    """GP upper confidence bound, minimisation form: -(mu - kappa s), s = sqrt(|var|) (experimentalDesign.py:889-923).

    Quirks kept from the reference: only the last row of `trainPoints` is scored; fBest = max(yTrain) is computed there and unused;
    the return value is a Python float (taken from the 1-element result without NumPy's array-to-scalar DeprecationWarning, which
    the reference's `float(array)` triggers)."""

    _acq = _dev.ACQ_UCB

    def __init__(self, gaussianProcess, kappa, xTrain, yTrain, nInputs, space, **kwargs):
        self.kappa = kappa  # kappa is tunable to balance exploit vs explore
        super(costFuncGPUCbound, self).__init__(gaussianProcess, xTrain, yTrain, nInputs, space)

    def _param(self):
        return self.kappa

    def _trackBest(self):
        return False

    def evaluate(self, trainPoints):
        predMean, predstd = self._posterior(trainPoints)
        return -float((predMean - self.kappa * predstd)[0])


class costFuncPI(_costFuncBO):
    """Probability of improvement, minimisation form: -Phi((fBest - mu) / s) with fBest = max(yTrain) (experimentalDesign.py:925-960).

    Quirks kept from the reference: only the last row of `trainPoints` is scored; fBest is the MAXIMUM of yTrain (paired with a
    minimised cost; not "fixed"); the return value is a Python float (without the array-to-scalar DeprecationWarning)."""

    _acq = _dev.ACQ_PI

    def __init__(self, gaussianProcess, xTrain, yTrain, nInputs, space, **kwargs):
        super(costFuncPI, self).__init__(gaussianProcess, xTrain, yTrain, nInputs, space)

    def evaluate(self, trainPoints):
        fBest = self._fBest()
        predMean, predstd = self._posterior(trainPoints)
        gamma = (fBest - predMean) / predstd
        phiGamma = spstats.norm.cdf(gamma)
        return -float(phiGamma[0])


class costFuncEI(_costFuncBO):
    """Expected improvement, minimisation form: -s (g Phi(g) + phi(g)), g = (fBest - mu) / s (experimentalDesign.py:962-1003).

    Quirks kept from the reference: only the last row of `trainPoints` is scored; fBest is the `fBest=` keyword when given, else the
    MAXIMUM of yTrain (paired with a minimised cost; not "fixed"); the return value is a NumPy scalar (`cost[0]`)."""

    _acq = _dev.ACQ_EI

    def __init__(self, gaussianProcess, xTrain, yTrain, nInputs, space, **kwargs):
        super(costFuncEI, self).__init__(gaussianProcess, xTrain, yTrain, nInputs, space)
        if 'fBest' in kwargs:
            self.fBest = kwargs['fBest']

    def _fBest(self):
        return self.fBest if hasattr(self, 'fBest') else np.max(self.yTrain)

    def _trackBest(self):
        return not hasattr(self, 'fBest')      # a given fBest= is the caller's constant

    def evaluate(self, trainPoints):
        fBest = self._fBest()
        predMean, predstd = self._posterior(trainPoints)
        gamma = (fBest - predMean) / predstd
        phiGamma = spstats.norm.cdf(gamma)
        probGamma = spstats.norm.pdf(gamma)
        cost = -predstd * (gamma * phiGamma + probGamma)
        return cost[0]

    # ---- joint (q-point) expected improvement by Monte Carlo ------------------------------------------------------------------
    def _jointCall(self, model, batches, nSamples, baseSamples, jitter, name, want_costs):
        """The body of jointEI / bestJointBatch and of vfeJointEI / vfeBestJointBatch.  `model()` (`_jointDense`, `_jointVfe`)
        returns (ready(name), the model's readiness rule, and call(ctx, spec, Zb, q, xi, fBest, nugget, want_costs=), its device
        entry) -- the way _thompsonBatch takes the sampler's constructor."""
        gp = self.gaussianProcess
        ready, call = model()
        ready(name)
        assert type(gp).gpPriorMean is _GP.gpPriorMean and "gpPriorMean" not in vars(gp), \
            "joint expected improvement assumes the base class's zero gpPriorMean"
        b = np.asarray(batches, dtype=float)
        if b.ndim == 2:
            b = b[None]
        if b.ndim != 3 or b.shape[0] < 1 or b.shape[2] != self.space.dimension:
            raise ValueError("%s: batches must be (B, q, %d) or (q, %d), not %r" % (name, self.space.dimension, self.space.dimension,
                                                                                 np.shape(batches)))
        nb, q = b.shape[0], b.shape[1]
        if not 1 <= q <= _dev.QEI_MAX_Q:
            raise ValueError("%s: the batch size must be in 1 .. %d, not %d" % (name, _dev.QEI_MAX_Q, q))
        xi = _drawBaseSamples(baseSamples, nSamples, q, name)
        ctx = _dev.context()
        spec = gp.kernel._spec()
        Zb = _dev.points(ctx, b.reshape(nb * q, b.shape[2]))
        nugget = gp._jitter(ctx, spec, Zb, jitter, name)
        return call(ctx, spec, Zb, q, xi, self._fBest(), nugget, want_costs=want_costs)

    def _jointDense(self):
        gp = self.gaussianProcess
        return gp._sampling_ready, lambda ctx, spec, Zb, *a, **kw: _dev.acq_qei(ctx, spec, gp._L, gp._X, gp.coeff, Zb, *a, **kw)

    def _jointVfe(self):
        gp = self.gaussianProcess
        return (lambda name: gp._vfe_sampling_ready(name, "jointEI"),
                lambda ctx, spec, Zb, *a, **kw: gp._fitc.acq_qei(gp.coeff, Zb, *a, **kw))

    def jointEI(self, batches, nSamples=256, baseSamples=None, jitter=None):
        """(B,) joint expected improvement of B batches of q points, minimisation form like `evaluate` (gpx_acq_qei):

            cost_b = -(1/S) sum_s max(0, fBest - min_j f_s(batches[b, j])),      f_s = mean_b + chol(C_b + jitter I) baseSamples[s]

        a sample average over S joint posterior draws of the batch with COMMON random numbers: the same `baseSamples` (S, q;
        np.random.standard_normal((nSamples, q)) when None) for every batch, so that two batches are compared on the same draws.
        `batches`: (B, q, d) or one batch (q, d), q <= 32.  `jitter`: nugget on every batch's q x q posterior covariance (default
        1e-10 * max k(z, z)).  A batch whose covariance does not factor with it (two identical points and jitter=0) costs NaN.
        With q = 1 the cost tends to evaluateBatch's closed form as S grows.  Dense models only."""
        return self._jointCall(self._jointDense, batches, nSamples, baseSamples, jitter, "jointEI", True)[2]

    def bestJointBatch(self, batches, nSamples=256, baseSamples=None, jitter=None):
        """(index, cost) of the batch with the lowest jointEI cost: the first minimum among the non-NaN costs, (-1, NaN) when every
        cost is NaN.  Arguments as jointEI; only the winner reaches the host."""
        best, cost, _, _ = self._jointCall(self._jointDense, batches, nSamples, baseSamples, jitter, "bestJointBatch", False)
        return best, cost

    def selectBatchJoint(self, candidates, nPoints, lies=("believer", "min", "max", "mean"), nSamples=256, baseSamples=None,
                         jitter=None):
        """The best of several greedy batches by their JOINT expected improvement: `selectBatch(candidates, nPoints, lie)` proposes
        one batch per entry of `lies`, one gpx_acq_qei call scores them all on common base samples, and the winner comes back as
        (indices (nPoints,) int64, its jointEI cost, its lie).  Arguments as selectBatch and jointEI."""
        return self._selectBatchJoint(self.bestJointBatch, "selectBatchJoint", candidates, nPoints, lies, nSamples, baseSamples,
                                      jitter)

    def _selectBatchJoint(self, bestJointBatch, name, candidates, nPoints, lies, nSamples, baseSamples, jitter):
        """The body of selectBatchJoint / vfeSelectBatchJoint; `bestJointBatch`: the scorer of the proposals."""
        lies = list(lies)
        if not lies:
            raise ValueError("%s: needs at least one lie" % name)
        candidates = np.asarray(candidates, dtype=float)
        picks = [self.selectBatch(candidates, nPoints, lie=lie)[0] for lie in lies]
        best, cost = bestJointBatch(np.stack([candidates[idx] for idx in picks]), nSamples, baseSamples, jitter)
        if best < 0:
            raise _dev._lib.GpxError("%s: no proposed batch has a non-NaN joint cost (a larger jitter factors them)" % name)
        return picks[best], cost, lies[best]

    def vfeJointEI(self, batches, nSamples=256, baseSamples=None, jitter=None):
        """jointEI on a VFE model (gpx_vfe_acq_qei): (B,) joint expected improvement of B batches of q points under the variational
        posterior -- evaluate's means, and per batch the q x q block of vfePosteriorCovariance, (k - Wu^T Wu) + Wa^T Wa, formed in
        the inducing space: O(nu q^2) a batch, whatever the training-set size.  Arguments, the common base samples, the jitter and
        the NaN rule as jointEI.  Every kernel.  ValueError on a dense or FITC model and before train; under a multi-process
        session the call runs replicated, and baseSamples=None raises ValueError there."""
        return self._jointCall(self._jointVfe, batches, nSamples, baseSamples, jitter, "vfeJointEI", True)[2]

    def vfeBestJointBatch(self, batches, nSamples=256, baseSamples=None, jitter=None):
        """bestJointBatch on a VFE model: (index, cost) of the batch with the lowest vfeJointEI cost, the first minimum among the
        non-NaN costs, (-1, NaN) when every cost is NaN; only the winner reaches the host."""
        best, cost, _, _ = self._jointCall(self._jointVfe, batches, nSamples, baseSamples, jitter, "vfeBestJointBatch", False)
        return best, cost

    def vfeSelectBatchJoint(self, candidates, nPoints, lies=("believer", "min", "max", "mean"), nSamples=256, baseSamples=None,
                            jitter=None):
        """selectBatchJoint on a VFE model: `selectBatch` (gpx_vfe_acq_batch) proposes one batch per entry of `lies`, one
        gpx_vfe_acq_qei call scores them on common base samples, and the winner comes back as (indices (nPoints,) int64, its
        vfeJointEI cost, its lie)."""
        self.gaussianProcess._vfe_sampling_ready("vfeSelectBatchJoint", "jointEI")
        return self._selectBatchJoint(self.vfeBestJointBatch, "vfeSelectBatchJoint", candidates, nPoints, lies, nSamples,
                                      baseSamples, jitter)


_MES_T0, _MES_CF_TERMS = 2.0, 73      # acq.hip's MES_T0 / MES_CF_TERMS


def mesEntropyTerm(gamma):
    """h(gamma) = gamma lambda / 2 - log Phi(gamma), lambda = phi / Phi, in float64 for an array of gamma: the device's formulation
    (acq.hip, mes_h) restated in NumPy -- the continued fraction of erfcx where -gamma / sqrt 2 >= 2, else the composition with an
    exactly formed gamma^2 / 2 (through the upper tail and log1p for gamma > 0).  h(+inf) = 0, h(-inf) = +inf, NaN for NaN.
    One of three hand-kept statements of the formulation -- mes_h on the device, this one, and tests/acq_mes_ref.terms_f64 -- each
    with its own seam T0, term count and exact square; tests/test_acq_mes_host.py pins the constants and this function's values to
    the other two.  Only h is formed here: `evaluate` needs no more, and the class has no host h' (gradients come from the
    device, gpx_acq_mes_grad)."""
    import math
    erfc = np.vectorize(math.erfc, otypes=[float])      # (SciPy's erfc gives 0 beyond 26.6, where the C library's is a subnormal)
    g = np.asarray(gamma, dtype=float)
    with np.errstate(all="ignore"):
        t = -g * np.sqrt(0.5)
        cf = t >= _MES_T0
        tt = np.where(cf, t, _MES_T0)
        f = tt.copy()
        for k in range(_MES_CF_TERMS, 2, -1):
            f = tt + (0.5 * k) / f
        C2 = 1.0 / f
        den = tt + C2
        h_cf = np.log(3.5449077018110320546 * (tt + 0.5 / den)) - 0.5 * (1.0 - C2 / den)
        gm = np.where(cf | ~(g <= 40.0), 0.0, g)
        p = gm * gm
        # gamma^2 = p + e exactly (Dekker's product of the split halves)
        c = 134217729.0 * gm
        hi = c - (c - gm)
        lo = gm - hi
        e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
        E = np.exp(-0.5 * p)
        phi = (E - 0.5 * e * E) * 0.3989422804014326779
        Q = 0.5 * erfc(np.abs(gm) * np.sqrt(0.5))
        neg = gm <= 0.0
        lam = phi / np.where(neg, Q, 1.0 - Q)
        h_c = 0.5 * gm * lam - np.where(neg, np.log(Q), np.log1p(-Q))
        return np.where(cf, h_cf, np.where(g <= 40.0, h_c, np.where(g > 40.0, 0.0, np.nan)))


def gumbelOptima(mean, std, uniforms, minimize=True):
    """Samples of the optimum VALUE over a finite set by Wang & Jegelka's Gumbel approximation (host): the points' posterior means
    and standard deviations (independent marginals), `uniforms` (K,) in (0, 1).  For a minimum, P(min_j f_j > y) = prod_j
    Phi((mean_j - y) / std_j); its 25 / 50 / 75 % points are found by bisection on the sum of scipy.special.log_ndtr, a Gumbel
    distribution is fitted to them (on -f), and it is sampled at the uniforms by its inverse: (K,) values.  minimize=False mirrors."""
    from scipy.special import log_ndtr
    m = np.asarray(mean, dtype=float).ravel()
    s = np.asarray(std, dtype=float).ravel()
    r = np.asarray(uniforms, dtype=float).ravel()
    if m.size < 1 or m.shape != s.shape or not (np.all(np.isfinite(m)) and np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError("gumbelOptima: needs finite means and positive finite standard deviations of the same length")
    if r.size < 1 or not np.all((r > 0.0) & (r < 1.0)):
        raise ValueError("gumbelOptima: uniforms must lie strictly between 0 and 1")
    if minimize:
        m = -m                                       # max(-f): P(max < z) = prod Phi((z - m_j) / s_j)

    def logcdf(z):
        return float(np.sum(log_ndtr((z - m) / s)))

    def quantile(prob):
        target = np.log(prob)
        lo, hi = float(np.min(m - 5.0 * s)), float(np.max(m + 5.0 * s))
        w = hi - lo
        while logcdf(lo) > target:
            lo -= w
        while logcdf(hi) < target:
            hi += w
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if not lo < mid < hi:
                break
            if logcdf(mid) < target:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)

    y1, y2, y3 = quantile(0.25), quantile(0.5), quantile(0.75)
    b = (y1 - y3) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    a = y2 + b * np.log(np.log(2.0))
    z = a - b * np.log(-np.log(r))
    return -z if minimize else z


class costFuncMES(_costFuncBO):
    """Max-value entropy search (Wang & Jegelka 2017), minimisation form: with K samples y*_k of the global optimum VALUE,

        cost = -(1/K) sum_k h(gamma_k),   h(gamma) = gamma lambda(gamma) / 2 - log Phi(gamma),   lambda = phi / Phi,

    gamma_k = (mu - y*_k) / s when the y* are sampled minima (minimize=True), (y*_k - mu) / s for sampled maxima: the expected drop
    in entropy of the candidate's predictive distribution once it is truncated at y*.  One posterior pass per call, like EI.

    `yStar` (K,), K <= 1024, is given to the constructor, assigned, or drawn by `sampleOptima`; the batched calls raise ValueError
    while it is None.  `evaluate` scores the last row of its argument through a single-row GP.evaluate and the float64 host
    composition `mesEntropyTerm`; evaluateBatch, bestCandidate, evaluateBatchWithDerivative, derivativeBatch, derivative,
    selectBatch (the sampled optima stay fixed from pick to pick) and optimizeAcquisition run on the device (gpx_acq_mes,
    gpx_acq_mes_grad, gpx_acq_mes_batch and their gpx_vfe_ forms) on dense and VFE models.  A FITC model raises
    NotImplementedError from the batched calls; gradients on a Mehler kernel raise the library's GpxError (an argument error of
    gpx_acq_mes_grad, as for the other three costs).  Where the variance is exactly 0 and the mean lies on the optimum side of a
    y*, the cost is -inf by the formula as written (include/gpx.h)."""

    _acq = _dev.ACQ_MES

    def __init__(self, gaussianProcess, xTrain, yTrain, nInputs, space, yStar=None, minimize=True, **kwargs):
        super(costFuncMES, self).__init__(gaussianProcess, xTrain, yTrain, nInputs, space)
        self.minimize = bool(minimize)
        self.yStar = None if yStar is None else np.array(yStar, dtype=float).ravel()

    def _sign(self):
        return 1 if self.minimize else -1

    def _param(self):
        if self.yStar is None:
            raise ValueError("costFuncMES: yStar is None -- give the sampled optima to the constructor or call sampleOptima first")
        return (np.asarray(self.yStar, dtype=float).ravel(), self._sign())

    def _trackBest(self):
        return False

    def evaluate(self, trainPoints):
        yStar, sign = self._param()
        predMean, predstd = self._posterior(trainPoints)
        with np.errstate(all="ignore"):
            gamma = sign * (float(np.ravel(predMean)[0]) - yStar) / float(np.ravel(predstd)[0])
        h = mesEntropyTerm(gamma)
        total = 0.0
        for v in h:                       # (the device's order k = 0 .. K-1)
            total += float(v)
        return -(total / h.size)

    def sampleOptima(self, candidates, nOptima=16, method="paths", nFeatures=1024, base=None, uniforms=None, polish=False,
                     lbounds=None, rbounds=None, maxiter=50):
        """Draw `nOptima` samples of the optimum value over the candidates, set `yStar` and return it (nOptima,).
        method="paths": the `values` of thompsonPaths (vfeThompsonPaths on a VFE model) -- the optimum of every sampled posterior
          path over the candidates, polished inside [lbounds, rbounds] when polish=True; `base`: the PathBase of the draws
          (stationary kernels, scalar noise; None draws with NumPy, and raises ValueError under a multi-process session).
        method="gumbel": Wang & Jegelka's approximation on the host (`gumbelOptima`) from the means and variances of ONE
          GP.evaluate(candidates, compvar=1), sampled at `uniforms` (nOptima,) in (0, 1) (np.random.uniform when None; ValueError
          under a multi-process session).  Serves every kernel and per-point noise.
        minimize=False (the constructor's) samples maxima."""
        K = int(nOptima)
        if not 1 <= K <= _dev.MES_MAX_K:
            raise ValueError("sampleOptima: nOptima must be in 1 .. %d, not %r" % (_dev.MES_MAX_K, nOptima))
        if method == "paths":
            gp = self.gaussianProcess
            vfe = getattr(gp, "_fitc", None) is not None and gp._vfe()
            draw = self.vfeThompsonPaths if vfe else self.thompsonPaths
            values = draw(candidates, K, nFeatures=nFeatures, base=base, minimize=self.minimize, polish=polish, lbounds=lbounds,
                          rbounds=rbounds, maxiter=maxiter)[1]
        elif method == "gumbel":
            if uniforms is None:
                if _dist.session() is not None:
                    raise ValueError("sampleOptima: under a multi-process session uniforms must be given (the call runs replicated "
                                     "and every rank would draw its own)")
                uniforms = np.random.uniform(size=K)
            uniforms = np.asarray(uniforms, dtype=float).ravel()
            if uniforms.shape != (K,):
                raise ValueError("sampleOptima: uniforms must have shape (%d,), not %r" % (K, uniforms.shape))
            candidates = self._thompsonCandidates(candidates)
            mean, var = self.gaussianProcess.evaluate(candidates, compvar=1)
            values = gumbelOptima(np.ravel(mean), np.sqrt(np.ravel(var)), uniforms, minimize=self.minimize)
        else:
            raise ValueError("sampleOptima: method must be 'paths' or 'gumbel', not %r" % (method,))
        self.yStar = np.array(values, dtype=float).ravel()
        return self.yStar


def optimizeAcquisition(costFunction, candidates, nStarts=8, lbounds=None, rbounds=None, maxiter=50):
    """Minimise a Bayesian-optimisation cost (costFuncGPUCbound / costFuncPI / costFuncEI / costFuncMES) over a box: one discrete pass over the
    candidates on the device (gpx_acq), then SciPy L-BFGS-B from the `nStarts` best distinct candidates at once -- the objective is
    the SUM of the starts' costs over the stacked nStarts x d vector (separable), so every iteration is ONE gpx_acq_grad call.
    The box defaults to the candidates' bounding box; candidates outside it take no part.

    Returns (point (1 x d), cost, discreteIndex): the best polished start when it beats the discrete winner, else the discrete winner
    itself -- the cost is never above the discrete winner's and never NaN.  Deterministic: the same inputs give the same output."""
    allCandidates = np.asarray(candidates, dtype=float)
    d = allCandidates.shape[1]
    lb = np.min(allCandidates, axis=0) if lbounds is None else np.broadcast_to(np.asarray(lbounds, dtype=float), (d,))
    ub = np.max(allCandidates, axis=0) if rbounds is None else np.broadcast_to(np.asarray(rbounds, dtype=float), (d,))
    # candidates outside the box take no part (discreteIndex still counts rows of `candidates`)
    inside = np.flatnonzero(np.all((allCandidates >= lb) & (allCandidates <= ub), axis=1))
    candidates = allCandidates[inside]
    if len(candidates) == 0:
        raise ValueError("optimizeAcquisition: no candidate lies inside the bounds")
    ctx, gp, Z = costFunction._dense(candidates)
    calls = _AcqCalls(ctx, gp)
    best, bestCost, costs = calls.acq(Z, costFunction._acq, costFunction._param())
    if best < 0:
        raise ValueError("optimizeAcquisition: every candidate's cost is NaN")
    # starts: the nStarts best candidates (NaN costs last, ties in index order), duplicates of a chosen row skipped
    order = np.argsort(np.where(np.isnan(costs), np.inf, costs), kind="stable")
    starts = []
    for j in order:
        if len(starts) >= int(nStarts) or np.isnan(costs[j]):
            break
        if not any(np.array_equal(candidates[j], candidates[s]) for s in starts):
            starts.append(int(j))
    k = len(starts)
    x0 = np.clip(candidates[starts], lb, ub).ravel()
    bounds = list(zip(np.tile(lb, k), np.tile(ub, k)))

    def objective(x):
        P = np.ascontiguousarray(np.reshape(x, (k, d)))
        c, g = calls.acq_grad(_dev.points(ctx, P), costFunction._acq, costFunction._param())
        if not np.all(np.isfinite(c)) or not np.all(np.isfinite(g)):   # (var == 0 exactly: steer the line search away)
            return 1e300, np.zeros(k * d)
        return float(np.sum(c)), g.ravel()

    x = _bfgs(objective, x0, bounds=bounds, maxiter=int(maxiter))[0]
    P = np.clip(np.reshape(x, (k, d)), lb, ub)
    j, c = calls.acq(_dev.points(ctx, P), costFunction._acq, costFunction._param(), want_costs=False)[:2]
    if j >= 0 and c < bestCost:
        return P[j:j + 1].copy(), float(c), int(inside[best])
    return candidates[best:best + 1].copy(), float(bestCost), int(inside[best])
