"""Point gradients of the posterior variance for the isotropic Matern kernels on the device (-m gpu): GP.varianceGradient,
GP.varianceGradientWRTnewpt, costFunctionGP_IVAR.derivative and the design drivers on top of them, against the dense closed
form of tests/matern_pointgrad_ref.py (validated against central differences of the oracle in
tests/test_matern_pointgrad_host.py).  Tolerances are those of tests/test_gpu_f1.py: 1e-9 against the closed form (max-norm
relative, helpers.rel), 1e-8 on FITC, 1e-13 / 1e-12 / 1e-11 for the self-consistency checks the squared-exponential tests
hold to them."""
import os

import numpy as np
import pytest

from helpers import NoiseFunc, rel
import matern_pointgrad_ref as mref

pytestmark = pytest.mark.gpu

RHO, SIG, NOISE = 0.7, 1.3, 0.05          # signalSize != 1: a doubled signalSize (the SE convention) would show
NU = {"matern32": 1.5, "matern52": 2.5}


def kernel_of(kind, d):
    from gpExp.kernels import KernelIsoMatern
    return KernelIsoMatern(RHO, SIG, d, nu=NU[kind])


def dev_spec(kind, d):
    from gpexp_amd import device as dev
    return dev.KernelSpec(dev.K_MATERN32 if kind == "matern32" else dev.K_MATERN52, d, [RHO, SIG])


def space_of(d, nf=None):
    from gpExp.approximation import Space
    return Space(d, lambda size: np.random.rand(size[0], size[1]) * 2 - 1, lambda p: np.ones(len(p)) / 2 ** d, noise=nf)


class cross_bytes(object):
    """GPX_CROSS_BYTES for the duration of a block (the evaluation chunk of the gradient routines)."""

    def __init__(self, value):
        self.value = str(value)

    def __enter__(self):
        self.old = os.environ.get("GPX_CROSS_BYTES")
        os.environ["GPX_CROSS_BYTES"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("GPX_CROSS_BYTES", None)
        else:
            os.environ["GPX_CROSS_BYTES"] = self.old


@pytest.mark.parametrize("with_nf,dups", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("d", [3, 1])
@pytest.mark.parametrize("kind", ["matern32", "matern52"])
def test_small_and_ragged_vs_closed_form(kind, d, with_nf, dups):
    """n = 150 training points (ragged against the 128 tiles), M = 333 evaluation points in chunks of 128 (GPX_CROSS_BYTES);
    d = 3 takes the DMAX = 4 row kernels, d = 1 the DMAX = 1 ones; duplicated training points exercise the coincidence mask."""
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFunctionGP_IVAR
    rng = np.random.default_rng(11 + d)
    n, m = 150, 333
    X = rng.uniform(-1, 1, (n, d))
    if dups:
        X[17] = X[3]
        X[140] = X[3]
    Z = rng.uniform(-1, 1, (m, d))
    nf = NoiseFunc(d) if with_nf else None
    nug = nf(X) if with_nf else NOISE
    want_f, want_n, want_g = mref.gradients(kind, RHO, SIG, X, Z, nug, nf)
    g = GP(kernel_of(kind, d), NOISE)
    g.addNodesAndComputeCovariance(X, noiseIn=(nug if with_nf else None))
    with cross_bytes(3 * 256 * 8 * 128):                      # 128 evaluation points per chunk
        got = g.varianceGradient(Z, noiseFunc=nf)
        gnew = g.varianceGradientWRTnewpt(Z)
    assert got.shape == (n * d, m) and gnew.shape == (m * d,)
    print("full %.2e  newpt %.2e" % (rel(got, want_f), rel(gnew, want_n)))
    assert rel(got, want_f) <= 1e-9
    assert rel(gnew, want_n) <= 1e-9
    assert rel(g.varianceGradient(Z, noiseFunc=nf), got) <= 1e-13           # one chunk == several chunks
    assert rel(g.varianceGradientWRTnewpt(Z), gnew) <= 1e-13
    cf = costFunctionGP_IVAR(GP(kernel_of(kind, d), NOISE), n, space_of(d, nf), mcPoints=Z)
    gi = cf.derivative(X)
    print("ivar %.2e" % rel(gi, want_g))
    assert gi.shape == (n * d,) and rel(gi, want_g) <= 1e-9
    assert rel(gi, want_f.sum(axis=1) / m) <= 1e-9


def test_whole_set_coincidence_branch():
    """ONE evaluation point equal to a training point + noiseFunc: the eval_bias / dk_bias terms (gp.py:318-320)."""
    from gpExp.gp import GP
    rng = np.random.default_rng(3)
    n, d = 150, 3
    X = rng.uniform(-1, 1, (n, d))
    Z = X[41:42].copy()
    nf = NoiseFunc(d)
    want = mref.gradients("matern52", RHO, SIG, X, Z, nf(X), nf)[0]
    plain = mref.gradients("matern52", RHO, SIG, X, Z + 1e-9, nf(X), nf)[0]
    assert rel(plain, want) > 1e-3                            # the branch matters at this point
    g = GP(kernel_of("matern52", d), NOISE)
    g.addNodesAndComputeCovariance(X, noiseIn=nf(X))
    assert rel(g.varianceGradient(Z, noiseFunc=nf), want) <= 1e-9


def test_large_factor_path():
    """From np >= 4096 both solves for beta go through the factor's block inverses and S = beta beta^T runs as slices of its k
    range; n = 4100 (ragged), M = 8200, d = 5 (DMAX = 8), nu = 5/2.  The closed form is first checked at n = 150 through the
    same calls."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    kind, d = "matern52", 5
    sp = dev_spec(kind, d)
    for n, m in ((150, 333), (4100, 8200)):
        rng = np.random.default_rng(n)
        X, Z = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))
        want_f, want_n, want_g = mref.gradients(kind, RHO, SIG, X, Z, NOISE, full_cols=300)
        Xd, Zd = dev.points(ctx, X), dev.points(ctx, Z)
        L = dev.potrf(ctx, dev.kfill(ctx, sp, Xd, nugget=NOISE))
        got_g = np.asarray(dev.ivar_grad(ctx, sp, L, Xd, Zd)).reshape(-1)
        got_n = np.asarray(dev.var_grad_newpt(ctx, sp, L, Xd, Zd)).reshape(-1)
        got_f = dev.var_grad(ctx, sp, L, Xd, dev.points(ctx, Z[:300]))
        print("n = %d: ivar %.2e  newpt %.2e  full %.2e" % (n, rel(got_g, want_g), rel(got_n, want_n), rel(got_f, want_f)))
        assert rel(got_g, want_g) <= 1e-9
        assert rel(got_n, want_n) <= 1e-9
        assert rel(got_f, want_f) <= 1e-9


def test_kept_solve_and_pinned_rows():
    """n = 1100, M = 8300, d = 3, nu = 3/2: the gradient from the forward solve the cost kept (gpx_ivar_grad_w), through the class
    API without a refit, and -- with the last 150 points moved and the others pinned -- for the free rows alone
    (gpx_ivar_grad_rows)."""
    from gpexp_amd import device as dev
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFunctionGP_IVAR
    ctx = dev.context()
    kind, n, m, d = "matern32", 1100, 8300, 3
    rng = np.random.default_rng(n + m)
    X, Z = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))
    sp = dev_spec(kind, d)
    Xd, Zd = dev.points(ctx, X), dev.points(ctx, Z)
    L = dev.potrf(ctx, dev.kfill(ctx, sp, Xd, nugget=NOISE))
    cost, W = dev.ivar(ctx, sp, L, Xd, Zd, keep=True)
    assert W is not None
    g0 = dev.ivar_grad(ctx, sp, L, Xd, Zd)
    assert rel(g0, mref.gradients(kind, RHO, SIG, X, Z, NOISE, full_cols=1)[2]) <= 1e-9
    assert rel(dev.ivar_grad(ctx, sp, L, Xd, Zd, W=W), g0) <= 1e-12
    del W
    cf = costFunctionGP_IVAR(GP(kernel_of(kind, d), NOISE), n, space_of(d), mcPoints=Z)
    c1 = cf.evaluate(X)
    assert cf._w_kept is not None and c1 == pytest.approx(abs(cost), rel=1e-13)
    kept_factor = cf.gaussianProcess._L
    g1 = cf.derivative(X)
    assert cf.gaussianProcess._L is kept_factor and cf._w_kept[0] is kept_factor     # no refit; the kept solve stays
    assert rel(g1, g0) <= 1e-12
    # the batch loop: the last points move, the refit and the kept solve keep their leading rows
    X3 = X.copy()
    X3[-150:] = rng.uniform(-1, 1, (150, d))
    W_before = cf._w_kept[1]
    cf.evaluate(X3)
    assert cf.gaussianProcess._last_refit is not None and cf._w_kept[1] is W_before
    f3 = costFunctionGP_IVAR(GP(kernel_of(kind, d), NOISE), n, space_of(d), mcPoints=Z)
    f3.gaussianProcess.reuseFactor = False
    g_full = f3.derivative(X3)
    assert rel(cf.derivative(X3), g_full) <= 1e-11
    cf.pinnedPoints = n - 150
    r0 = ((n - 150) // 128) * 128
    g_free = cf.derivative(X3)
    assert np.all(g_free[:r0 * d] == 0.0) and np.any(g_free[r0 * d:] != 0.0)
    assert rel(g_free[r0 * d:], g_full[r0 * d:]) <= 1e-11


def test_fitc_model():
    """n = 150, FITC = 0.5, nu = 5/2: the same closed form with the FITC (Woodbury) precision, FitcModel.dense(prec=True)."""
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFunctionGP_IVAR
    kind, n, m, d = "matern52", 150, 333, 3
    rng = np.random.default_rng(8)
    X, Z = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))
    np.random.seed(4)
    g = GP(kernel_of(kind, d), NOISE, FITC=0.5)
    g.addNodesAndComputeCovariance(X)
    assert g.fitcnodes.shape == (75, d)
    want_f, want_n, _ = mref.gradients(kind, RHO, SIG, X, Z, None, prec=g._fitc.dense(cov=False, prec=True)[1])
    got = g.varianceGradient(Z)
    assert got.shape == want_f.shape and rel(got, want_f) <= 1e-8
    assert rel(g.varianceGradientWRTnewpt(Z), want_n) <= 1e-8
    cf = costFunctionGP_IVAR(GP(kernel_of(kind, d), NOISE, FITC=0.5), n, space_of(d), mcPoints=Z)
    gi = cf.derivative(X)
    P = cf.gaussianProcess._fitc.dense(cov=False, prec=True)[1]           # (the cost function's GP drew its own inducing points)
    assert rel(gi, mref.gradients(kind, RHO, SIG, X, Z, None, prec=P)[2]) <= 1e-8


def test_slsqp_driver_on_a_matern_gp():
    """ExperimentalDesignDerivative.begin, unchanged, on a Matern-5/2 GP: it returns, and the IVAR cost at the result is not
    above the cost at the start."""
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFunctionGP_IVAR, ExperimentalDesignDerivative
    d, npts = 2, 6
    rng = np.random.default_rng(21)
    Z = rng.uniform(-1, 1, (200, d))
    start = rng.uniform(-0.5, 0.5, (npts, d))
    cf = costFunctionGP_IVAR(GP(kernel_of("matern52", d), NOISE), npts, space_of(d), mcPoints=Z)
    c0 = cf.evaluate(start)
    design = ExperimentalDesignDerivative(cf, npts, d).begin([start], -np.ones(npts * d), np.ones(npts * d))
    assert design.shape == (npts, d) and np.all(np.abs(design) <= 1.0 + 1e-12)
    assert cf.evaluate(design) <= c0


def test_gates_kept_and_reference_conventions_unchanged():
    """The reference-named methods still refuse a Matern GP; KernelMehlerND (d = 2) is refused by the new names too; for the
    squared exponential the new names return exactly what the reference-named methods return."""
    from gpExp.gp import GP
    from gpExp.kernels import KernelMehlerND, KernelSquaredExponential
    X = np.random.default_rng(0).uniform(-1, 1, (9, 2))
    g = GP(kernel_of("matern52", 2), 0.01)
    g.addNodesAndComputeCovariance(X)
    with pytest.raises(AttributeError):
        g.evaluateVarianceDerivative(X[:3])
    with pytest.raises(AttributeError):
        g.evaluateVarianceDerivWRTnewpt(X[:3])
    assert g.varianceGradient(X[:3]).shape == (18, 3)
    g2 = GP(KernelMehlerND([0.5, 0.3], 2), 0.01)
    g2.addNodesAndComputeCovariance(X)
    with pytest.raises(AttributeError):
        g2.varianceGradient(X[:3])
    with pytest.raises(AttributeError):
        g2.varianceGradientWRTnewpt(X[:3])
    g3 = GP(KernelSquaredExponential([0.5, 0.8], 1.3, 2), 0.01)
    g3.addNodesAndComputeCovariance(X)
    nf = NoiseFunc(2)
    assert np.array_equal(g3.varianceGradient(X[:3] + 0.1, noiseFunc=nf), g3.evaluateVarianceDerivative(X[:3] + 0.1, noiseFunc=nf))
    assert np.array_equal(g3.varianceGradientWRTnewpt(X[:3] + 0.1), g3.evaluateVarianceDerivWRTnewpt(X[:3] + 0.1))
