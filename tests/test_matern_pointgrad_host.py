"""CPU tests of the Matern point gradients: the closed form the GPU tests compare against (tests/matern_pointgrad_ref.py)
is the derivative of what the oracle computes -- central differences (h = 1e-5) of `oracle.posterior(..., compvar=1)` and
`oracle.ivar` on refitted models, bound 2e-6 as for the project's other central differences (measured: 2.5e-9) -- and
`KernelIsoMatern.pointDerivative` is the derivative of `oracle.kernel_eval`."""
import numpy as np
import pytest

from oracle import gpexp_oracle as orc
from helpers import rel
import matern_pointgrad_ref as mref

RHO, SIG, NUG, H = 0.7, 1.3, 0.05, 1e-5
CASES = [(9, 7, 2), (40, 60, 3)]
KINDS = ["matern32", "matern52"]
NU = {"matern32": 1.5, "matern52": 2.5}


def points(n, m, d):
    rng = np.random.default_rng(100 * n + d)
    return rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))


def variance(spec, X, Z):
    return orc.posterior(spec, orc.fit(spec, X, None, NUG), Z, compvar=1)[1]


@pytest.mark.parametrize("n,m,d", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_is_the_derivative_of_the_oracle_variance(kind, n, m, d):
    X, Z = points(n, m, d)
    spec = mref.spec_of(kind, RHO, SIG, d)
    full, newpt, ivar = mref.gradients(kind, RHO, SIG, X, Z, NUG)
    fd_full, fd_ivar = np.zeros((n * d, m)), np.zeros(n * d)
    for j in range(n):
        for l in range(d):
            Xp, Xm = X.copy(), X.copy()
            Xp[j, l] += H
            Xm[j, l] -= H
            vp, vm = variance(spec, Xp, Z), variance(spec, Xm, Z)
            fd_full[j * d + l] = (vp - vm) / (2 * H)
            # orc.ivar is |mean var|; the variances are positive here
            fd_ivar[j * d + l] = (orc.ivar(spec, Xp, Z, NUG) - orc.ivar(spec, Xm, Z, NUG)) / (2 * H)
            assert np.all(vp > 0) and np.all(vm > 0)
    fd_new = np.zeros((m, d))
    model = orc.fit(spec, X, None, NUG)
    for l in range(d):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[:, l] += H
        Zm[:, l] -= H
        fd_new[:, l] = (orc.posterior(spec, model, Zp)[1] - orc.posterior(spec, model, Zm)[1]) / (2 * H)
    print("closed form vs central differences: full %.2e  ivar %.2e  newpt %.2e"
          % (rel(full, fd_full), rel(ivar, fd_ivar), rel(newpt, fd_new.reshape(-1))))
    assert full.shape == (n * d, m) and newpt.shape == (m * d,) and ivar.shape == (n * d,)
    assert rel(full, fd_full) <= 2e-6
    assert rel(ivar, fd_ivar) <= 2e-6
    assert rel(ivar, full.mean(axis=1)) <= 1e-12            # (the helper sums it through S = beta beta^T)
    assert rel(newpt, fd_new.reshape(-1)) <= 2e-6


@pytest.mark.parametrize("kind", KINDS)
def test_helper_kernel_is_the_oracle_kernel(kind):
    X, Z = points(9, 7, 2)
    spec = mref.spec_of(kind, RHO, SIG, 2)
    assert rel(mref.kmat(kind, RHO, SIG, Z, X), orc.cross_matrix(spec, Z, X)) <= 1e-15


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_point_derivative_of_the_kernel_class(kind, d):
    """KernelIsoMatern.pointDerivative: central differences of oracle.kernel_eval, the helper's closed form, 0 at x1 = x2,
    the shape rules of KernelSquaredExponential.derivative -- and the name `derivative` stays absent."""
    from gpExp.kernels import KernelIsoMatern
    k = KernelIsoMatern(RHO, SIG, d, nu=NU[kind])
    assert not hasattr(k, "derivative")
    spec = mref.spec_of(kind, RHO, SIG, d)
    rng = np.random.default_rng(d)
    x1, x2 = rng.uniform(-1, 1, (11, d)), rng.uniform(-1, 1, (1, d))
    got = k.pointDerivative(x1, x2)
    assert got.shape == (11, d)
    fd = np.zeros((11, d))
    for l in range(d):
        xp, xm = x1.copy(), x1.copy()
        xp[:, l] += H
        xm[:, l] -= H
        fd[:, l] = (orc.kernel_eval(spec, xp, x2) - orc.kernel_eval(spec, xm, x2)) / (2 * H)
    assert rel(got, fd) <= 2e-6
    assert rel(got, mref.dkmat(kind, RHO, SIG, x1, x2)[:, 0, :]) <= 1e-14
    at = k.pointDerivative(np.vstack((x2, x1[:1])), x2)
    assert np.all(at[0] == 0.0) and np.all(np.isfinite(at))
    with pytest.raises(AssertionError):
        k.pointDerivative(x1, x1[:2])                      # x2 must be ONE point
    with pytest.raises(AssertionError):
        k.pointDerivative(x1[0], x2)                       # nd arrays only
    with pytest.raises(AssertionError):
        k.pointDerivative(np.zeros((3, d + 1)), x2)


def test_gates_of_the_gp_methods_without_a_device():
    """The reference-named methods keep their gate for Matern; the new names refuse KernelMehlerND (d > 1).  The gate is
    host logic in front of any device work, so a stand-in for the fitted state is enough."""
    from gpExp.gp import GP
    from gpExp.kernels import KernelIsoMatern, KernelMehlerND
    X = np.random.default_rng(0).uniform(-1, 1, (9, 2))
    g = GP(KernelIsoMatern(RHO, SIG, 2, nu=2.5), NUG)
    g.pts, g._Ld = X, object()
    with pytest.raises(AttributeError):
        g._point_derivative_ready(X[:3])
    g._point_derivative_ready(X[:3], referenceOnly=False)
    g2 = GP(KernelMehlerND([0.5, 0.3], 2), NUG)
    g2.pts, g2._Ld = X, object()
    for ref_only in (True, False):
        with pytest.raises(AttributeError):
            g2._point_derivative_ready(X[:3], referenceOnly=ref_only)
