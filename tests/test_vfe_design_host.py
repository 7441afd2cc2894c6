"""The NumPy forms behind IVAR design on a VFE model (tests/vfe_design_ref.py) tied to each other and to something that needs no
closed form -- the gradient to a directional central difference of the direct cost, the new-point derivative to central differences
of vfe_ref.predict's variance -- and the host logic of costFunctionVFE_IVAR on a NumPy double of device.VfeDesign.  No device.

Cases: the six of fitc_grad_ref (Z as tests/test_gpu_vfe.py draws it: 300 points, five of them training points) and the 15 of
grad_dims_cases.PARAMS (its X, S, Z, noise)."""
import functools
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as ref
import grad_dims_cases as gd
import vfe_design_ref as dref
import vfe_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCASES = dict(zip(ref.IDS, ref.CASES))
ALL = list(ref.IDS) + list(gd.IDS)
ENTRIES = ("gpx_vfe_design_create", "gpx_vfe_design_pin", "gpx_vfe_design_eval", "gpx_vfe_design_shape", "gpx_vfe_design_free",
           "gpx_vfe_var_grad", "gpx_vfe_var_grad_newpt")


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, noise, Z): drawn once, read-only."""
    if cid in FCASES:
        spec, X, S, _, noise = ref.case(FCASES[cid])
        Z = np.random.default_rng(31).uniform(-1.2, 1.2, (300, spec["d"]))
        Z[:5] = X[:5]
    else:
        c = gd.case(*gd.PARAMS[gd.IDS.index(cid)])
        spec, X, S, noise, Z = c.spec, c.X, c.S, c.noise, c.Z
    for a in (X, S, Z):
        a.setflags(write=False)
    return spec, X, S, noise, Z


@pytest.mark.parametrize("cid", ALL)
def test_the_forms_agree(cid):
    """`grad` against the column mean of `var_grad`, `gram_path` (all free, and split 128 / rest or 1 / rest) against `cost` and
    `grad`: 1e-10 of signalSize and 1e-10 of the largest |entry| (measured on all 21 cases: cost <= 7.7e-14, mean of var_grad
    <= 2.4e-13, gram-path gradient <= 6.3e-11)."""
    spec, X, S, noise, Z = problem(cid)
    s = spec["signalSize"]
    G = dref.grad(spec, X, S, noise, Z)
    c = dref.cost(spec, X, S, noise, Z)
    full = dref.var_grad(spec, X, S, noise, Z)
    gmax = np.max(np.abs(G))
    e_mean = np.max(np.abs(full.mean(axis=1) - G.ravel())) / gmax
    c1, g1 = dref.gram_path(spec, None, X, S, noise, Z)
    r0 = 128 if X.shape[0] > 200 else 1
    c2, g2 = dref.gram_path(spec, X[:r0], X[r0:], S, noise, Z)
    e_c = max(abs(c1 - c), abs(c2 - c)) / s
    e_g = max(np.max(np.abs(g1 - G)), np.max(np.abs(g2 - G[r0:]))) / gmax
    print("%s: mean of var_grad %.2e; gram path cost %.2e gradient %.2e" % (cid, e_mean, e_c, e_g))
    assert full.shape == (X.size, Z.shape[0]) and G.shape == X.shape and g2.shape == (X.shape[0] - r0, X.shape[1])
    assert e_mean <= 1e-10 and e_c <= 1e-10 and e_g <= 1e-10, (e_mean, e_c, e_g)


@pytest.mark.parametrize("cid", ALL)
def test_gradient_against_a_directional_central_difference(cid):
    """Along V = sign(grad), h = 1e-5, relative to sum |grad|: 1e-6, the project's central-difference figure (measured <= 8.1e-8 on
    all 21 cases).  Directional, because single entries are ~1e-5 of the cost: per-entry differences of the cost do not resolve
    them (measured up to 2.5e-5 of the largest entry on the sweep cases)."""
    spec, X, S, noise, Z = problem(cid)
    G = dref.grad(spec, X, S, noise, Z)
    V = np.sign(G)
    fd = dref.directional_fd(lambda P: dref.cost(spec, P, S, noise, Z), np.array(X), V, 1e-5)
    total = float(np.sum(np.abs(G)))
    err = abs(fd - float(np.sum(G * V))) / total
    print("%s: directional difference %.2e (sum |grad| %.3e)" % (cid, err, total))
    assert total > 0.0 and err <= 1e-6, err


@pytest.mark.parametrize("cid", ALL)
def test_new_point_derivative_against_central_differences(cid):
    """Per entry against central differences of vfe_ref.predict's variance, h = 1e-5, 1e-6 of the largest entry: the figure
    tests/test_vfe_acq_host.py holds for the same quantity (measured <= 9.2e-9)."""
    spec, X, S, noise, Z = problem(cid)
    Z = np.array(Z[:40])
    y = np.zeros(X.shape[0])
    g = dref.var_grad_newpt(spec, X, S, noise, Z).reshape(Z.shape)
    fd = np.empty(Z.shape)
    for l in range(Z.shape[1]):
        e = np.zeros(Z.shape[1])
        e[l] = 1e-5
        fd[:, l] = (vref.predict(spec, X, S, y, noise, Z + e)[1] - vref.predict(spec, X, S, y, noise, Z - e)[1]) / 2e-5
    err = float(np.max(np.abs(g - fd)) / np.max(np.abs(fd)))
    print("%s: new-point derivative against central differences %.2e" % (cid, err))
    assert err <= 1e-6, err


# ---- the class, on the NumPy double ---------------------------------------------------------------------------------------------------
@pytest.fixture
def host_device(monkeypatch):
    from gpexp_amd import experimentalDesign as ed
    monkeypatch.setattr(ed._dev, "VfeDesign", dref.NumpyVfeDesign, raising=False)
    monkeypatch.setattr(ed._dev, "context", lambda: None)
    monkeypatch.setattr(ed._dev, "points", lambda ctx, x: dref.HostPoints(x))
    for k in dref.NumpyVfeDesign.calls:
        dref.NumpyVfeDesign.calls[k] = 0
    return ed, dref.NumpyVfeDesign.calls


def make_gp(spec, noise, **kw):
    from gpexp_amd.kernels import KernelIsoMatern, KernelSquaredExponential
    from gpexp_amd.gp import GP
    if spec["kind"] == "se":
        k = KernelSquaredExponential(list(spec["cl"]), spec["signalSize"], spec["d"])
    else:
        k = KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)
    return GP(k, noise, **kw)


def small(cid="se-d1-nu40", n=12, m=50):
    from gpexp_amd.approximation import Space
    spec, X, S, noise, Z = problem(cid)
    d = spec["d"]
    space = Space(d, lambda size: np.random.default_rng(1).uniform(-1, 1, size), lambda p: np.ones(len(p)))
    gp = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    gp.fitcnodes = np.array(S[:10])
    return spec, np.array(X[:n]), gp, space, np.array(Z[:m]), noise


def test_constructor_refuses_a_model_without_vfe_or_without_inducing_points(host_device):
    ed, _ = host_device
    spec, X, gp, space, Z, noise = small()
    for other in (make_gp(spec, noise), make_gp(spec, noise, FITC=0.5)):
        other.fitcnodes = gp.fitcnodes
        with pytest.raises(ValueError, match="VFE"):
            ed.costFunctionVFE_IVAR(other, len(X), space, mcPoints=Z)
    with pytest.raises(ValueError, match="fitcnodes"):
        ed.costFunctionVFE_IVAR(make_gp(spec, noise, FITC=0.5, sparse="vfe"), len(X), space, mcPoints=Z)
    assert issubclass(ed.costFunctionVFE_IVAR, ed.costFunctionGP_IVAR)


def test_values_pinned_zeros_and_one_device_call_per_design(host_device):
    ed, calls = host_device
    spec, X, gp, space, Z, noise = small()
    S = gp.fitcnodes
    cf = ed.costFunctionVFE_IVAR(gp, len(X), space, mcPoints=Z)
    assert calls == {"create": 0, "pin": 0, "eval": 0}                      # lazy
    c = cf.evaluate(X)
    g = cf.derivative(X)
    assert calls == {"create": 1, "pin": 1, "eval": 1}                      # the pair at one design: one device call
    assert abs(c - abs(dref.cost(spec, X, S, noise, Z))) <= 1e-10 * spec["signalSize"]
    G = dref.grad(spec, X, S, noise, Z)
    assert g.shape == (X.size,) and np.max(np.abs(g - G.ravel())) <= 1e-10 * np.max(np.abs(G))
    c2, g2 = cf.evaluateWithDerivative(X)
    assert c2 == c and np.array_equal(g2, g) and calls["eval"] == 1
    # pinned leading points: zeros in their entries, the free rows' gradient, pin once while the block is unchanged
    cf.pinnedPoints = 5
    gp_ = cf.derivative(X)
    assert np.all(gp_[:5 * X.shape[1]] == 0.0)
    assert np.max(np.abs(gp_[5 * X.shape[1]:] - G[5:].ravel())) <= 1e-10 * np.max(np.abs(G))
    assert calls["pin"] == 2 and calls["create"] == 1
    X2 = X.copy()
    X2[7:] += 0.01
    cf.evaluate(X2)
    cf.derivative(X2)
    assert calls["pin"] == 2 and calls["eval"] == 3
    X3 = X2.copy()
    X3[0] += 0.01
    cf.evaluate(X3)
    assert calls["pin"] == 3
    # the GP copy is not touched
    assert cf.gaussianProcess.pts is None and cf.gaussianProcess._fitc is None


def test_state_is_rebuilt_when_its_inputs_change(host_device):
    ed, calls = host_device
    spec, X, gp, space, Z, noise = small()
    cf = ed.costFunctionVFE_IVAR(gp, len(X), space, mcPoints=Z)
    c0 = cf.evaluate(X)
    cf.mcPoints = Z[:30]
    c1 = cf.evaluate(X)
    assert calls["create"] == 2 and c1 != c0
    assert abs(c1 - abs(dref.cost(spec, X, gp.fitcnodes, noise, Z[:30]))) <= 1e-10 * spec["signalSize"]
    hp = dict(cf.gaussianProcess.kernel.hyperParam)
    hp["signalSize"] = 2.0 * spec["signalSize"]
    cf.gaussianProcess.kernel.updateHyperParameters(hp)
    c2 = cf.evaluate(X)
    assert calls["create"] == 3 and c2 != c1
    cf.gaussianProcess.noise = 2.0 * noise
    cf.evaluate(X)
    assert calls["create"] == 4
    cf.gaussianProcess.fitcnodes = cf.gaussianProcess.fitcnodes + 0.01
    cf.evaluate(X)
    assert calls["create"] == 5
    cf.evaluate(X)
    assert calls["create"] == 5
    cf.reset()
    cf.evaluate(X)
    assert calls["create"] == 6


def test_per_point_noise_is_refused(host_device):
    ed, _ = host_device
    spec, X, gp, space, Z, noise = small()
    space.noiseFunc = lambda p: np.full(len(p), 0.1)
    cf = ed.costFunctionVFE_IVAR(gp, len(X), space, mcPoints=Z)
    with pytest.raises(NotImplementedError, match="noise"):
        cf.evaluate(X)
    with pytest.raises(NotImplementedError, match="noise"):
        cf.derivative(X)


def test_batch_driver_builds_the_cost_of_its_own_class(host_device, monkeypatch):
    ed, calls = host_device
    spec, X, gp, space, Z, noise = small()
    seen = []

    def fake(self, nodesKeep=None, lbounds=[], rbounds=[]):
        seen.append((type(self.costFunction), self.costFunction.pinnedPoints, self.nPoints))
        return np.vstack([nodesKeep, X[len(nodesKeep):self.nPoints]])

    monkeypatch.setattr(ed.ExperimentalDesignDerivative, "beginWithVarGreedy", fake)
    cf = ed.costFunctionVFE_IVAR(gp, 4, space, mcPoints=Z)
    pts = ed.ExperimentalDesignGreedyWithDerivatives(cf, 8, 4, spec["d"]).begin()
    assert seen == [(ed.costFunctionVFE_IVAR, 0, 4), (ed.costFunctionVFE_IVAR, 4, 8)]
    assert np.array_equal(pts, X[:8])


def test_declarations():
    from gpexp_amd import _lib, device
    header = open(os.path.join(ROOT, "include", "gpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, code), name
    assert "typedef struct gpx_vfe_design gpx_vfe_design;" in code
    assert "#define GPX_ABI_VERSION 2" in header
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert [len(_lib._SIGS[n][1]) for n in ENTRIES] == [9, 3, 5, 4, 2, 10, 5]
    for meth in ("design_var_grad", "design_var_grad_newpt"):
        assert callable(getattr(device.VfeModel, meth)) and not hasattr(device.FitcModel, meth)
    for meth in ("pin", "eval", "shape", "__del__"):
        assert callable(getattr(device.VfeDesign, meth))
    if os.path.exists(_lib.LIB_PATH):
        assert all(hasattr(_lib.load(), n) for n in ENTRIES)
