"""CPU: tests/vfe_sample_ref.py pinned -- its identities against vfe_ref's predictor, the linear-map identity, every mutant caught --
and the parts of posterior sampling on VFE models that need no device: the split of the base draws, the shared Thompson bodies and
the refusals on a NumPy stand-in for the device model, the header, the binding and the Makefile."""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as FR
import path_ref as PR
import sample_ref as SR
import vfe_ref
import vfe_sample_ref as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (kind, d, lengths, signalSize, N, nu, noise, seed), as fitc_grad_ref.case takes them
CASES = [("se", 1, [0.1], 1.0, 5, 1, 1e-2, 31), ("matern32", 2, [0.5], 1.4, 9, 3, 1e-2, 32), ("matern52", 3, [0.7], 1.1, 40, 17, 1e-2, 33),
         ("se", 8, [1.0, 1.2, 0.8, 1.5, 0.9, 1.1, 1.3, 0.7], 1.0, 130, 40, 1e-2, 34)]
IDS = ["se-d1-nu1", "m32-d2-nu3", "m52-d3-nu17", "se-d8-nu40"]


def _points(c, S, m=9):
    Z = np.random.default_rng(c[7]).uniform(-1.0, 1.0, (m, c[1]))
    Z[1] = S[0]                                             # ON an inducing point
    return Z


# ---- the reference's identities and its mutants -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [VS.LD, float], ids=["longdouble", "float64"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_identities(c, dtype):
    """With K(J, J) in place of Phi_J Phi_J^T the finite-feature covariance is the exact one, whose diagonal -- and the mean -- are
    vfe_ref.predict's, to 1e-10 relative; J_map J_map^T is the finite-feature covariance; the zero-draw path is the mean."""
    spec, X, S, y, noise = FR.case(c)
    Z = _points(c, S)
    m = VS.model(spec, X, S, y, noise, dtype)
    mu, var = vfe_ref.predict(spec, X, S, y, noise, Z)
    C = VS.exact_cov(spec, S, m, Z, dtype)
    figs = [VS.rel(VS.mean(spec, S, m, Z, dtype), mu), float(np.max(np.abs(np.diag(C) - var)) / np.max(np.abs(C))),
            VS.rel(VS.feature_cov(spec, S, noise, m, None, None, Z, dtype, prior="exact"), C)]
    b = PR.base_draws(spec, 1, 5, 0, seed=1)
    om = PR.frequencies(spec, b["g"], b["u"])
    mean, J = VS.linear_map(VS.unit_paths(spec, S, noise, m, om, b["phase"], Z, dtype))
    figs += [VS.rel(mean, mu), VS.rel(VS.mm(J, J.T, dtype), VS.feature_cov(spec, S, noise, m, om, b["phase"], Z, dtype))]
    print("  mean %.2e  variance %.2e  exact-prior covariance %.2e  zero path %.2e  J J^T %.2e" % tuple(figs))
    assert max(figs) <= 1e-10, figs


@pytest.mark.parametrize("c", CASES[1:], ids=IDS[1:])
def test_mutants_are_caught(c):
    """Every mutant that changes the distribution of V misses the linear-map identity by 1e-6 at least, where it holds to 1e-10; exchanging Xi1 and Xi2
    changes no distribution, and is seen where V itself is compared under one base (as the device's is)."""
    spec, X, S, y, noise = FR.case(c)
    Z = _points(c, S)
    m = VS.model(spec, X, S, y, noise, float)
    b = PR.base_draws(spec, 3, 5, 2 * S.shape[0], seed=2)
    om, cw = PR.frequencies(spec, b["g"], b["u"]), PR.feature_weights(spec, b["w"])
    cref = VS.feature_cov(spec, S, noise, m, om, b["phase"], Z, float)
    nu = S.shape[0]
    V = VS.weights(spec, S, noise, m, cw, om, b["phase"], b["xi"][:, :nu], b["xi"][:, nu:], float)
    for mutant in VS.MUTANTS:
        _, J = VS.linear_map(VS.unit_paths(spec, S, noise, m, om, b["phase"], Z, float, mutant))
        miss = VS.rel(J @ J.T, cref)
        Vm = VS.weights(spec, S, noise, m, cw, om, b["phase"], b["xi"][:, :nu], b["xi"][:, nu:], float, mutant)
        print("  %-14s J J^T misses by %.2e, V by %.2e" % (mutant, miss, VS.rel(Vm, V)))
        assert VS.rel(Vm, V) > 1e-6, mutant                         # (the identities hold to 1e-10)
        assert (miss <= 1e-10) if mutant == "swap" else (miss > 1e-6), mutant


def test_blocked_cholesky_is_chol_ld():
    """The blocked longdouble factorisation the large reference uses, against design_replay_ref.chol_ld itself."""
    A = np.random.default_rng(0).standard_normal((70, 40))
    A = (A @ A.T + 70 * np.eye(70)).astype(VS.LD)
    assert VS.rel(VS.chol(A, VS.LD, nb=16), VS.DR.chol_ld(A)) <= 1e-17


# ---- the Python layer on a NumPy stand-in -------------------------------------------------------------------------------------------------
class _Dev(SR.NumpySampleDevice):
    K_SE, K_MATERN32, K_MATERN52 = 0, 1, 2


class _Paths(object):
    """device.PathSampler's methods from the definitions (float64)."""

    def __init__(self, spec, S, cw, omega, phase, V):
        self.a = (spec, cw, omega, phase, V, S)
        self.S = cw.shape[0]

    def evaluate(self, Z):
        return VS.paths(*self.a, Z, float)

    def argbest(self, Z, minimize=True, want_values=False):
        f = self.evaluate(Z)
        idx = PR.first_argbest(f, minimize).astype(np.int64)
        out = (idx, f[np.arange(len(idx)), idx])
        return out + (f,) if want_values else out

    def gradient(self, Zp, path, want_values=False):
        g = VS.gradient(*self.a, Zp, path, float)
        return (g, self.evaluate(Zp)[path, np.arange(len(path))]) if want_values else g

    def close(self):
        pass


class _Vfe(object):
    """device.VfeModel's three new methods on host arrays (float64 restatement), recording what they were given."""

    def __init__(self, spec, X, S, y, noise):
        self.spec, self.S, self.noise, self.calls = spec, S, noise, []
        self.m = VS.model(spec, X, S, y, noise, float)

    def path_sampler(self, S, coeff, omega, phase, w, eps_u, xi_q):
        self.calls.append(("paths", np.array(eps_u), np.array(xi_q)))
        cw = PR.feature_weights(self.spec, w)
        return _Paths(self.spec, self.S, cw, omega, phase, VS.weights_eps(self.spec, self.S, self.m, cw, omega, phase, eps_u, xi_q, float))

    def posterior_cov(self, Z):
        return VS.exact_cov(self.spec, self.S, self.m, Z, float)

    def posterior(self, coeff, Z, want_mean=True, want_var=True):
        return VS.mean(self.spec, self.S, self.m, Z, float), np.diag(self.posterior_cov(Z)).copy()

    def posterior_sampler(self, coeff, Z, nugget):
        from gpexp_amd import device
        self.calls.append(("psampler", Z.shape[0], float(nugget)))
        if nugget == 0.0 and SR.first_repeated_row(Z):
            raise device._sampler_not_pd(SR.first_repeated_row(Z), 0.0)
        C = self.posterior_cov(Z)
        return SR._NumpySampler(SR.NumpySampleDevice(), self.posterior(coeff, Z)[0], 0.5 * (C + C.T), float(nugget), Z)


class _Space(object):
    def __init__(self, d):
        self.dimension = d


@pytest.fixture
def standin(monkeypatch):
    import gpexp_amd.experimentalDesign as edm
    import gpexp_amd.gp as gpm
    be = _Dev()
    monkeypatch.setattr(gpm, "_dev", be)
    monkeypatch.setattr(edm, "_dev", be)
    return be


CASE = ("matern32", 2, [0.5], 1.4, 40, 11, 1e-2, 5)


def fitted(c=CASE, kernel=None, **kw):
    """A GP that looks trained on the stand-in: host points, the stand-in model, any coefficients."""
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    spec, X, S, y, noise = FR.case(c)
    kw = kw or dict(FITC=0.3, sparse="vfe")
    g = GP(kernel or KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5), noise, **kw)
    g.pts, g._X, g.coeff = X, X, np.zeros(len(y))
    if "FITC" in kw:
        g.fitcnodes, g._fitc = S, _Vfe(spec, X, S, y, noise)
    else:
        g._Ld = object()
    return g, (spec, X, S, y, noise)


def cost_on(g, data, cls=None):
    from gpexp_amd.experimentalDesign import costFuncEI
    cf = object.__new__(cls or costFuncEI)
    cf.space, cf.xTrain, cf.yTrain, cf.gaussianProcess = _Space(data[0]["d"]), data[1], data[3], g
    return cf


def test_base_split_and_path_sampler(standin):
    """A PathBase drawn with nTrain = 2 nu: xi[:, :nu] reaches the model as eps_u = sqrt(noise) Xi1, xi[:, nu:] as xi_q = Xi2."""
    from gpexp_amd.gp import PathBase
    g, (spec, X, S, y, noise) = fitted()
    nu, Z = S.shape[0], _points(CASE, S, 30)
    base = PathBase.draw(4, 16, 2 * nu, 2, g.kernel, rng=3)
    smp = g.vfePathSampler(base=base)
    _, eps_u, xi_q = g._fitc.calls[-1]
    assert np.array_equal(eps_u, np.sqrt(noise) * base.xi[:, :nu]) and np.array_equal(xi_q, base.xi[:, nu:])
    assert smp.base is base and smp.nPaths == 4
    f = smp.evaluate(Z)
    assert f.shape == (4, 30) and np.array_equal(g.vfeSamplePaths(Z, base=base), f)
    om = PR.frequencies(spec, base.g, base.u)
    V = VS.weights(spec, S, noise, g._fitc.m, PR.feature_weights(spec, base.w), om, base.phase, base.xi[:, :nu], base.xi[:, nu:], float)
    assert np.array_equal(f, VS.paths(spec, PR.feature_weights(spec, base.w), om, base.phase, V, S, Z, float))
    smp.close()
    with pytest.raises(ValueError, match="closed"):
        smp.evaluate(Z)
    assert g.vfePathSampler(3, 8).base.nTrain == 2 * nu                     # base=None: drawn with nTrain = 2 nu
    for bad in (PathBase.draw(4, 16, nu, 2, g.kernel, rng=3), PathBase.draw(4, 16, 2 * nu, 3, g.kernel, rng=3),
                PathBase.draw(4, 16, 2 * nu, 2, 0, rng=3)):                  # nTrain = nu; another d; a squared-exponential base
        with pytest.raises(ValueError, match="base was drawn"):
            g.vfePathSampler(base=bad)
    with pytest.raises(ValueError, match="PathBase"):
        g.vfePathSampler(base=np.zeros((4, 2 * nu)))


def test_joint_sampler_covariance_and_thompson(standin):
    from gpexp_amd.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    from gpexp_amd.gp import PathBase
    from gpexp_amd._lib import NotPositiveDefinite
    g, data = fitted()
    spec, X, S, y, noise = data
    Z = _points(CASE, S, 30)
    cov = g.vfePosteriorCovariance(Z)
    assert cov.shape == (30, 30)
    smp = g.vfePosteriorSampler(Z)
    assert g._fitc.calls[-1] == ("psampler", 30, 1e-10 * spec["signalSize"])                 # the default jitter: 1e-10 max k(z, z)
    xi = SR.base_samples(4, 30, seed=8)
    rows = smp.draw(baseSamples=xi)
    assert rows.shape == (4, 30) and np.array_equal(g.vfeSamplePosterior(Z, baseSamples=xi), rows)
    smp.close()
    g.vfePosteriorSampler(Z, jitter=1e-6, addNoise=True).close()
    assert g._fitc.calls[-1][2] == 1e-6 + noise
    for bad in (-1e-12, float("nan")):
        with pytest.raises(ValueError):
            g.vfePosteriorSampler(Z, jitter=bad)
    with pytest.raises(NotPositiveDefinite, match="point 8"):
        g.vfePosteriorSampler(np.vstack([Z[:8], Z[:8]]), jitter=0.0)
    base = PathBase.draw(4, 16, 2 * S.shape[0], 2, g.kernel, rng=3)
    for cls in (costFuncEI, costFuncPI, costFuncGPUCbound):
        cf = cost_on(g, data, cls)
        for minimize in (True, False):
            idx, val = cf.vfeThompsonBatch(Z, 4, baseSamples=xi, minimize=minimize)
            assert idx.dtype == np.int64
            SR.check_argbest(idx, val, rows, minimize)
            pts, vals, ids = cf.vfeThompsonPaths(Z, 4, base=base, minimize=minimize)
            PR.check_argbest(ids, vals, g.vfeSamplePaths(Z, base=base), minimize)
            assert np.array_equal(pts, Z[ids])
            pp, pv, pi = cf.vfeThompsonPaths(Z, 4, base=base, minimize=minimize, polish=True, maxiter=10)
            assert np.array_equal(pi, ids) and (np.all(pv <= vals) if minimize else np.all(pv >= vals))
            assert np.all(pp >= Z.min(axis=0)) and np.all(pp <= Z.max(axis=0))
        assert cf.vfeThompsonBatch(Z, 3)[0].shape == (3,) and cf.vfeThompsonPaths(Z, 2, nFeatures=8)[0].shape == (2, 2)
    with pytest.raises(ValueError, match="no candidate lies inside"):
        cf.vfeThompsonPaths(Z, 2, base=base, polish=True, lbounds=[5.0, 5.0], rbounds=[6.0, 6.0])


def test_refusals(standin, monkeypatch):
    import gpexp_amd.gp as gpm
    from gpexp_amd.kernels import KernelMehlerND
    Z = np.zeros((3, 2))

    def calls(g, cf):
        return (lambda: g.vfePathSampler(2, 8), lambda: g.vfeSamplePaths(Z), lambda: g.vfePosteriorSampler(Z),
                lambda: g.vfeSamplePosterior(Z), lambda: g.vfePosteriorCovariance(Z), lambda: cf.vfeThompsonPaths(Z, 2),
                lambda: cf.vfeThompsonBatch(Z, 2))
    for g, data in (_dense(), fitted(FITC=0.3)):                              # a dense and a FITC model
        for call in calls(g, cost_on(g, data)):
            with pytest.raises(ValueError, match="VFE models"):
                call()
    g, data = fitted()
    g.coeff = None                                                            # nodes set, never trained
    for call in calls(g, cost_on(g, data)):
        with pytest.raises(ValueError, match="trained model"):
            call()
    g, data = fitted(kernel=KernelMehlerND([0.3, 0.5], 2))
    cf = cost_on(g, data)
    for call in (lambda: g.vfePathSampler(2, 8), lambda: g.vfeSamplePaths(Z), lambda: cf.vfeThompsonPaths(Z, 2)):
        with pytest.raises(NotImplementedError, match="spectral density"):
            call()
    g, data = fitted()
    cf = cost_on(g, data)
    # the old names refuse the model as before
    for call in (lambda: g.pathSampler(2, 8), lambda: g.posteriorSampler(Z), lambda: cf.thompsonPaths(Z, 2), lambda: cf.thompsonBatch(Z, 2)):
        with pytest.raises(NotImplementedError, match="FITC / VFE"):
            call()
    with pytest.raises(NotImplementedError, match="VFE model"):
        g.evaluate(Z, compvar=2)
    monkeypatch.setattr(gpm._dist, "session", lambda: object())                # replicated calls: the draws must be given
    for call in (lambda: g.vfePathSampler(2, 8), lambda: g.vfeSamplePaths(Z), lambda: g.vfeSamplePosterior(Z, 2),
                 lambda: cf.vfeThompsonPaths(Z, 2), lambda: cf.vfeThompsonBatch(Z, 2)):
        with pytest.raises(ValueError, match="session"):
            call()


def _dense():
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    spec, X, S, y, noise = FR.case(CASE)
    g = GP(KernelIsoMatern(spec["rho"], spec["signalSize"], 2, nu=1.5), noise)
    g.pts, g._X, g.coeff, g._Ld = X, X, np.zeros(len(y)), object()
    return g, (spec, X, S, y, noise)


# ---- header, binding, Makefile ----------------------------------------------------------------------------------------------------------------
NAMES = ["gpx_vfe_paths_create", "gpx_vfe_posterior_cov", "gpx_vfe_psampler_create"]


def test_header_binding_and_makefile():
    from gpexp_amd import _lib
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert "#define GPX_ABI_VERSION 2" in text
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert name in _lib._SIGS and name in _lib.exported_symbols(), name
    mk = open(os.path.join(ROOT, "gpexp_amd", "csrc", "Makefile")).read()
    for src in ("fitc.hip", "paths.hip", "sample.hip"):                     # where the entries and their bodies live
        assert src in mk
        body = open(os.path.join(ROOT, "gpexp_amd", "csrc", src)).read()
        assert any(n.replace("gpx_", "") in body for n in NAMES), src
    so = os.path.join(ROOT, "gpexp_amd", "libgpx_hip.so")
    if os.path.exists(so):
        lib = _lib.load()
        for name in NAMES:
            assert hasattr(lib, name)


def test_methods_reachable_through_both_import_paths():
    import gpExp.experimentalDesign as shim
    import gpExp.gp as gshim
    import gpexp_amd.experimentalDesign as impl
    for name in ("costFuncGPUCbound", "costFuncPI", "costFuncEI"):
        for m in ("vfeThompsonBatch", "vfeThompsonPaths"):
            assert getattr(getattr(shim, name), m) is getattr(getattr(impl, name), m)
    for m in ("vfePathSampler", "vfeSamplePaths", "vfePosteriorSampler", "vfeSamplePosterior", "vfePosteriorCovariance"):
        assert callable(getattr(gshim.GP, m))
