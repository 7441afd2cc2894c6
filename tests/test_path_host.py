"""CPU: tests/path_ref.py pinned -- the spectral scaling of gpexp_amd.paths against the kernels themselves, the closed-form
distribution of the paths, the identities, every mutant caught by the comparator aimed at it, the float64 replay inside the cap the
device is held to -- and the parts of the Python layer that need no device: PathBase, the refusals, the header and the binding."""
import os
import re

import numpy as np
import pytest

import path_ref as PR
import sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("se", "matern32", "matern52")


# ---- 1: the spectral scaling ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_spectral_scaling(kind, d):
    """Phi Phi^T -> K: with L = 65536 features every entry over 12 points is within the Hoeffding figure (0.058; measured 0.008 ..
    0.014).  A Matern kernel's frequencies drawn as a squared exponential's miss it."""
    spec, L = SR.kernel_spec(kind, d), 65536
    b = PR.base_draws(spec, 1, L, 0, seed=100 + d)
    # 12 points on a line, 0.105 apart: the pair distances walk 0.15 rho .. 1.65 rho, through 0.9 rho where a Matern kernel and the
    # squared exponential of the same length differ most (0.12 for nu = 3/2, 0.083 for nu = 5/2) -- random points in [-1, 1]^8 are
    # all far apart, every kernel is 0 between them and no scaling could be told from another
    Z = (np.arange(12.0) - 5.5)[:, None] * 0.105 * np.ones((1, d)) / np.sqrt(d)
    t = PR.hoeffding_t(12 * 12, L)      # 0.0568 for the 144 entries
    assert t <= 0.058
    err = PR.feature_gram_error(spec, PR.frequencies(spec, b["g"], b["u"]), b["phase"], Z)
    print("  %s d=%d: max |Phi Phi^T - K| / sig = %.4f (t = %.4f)" % (kind, d, err, t))
    assert err <= t
    if kind != "se":
        bad = PR.feature_gram_error(spec, PR.frequencies(spec, b["g"], b["u"], mutant="matern_as_se"), b["phase"], Z)
        assert bad > t, (kind, d, bad)


def test_product_scaling_is_the_reference_scaling():
    """gpexp_amd.paths.spectralFrequencies, from the flat hyper-parameters the device is given, equals path_ref.frequencies bit for bit."""
    from gpexp_amd import device as dev
    from gpexp_amd.paths import PathBase, spectralFrequencies
    import kernel_reference as KR
    import posterior_ref as P
    for kind in KINDS:
        spec = SR.kernel_spec(kind, 3)
        ks = dev.KernelSpec(P.KIND_ID[kind], 3, KR.hyp_of(spec))
        b = PathBase.draw(2, 33, 5, 3, ks, rng=3)
        assert (b.u is None) == (kind == "se") and b.g.shape == (33, 3) and b.w.shape == (2, 33) and b.xi.shape == (2, 5)
        assert np.all((b.phase >= 0.0) & (b.phase < 2.0 * np.pi))
        assert np.array_equal(spectralFrequencies(ks, b.g, b.u), PR.frequencies(spec, b.g, b.u))
        b2 = PathBase.draw(2, 33, 5, 3, ks, rng=3)
        assert all(np.array_equal(getattr(b, k), getattr(b2, k)) for k in ("g", "phase", "w", "xi"))
        r = b.rows([1])
        assert np.array_equal(r.w, b.w[1:2]) and np.array_equal(r.xi, b.xi[1:2]) and r.g is not None
    with pytest.raises(NotImplementedError):
        PathBase.draw(1, 4, 0, 2, dev.K_MEHLER)
    with pytest.raises(ValueError):
        PathBase(np.zeros((4, 2)), None, np.zeros(4), np.zeros((2, 5)), np.zeros((2, 3)))


# ---- 2: the distribution ---------------------------------------------------------------------------------------------------------------
def _dist_case():
    spec = SR.kernel_spec("matern52", 2)
    rng = np.random.default_rng(11)
    X = rng.uniform(-1.0, 1.0, (8, 2))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(8)
    Z = rng.uniform(-1.0, 1.0, (5, 2))
    Z[0] = X[0]                       # ON a training point: there the noise draw carries nearly all of the variance
    return spec, X, y, Z, 1e-2, PR.base_draws(spec, 20000, 512, 8, seed=12)


def _dist_samples(case, mutant=None):
    spec, X, y, Z, noise, b = case
    om = PR.frequencies(spec, b["g"], b["u"])
    c = PR.feature_weights(spec, b["w"], mutant)
    V = PR.update_weights(spec, X, y, noise, c, om, b["phase"], np.sqrt(noise) * b["xi"], float, mutant)
    return PR.paths(spec, c, om, b["phase"], V, X, Z, float)


def test_distribution_and_its_mutants():
    """20000 paths at fixed features: sample mean against G y and sample covariance against A (Phi_J Phi_J^T) A^T + noise G G^T,
    each within 6 standard errors (measured: 1.7 and 1.6 at most).  Every V / eps / amplitude mutant misses."""
    case = _dist_case()
    spec, X, y, Z, noise, b = case
    mean, cov = PR.path_distribution(spec, X, y, noise, PR.frequencies(spec, b["g"], b["u"]), b["phase"], Z)
    zm, zc = PR.distribution_z(_dist_samples(case), mean, cov)
    print("  distribution: mean %.2f, covariance %.2f standard errors" % (zm, zc))
    assert zm <= 6.0 and zc <= 6.0
    for mutant in ("amplitude", "no_eps", "plus"):
        zm, zc = PR.distribution_z(_dist_samples(case, mutant), mean, cov)
        print("  mutant %-10s mean %.2f, covariance %.2f standard errors" % (mutant, zm, zc))
        assert max(zm, zc) > 6.0, mutant


# ---- 3: identities, and the float64 replay inside the device's cap ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_identities_and_f64_replay_inside_the_cap(kind):
    c0 = SR.points_case(kind, 40, 17, 3, 1e-2)
    spec, X, y, Z, noise = c0["spec"], c0["X"], c0["y"], c0["Z"], c0["noise"]
    b = PR.base_draws(spec, 3, 65, 40, seed=5)
    om = PR.frequencies(spec, b["g"], b["u"])
    # w = 0 and xi = 0: the posterior mean
    zero = np.zeros_like(b["w"])
    V0 = PR.update_weights(spec, X, y, noise, zero, om, b["phase"], 0.0 * b["xi"])
    K = SR.cov_f64(spec, X)
    K[np.diag_indices_from(K)] += noise
    coeff = np.linalg.solve(K, y)
    assert np.array_equal(V0, np.tile(coeff, (3, 1)))
    f0 = PR.paths(spec, zero, om, b["phase"], V0, X, Z, float)
    mean_ld = (PR.LD(1) * coeff) @ PR._cov(spec, X, Z, PR.LD)
    PR.check_within(f0, mean_ld[None, :], PR.value_bound(spec, zero, om, b["phase"], V0, X, Z), "%s mean identity" % kind)
    # prior paths have no update
    assert np.array_equal(PR.paths(spec, zero, om, b["phase"], None, None, Z, float), np.zeros((3, 17)))
    # the float64 replay sits inside the cap the device is held to (values and gradients), from the same V
    c = PR.feature_weights(spec, b["w"])
    V = PR.update_weights(spec, X, y, noise, c, om, b["phase"], np.sqrt(noise) * b["xi"])
    bound = PR.value_bound(spec, c, om, b["phase"], V, X, Z)
    PR.check_within(PR.paths(spec, c, om, b["phase"], V, X, Z, float), PR.paths(spec, c, om, b["phase"], V, X, Z), bound,
                    "%s float64 replay" % kind)
    path = np.arange(17) % 3
    gb = PR.gradient_bound(spec, c, om, b["phase"], V, X, Z, path)
    PR.check_within(PR.gradient(spec, c, om, b["phase"], V, X, Z, path, float), PR.gradient(spec, c, om, b["phase"], V, X, Z, path),
                    gb, "%s float64 gradient replay" % kind)
    # the replayed gradient is the derivative of the replayed value (central differences in longdouble, h = 1e-5)
    h = 1e-5
    g = PR.gradient(spec, c, om, b["phase"], V, X, Z, path)
    for l in range(3):
        E = np.zeros((1, 3))
        E[0, l] = h
        fd = (PR.paths(spec, c, om, b["phase"], V, X, Z + E)[path, np.arange(17)] -
              PR.paths(spec, c, om, b["phase"], V, X, Z - E)[path, np.arange(17)]) / (2 * h)
        on_point = np.any(np.all(Z[:, None, :] == X[None, :, :], axis=2), axis=1)     # Matern 3/2 has no third derivative there
        scale = np.max(np.abs(g)) + 1.0
        tol = np.where(on_point & (kind == "matern32"), 1e-3, 1e-6) * scale
        assert np.all(np.abs(fd - g[:, l]).astype(float) <= tol), (kind, l, float(np.max(np.abs(fd - g[:, l]))))


# ---- 4: every comparator catches the mutants aimed at it -------------------------------------------------------------------------------
def test_mutants_are_caught():
    c0 = SR.points_case("matern32", 40, 17, 2, 1e-2)
    spec, X, y, Z, noise = c0["spec"], c0["X"], c0["y"], c0["Z"], c0["noise"]
    b = PR.base_draws(spec, 3, 65, 40, seed=6)
    om = PR.frequencies(spec, b["g"], b["u"])
    c = PR.feature_weights(spec, b["w"])
    V = PR.update_weights(spec, X, y, noise, c, om, b["phase"], np.sqrt(noise) * b["xi"])
    ref, bound = PR.paths(spec, c, om, b["phase"], V, X, Z), PR.value_bound(spec, c, om, b["phase"], V, X, Z)
    for mutant in ("phase", "next_path"):
        with pytest.raises(AssertionError):
            PR.check_within(PR.paths(spec, c, om, b["phase"], V, X, Z, float, mutant), ref, bound, mutant)
    with pytest.raises(AssertionError):      # amplitude sqrt(1 / L): through the feature weights
        PR.check_within(PR.paths(spec, PR.feature_weights(spec, b["w"], "amplitude"), om, b["phase"], V, X, Z, float), ref, bound, "amp")
    for mutant in ("no_eps", "plus"):        # through V, against the weights of the definition
        Vm = PR.update_weights(spec, X, y, noise, c, om, b["phase"], np.sqrt(noise) * b["xi"], float, mutant)
        with pytest.raises(AssertionError):
            PR.check_within(PR.paths(spec, c, om, b["phase"], Vm, X, Z, float), ref, bound, mutant)
    path = np.arange(17) % 3
    gref, gb = PR.gradient(spec, c, om, b["phase"], V, X, Z, path), PR.gradient_bound(spec, c, om, b["phase"], V, X, Z, path)
    with pytest.raises(AssertionError):
        PR.check_within(PR.gradient(spec, c, om, b["phase"], V, X, Z, path, float, "sine_sign"), gref, gb, "sine_sign")
    rows = np.asarray(ref, dtype=float)
    rows[:, 11] = rows[:, 4] = np.min(rows, axis=1) - 1.0           # an exact tie: the first index wins
    for minimize in (True, False):
        r = rows if minimize else -rows
        idx = PR.first_argbest(r, minimize)
        assert np.all(idx == 4)
        PR.check_argbest(idx, r[np.arange(3), idx], r, minimize)
        with pytest.raises(AssertionError):
            bad = PR.mutant_argbest_last(r, minimize)
            PR.check_argbest(bad, r[np.arange(3), bad], r, minimize)


# ---- the refusals that need no device ---------------------------------------------------------------------------------------------------
def _shell(kernel, noise=1e-2, **kw):
    """A GP that looks trained to the checks in front of the device calls (those are never reached here)."""
    from gpexp_amd.gp import GP
    g = GP(kernel, noise, **kw)
    g.pts, g.coeff = np.zeros((4, kernel.dimension)), np.zeros(4)
    if not kw:
        g._Ld = object()
    return g


def test_refusals(monkeypatch):
    import gpexp_amd.gp as gpm
    from gpexp_amd.kernels import KernelIsoMatern, KernelMehlerND, KernelSquaredExponential
    from gpexp_amd.paths import PathBase
    se = KernelSquaredExponential([0.5, 0.6], 1.0, 2)
    for kw in (dict(FITC=0.5), dict(FITC=0.5, sparse="vfe")):
        g = _shell(se, **kw)
        for call in (lambda: g.pathSampler(2, 8), lambda: g.samplePaths(np.zeros((3, 2))), lambda: g.priorPathSampler(2, 8)):
            with pytest.raises(NotImplementedError, match="FITC / VFE"):
                call()
    with pytest.raises(NotImplementedError, match="spectral density"):
        _shell(KernelMehlerND([0.3, 0.5], 2)).pathSampler(2, 8)
    with pytest.raises(NotImplementedError, match="spectral density"):
        _shell(KernelMehlerND([0.3, 0.5], 2)).priorPathSampler(2, 8)
    with pytest.raises(NotImplementedError, match="scalar noise"):
        _shell(se, noise=np.full(4, 1e-2)).pathSampler(2, 8)
    g = _shell(se)
    with pytest.raises(ValueError, match="base was drawn"):       # a Matern base on a squared-exponential model
        g.pathSampler(base=PathBase.draw(2, 8, 4, 2, KernelIsoMatern(0.7, 1.0, 2)._spec(), rng=0))
    with pytest.raises(ValueError, match="base was drawn"):       # another training-set size
        g.pathSampler(base=PathBase.draw(2, 8, 5, 2, se._spec(), rng=0))
    monkeypatch.setattr(gpm._dist, "session", lambda: object())
    for call in (lambda: g.pathSampler(2, 8), lambda: g.samplePaths(np.zeros((3, 2))), lambda: g.priorPathSampler(2, 8)):
        with pytest.raises(ValueError, match="session"):
            call()


# ---- 5: header and binding ---------------------------------------------------------------------------------------------------------------
NAMES = ["gpx_paths_create", "gpx_paths_eval", "gpx_paths_grad", "gpx_paths_coeff", "gpx_paths_shape", "gpx_paths_free"]


def test_header_and_binding():
    from gpexp_amd import _lib
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert "#define GPX_ABI_VERSION 2" in text
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert name in _lib._SIGS, name
    mk = open(os.path.join(ROOT, "gpexp_amd", "csrc", "Makefile")).read()
    assert "paths.hip" in mk
