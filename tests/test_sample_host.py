"""CPU-only: the comparators of tests/sample_ref.py are pinned -- the references pass them, every mutant fails -- and the Python layer
of joint sampling, Thompson picks and Monte-Carlo q-EI (GP.posteriorSampler / samplePosterior / samplePrior, thompsonBatch, jointEI,
bestJointBatch, selectBatchJoint) runs on the NumPy stand-in: shapes, errors, the base-sample rules and the session rule."""
import os
import re

import numpy as np
import pytest

import sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in SR.SAMPLER_CASES if c[2] <= 130]


def nugget_of(c):
    return 1e-10 * SR.prior_max(c["spec"], c["Z"])


# ---- the nugget rule on every case of the device tests -------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.SAMPLER_CASES, ids=SR.case_id)
def test_default_nugget_factors_every_case(case):
    kind, n, m, d, noise, _ = case
    c = SR.points_case(kind, n, m, d, noise)
    mean, Cm = SR.host_posterior(c)
    nug = nugget_of(c)
    F = np.linalg.cholesky(Cm + nug * np.eye(m))            # raises if the nugget does not make it positive definite
    w = np.linalg.eigvalsh(Cm)
    print("%s: most negative eigenvalue of C %.3e, nugget %.3e" % (SR.case_id(case), w[0], nug))
    assert w[0] > -1e-4 * nug                               # four orders of margin
    SR.check_factor(F, Cm + nug * np.eye(m), SR.case_id(case))


# ---- comparators: references pass, mutants fail ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL[:6], ids=SR.case_id)
def test_factor_comparator_and_mutants(case):
    kind, n, m, d, noise, _ = case
    c = SR.points_case(kind, n, m, d, noise)
    _, Cm = SR.host_posterior(c)
    nug = nugget_of(c)
    Chat = Cm.copy()
    Chat[np.diag_indices(m)] += nug
    F = np.linalg.cholesky(Chat)
    SR.check_factor(F, Chat, "reference")
    with pytest.raises(AssertionError, match="upper triangle"):
        SR.check_factor(SR.mutant_factor_upper_leak(F), Chat, "mutant upper leak")
    with pytest.raises(AssertionError, match="residual"):
        SR.check_factor(SR.mutant_factor_no_nugget(Cm), Chat, "mutant no nugget")


@pytest.mark.parametrize("case", SMALL[:4], ids=SR.case_id)
def test_draw_comparator_and_mutant(case):
    kind, n, m, d, noise, s = case
    c = SR.points_case(kind, n, m, d, noise)
    mean, Cm = SR.host_posterior(c)
    F = np.linalg.cholesky(Cm + nugget_of(c) * np.eye(m))
    xi = SR.base_samples(max(s, 2), m)
    SR.check_draw(np.asarray(SR.draw_replay(mean, F, xi), dtype=float), mean, F, xi, "replay rounded")
    SR.check_draw(mean[None, :] + xi @ F.T, mean, F, xi, "float64 product")
    with pytest.raises(AssertionError, match="forward bound"):
        SR.check_draw(SR.mutant_draw_other_row(mean, F, xi), mean, F, xi, "mutant other row")


def test_argbest_comparator_and_mutant():
    rows = np.random.default_rng(3).standard_normal((6, 9))
    rows[:, 7] = rows[:, 2]                                 # exact ties ...
    rows[0, [2, 7]] = rows[0].min() - 1.0                   # ... that win
    rows[1, [2, 7]] = rows[1].max() + 1.0
    for minimize in (True, False):
        idx = SR.first_argbest(rows, minimize)
        SR.check_argbest(idx, rows[np.arange(6), idx], rows, minimize)
        bad = SR.mutant_argbest_last(rows, minimize)
        with pytest.raises(AssertionError, match="FIRST"):
            SR.check_argbest(bad, rows[np.arange(6), bad], rows, minimize)
    assert SR.first_argbest(rows, True)[0] == 2 and SR.first_argbest(rows, False)[1] == 2


@pytest.mark.parametrize("q,s", [(5, 130), (3, 3), (16, 128)])
def test_qei_comparator_and_mutants(q, s):
    c = SR.points_case("matern32", 40, q, 2, 1e-2)
    mu, Cb = SR.host_posterior(c)
    F = np.linalg.cholesky(Cb + nugget_of(c) * np.eye(q))
    xi = SR.base_samples(s, q, seed=5)
    fBest = float(np.max(c["y"]))
    ref64 = float(SR.qei_replay(mu, F, xi, fBest, dtype=np.float64))
    assert ref64 < 0.0
    SR.check_qei(ref64, mu, F, xi, fBest, "float64 replay")
    for name, mutant in (("min after the clamp", SR.mutant_qei_min_after_clamp), ("S - 1 samples", SR.mutant_qei_short_average)):
        with pytest.raises(AssertionError, match="misses the replay"):
            SR.check_qei(mutant(mu, F, xi, fBest), mu, F, xi, fBest, name)


def test_qei_q1_tends_to_the_closed_form():
    c = SR.points_case("matern32", 40, 1, 2, 1e-2)
    c["Z"] = np.array([[0.3, -0.2]])
    mu, Cb = SR.host_posterior(c)
    fBest = float(np.max(c["y"]))
    nug = 1e-10 * 1.1
    got = float(SR.qei_replay(mu, np.sqrt(Cb + nug), SR.stratified_normal(4096), fBest))
    want = float(SR.closed_form_ei(mu[0], Cb[0, 0] + nug, fBest))
    assert abs(got - want) <= 1e-4 * abs(want)


# ---- the Python layer on the stand-in --------------------------------------------------------------------------------------------
class _Space(object):
    def __init__(self, d):
        self.dimension = d


@pytest.fixture
def standin(monkeypatch):
    import gpexp_amd.experimentalDesign as edm
    import gpexp_amd.gp as gpm
    be = SR.NumpySampleDevice()
    monkeypatch.setattr(gpm, "_dev", be)
    monkeypatch.setattr(edm, "_dev", be)
    return be


def fitted(c, **kw):
    """A GP whose device state is the stand-in's: host points, the host factor, alpha."""
    import scipy.linalg as sl
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    spec = c["spec"]
    g = GP(KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5), c["noise"], **kw)
    K = SR.cov_f64(spec, c["X"])
    K[np.diag_indices_from(K)] += c["noise"]
    cf = sl.cho_factor(K, lower=True)
    g.pts, g._X, g.coeff = c["X"], c["X"], sl.cho_solve(cf, c["y"])
    if not kw:
        g._Ld = SR.HostFactor(np.tril(cf[0]))
    return g


def cost_on(g, c, cls=None):
    from gpexp_amd.experimentalDesign import costFuncEI
    cf = object.__new__(cls or costFuncEI)
    cf.space, cf.xTrain, cf.yTrain, cf.gaussianProcess = _Space(c["spec"]["d"]), c["X"], c["y"], g
    return cf


def test_sampler_shapes_and_determinism(standin):
    c = SR.points_case("matern32", 40, 9, 2, 1e-2)
    g = fitted(c)
    smp = g.posteriorSampler(c["Z"])
    assert standin.calls[-1] == ("psampler", 9, 1e-10 * 1.1, False)          # the default jitter: 1e-10 max k(z, z)
    xi = SR.base_samples(4, 9)
    a, b = smp.draw(baseSamples=xi), smp.draw(nSamples=77, baseSamples=xi)    # a given array brings its own sample count
    assert a.shape == (4, 9) and np.array_equal(a, b)
    assert smp.draw().shape == (1, 9) and smp.draw(3).shape == (3, 9)
    idx, val, rows = smp.argbest(baseSamples=xi, returnSamples=True)
    assert np.array_equal(rows, a)
    SR.check_argbest(idx, val, rows, True)
    idx2, val2 = smp.argbest(baseSamples=xi, minimize=False)
    SR.check_argbest(idx2, val2, rows, False)
    smp.close()
    smp.close()
    with pytest.raises(ValueError, match="closed"):
        smp.draw(baseSamples=xi)
    assert np.array_equal(g.samplePosterior(c["Z"], baseSamples=xi), a)
    g.posteriorSampler(c["Z"], jitter=1e-6, addNoise=True).close()
    assert standin.calls[-1][2] == 1e-6 + c["noise"]
    mean, _ = SR.host_posterior(c)
    assert np.allclose(g.samplePosterior(c["Z"], baseSamples=np.zeros((1, 9)))[0], mean, rtol=0, atol=1e-12)


def test_base_sample_and_argument_errors(standin):
    c = SR.points_case("matern32", 40, 9, 2, 1e-2)
    g = fitted(c)
    smp = g.posteriorSampler(c["Z"])
    for bad in (np.zeros((3, 8)), np.zeros(9), np.zeros((0, 9)), np.full((2, 9), np.nan), np.full((2, 9), np.inf)):
        with pytest.raises(ValueError):
            smp.draw(baseSamples=bad)
        with pytest.raises(ValueError):
            smp.argbest(baseSamples=bad)
    with pytest.raises(ValueError):
        smp.draw(0)
    for bad in (-1e-12, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            g.posteriorSampler(c["Z"], jitter=bad)
    with pytest.raises(AssertionError):
        g.posteriorSampler(np.zeros((3, 5)))


def test_duplicates_without_jitter_raise_not_positive_definite(standin):
    from gpexp_amd._lib import NotPositiveDefinite
    c = SR.points_case("matern32", 40, 9, 2, 1e-2)
    with pytest.raises(NotPositiveDefinite):
        fitted(c).posteriorSampler(c["Z"], jitter=0.0)


def test_device_error_message_names_the_point_and_the_jitter():
    from gpexp_amd import device
    from gpexp_amd._lib import NotPositiveDefinite
    e = device._sampler_not_pd(6, 0.0)
    assert isinstance(e, NotPositiveDefinite) and e.pivot == 6
    assert "point 5" in str(e) and "larger jitter" in str(e)


def test_prior_sampler(standin):
    c = SR.points_case("matern32", 40, 7, 2, 1e-2)
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    g = GP(KernelIsoMatern(0.7, 1.0, 2, nu=1.5), 0.1)       # never trained
    far = 1e3 * np.arange(7.0)[:, None] * np.ones((1, 2))   # far apart: K = I exactly
    xi = SR.base_samples(5, 7)
    out = g.samplePrior(far, baseSamples=xi)
    assert standin.calls[-1] == ("psampler", 7, 1e-10, True)
    assert np.allclose(out, np.sqrt(1.0 + 1e-10) * xi, rtol=1e-15, atol=0)
    assert g.samplePrior(c["Z"], nSamples=4, noise=1e-3).shape == (4, 7) and standin.calls[-1][2] == 1e-3


def test_thompson_batch(standin):
    c = SR.points_case("matern32", 40, 30, 2, 1e-2)
    from gpexp_amd.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    xi = SR.base_samples(4, 30, seed=8)
    for cls in (costFuncEI, costFuncPI, costFuncGPUCbound):
        cf = cost_on(fitted(c), c, cls)
        idx, val = cf.thompsonBatch(c["Z"], 4, baseSamples=xi)
        assert idx.shape == (4,) and idx.dtype == np.int64 and val.shape == (4,)
        rows = fitted(c).samplePosterior(c["Z"], baseSamples=xi)
        SR.check_argbest(idx, val, rows, True)
        idx2, val2 = cf.thompsonBatch(c["Z"], 4, baseSamples=xi, minimize=False)
        SR.check_argbest(idx2, val2, rows, False)
        assert cf.thompsonBatch(c["Z"], 3)[0].shape == (3,)


def test_joint_ei_plumbing(standin):
    c = SR.points_case("matern32", 40, 30, 2, 1e-2)
    cf = cost_on(fitted(c), c)
    batches = c["Z"][:24].reshape(6, 4, 2)
    xi = SR.base_samples(64, 4, seed=2)
    costs = cf.jointEI(batches, baseSamples=xi)
    assert standin.calls[-1][:4] == ("qei", 6, 4, (64, 4)) and standin.calls[-1][4] == float(np.max(c["y"]))
    assert costs.shape == (6,) and np.all(costs <= 0.0)
    assert np.array_equal(cf.jointEI(batches[2], baseSamples=xi), costs[2:3])          # one batch (q, d)
    j, cost = cf.bestJointBatch(batches, baseSamples=xi)
    assert j == int(np.argmin(costs)) and cost == costs[j]
    assert cf.jointEI(batches, nSamples=16).shape == (6,) and standin.calls[-1][3] == (16, 4)
    for bad in (np.zeros((2, 4, 3)), np.zeros((2, 33, 2)), np.zeros((2, 0, 2)), np.zeros(4), np.zeros((0, 4, 2))):
        with pytest.raises(ValueError):
            cf.jointEI(bad, baseSamples=xi)
    with pytest.raises(ValueError):
        cf.jointEI(batches, baseSamples=xi[:, :3])
    with pytest.raises(ValueError):
        cf.jointEI(batches, nSamples=0)
    # two identical points with jitter 0: NaN, skipped by the arg-min
    twin = batches.copy()
    twin[int(np.argmin(costs)), 1] = twin[int(np.argmin(costs)), 0]
    c0 = cf.jointEI(twin, baseSamples=xi, jitter=0.0)
    assert np.isnan(c0[int(np.argmin(costs))]) and np.count_nonzero(np.isnan(c0)) == 1
    assert cf.bestJointBatch(twin, baseSamples=xi, jitter=0.0)[0] == int(np.nanargmin(c0))


def test_select_batch_joint(standin, monkeypatch):
    import gpexp_amd.experimentalDesign as edm
    c = SR.points_case("matern32", 40, 30, 2, 1e-2)
    cf = cost_on(fitted(c), c)
    proposals = {"believer": [0, 3, 6], "min": [1, 4, 7], "max": [2, 5, 8], "mean": [9, 10, 11]}
    monkeypatch.setattr(edm._costFuncBO, "selectBatch",
                        lambda self, C, q, lie="believer", returnAllCosts=False: (np.array(proposals[lie], dtype=np.int64), np.zeros(q)))
    xi = SR.base_samples(32, 3, seed=4)
    idx, cost, lie = cf.selectBatchJoint(c["Z"], 3, baseSamples=xi)
    four = [cf.jointEI(c["Z"][proposals[name]], baseSamples=xi)[0] for name in ("believer", "min", "max", "mean")]
    assert idx.tolist() == proposals[lie] and cost == min(four) and cost == four[("believer", "min", "max", "mean").index(lie)]
    with pytest.raises(ValueError):
        cf.selectBatchJoint(c["Z"], 3, lies=(), baseSamples=xi)


def test_sparse_models_are_refused(standin):
    c = SR.points_case("matern32", 40, 9, 2, 1e-2)
    xi = SR.base_samples(2, 9)
    for kw in (dict(FITC=0.5), dict(FITC=0.5, sparse="vfe")):
        g = fitted(c, **kw)
        cf = cost_on(g, c)
        for call in (lambda: g.posteriorSampler(c["Z"]), lambda: g.samplePosterior(c["Z"], baseSamples=xi),
                     lambda: g.samplePrior(c["Z"], baseSamples=xi), lambda: cf.thompsonBatch(c["Z"], 2, baseSamples=xi),
                     lambda: cf.jointEI(c["Z"][:8].reshape(2, 4, 2)), lambda: cf.bestJointBatch(c["Z"][:8].reshape(2, 4, 2)),
                     lambda: cf.selectBatchJoint(c["Z"], 2)):
            with pytest.raises(NotImplementedError):
                call()
    assert not standin.calls


def test_session_rule(standin, monkeypatch):
    """Under an attached multi-process session the calls run replicated: given base samples work, baseSamples=None is refused."""
    import gpexp_amd.gp as gpm
    c = SR.points_case("matern32", 40, 9, 2, 1e-2)
    g = fitted(c)
    cf = cost_on(g, c)
    xi = SR.base_samples(2, 9)
    monkeypatch.setattr(gpm._dist, "session", lambda: object())
    assert g.samplePosterior(c["Z"], baseSamples=xi).shape == (2, 9)
    assert cf.jointEI(c["Z"][:8].reshape(2, 4, 2), baseSamples=SR.base_samples(8, 4)).shape == (2,)
    for call in (lambda: g.samplePosterior(c["Z"]), lambda: g.samplePrior(c["Z"]), lambda: g.posteriorSampler(c["Z"]).argbest(),
                 lambda: cf.thompsonBatch(c["Z"], 2), lambda: cf.jointEI(c["Z"][:8].reshape(2, 4, 2)),
                 lambda: cf.bestJointBatch(c["Z"][:8].reshape(2, 4, 2))):
        with pytest.raises(ValueError, match="session"):
            call()


def test_generate_samples_still_raises():
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelSquaredExponential
    g = GP(KernelSquaredExponential([0.3], 1.0, 1), 0.1)
    with pytest.raises(NotImplementedError) as e:
        g.generateSamples(np.zeros((3, 1)))
    assert str(e.value) == "generateSamples (SVD sampling, gp.py:343-371) is outside the GPU hot path"


# ---- header and binding -------------------------------------------------------------------------------------------------------------
NAMES = ["gpx_psampler_create", "gpx_psampler_draw", "gpx_psampler_argbest", "gpx_psampler_shape", "gpx_psampler_free", "gpx_acq_qei"]


def test_header_declares_and_lib_binds_the_entry_points():
    from gpexp_amd import _lib
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_debug.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, pub), n
    assert re.search(r"\bgpx_dbg_qei_blocks\s*\(", dbg) and "gpx_dbg_qei_blocks" not in pub
    assert "#define GPX_QEI_MAX_Q 32" in pub
    assert set(NAMES + ["gpx_dbg_qei_blocks"]) <= set(_lib.exported_symbols())
    so = os.path.join(ROOT, "gpexp_amd", "libgpx_hip.so")
    if os.path.exists(so):
        lib = _lib.load()
        for n in NAMES + ["gpx_dbg_qei_blocks"]:
            assert hasattr(lib, n)


def test_methods_reachable_through_both_import_paths():
    import gpExp.experimentalDesign as shim
    import gpExp.gp as gshim
    import gpexp_amd.experimentalDesign as impl
    for name in ("costFuncGPUCbound", "costFuncPI", "costFuncEI"):
        assert getattr(shim, name).thompsonBatch is getattr(impl, name).thompsonBatch
    for m in ("jointEI", "bestJointBatch", "selectBatchJoint"):
        assert callable(getattr(shim.costFuncEI, m))
    for m in ("posteriorSampler", "samplePosterior", "samplePrior", "generateSamples"):
        assert callable(getattr(gshim.GP, m))
