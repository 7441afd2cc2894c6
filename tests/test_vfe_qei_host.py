"""CPU: the parts of Monte-Carlo q-EI on VFE models (gpx_vfe_acq_qei) that need no device -- the header, the binding and the built
library's exports; the class API (vfeJointEI, vfeBestJointBatch, vfeSelectBatchJoint) on tests/vfe_qei_ref.py's NumPy stand-in; and the
float64 restatement of the kernel's signed Gram, in its slice order, against vfe_sample_ref.exact_cov in longdouble, with both mutants
caught.  Every test prints its worst figure before it asserts (run with -s)."""
import os
import re

import numpy as np
import pytest

import fitc_grad_ref as FR
import sample_ref as SR
import vfe_qei_ref as QR
import vfe_sample_ref as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: header, binding, exports -----------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    from gpexp_amd import _lib
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx_debug.h")).read(), flags=re.S)
    assert re.search(r"\bgpx_vfe_acq_qei\s*\(", pub)
    assert re.search(r"\bgpx_dbg_vfe_qei_blocks\s*\(", dbg) and "gpx_dbg_vfe_qei_blocks" not in pub
    names = ["gpx_vfe_acq_qei", "gpx_dbg_vfe_qei_blocks"]
    assert set(names) <= set(_lib.exported_symbols()) and all(n in _lib._SIGS for n in names)
    print("  declared and bound: %s" % ", ".join(names))
    so = os.path.join(ROOT, "gpexp_amd", "libgpx_hip.so")
    if os.path.exists(so):
        lib = _lib.load()
        for n in names:
            assert hasattr(lib, n), n


def test_methods_reachable_through_both_import_paths():
    import gpExp.experimentalDesign as shim
    import gpexp_amd.experimentalDesign as impl
    for m in ("vfeJointEI", "vfeBestJointBatch", "vfeSelectBatchJoint"):
        assert getattr(shim.costFuncEI, m) is getattr(impl.costFuncEI, m)
    from gpexp_amd import device
    assert callable(device.VfeModel.acq_qei) and callable(device.VfeModel.dbg_qei_blocks)


# ---- 2: the class API on the stand-in ---------------------------------------------------------------------------------------------------
class _Dev(SR.NumpySampleDevice):
    K_SE, K_MATERN32, K_MATERN52 = 0, 1, 2


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


def fitted(**kw):
    """A GP that looks trained on the stand-in: host points, the stand-in model, the true coefficients' place held by zeros (the
    stand-in takes its mean from y)."""
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    spec, X, S, y, noise = FR.case(CASE)
    kw = kw or dict(FITC=0.3, sparse="vfe")
    g = GP(KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5), noise, **kw)
    g.pts, g._X, g.coeff = X, X, np.zeros(len(y))
    if "FITC" in kw:
        g.fitcnodes, g._fitc = S, QR.VfeStandin(spec, X, S, y, noise)
    else:
        g._Ld = object()
    return g, (spec, X, S, y, noise)


def cost_on(g, data):
    from gpexp_amd.experimentalDesign import costFuncEI
    cf = object.__new__(costFuncEI)
    cf.space, cf.xTrain, cf.yTrain, cf.gaussianProcess = _Space(data[0]["d"]), data[1], data[3], g
    return cf


def _batches(nb=6, q=4, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (nb, q, 2))


def test_joint_ei_plumbing(standin):
    g, data = fitted()
    spec, X, S, y, noise = data
    cf = cost_on(g, data)
    batches, xi = _batches(), SR.base_samples(64, 4, seed=2)
    costs = cf.vfeJointEI(batches, baseSamples=xi)
    assert g._fitc.calls[-1] == ("vfe_qei", 6, 4, (64, 4), float(np.max(y)), 1e-10 * spec["signalSize"])
    assert costs.shape == (6,) and np.all(costs <= 0.0) and not standin.calls            # the dense entry is never called
    # the stand-in's definition, restated: exact_cov + mean + replay
    m = g._fitc.m
    F = np.linalg.cholesky(VS.exact_cov(spec, S, m, batches[2], float) + 1e-10 * spec["signalSize"] * np.eye(4))
    want = float(SR.qei_replay(VS.mean(spec, S, m, batches[2], float), F, xi, np.max(y), dtype=np.float64))
    print("  vfeJointEI against exact_cov + mean + replay: |difference| %.3e" % abs(costs[2] - want))
    assert abs(costs[2] - want) <= 1e-12 * abs(want)
    one = cf.vfeJointEI(batches[2], baseSamples=xi)                                        # one batch (q, d)
    assert one.shape == (1,) and np.array_equal(one, costs[2:3])
    j, cost = cf.vfeBestJointBatch(batches, baseSamples=xi)
    assert j == int(np.nanargmin(costs)) and cost == costs[j]
    assert cf.vfeJointEI(batches, nSamples=16).shape == (6,) and g._fitc.calls[-1][3] == (16, 4)
    cf.vfeJointEI(batches, baseSamples=xi, jitter=1e-6)
    assert g._fitc.calls[-1][5] == 1e-6
    # two identical points with jitter 0: NaN, skipped by the arg-min
    twin = batches.copy()
    w = int(np.argmin(costs))
    twin[w, 1] = twin[w, 0]
    c0 = cf.vfeJointEI(twin, baseSamples=xi, jitter=0.0)
    assert np.isnan(c0[w]) and np.count_nonzero(np.isnan(c0)) == 1
    assert cf.vfeBestJointBatch(twin, baseSamples=xi, jitter=0.0)[0] == int(np.nanargmin(c0))


def test_select_batch_joint(standin, monkeypatch):
    import gpexp_amd.experimentalDesign as edm
    g, data = fitted()
    cf = cost_on(g, data)
    C = np.random.default_rng(7).uniform(-1.0, 1.0, (30, 2))
    lies = ("believer", "min", "max", "mean")
    proposals = {"believer": [0, 3, 6], "min": [1, 4, 7], "max": [2, 5, 8], "mean": [9, 10, 11]}
    monkeypatch.setattr(edm._costFuncBO, "selectBatch",
                        lambda self, C, q, lie="believer", returnAllCosts=False: (np.array(proposals[lie], dtype=np.int64), np.zeros(q)))
    xi = SR.base_samples(32, 3, seed=4)
    idx, cost, lie = cf.vfeSelectBatchJoint(C, 3, baseSamples=xi)
    four = [cf.vfeJointEI(C[proposals[name]], baseSamples=xi)[0] for name in lies]
    print("  proposals' costs %s, winner %r" % (four, lie))
    assert lie in lies and idx.tolist() == proposals[lie]                                  # one of selectBatch's proposals ...
    assert cost == min(four) and cost == four[lies.index(lie)]                             # ... with that proposal's own cost
    with pytest.raises(ValueError, match="vfeSelectBatchJoint"):
        cf.vfeSelectBatchJoint(C, 3, lies=(), baseSamples=xi)


def test_refusals(standin, monkeypatch):
    import gpexp_amd.gp as gpm
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelIsoMatern
    b, xi = _batches(2, 4), SR.base_samples(8, 4)

    def calls(cf):
        return (lambda: cf.vfeJointEI(b, baseSamples=xi), lambda: cf.vfeBestJointBatch(b, baseSamples=xi),
                lambda: cf.vfeSelectBatchJoint(b.reshape(-1, 2), 2, baseSamples=SR.base_samples(8, 2)))
    spec, X, S, y, noise = FR.case(CASE)
    dense = GP(KernelIsoMatern(spec["rho"], spec["signalSize"], 2, nu=1.5), noise)
    dense.pts, dense._X, dense.coeff, dense._Ld = X, X, np.zeros(len(y)), object()
    for g, data in ((dense, (spec, X, S, y, noise)), fitted(FITC=0.3)):                    # a dense and a FITC model
        for call in calls(cost_on(g, data)):
            with pytest.raises(ValueError, match="VFE models"):
                call()
    g, data = fitted()
    g.coeff = None                                                                         # nodes set, never trained
    for call in calls(cost_on(g, data)):
        with pytest.raises(ValueError, match="trained model"):
            call()
    g, data = fitted()
    cf = cost_on(g, data)
    for bad in (np.zeros((2, 0, 2)), np.zeros((2, 33, 2)), np.zeros((2, 4, 3)), np.zeros(4), np.zeros((0, 4, 2))):
        with pytest.raises(ValueError):
            cf.vfeJointEI(bad, baseSamples=xi)
    with pytest.raises(ValueError):
        cf.vfeJointEI(b, baseSamples=xi[:, :3])                                            # base samples of the wrong shape
    with pytest.raises(ValueError):
        cf.vfeJointEI(b, nSamples=0)
    with pytest.raises(ValueError):
        cf.vfeJointEI(b, baseSamples=xi, jitter=-1e-12)
    assert not g._fitc.calls                                                               # nothing reached the model
    # the old names refuse the model as before
    for call in (lambda: cf.jointEI(b, baseSamples=xi), lambda: cf.bestJointBatch(b, baseSamples=xi)):
        with pytest.raises(NotImplementedError, match="FITC / VFE"):
            call()
    monkeypatch.setattr(gpm._dist, "session", lambda: object())                            # replicated calls: the draws must be given
    assert cf.vfeJointEI(b, baseSamples=xi).shape == (2,)
    for call in (lambda: cf.vfeJointEI(b), lambda: cf.vfeBestJointBatch(b)):
        with pytest.raises(ValueError, match="session"):
            call()


# ---- 3: the signed Gram in the kernel's slice order --------------------------------------------------------------------------------------
def test_plan_is_the_kernels():
    """G q <= 32 columns, G npair nsl <= 768 items, nsl divides the tile of 64 rows (so the slice of a row does not depend on the tile)."""
    for q in range(1, 33):
        G, T, nsl, npair = QR.plan(q)
        assert G * q <= 32 and G * T <= 256 and G * npair * nsl <= 768 and 64 % nsl == 0 and npair == q * (q + 1) // 2
    assert [QR.plan(q)[2] for q in QR.QS] == [8, 4, 2, 1, 1]


@pytest.mark.parametrize("c", QR.SMALL + [QR.MEHLER], ids=QR.case_id)
def test_signed_gram_restatement_and_mutants(c):
    spec, X, S, y, noise = QR.build(c)
    mld, m64 = VS.model(spec, X, S, None, noise), VS.model(spec, X, S, None, noise, float)
    worst, least = 0.0, {k: np.inf for k in QR.MUTANTS}
    for q in QR.QS:
        Zb = QR.batches(c, S, q, 3)
        ref = QR.blocks_ref(spec, S, mld, Zb, q)
        worst = max(worst, QR.worst_rel(QR.blocks_f64(spec, S, m64, Zb, q), ref))
        for k in QR.MUTANTS:
            least[k] = min(least[k], QR.worst_rel(QR.blocks_f64(spec, S, m64, Zb, q, mutant=k), ref))
    print("  %-36s float64 route - longdouble: %.3e x max |cov| (cap %g); mutants miss by at least %s"
          % (QR.case_id(c), worst, QR.TOL, ", ".join("%s %.2e" % kv for kv in least.items())))
    assert worst <= QR.TOL
    for k in QR.MUTANTS:
        assert least[k] > 1e3 * QR.TOL, k


def test_blocks_ref_is_exact_cov():
    """The blocks of the reference are the diagonal blocks of vfe_sample_ref.exact_cov (the quantity the issue names)."""
    c = QR.SMALL[2]
    spec, X, S, y, noise = QR.build(c)
    m = VS.model(spec, X, S, None, noise)
    Zb = QR.batches(c, S, 5, 3)
    full, blocks = VS.exact_cov(spec, S, m, Zb), QR.blocks_ref(spec, S, m, Zb, 5)
    miss = max(float(np.max(np.abs(blocks[b] - full[5 * b:5 * b + 5, 5 * b:5 * b + 5]))) for b in range(3))
    print("  blocks_ref against exact_cov's diagonal blocks: %.3e" % miss)
    assert miss <= 1e-17 * float(np.max(np.abs(full)))
