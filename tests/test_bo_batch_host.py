"""CPU tests of q-point batch acquisition (selectBatch / gpx_acq_batch): the rank-one recurrence the device implements against the
literal refit loop (both NumPy), the C ABI declaration and binding, and the host-side argument rules of selectBatch."""
import os
import re

import numpy as np
import pytest

import bo_compose as bc
import bo_batch_compose as bb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) the recurrence is the refit loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se3", "m52", "m32"])
@pytest.mark.parametrize("acq,rule", [(bc.UCB, 2.0), (bc.EI, "best")])
@pytest.mark.parametrize("lie", ["believer", "min", "max"])
def test_rank1_path_equals_refit_path(name, acq, rule, lie):
    spec, X, y, C, noise = bb.problem(name)
    lv = lie if lie == "believer" else float(getattr(np, lie)(y))
    p1, r1, l1 = bb.rank1_path(spec, X, y, noise, C, acq, rule, lv, 8)
    p0, r0, l0 = bb.refit_path(spec, X, y, noise, C, acq, rule, lv, 8)
    assert p1 == p0 and len(set(p0)) == 8
    errs = [bb.row_err(r1[t], r0[t]) for t in range(8)]
    print("%s acq=%d lie=%s worst row error %.2e" % (name, acq, lie, max(errs)))
    assert max(errs) <= 1e-10, errs
    assert np.max(np.abs(l1 - l0)) <= 1e-10 * max(1.0, np.max(np.abs(l0)))


def test_forced_replay_reproduces_the_free_run():
    spec, X, y, C, noise = bb.problem("m32")
    p0, r0, l0 = bb.refit_path(spec, X, y, noise, C, bc.EI, "best", "believer", 4)
    pf, rf, lf = bb.refit_path(spec, X, y, noise, C, bc.EI, "best", "believer", 4, forced=p0)
    assert pf == p0 and np.array_equal(rf, r0, equal_nan=True) and np.array_equal(lf, l0)


# ---- (b) ABI, binding, import paths, argument rules ----------------------------------------------------------------------------
def test_header_declares_and_lib_binds_batch_entry_point():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"enum gpx_acq_lie \{ GPX_LIE_BELIEVER = 0, GPX_LIE_CONSTANT = 1 \};", txt)
    assert re.search(r"\bint gpx_acq_batch\(", txt)
    from gpexp_amd import _lib, device
    assert "gpx_acq_batch" in _lib.exported_symbols()
    res, args = _lib._SIGS["gpx_acq_batch"]
    assert len(args) == 20 and args[-4] is _lib.c_ip
    assert (device.LIE_BELIEVER, device.LIE_CONSTANT) == (0, 1)
    assert callable(device.acq_batch)
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "gpx_acq_batch")


def test_select_batch_reachable_through_both_import_paths():
    import gpexp_amd.experimentalDesign as impl
    import gpExp.experimentalDesign as shim
    for name in ("costFuncGPUCbound", "costFuncPI", "costFuncEI"):
        assert callable(getattr(shim, name).selectBatch)
        assert getattr(shim, name).selectBatch is getattr(impl, name).selectBatch


class _Space(object):
    dimension = 2


class _FakeGP(object):
    noise = 0.25
    pts = np.zeros((5, 2))
    coeff = np.zeros(5)
    _L = _X = None

    class kernel(object):
        @staticmethod
        def _spec():
            return "spec"


class _FakeCtx(object):
    _hbm_bytes = 1e12


def _bare(cls, y, **attrs):
    """A cost object without a fit: only what selectBatch reads on the host."""
    cf = object.__new__(cls)
    cf.space, cf.yTrain, cf.xTrain = _Space(), np.asarray(y, dtype=float), np.zeros((len(y), 2))
    for k, v in attrs.items():
        setattr(cf, k, v)
    return cf


@pytest.fixture
def recorded(monkeypatch):
    import gpexp_amd.experimentalDesign as impl
    calls = []

    def fake_batch(ctx, spec, L, X, alpha, C, noise, kind, param, track_best, lie, lie_value, q, want_all=False):
        calls.append(dict(noise=noise, kind=kind, param=param, track_best=track_best, lie=lie, lie_value=lie_value, q=q,
                          want_all=want_all))
        out = (np.arange(q, dtype=np.int64), np.zeros(q), np.zeros(q))
        return out + (np.zeros((q, len(C))),) if want_all else out

    monkeypatch.setattr(impl._dev, "acq_batch", fake_batch)
    monkeypatch.setattr(impl._costFuncBO, "_dense", lambda self, c: (_FakeCtx(), _FakeGP(), np.asarray(c, dtype=float)))
    return calls


def test_select_batch_lie_parsing(recorded):
    from gpExp.experimentalDesign import costFuncEI
    from gpexp_amd import device
    y = [0.5, -2.0, 3.0, 0.5]
    cf = _bare(costFuncEI, y)
    C = np.zeros((7, 2))
    for lie, kind, value in (("believer", device.LIE_BELIEVER, None), ("min", device.LIE_CONSTANT, -2.0),
                             ("max", device.LIE_CONSTANT, 3.0), ("mean", device.LIE_CONSTANT, 0.5),
                             (1.25, device.LIE_CONSTANT, 1.25), (np.float64(-4.0), device.LIE_CONSTANT, -4.0)):
        idx, costs = cf.selectBatch(C, 3, lie=lie)
        call = recorded[-1]
        assert call["lie"] == kind and call["q"] == 3 and call["noise"] == 0.25 and not call["want_all"]
        if value is not None:
            assert call["lie_value"] == value
        assert idx.shape == (3,) and idx.dtype == np.int64 and costs.shape == (3,)
    out = cf.selectBatch(C, 2, returnAllCosts=True)
    assert len(out) == 3 and out[2].shape == (2, 7) and recorded[-1]["want_all"]
    n = len(recorded)
    for bad in ("median", "Believer", ""):
        with pytest.raises(ValueError):
            cf.selectBatch(C, 3, lie=bad)
    with pytest.raises(ValueError):
        cf.selectBatch(C, 8)
    assert len(recorded) == n


def test_select_batch_track_best_rule_per_class(recorded):
    from gpExp.experimentalDesign import costFuncEI, costFuncGPUCbound, costFuncPI
    from gpexp_amd import device
    y = [0.5, -2.0, 3.0]
    C = np.zeros((4, 2))
    _bare(costFuncGPUCbound, y, kappa=1.5).selectBatch(C, 2)
    assert recorded[-1]["kind"] == device.ACQ_UCB and recorded[-1]["param"] == 1.5 and recorded[-1]["track_best"] is False
    _bare(costFuncPI, y).selectBatch(C, 2)
    assert recorded[-1]["kind"] == device.ACQ_PI and recorded[-1]["param"] == 3.0 and recorded[-1]["track_best"] is True
    _bare(costFuncEI, y).selectBatch(C, 2)
    assert recorded[-1]["kind"] == device.ACQ_EI and recorded[-1]["param"] == 3.0 and recorded[-1]["track_best"] is True
    _bare(costFuncEI, y, fBest=0.75).selectBatch(C, 2)
    assert recorded[-1]["kind"] == device.ACQ_EI and recorded[-1]["param"] == 0.75 and recorded[-1]["track_best"] is False
