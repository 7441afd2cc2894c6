"""The NumPy forms behind the VFE acquisition calls (tests/vfe_acq_ref.py), tied to something that needs no closed form: the
gradient to central differences of the costs of vfe_ref.predict, the rank-one batch recurrence to literally refitting the VFE model
on the data grown by the picks with the same inducing points.  No device."""
import functools
import os
import re

import numpy as np
import pytest

import bo_batch_compose as bb
import bo_compose as bc
import fitc_grad_ref as ref
import vfe_acq_ref as aref
import vfe_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dict(zip(ref.IDS, ref.CASES))
ENTRIES = ("gpx_vfe_acq", "gpx_vfe_acq_grad", "gpx_vfe_acq_batch")


@pytest.mark.parametrize("cid", ref.IDS)
def test_closed_form_gradient_against_central_differences(cid):
    """h = 1e-5; tolerance 1e-6 of the largest entry (tests/test_gpu_bo.py's figure; measured <= 4.4e-8).  The variance on these
    inputs is >= 3e-2 signalSize: nothing sits on a cancellation."""
    spec, X, S, y, noise = ref.case(CASES[cid])
    Z = aref.grad_inputs(spec, X, y)
    var = vref.predict(spec, X, S, y, noise, Z)[1]
    assert np.min(var) >= 3e-2 * spec["signalSize"], np.min(var)
    for name, (acq, param_of) in aref.ACQ_PARAMS.items():
        p = param_of(y)
        G = aref.grad(spec, X, S, y, noise, acq, p, Z)
        fd = aref.central_differences(lambda P: bc.costs(acq, p, *vref.predict(spec, X, S, y, noise, P)), Z)
        err = float(np.max(np.abs(G - fd)) / np.max(np.abs(fd)))
        other = float(np.max(np.abs(G - aref.grad(spec, X, S, y, noise, acq, p, Z, reordered=True))) / np.max(np.abs(G)))
        print("%s %s: closed form against central differences %.2e; two summation orders %.2e" % (cid, name, err, other))
        assert G.shape == Z.shape and np.max(np.abs(fd)) > 1e-3
        assert err <= 1e-6, (name, err)
        assert other <= 1e-10, (name, other)


@functools.lru_cache(maxsize=None)
def batch_problem(cid):
    spec, X, S, y, noise = ref.case(CASES[cid])
    C = np.random.default_rng(41).uniform(-1.0, 1.0, (400, spec["d"]))
    for a in (X, S, y, C):
        a.setflags(write=False)
    return spec, X, S, y, noise, C


@pytest.mark.parametrize("cid", ["se-d3", "m32-d2", "m52-d8"])
@pytest.mark.parametrize("acqname", ["ucb", "pi", "ei"])
@pytest.mark.parametrize("lie", ["believer", "min", "max"])
def test_rank_one_recurrence_against_the_refit_loop(cid, acqname, lie):
    """q = 8 on 400 candidates.  Rows against the refit loop forced to the recurrence's picks: <= 1e-10 of the row's largest entry
    (measured <= 7e-12); UCB and EI: the free-running picks identical and distinct (the winner's margin over the runner-up is
    >= 3.9e-5 of the row here).  PI saturates to ties on these inputs: the forced comparison only, as tests/test_gpu_bo_batch.py."""
    spec, X, S, y, noise, C = batch_problem(cid)
    acq = aref.ACQ_PARAMS[acqname][0]
    rule = 2.0 if acq == bc.UCB else "best"
    lv = lie if lie == "believer" else float(getattr(np, lie)(y))
    picks, rows, lies = aref.rank1_path(spec, X, S, y, noise, C, acq, rule, lv, 8)
    _, want, wlies = aref.refit_path(spec, X, S, y, noise, C, acq, rule, lv, 8, forced=picks)
    errs = [bb.row_err(rows[t], want[t]) for t in range(8)]
    print("%s %s %s: worst row error against the forced refit loop %.2e" % (cid, acqname, lie, max(errs)))
    assert max(errs) <= 1e-10, errs
    assert np.max(np.abs(lies - wlies)) <= 1e-10 * max(1.0, np.max(np.abs(wlies)))
    if acq != bc.PI:
        free = aref.refit_path(spec, X, S, y, noise, C, acq, rule, lv, 8)[0]
        assert picks == free and len(set(picks)) == 8


def test_the_recurrence_is_not_conditioning_with_the_predictive_variance():
    """delta = noise + t_s, not v_s + noise: with the other pivot the second row leaves the refit loop's by far more than round-off,
    so the forced comparison above discriminates between the two."""
    spec, X, S, y, noise, C = batch_problem("se-d3")
    picks, rows, _ = aref.rank1_path(spec, X, S, y, noise, C, bc.UCB, 2.0, "believer", 2)
    m = vref._model(spec, X, S, y, noise)
    Ku = ref.kparts(spec, S, C)[0]
    Wa = np.linalg.solve(m["La"], Ku)
    mu, var = vref.predict(spec, X, S, y, noise, C)
    s = picks[0]
    u = (Wa[:, s] @ Wa) / np.sqrt(var[s] + noise)
    wrong = bc.costs(bc.UCB, 2.0, mu, var - u * u)
    wrong[s] = np.nan
    assert bb.row_err(wrong, rows[1]) > 1e-4


def test_declarations():
    from gpexp_amd import _lib, device
    header = open(os.path.join(ROOT, "include", "gpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(gpx_ctx\* ctx, const gpx_fitc\* f, const gpx_mat\* S, const double\* coeff," % name, code), name
    assert "#define GPX_ABI_VERSION 2" in header
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert [len(_lib._SIGS[n][1]) for n in ENTRIES] == [10, 9, 15]
    for meth in ("acq", "acq_grad", "acq_batch"):
        assert callable(getattr(device.VfeModel, meth)) and meth not in vars(device.FitcModel)
    if os.path.exists(_lib.LIB_PATH):
        assert all(hasattr(_lib.load(), n) for n in ENTRIES)
