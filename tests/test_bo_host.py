"""CPU tests of the Bayesian-optimisation costs (costFuncGPUCbound / costFuncPI / costFuncEI, experimentalDesign.py:889-1003): the
reference fixture is reproduced by the NumPy composition the GPU tests compare against, the names are exported by both import
paths, the selection rule, and the C ABI declares and binds the two entry points."""
import json
import os
import re

import numpy as np
import pytest

from oracle import gpexp_oracle as orc
import bo_compose as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gpexp_golden_bo")


def load_bo():
    arrs = np.load(GOLD + ".npz")
    with open(GOLD + ".json") as f:
        index = json.load(f)
    return arrs, index


def fixture_queries():
    """(case, key, acq, param) of every fixture vector."""
    _, index = load_bo()
    arrs = np.load(GOLD + ".npz")
    out = []
    for case, ix in sorted(index.items()):
        fmax = float(np.max(arrs[case + "/y"]))
        for ik, kappa in enumerate(ix["kappas"]):
            out.append((case, "ucb%d" % ik, bc.UCB, kappa))
        out.append((case, "pi", bc.PI, fmax))
        out.append((case, "ei", bc.EI, fmax))
        out.append((case, "ei_fbest", bc.EI, ix["fBest"]))
    return out


def test_fixture_is_small_and_complete():
    arrs, index = load_bo()
    assert os.path.getsize(GOLD + ".npz") < 64 * 1024
    kinds = sorted((v["kernel"]["kind"], v["kernel"]["d"]) for v in index.values())
    assert kinds == [("matern32", 2), ("se", 1), ("se", 3)]
    for case, ix in index.items():
        n = arrs[case + "/X"].shape[0]
        assert 30 <= n <= 200 and ix["noise"] >= 1e-6
        for key in ("ucb0", "ucb1", "pi", "ei", "ei_fbest"):
            assert arrs["%s/%s" % (case, key)].shape == (20,)
    ard = index["bo_se_ard_d3"]["kernel"]
    assert ard["signalSize"] != 1.0 and len(set(ard["cl"])) == 3


@pytest.mark.parametrize("case,key,acq,param", fixture_queries())
def test_numpy_composition_reproduces_reference(case, key, acq, param):
    """The oracle's posterior (pinv, as gp.py:181), then abs, sqrt and scipy.stats.norm: the reference's evaluate, per point."""
    arrs, index = load_bo()
    ix = index[case]
    model = orc.fit(ix["kernel"], arrs[case + "/X"], arrs[case + "/y"], ix["noise"])
    mean, var = orc.posterior(ix["kernel"], model, arrs[case + "/Q"])
    want = arrs["%s/%s" % (case, key)]
    got = bc.costs(acq, param, mean, var)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-12


def test_names_importable_from_both_paths():
    import gpexp_amd.experimentalDesign as impl
    import gpExp.experimentalDesign as shim
    for name in ("costFuncGPUCbound", "costFuncPI", "costFuncEI", "optimizeAcquisition"):
        assert name in impl.__all__
        assert getattr(shim, name) is getattr(impl, name)
    ns = {}
    exec("from gpExp.experimentalDesign import *", ns)
    assert {"costFuncGPUCbound", "costFuncPI", "costFuncEI"} <= set(ns)


def test_selection_rule_first_min_nan_skipping():
    from gpexp_amd.experimentalDesign import firstMinIndex
    nan = np.nan
    assert firstMinIndex([3.0, 1.0, 2.0, 1.0]) == 1
    assert firstMinIndex([nan, 1.0, nan, 0.5, 0.5]) == 3
    assert firstMinIndex([nan, nan]) == -1
    assert firstMinIndex([0.0, -0.0]) == 0
    assert firstMinIndex([nan, -np.inf, -np.inf]) == 1
    assert firstMinIndex(np.array([2.0])) == 0


def test_header_declares_acquisition_entry_points():
    txt = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"enum gpx_acq_kind \{ GPX_ACQ_UCB = 0, GPX_ACQ_PI = 1, GPX_ACQ_EI = 2 \};", txt)
    for f in ("gpx_acq", "gpx_acq_grad"):
        assert re.search(r"\bint %s\(" % f, txt), f
    assert "experimentalDesign.py:899-923" in txt and "experimentalDesign.py:973-1003" in txt
    from gpexp_amd import _lib, device
    assert {"gpx_acq", "gpx_acq_grad"} <= set(_lib.exported_symbols())
    assert (device.ACQ_UCB, device.ACQ_PI, device.ACQ_EI) == (0, 1, 2)
    assert "acq.hip" in open(os.path.join(ROOT, "gpexp_amd", "csrc", "Makefile")).read()
