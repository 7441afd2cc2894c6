"""The replay references of the design selectors, judged on the CPU alone (no GPU): the longdouble covariances against the
50-digit reference, the conditions the replay configurations must meet, the float64 emulations under the helpers, three
deliberately wrong emulations that the helpers must reject, and the recorded tau table.

Recording the table (writes TAU_TABLE into tests/design_replay_ref.py between its markers):
    python tests/test_design_replay_host.py --record
"""
import datetime
import functools
import os
import re
import sys

import numpy as np
import pytest

import design_replay_ref as ref
from kernel_reference import Reference

LD = ref.LD


# ---- the emulations' own runs, computed once and left unchanged ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gvar_run(name):
    spec, C, nsel, w, keep = ref.gvar_inputs(name)
    picks, dhist = ref.emu_greedy_var(spec, C, nsel, weights=w, keep=keep)
    return picks, dhist


@functools.lru_cache(maxsize=None)
def mi_run(name, noise):
    spec, C = ref.mi_inputs(name)
    return ref.emu_mi(spec, C, noise, ref.MI_NSEL, ref.MI_START)


@functools.lru_cache(maxsize=None)
def mi_large_run():
    name, spec, M, noise, nsel, _ = ref.MI_LARGE
    return ref.emu_mi(spec, ref.mi_inputs(name)[1], noise, nsel, ref.MI_START)


@functools.lru_cache(maxsize=None)
def givar_run(name):
    spec, X0, C, Z, noise, nsel = ref.givar_inputs(name)
    return ref.emu_givar(spec, X0, C, Z, noise, nsel)


@functools.lru_cache(maxsize=None)
def judged(key):
    """The judge of configuration `key` on the emulation's own run, in measuring mode (no tau yet)."""
    if key in ref.GVAR:
        picks, dhist = gvar_run(key)
        return ref.judge_gvar(key, picks, lambda t: dhist[t])
    if key in ref.GIVAR:
        return ref.judge_givar(key, *givar_run(key))
    if key == ref.MI_LARGE[0]:
        return ref.judge_mi_large(*mi_large_run())
    name, noise = key.split("/")
    return ref.judge_mi(name, float(noise), *mi_run(name, float(noise)))


def measured(key):
    return judged(key).out


KEYS = (list(ref.GVAR) + [ref.mi_key(n, z) for n in ref.MI for z in ref.MI_NOISES] + [ref.MI_LARGE[0]] + list(ref.GIVAR))


# ---- covariances -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [ref.SE2, ref.SE1, ref.M32_2, ref.M52_3], ids=lambda s: "%s-d%d" % (s["kind"], s["d"]))
def test_longdouble_covariances_match_the_50_digit_reference(spec):
    """A sample of pairs of the replay's own point sets (near, far and identical points), to 4 * 2^-64 relative."""
    rng = np.random.default_rng(77)
    A = rng.uniform(-1.0, 1.0, (48, spec["d"]))
    A[1] = A[0]                                             # an identical pair
    A[3] = A[2] + 1e-9                                      # a near pair
    A[4], A[5] = -1.0, 1.0                                  # the farthest pair of the box
    R = Reference(spec, A)
    K = ref.cov_ld(spec, A)
    worst = 0.0
    for p in range(R.I.size):
        i, j = int(R.I[p]), int(R.J[p])
        hi = float(K[i, j])
        lo = float(K[i, j] - LD(hi))
        with ref.decimal.localcontext(ref._DCTX):
            err = abs(ref.Decimal(hi) + ref.Decimal(lo) - R.k[p]) / R.k[p]
        worst = max(worst, float(err))
    print("%s d=%d: largest relative error of the longdouble covariance %.3g = %.2f x 2^-64"
          % (spec["kind"], spec["d"], worst, worst * 2.0 ** 64))
    assert worst <= 4.0 * 2.0 ** -64


# ---- conditions on the inputs, checked on the reference alone --------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.GVAR))
def test_greedy_variance_pivots_stay_far_from_the_drop_rule(name):
    """The longdouble pivot / prior of every pick of the emulation is >= 1e-5 (the drop rule sits at 1e-13), and the picks of the
    longdouble greedy sequence itself meet the same condition."""
    spec, C, nsel, w, keep = ref.gvar_inputs(name)
    picks, dhist = gvar_run(name)
    minpiv = judged(name).minpiv
    d, piv = ref.cond_var(spec, C, picks)
    print("%s: smallest pivot / prior %.3g (at the checked steps %.3g)" % (name, float(np.min(piv)), minpiv))
    assert float(np.min(piv)) >= 1e-5 and minpiv >= 1e-5
    assert ref.STEPS(nsel)[-1] == nsel - 1 and picks[:len(keep)].tolist() == keep


def test_refined_ratio_equals_the_full_longdouble_inverse():
    """M = 130 (Matern 3/2, every noise value): the one-candidate refined solve against mi_ratios, to 1e-16 relative."""
    spec, C = ref.mi_inputs("mi-m32")
    worst = 0.0
    for noise in ref.MI_NOISES:
        A = [5, 77, 12, 101]
        full = ref.mi_ratios(spec, C, noise, A)
        for c in (0, 64, 129):
            one = ref.refined_ratio(spec, C, noise, A, c)
            worst = max(worst, float(abs(one - full[c]) / abs(full[c])))
    print("refined_ratio against mi_ratios: %.3g relative" % worst)
    assert worst <= 1e-16


def test_givar_costs_equal_refits():
    """The rank-one formula of givar_costs against actual refits in longdouble (three candidates, picks in the design)."""
    spec, X0, C, Z, noise, nsel = ref.givar_inputs("givar-se2")
    picks = [3, 200, 41]
    cost = ref.givar_costs(spec, X0, C, Z, noise, picks)
    for j in (0, 41, 259):
        D = np.vstack([X0, C[picks], C[j:j + 1]])
        Sig = ref.cov_ld(spec, D)
        Sig[np.diag_indices_from(Sig)] += LD(noise)
        W = ref.solve_lower_ld(ref.chol_ld(Sig), ref.cov_ld(spec, D, Z))
        ivar = np.sum(LD(spec["signalSize"]) - np.sum(W * W, axis=0)) / LD(Z.shape[0])
        assert float(abs(ivar - cost[j]) / ivar) <= 1e-15


# ---- the emulations under the helpers, and the table -----------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_emulation_passes_and_the_recorded_tau_stands(key):
    """The emulation's own picks satisfy assertions 1-3 under the recorded tau; the table's tau is 32 x its recorded deviation
    (floor 64 u); and the deviation measured now is what was recorded (to a factor 4: another BLAS may sum in another order)."""
    assert key in ref.TAU_TABLE, "no recorded tau for %s: run `python tests/test_design_replay_host.py --record`" % key
    dev, tau = ref.TAU_TABLE[key]
    assert tau == ref.tau_of(dev)
    got = measured(key)
    print("%s: measured value deviation %.3e, pick shortfall %.3e; recorded %.3e, tau %.3e" % (key, got["value"], got["pick"], dev, tau))
    assert got["value"] <= 4.0 * dev and dev <= 4.0 * got["value"]
    judged(key).assert_under(tau)


# ---- three deliberately wrong emulations ------------------------------------------------------------------------------------
def test_a_last_maximum_tie_rule_is_rejected():
    """Every candidate twice (bitwise-equal scores at every step): the first-maximum rule picks below M, a last-maximum rule picks
    the upper copies -- the same candidates to the replay, so assertion 2 cannot see it; the exact comparison the GPU test makes
    (tile(B, r) against B) does."""
    spec, C, nsel, w, keep = ref.gvar_inputs("gvar-se2")
    C2, w2 = np.tile(C, (2, 1)), np.tile(w, 2)
    base = ref.emu_greedy_var(spec, C, 6, weights=w)[0]
    first = ref.emu_greedy_var(spec, C2, 6, weights=w2)[0]
    last = ref.emu_greedy_var(spec, C2, 6, weights=w2, tie="last")[0]
    assert np.array_equal(first, base)
    assert not np.array_equal(last, base) and np.array_equal(last % C.shape[0], base)


def test_a_perturbed_d_is_rejected():
    """d off by 1e-9 relative from step 3 on -- what today's index-only comparison lets through -- fails the value assertion."""
    name = "gvar-se2"
    spec, C, nsel, w, keep = ref.gvar_inputs(name)
    picks, dhist = ref.emu_greedy_var(spec, C, nsel, weights=w, keep=keep, perturb=(3, 1e-9))
    with pytest.raises(AssertionError, match="over tau"):
        ref.judge_gvar(name, picks, lambda t: dhist[t], ref.tau(name))


def test_a_downdate_that_overwrites_the_pivot_row_is_rejected():
    """The down-date run over the rows in place without sparing row s: the rows after s see an overwritten pivot row.  The picks
    stay what they were and the winning ratios move by 2e-10 ... 1e-3 relative -- the first of them inside the 1e-7 the suite
    used to allow; the value assertion fails."""
    name, noise = "mi-m32", 1e-3
    spec, C = ref.mi_inputs(name)
    picks, ratios = ref.emu_mi(spec, C, noise, ref.MI_NSEL, ref.MI_START, overwrite_row=True)
    assert np.array_equal(picks, mi_run(name, noise)[0])
    with pytest.raises(AssertionError, match="over tau"):
        ref.judge_mi(name, noise, picks, ratios, ref.tau(ref.mi_key(name, noise)))


# ---- recording -----------------------------------------------------------------------------------------------------------
def record():
    lines = ["# BEGIN TAU_TABLE",
             "# measured %s by `python tests/test_design_replay_host.py --record` (NumPy %s)"
             % (datetime.date.today().isoformat(), np.__version__),
             "TAU_TABLE = {"]
    for key in KEYS:
        got = measured(key)
        dev = float("%.3e" % got["value"])
        lines.append("    %-18s (%r, %r),   # the emulation's pick shortfall: %.1e" % ('"%s":' % key, dev, ref.tau_of(dev), got["pick"]))
        print(lines[-1], flush=True)
    lines += ["}", "# END TAU_TABLE"]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "design_replay_ref.py")
    with open(path) as f:
        text = f.read()
    text = re.sub(r"# BEGIN TAU_TABLE.*# END TAU_TABLE", lambda m: "\n".join(lines), text, flags=re.S)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
