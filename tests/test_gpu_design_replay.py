"""The sequential design selectors held to a high-precision replay of their own picks (-m gpu).

gpx_greedy_var, gpx_mi_greedy / gpx_mi_* and multi-pick gpx_greedy_ivar carry a state through up to nsel rank-one steps.  At
every checked step the picks the DEVICE made before it are taken as given, every candidate's score is recomputed from scratch
in np.longdouble (tests/design_replay_ref.py), and the device is held to: the value it reports within tau, its pick within tau of
the replay's best, distinct picks.  No step is skipped for want of a clear winner.  tau comes from the table recorded by
tests/test_design_replay_host.py (32 x the deviation of a float64 emulation of the same recurrence, floor 64 u) and never from a
device result; every figure is printed before it is asserted.  The structural rules that have no tolerance -- the first-maximum
rule across threads, blocks and the grid-stride wrap of argmax_stage1, the dropped pivot of greedy_row_kernel, the row-sharded MI
state machine against the single call -- are compared exactly.

Device deviations observed on an MI355X next to their tau (2026-10-19; every pick was the replay's best, shortfall 0):
    gvar-se2 2.0e-15 / 4.8e-14    gvar-m32 4.3e-15 / 1.2e-13    gvar-m52 1.7e-15 / 7.8e-14    gvar-se1 5.1e-16 / 1.9e-14
    mi-se2   noise 0.1: 4.4e-14 / 8.8e-13    1e-3: 1.6e-11 / 3.4e-10    1e-6: 7.4e-9 / 5.3e-8
    mi-m52   noise 0.1: 6.8e-14 / 1.9e-12    1e-3: 7.6e-13 / 2.0e-11    1e-6: 5.2e-12 / 2.2e-10
    mi-m32   noise 0.1: 2.0e-14 / 1.0e-12    1e-3: 7.7e-13 / 1.5e-11    1e-6: 9.0e-12 / 2.4e-10
    mi-large 1.1e-13 / 2.3e-12    givar-se2 1.6e-14 / 3.2e-13    givar-m52 8.1e-15 / 2.3e-13
"""
import numpy as np
import pytest

import design_replay_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def spec_of(dev, s):
    from test_gpu_parity import spec_of as f
    return f(dev, s)


# ---- greedy variance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.GVAR))
def test_greedy_variance_replay(dev, ctx, name):
    """Per checked step t: the hook's d on the device's first t picks against cond_var (tau relative to the prior), and the
    device's pick t against cond_var * weights."""
    s, C, nsel, w, keep = ref.gvar_inputs(name)
    spec, Cd = spec_of(dev, s), dev.points(ctx, C)
    picks = dev.greedy_var(ctx, spec, Cd, nsel, keep=keep, weights=w)
    assert picks[:len(keep)].tolist() == keep
    jd = ref.judge_gvar(name, picks, lambda t: dev.dbg_greedy_var_scores(ctx, spec, Cd, picks[:t]), ref.tau(name))
    print("%s: smallest longdouble pivot / prior among the device's picks %.3g" % (name, jd.minpiv))
    assert jd.minpiv >= 1e-5


_base = {}


def tie_base(dev, ctx):
    """300 points (SE, d = 2) with weights, and greedy_var's six picks on them; computed once."""
    if not _base:
        s, C, nsel, w, keep = ref.gvar_inputs("gvar-se2")
        _base["in"] = (s, C, w)
        _base["picks"] = dev.greedy_var(ctx, spec_of(dev, s), dev.points(ctx, C), 6, weights=w)
    return _base["in"] + (_base["picks"],)


@pytest.mark.parametrize("r", [2, 4, 875])
def test_first_maximum_rule_is_exact(dev, ctx, r):
    """r bitwise copies of every candidate have bitwise-equal scores at every step, so the lowest copy must win: the picks on
    tile(B, r) ARE the picks on B.  r = 875: M = 262500, past the 1024-block cap of argmax_stage1 (the grid-stride wrap)."""
    s, C, w, base = tie_base(dev, ctx)
    got = dev.greedy_var(ctx, spec_of(dev, s), dev.points(ctx, np.tile(C, (r, 1))), 6, weights=np.tile(w, r))
    print("r = %d: %s against %s" % (r, got.tolist(), base.tolist()))
    assert got.tolist() == base.tolist()


def test_dropped_pivot_conditions_nothing(dev, ctx):
    """C[j] a bitwise copy of C[i]: after keep = [i] the pivot of j is at round-off, is dropped (w = 0) and must leave d and every
    later pick exactly as they were."""
    s, C, w, _ = tie_base(dev, ctx)
    i, j, n = 7, 150, 8
    C = C.copy()
    C[j] = C[i]
    spec, Cd = spec_of(dev, s), dev.points(ctx, C)
    d1 = dev.dbg_greedy_var_scores(ctx, spec, Cd, [i])
    d2 = dev.dbg_greedy_var_scores(ctx, spec, Cd, [i, j])
    print("pivot of the copy after its original: %.3g (prior %.3g)" % (d1[j], s["signalSize"]))
    assert abs(d1[j]) <= 1e-13 * s["signalSize"]          # the case really is the dropped one
    assert d2.tobytes() == d1.tobytes()
    a = dev.greedy_var(ctx, spec, Cd, n + 1, keep=[i, j])
    b = dev.greedy_var(ctx, spec, Cd, n, keep=[i])
    assert a[:2].tolist() == [i, j] and a[2:].tolist() == b[1:].tolist()


# ---- mutual information ------------------------------------------------------------------------------------------------------
_mi = {}


def mi_device(dev, ctx, name, noise):
    """mi_greedy's picks and ratios of a configuration; computed once and left unchanged."""
    if (name, noise) not in _mi:
        s, C = ref.mi_inputs(name)
        _mi[(name, noise)] = dev.mi_greedy(ctx, spec_of(dev, s), dev.points(ctx, C), noise, ref.MI_NSEL, start=ref.MI_START)
    return _mi[(name, noise)]


@pytest.mark.parametrize("noise", ref.MI_NOISES)
@pytest.mark.parametrize("name", list(ref.MI))
def test_mutual_information_replay(dev, ctx, name, noise):
    """Steps {1, 2, 12, 23} of 24: out_ratio[t - 1] against the replay's ratio at the device's pick (var(c | A) with noisy
    observations over 1 / [(K_SS + noise I)^-1]_cc - noise, the longdouble inverse recomputed for this A), near-optimality over
    all live candidates, distinct picks."""
    picks, ratios = mi_device(dev, ctx, name, noise)
    assert picks[0] == ref.MI_START
    ref.judge_mi(name, noise, picks, ratios, ref.tau(ref.mi_key(name, noise)))


def test_mutual_information_replay_large(dev, ctx):
    """M = 1100 (five column blocks, past the 1024-stride of argmax_block_kernel), every step: the winning ratio against
    refined_ratio, and the winner's refined ratio against the eight best of a from-scratch float64 ranking."""
    name, s, M, noise, nsel, _ = ref.MI_LARGE
    C = ref.mi_inputs(name)[1]
    picks, ratios = dev.mi_greedy(ctx, spec_of(dev, s), dev.points(ctx, C), noise, nsel, start=ref.MI_START)
    ref.judge_mi_large(picks, ratios, ref.tau(name))


@pytest.mark.parametrize("name", [n for n in ref.MI if ref.MI[n][1] == 260])
def test_mi_state_machine_is_the_replayed_selector(dev, ctx, name):
    """The M = 260, noise 1e-3 cases through gpx_mi_* with lo = 0, hi = M, and split as (0, 130) + (130, 260): the picks and
    ratios of mi_greedy bit for bit, so the replay's verdict covers the form the distributed design runs."""
    from gpexp_amd import dist
    noise = 1e-3
    want_p, want_r = mi_device(dev, ctx, name, noise)
    s, C = ref.mi_inputs(name)
    M = C.shape[0]
    spec, Cd = spec_of(dev, s), dev.points(ctx, C)
    for ranges in ([(0, M)], [(0, 130), (130, M)]):
        states = [dev.MiState(ctx, spec, Cd, noise, ref.MI_NSEL, ref.MI_START, lo, hi) for lo, hi in ranges]
        row = dev.alloc_vector(ctx, M)
        picks, ratios = [ref.MI_START], []
        for cur in range(ref.MI_NSEL - 1):
            for st in states:
                st.row(cur, row)            # only the owner of picks[-1] writes the buffer
            ctx.sync()
            res = [st.score(cur, row) for st in states]
            best = dist.merge_argmax([v for v, _ in res], [i for _, i in res])
            for st in states:
                st.select(cur + 1, best[1])
            picks.append(best[1])
            ratios.append(best[0])
        assert picks == want_p.tolist(), ranges
        assert np.array(ratios).tobytes() == want_r.tobytes(), ranges


# ---- multi-pick greedy IVAR ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.GIVAR))
def test_greedy_ivar_replay(dev, ctx, name):
    """Rows {0, 1, nsel/2, nsel-1} of all_costs against givar_costs on the device's picks: all M entries, each within tau of the
    row's smallest cost; near-optimality of each checked pick."""
    s, X0, C, Z, noise, nsel = ref.givar_inputs(name)
    spec, Xd = spec_of(dev, s), dev.points(ctx, X0)
    L = dev.potrf(ctx, dev.kfill(ctx, spec, Xd, nugget=float(noise)))
    idx, cost, allc = dev.greedy_ivar(ctx, spec, L, Xd, dev.points(ctx, C), dev.points(ctx, Z), noise, nsel, want_all=True)
    assert all(cost[t] == allc[t, idx[t]] for t in range(nsel))
    ref.judge_givar(name, idx, allc, ref.tau(name))
