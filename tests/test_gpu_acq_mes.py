"""GPU (-m gpu): max-value entropy search -- gpx_acq_mes, its gradient and q-batch, the VFE forms and costFuncMES -- held to the
per-candidate bounds of the other three costs.

References, the float64 composition, the bound and the mutants: tests/acq_mes_ref.py (pinned on the CPU by
tests/test_acq_mes_host.py); metrics, comparators and the bound rule: tests/acq_ref.py, whose three cost-specific functions stand for
the MES ones inside acq_mes_ref.acq_ref_for_mes.  Fits and batch models: tests/test_gpu_acq_bounds.py's.

  A  the epilogue alone (gpx_dbg_acq_mes_epilogue): gamma from -1e150 to 38.6 at var 1, 1e-6, 1e-300 and 4, negative / zero /
     infinite variances, NaN and infinite means; K = 1, 3, 17, both signs: every cost and (a, b) within epilogue_bound_mes (FIXED
     constants) of the longdouble value, the special values exactly the float64 composition's, the arg-min the first minimum among
     the non-NaN costs for chunks of 0, 128 and 256.
  B  gpx_acq_mes end to end: every candidate of the four cases x y* at / below / above min y in omega_A, device <= 8 x max(LAPACK,
     emulation b = 128) + the float64 composition; once more from the points; one chunked run in a fresh child, equal bits.
  C  gpx_acq_mes_grad: omega_G against the comparators, its costs gpx_acq_mes's bits, every row finite; d = 1 and d = 9.
  D  the winner: the regret check, inside B.
  E  gpx_acq_mes_batch: q = 6, believer and constant liar, 257 candidates with duplicates of training points: every row against the
     longdouble replay of the device's own picks, masked entries NaN, row 0 gpx_acq_mes's bits, two runs bit-identical.
  F  VFE: gpx_vfe_acq_mes = the hook on gpx_vfe_posterior's values, bit for bit; gradient rows, each relative to its own largest
     entry, against Richardson-extrapolated central differences of the longdouble reference cost; batch row 0; a FITC model refused
     by name.
  G  costFuncMES on a dense and a VFE model.

Run with -s: every case prints device, comparators and ratio ("Acquisition accuracy", the MES addendum, quotes
them).

Measured on an MI355X (device / comparators, or device / bound):
  A  |device - longdouble| / epilogue_bound_mes, worst over all rows, sizes, K and signs: cost 0.186, a 0.255, b 0.255 (the float64
     composition on the same rows: 0.186 / 0.255 / 0.255).  No constant was widened.  (A library built with T0 = 3 and 41 terms
     misses this bound 24-fold in a and b at gamma = -4, 2000 u in h': the composition's cancellation below the seam.)
  B  omega_A, tight rule: device 0.23 .. 6.0, device / larger comparator 0.27 .. 1.37 of 8; from the points, after the allowance,
     0 .. 0.03.
  C  omega_G, device / larger comparator: 0.35 .. 1.81 on the cases, 0.59 .. 1.98 at d = 1 and d = 9.
  D  28 picks, all the reference's own best.
  E  omega_A per row: device 0.98 .. 6.4, device / largest comparator 0.25 .. 1.63 of 8.
  F  gradient against longdouble central differences (relative to the largest entry): device 9.2e-10 / 2.5e-9 (sign +1 / -1), the
     NumPy closed form 9.2e-10 / 2.5e-9, the differences' own truncation 2.7e-9 / 7.7e-9."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import acq_mes_ref as M
import acq_ref as A
import posterior_ref as P
import sample_ref as SR
import test_gpu_acq_bounds as TB

pytestmark = pytest.mark.gpu

ROOT, TESTS = TB.ROOT, TB.TESTS
LD = M.LD


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


# ---- A. the epilogue alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", A.EPI_SIZES)
@pytest.mark.parametrize("K", M.EPI_K)
@pytest.mark.parametrize("sign", M.SIGNS)
def test_mes_epilogue_within_its_bound(dev, ctx, sign, K, m):
    ys = M.ystar_of(K)
    worst = {"A": 0.0, "a": 0.0, "b": 0.0}
    failures = []
    rows = M.epilogue_rows_mes(m, sign)
    for r, (mean, var) in enumerate(rows):
        best, best_cost, cost, coef = dev.dbg_acq_mes_epilogue(ctx, ys, sign, mean, var)
        ref = M.reference_costs_mes(ys, sign, mean, var, second=False)
        R = M.epilogue_bound_mes(ys, sign, mean, var)
        want = dict(zip("Aab", M.costs_f64_mes(ys, sign, mean, var)))
        for k, got in (("A", cost), ("a", coef[:, 0]), ("b", coef[:, 1])):
            w = A.judged(ref[k], R[k])
            q = A.bound_ratio(got, ref[k], R[k], w)
            worst[k] = max(worst[k], q)
            if not q <= 1.0:
                j = int(np.flatnonzero(w)[np.argmax(np.asarray(np.abs(got.astype(LD) - ref[k])[w] / R[k][w], dtype=float))])
                failures.append("K=%d sign=%d m=%d row %d %s: |device - reference| = %.3g x bound at mean %r var %r (device %r reference %r)"
                                % (K, sign, m, r, k, q, mean[j], var[j], got[j], float(ref[k][j])))
            if not A.same_pattern(got[~w], want[k][~w]):
                failures.append("K=%d sign=%d m=%d row %d %s: special values %r, the float64 composition's %r at mean %r var %r"
                                % (K, sign, m, r, k, got[~w], want[k][~w], mean[~w], var[~w]))
        SR.check_argbest_bits(np.array([best if best >= 0 else 0]), [best_cost], cost[None, :], label="K=%d m=%d row %d" % (K, m, r))
        assert (best == -1) == bool(np.all(np.isnan(cost)))
    print("\nK=%d sign=%+d m=%d (%d rows): worst |device - reference| / bound  cost %.3f  a %.3f  b %.3f" % (K, sign, m, len(rows), worst["A"], worst["a"], worst["b"]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("m", A.EPI_SIZES)
def test_mes_epilogue_argmin(dev, ctx, m):
    """The first minimum among the non-NaN costs, bit for bit: the row's minimum repeated at candidates 1, 127, 128 and m - 1, NaN at
    candidate 0 and inside the second block, a row of nothing but NaN -> (-1, NaN); chunks of 128 and 256 equal to one launch."""
    ys, sign = M.ystar_of(3), 1
    rng = np.random.default_rng(910 + m)
    mean, var = rng.uniform(-1.0, 1.0, m), rng.uniform(0.5, 2.0, m)
    j = dev.dbg_acq_mes_epilogue(ctx, ys, sign, mean, var)[0]
    ties = sorted({i for i in (1, 127, 128, m - 1) if 0 <= i < m})
    mean[ties], var[ties] = mean[j], var[j]
    rows = [("ties at %s" % ties, mean.copy(), var.copy(), min(ties + [j]))]
    mean[0] = np.nan
    if m > 130:
        mean[130] = np.nan
    rows.append(("NaN at candidate 0 and in the second block", mean.copy(), var.copy(), None))
    rows.append(("all NaN", np.full(m, np.nan), var.copy(), -1))
    for label, mu, v, want in rows:
        one = dev.dbg_acq_mes_epilogue(ctx, ys, sign, mu, v)
        best, best_cost, cost = one[:3]
        print("m=%d %-44s -> pick %d, cost %r" % (m, label, best, best_cost))
        for chunk in (128, 256):
            ch = dev.dbg_acq_mes_epilogue(ctx, ys, sign, mu, v, chunk=chunk)
            assert one[0] == ch[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one[1:], ch[1:])), (m, label, chunk)
        assert np.array_equal(np.isnan(cost), np.isnan(mu)), (m, label)
        if want == -1 or np.all(np.isnan(mu)):                   # (m = 1: the NaN at candidate 0 is the whole row)
            assert best == -1 and np.isnan(best_cost)
            continue
        SR.check_argbest_bits(np.array([best]), [best_cost], cost[None, :], label="m=%d %s" % (m, label))
        if want is not None:
            assert best == want, (m, label, best, want)
    mean, var = M.epilogue_rows_mes(257, -1)[0]                  # the made-to-order row, K = 17, in chunks
    one = dev.dbg_acq_mes_epilogue(ctx, M.ystar_of(17), -1, mean, var)
    for chunk in (128, 256):
        ch = dev.dbg_acq_mes_epilogue(ctx, M.ystar_of(17), -1, mean, var, chunk=chunk)
        assert one[0] == ch[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one[1:], ch[1:])), chunk


def test_mes_argument_errors(dev, ctx):
    from gpexp_amd._lib import GpxError
    mean, var = np.zeros(3), np.ones(3)
    for ys, sign, what in (([0.0, np.nan], 1, r"ystar\[1\]"), ([np.inf], 1, r"ystar\[0\]"), ([0.0], 0, "sign"), ([0.0], 2, "sign"),
                           (np.zeros(0), 1, "GPX_MES_MAX_K|ystar is NULL"), (np.zeros(dev.MES_MAX_K + 1), 1, "GPX_MES_MAX_K")):
        with pytest.raises(GpxError, match=what):
            dev.dbg_acq_mes_epilogue(ctx, ys, sign, mean, var)
    assert np.all(np.isfinite(dev.dbg_acq_mes_epilogue(ctx, np.zeros(dev.MES_MAX_K), 1, mean, var)[2]))


# ---- B, D. gpx_acq_mes end to end, and the winner ---------------------------------------------------------------------------------
def mes(dev, ctx, f, ys, sign=1, **kw):
    return dev.acq_mes(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, ys, sign, **kw)


def judge_costs(label, ys, sign, ref, arrays, best, best_cost, costs):
    with M.acq_ref_for_mes(ys, sign):
        return TB.judge_costs(label, M.MES, 0.0, ref, arrays, best, best_cost, costs)


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_mes_tight_rule(dev, ctx, name):
    f, ref = TB.fit_of(dev, ctx, name)
    failures = []
    print()
    for label, ys in M.ystar_cases(f.c["y"]).items():
        best, best_cost, costs = mes(dev, ctx, f, ys)
        assert mes(dev, ctx, f, ys, want_costs=False) == (best, best_cost, None)
        failures += judge_costs("%s y* %s" % (name, label), ys, 1, ref, (f.K, f.B, f.kd, f.alpha), best, best_cost, costs)
    ys = -M.ystar_cases(-f.c["y"])["at min y"]                              # sampled maxima, at max y
    best, best_cost, costs = mes(dev, ctx, f, ys, sign=-1)
    failures += judge_costs("%s y* at max y, sign -1" % name, ys, -1, ref, (f.K, f.B, f.kd, f.alpha), best, best_cost, costs)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [c for c in A.CASE_NAMES if c in P.FROM_POINTS])
def test_mes_from_points_rule(dev, ctx, name):
    f, _ = TB.fit_of(dev, ctx, name)
    c = f.c
    plans = []
    for args in ((f.dX,), (f.dX, f.dZ)):
        exact, centre = dev.kfill_plan(ctx, f.sp, *args)
        plans.append(("diff", None) if exact else ("expanded", centre))
    plans.append(("diff", None))
    ref = P.reference_from_points(c["spec"], f.X, f.Z, c["nugget"], alpha=f.alpha, forms=tuple(p[0] for p in plans),
                                  centers=tuple(p[1] for p in plans))
    h = ref["f64"]
    failures = []
    print()
    for label, ys in M.ystar_cases(c["y"]).items():
        best, best_cost, costs = mes(dev, ctx, f, ys)
        failures += judge_costs("%s y* %s (points)" % (name, label), ys, 1, ref, (h["K"], h["B"], h["kd"], f.alpha), best, best_cost, costs)
    assert not failures, "\n".join(failures)


def chunk_digest():
    """sha256 of gpx_acq_mes's and gpx_acq_mes_grad's outputs on TB.CHUNK_CASE (its own context: runs in the child as well)."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    f = TB.Fit(dev, ctx, TB.CHUNK_CASE)
    h = hashlib.sha256()
    for label, ys in M.ystar_cases(f.c["y"]).items():
        best, best_cost, costs = mes(dev, ctx, f, ys)
        c2, grad = dev.acq_mes_grad(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, ys, 1)
        for a in (np.int64(best), np.float64(best_cost), costs, c2, grad):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_mes_bits_do_not_depend_on_the_chunking():
    """A fresh child whose GPX_CROSS_BYTES allows 128 candidates per chunk: the 130 candidates go as 128 + 2, the bits stay."""
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_acq_mes as t\nprint('RESULT ' + t.chunk_digest(), flush=True)" % (ROOT, TESTS)],
                       env=dict(os.environ, GPX_CROSS_BYTES="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:] == chunk_digest()


# ---- C. gpx_acq_mes_grad ---------------------------------------------------------------------------------------------------------
def judge_grad(dev, ctx, label, f, ref, ys, sign=1):
    c = f.c
    costs, grad = dev.acq_mes_grad(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, ys, sign)
    assert np.array_equal(costs, mes(dev, ctx, f, ys, sign)[2]), label                                   # gpx_acq_mes's bits
    assert grad.shape == f.Z.shape and np.all(np.isfinite(grad)), label
    assert np.all(ref["val"]["v"] != 0)
    with M.acq_ref_for_mes(ys, sign):
        gref = A.grad_reference(c["spec"], f.X, f.Z, f.K, f.B, f.alpha, M.MES, 0.0, ref)
        cmp_ = A.grad_comparator_omegas(gref, c["spec"], f.X, f.Z, f.K, f.B, f.kd, f.alpha, M.MES, 0.0)
    try:
        A.check_bound("%s omega_G" % label, A.omega_G(grad, gref), cmp_)
    except AssertionError as e:
        return [str(e)]
    return []


def grad_ystars(y):
    cases = M.ystar_cases(y)
    return {k: cases[k] for k in ("at min y", "below min y")}


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_mes_grad_rows(dev, ctx, name):
    f, ref = TB.fit_of(dev, ctx, name)
    failures = []
    print()
    for label, ys in grad_ystars(f.c["y"]).items():
        failures += judge_grad(dev, ctx, "%s y* %s" % (name, label), f, ref, ys)
    failures += judge_grad(dev, ctx, "%s y* at max y, sign -1" % name, f, ref, -M.ystar_cases(-f.c["y"])["at min y"], -1)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d", [1, 9])
@pytest.mark.parametrize("kind", ["se", "matern32", "matern52"])
def test_mes_grad_dimension_classes(dev, ctx, kind, d):
    c = A.dims_case(kind, d)
    f = TB.Fit(dev, ctx, None, c)
    ref = P.reference(f.K, f.B, f.kd, alpha=f.alpha)
    failures = []
    print()
    for label, ys in grad_ystars(c["y"]).items():
        failures += judge_grad(dev, ctx, "%s d=%d y* %s" % (kind, d, label), f, ref, ys)
    assert not failures, "\n".join(failures)


# ---- E. gpx_acq_mes_batch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("liename", ["believer", "min y"])
@pytest.mark.parametrize("name", A.BATCH_CASES)
def test_mes_batch_rows_and_picks(dev, ctx, name, liename):
    b = TB.batch_model(dev, ctx, name)
    c, C = b["c"], b["C"]
    lie, lie_value = (dev.LIE_BELIEVER, 0.0) if liename == "believer" else (dev.LIE_CONSTANT, float(np.min(c["y"])))
    ys = M.ystar_cases(c["y"])["at min y"]
    label = "%s mes %s" % (name, liename)
    run = lambda: dev.acq_mes_batch(ctx, b["sp"], b["L"], b["dX"], b["alpha"], b["dC"], A.BATCH_NOISE, ys, 1, lie, lie_value, A.BATCH_Q,
                                    want_all=True)
    idx, cost, lies, allc = run()
    again = run()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip((idx, cost, lies, allc), again)), label    # two runs: the same bits
    assert len(set(idx.tolist())) == A.BATCH_Q, label
    if lie == dev.LIE_CONSTANT:
        assert np.array_equal(lies, np.full(A.BATCH_Q, lie_value)), label
    assert np.array_equal(allc[0], dev.acq_mes(ctx, b["sp"], b["L"], b["dX"], b["alpha"], b["dC"], ys, 1)[2]), label   # gpx_acq_mes's bits
    failures = []
    with M.acq_ref_for_mes(ys, 1):
        args = (c["spec"], c["X"], c["y"], A.BATCH_NOISE, C, idx, lies, M.MES, 0.0, 0)
        brefs = A.batch_reference(*args, base=b["base"])
        rows = {k: fn(*args, arrays=b["base"].arrays) for k, fn in A.BATCH_COMPARATORS.items()}
        print("\n  %s: picks %s" % (label, idx.tolist()))
        for t in range(A.BATCH_Q):
            assert np.array_equal(np.isnan(allc[t]), brefs[t]["masked"]), (label, t)                # masked entries NaN, no other
            SR.check_argbest_bits(idx[t:t + 1], cost[t:t + 1], allc[t:t + 1], label="%s pick %d" % (label, t))
            cmp_ = {k: A.omega_A_row(r[t], brefs[t]) for k, r in rows.items()}
            try:
                A.check_bound("  pick %d omega_A" % t, A.omega_A_row(allc[t], brefs[t]), cmp_)
                short, allowed = A.batch_regret(brefs[t], int(idx[t]), max(cmp_.values()))
                assert short <= allowed, "%s pick %d = candidate %d: worse than the reference's best by %.3e > %.3e" % (label, t, idx[t], short, allowed)
            except AssertionError as e:
                failures.append("%s: %s" % (label, e))
    assert not failures, "\n".join(failures)


# ---- F. VFE ------------------------------------------------------------------------------------------------------------------------
VFE_CASE = "se-d3"


def test_vfe_mes_values_gradient_batch_and_fitc(dev):
    import test_gpu_vfe_acq as TV
    import vfe_acq_ref as aref
    import vfe_ref as vref
    from gpexp_amd._lib import GpxError
    spec, X, S, y, noise, Z = TV.problem(VFE_CASE)[:6]
    Zg = np.array(TV.problem(VFE_CASE)[8])
    _, ctx, model, coeff = TV.device_model(VFE_CASE)
    Zd = dev.points(ctx, Z)
    dmean, dvar = model.posterior(coeff, Zd)
    for sign, ys in ((1, M.ystar_cases(y)["at min y"]), (-1, -M.ystar_cases(-np.asarray(y))["at min y"])):
        best, best_cost, costs = model.acq_mes(coeff, Zd, ys, sign)
        hook = dev.dbg_acq_mes_epilogue(ctx, ys, sign, dmean, dvar)
        assert np.array_equal(costs, hook[2]) and (best, best_cost) == hook[:2]                            # the hook's bits
        assert model.acq_mes(coeff, Zd, ys, sign, want_costs=False) == (best, best_cost, None)
        # gradient, row by row: Richardson-extrapolated central differences (steps h, 2 h, 4 h with h = 3e-4: truncation O(h^4)) of the
        # longdouble reference cost on vfe_ref's float64 predictor; the comparator is the closed form in NumPy (vfe_acq_ref.grad_setup
        # with the float64 composition's (a, b)).  Each row is judged relative to its own largest entry; the floor of a row is the
        # differences' own error there, |R(h) - R(2 h)| / 15 (the predictor's float64 rounding over h, and what is left of h^4)
        c2, G = model.acq_mes_grad(coeff, dev.points(ctx, Zg), ys, sign)
        assert np.array_equal(c2, model.acq_mes(coeff, dev.points(ctx, Zg), ys, sign)[2]) and np.all(np.isfinite(G))
        ref_cost = lambda Pts: np.asarray(M.reference_costs_mes(ys, sign, *vref.predict(spec, X, S, y, noise, Pts), second=False)["A"])
        f1, f2, f4 = (aref.central_differences(ref_cost, Zg, h=k * 3e-4) for k in (1, 2, 4))
        R1, R2 = (4 * f1 - f2) / 3, (4 * f2 - f4) / 3
        setup = aref.grad_setup(spec, X, S, y, noise, Zg)
        _, a, b = M.costs_f64_mes(ys, sign, setup["mean"], setup["var"])
        closed = np.array([dk.T @ (a[j] * setup["beta_u"] - 2.0 * b[j] * setup["gamma"][:, j]) for j, dk in enumerate(setup["dk"])])
        rowmax = lambda x: np.max(np.abs(np.asarray(x, dtype=float)), axis=1)
        scale = rowmax(R1)
        floor, e_dev, e_cmp = rowmax(R1 - R2) / 15.0 / scale, rowmax(G - R1) / scale, rowmax(closed - R1) / scale
        ratio = e_dev / np.maximum(e_cmp, floor)
        print("vfe %s sign %+d: gradient rows against Richardson differences: device %.2e .. %.2e, NumPy closed form %.2e .. %.2e, "
              "differences' own %.2e .. %.2e; device / max(closed form, floor) per row at most %.2f of %g"
              % (VFE_CASE, sign, e_dev.min(), e_dev.max(), e_cmp.min(), e_cmp.max(), floor.min(), floor.max(), ratio.max(), A.MARGIN))
        assert np.all(e_dev <= A.MARGIN * np.maximum(e_cmp, floor)), (e_dev, e_cmp, floor)
        # batch: row 0 holds gpx_vfe_acq_mes's bits; two runs agree
        run = lambda: model.acq_mes_batch(coeff, Zd, ys, sign, dev.LIE_BELIEVER, 0.0, 6, want_all=True)
        one, two = run(), run()
        assert np.array_equal(one[3][0], costs) and all(np.array_equal(x, z, equal_nan=True) for x, z in zip(one, two))
        TV.self_consistent(one[0], one[1], one[3])
    fitc = TV.device_model(VFE_CASE, cls="FitcModel")[2]
    ys = M.ystar_cases(y)["at min y"]
    for call, what in ((lambda: dev.VfeModel.acq_mes(fitc, coeff, Zd, ys, 1), "vfe_acq_mes:"),
                       (lambda: dev.VfeModel.acq_mes_grad(fitc, coeff, Zd, ys, 1), "vfe_acq_mes_grad:"),
                       (lambda: dev.VfeModel.acq_mes_batch(fitc, coeff, Zd, ys, 1, dev.LIE_BELIEVER, 0.0, 2), "vfe_acq_mes_batch:")):
        with pytest.raises(GpxError, match="FITC model") as e:
            call()
        assert what in str(e.value)


# ---- G. the class ------------------------------------------------------------------------------------------------------------------
def make_mes_cost(sparse, flip=False, yStar=None):
    import test_gpu_vfe_acq as TV
    from gpExp.experimentalDesign import costFuncMES
    spec, X, S, y, noise = TV.problem(VFE_CASE)[:5]
    X, y = np.array(X), np.array(y)
    np.random.seed(3)
    kw = {} if sparse == "dense" else (dict(FITC=0.5, sparse="vfe") if sparse == "vfe" else dict(FITC=0.5))
    gp = TV.make_gp(spec, noise, None if sparse == "dense" else S, **kw)
    return costFuncMES(gp, X, -y if flip else y, 2, TV.Space(spec["d"]), yStar=yStar, minimize=not flip)


@pytest.mark.parametrize("sparse", ["dense", "vfe"])
def test_costFuncMES(dev, sparse):
    import test_gpu_vfe_acq as TV
    from gpexp_amd.experimentalDesign import _AcqCalls, firstMinIndex, optimizeAcquisition
    from gpexp_amd.paths import PathBase
    spec, X, S, y, noise, Z = TV.problem(VFE_CASE)[:6]
    Z, d = np.array(Z), spec["d"]
    ys = M.ystar_cases(y)["at min y"]
    cf = make_mes_cost(sparse)
    for call in (cf.evaluateBatch, cf.bestCandidate, cf.derivativeBatch, lambda C: cf.selectBatch(C, 2), lambda C: cf.evaluate(C)):
        with pytest.raises(ValueError, match="yStar"):
            call(Z)
    cf.yStar = ys
    ctx, gp, Zd = cf._dense(Z)
    best, best_cost, want = _AcqCalls(ctx, gp).acq(Zd, dev.ACQ_MES, (ys, 1))
    costs = cf.evaluateBatch(Z)
    assert np.array_equal(costs, want) and cf.bestCandidate(Z) == (best, best_cost) and best == firstMinIndex(costs)   # the device call
    c2, G = cf.evaluateBatchWithDerivative(Z[:24])
    assert G.shape == (24, d) and np.array_equal(cf.derivativeBatch(Z[:24]), G) and cf.derivative(Z[:7]).shape == (d,)
    # evaluate of a row: a single-row GP.evaluate (|var|) and the host composition, to the composition's bound on that posterior.  Its
    # entry of evaluateBatch is the device epilogue on the BATCH posterior (mB, vB), whose fill is centred on another bounding box: the
    # two agree to both epilogue bounds plus the first-order effect of the posteriors' difference, |a| |m1 - mB| + |b| |v1 - vB|
    # (S_A's form with the measured differences in place of u S_m, u S_v), doubled for the second order like the bounds themselves
    mB, vB = (np.ravel(x) for x in cf.gaussianProcess.evaluate(Z, compvar=1))
    for j in (0, 7, 123, 299):
        one = cf.evaluate(Z[:j + 1])
        assert isinstance(one, float)
        m1, v1 = (np.ravel(x) for x in cf.gaussianProcess.evaluate(Z[j:j + 1], compvar=1))
        R1 = M.epilogue_bound_mes(ys, 1, m1, v1)["A"][0]
        ref1 = M.reference_costs_mes(ys, 1, m1, v1, second=False)
        assert abs(one - float(ref1["A"][0])) <= R1, (j, one, float(ref1["A"][0]), R1)
        RB = M.epilogue_bound_mes(ys, 1, mB[j:j + 1], vB[j:j + 1])["A"][0]
        moved = abs(float(ref1["a"][0])) * abs(m1[0] - mB[j]) + abs(float(ref1["b"][0])) * abs(v1[0] - vB[j])
        print("%s candidate %d: |evaluate - evaluateBatch| %.2e, allowed %.2e (bounds %.2e + %.2e, posterior moved %.2e)"
              % (sparse, j, abs(one - costs[j]), R1 + RB + 2.0 * moved, R1, RB, moved))
        assert abs(one - costs[j]) <= R1 + RB + 2.0 * moved, (j, one, costs[j], R1, RB, moved)
    idx, c, allc = cf.selectBatch(Z, 4, lie="min", returnAllCosts=True)
    TV.self_consistent(idx, c, allc)
    assert np.array_equal(allc[0], costs)
    pt, cost, j = optimizeAcquisition(cf, Z, nStarts=4, maxiter=20)
    assert pt.shape == (1, d) and j == best and cost <= best_cost
    # sampleOptima: the values of thompsonPaths on the same base; gumbel from one GP.evaluate
    nu = np.asarray(S).shape[0]
    base = PathBase.draw(5, 64, 2 * nu if sparse == "vfe" else np.asarray(X).shape[0], d, cf.gaussianProcess.kernel, rng=1)
    draw = cf.vfeThompsonPaths if sparse == "vfe" else cf.thompsonPaths
    got = cf.sampleOptima(Z, nOptima=5, nFeatures=64, base=base)
    assert got is cf.yStar and np.array_equal(got, draw(Z, 5, nFeatures=64, base=base)[1]) and np.all(np.isfinite(cf.evaluateBatch(Z)))
    r = np.array([0.1, 0.5, 0.9])
    mean, var = cf.gaussianProcess.evaluate(Z, compvar=1)
    from gpexp_amd.experimentalDesign import gumbelOptima
    assert np.array_equal(cf.sampleOptima(Z, nOptima=3, method="gumbel", uniforms=r), gumbelOptima(np.ravel(mean), np.sqrt(np.ravel(var)), r))
    with pytest.raises(ValueError):
        cf.sampleOptima(Z, nOptima=3, method="gumbel", uniforms=r[:2])
    with pytest.raises(ValueError):
        cf.sampleOptima(Z, nOptima=3, method="other")
    # minimize=False on -y reproduces minimize=True on y, bit for bit
    mirror = make_mes_cost(sparse, flip=True, yStar=-ys)
    assert np.array_equal(mirror.evaluateBatch(Z), costs)


def test_costFuncMES_refuses_fitc_and_mehler_gradients():
    import test_gpu_vfe_acq as TV
    from gpExp.experimentalDesign import costFuncMES
    from gpexp_amd._lib import GpxError
    Z = np.array(TV.problem(VFE_CASE)[5])
    fitc = make_mes_cost("fitc", yStar=[0.0])
    for call in (fitc.evaluateBatch, fitc.bestCandidate, fitc.derivativeBatch, lambda C: fitc.selectBatch(C, 2)):
        with pytest.raises(NotImplementedError):
            call(Z)
    ucb, C = TV.mehler_cost()
    cf = costFuncMES(ucb.gaussianProcess, ucb.xTrain, ucb.yTrain, 2, TV.Space(2), yStar=[float(np.min(ucb.yTrain))])
    assert np.all(np.isfinite(cf.evaluateBatch(C)))
    with pytest.raises((GpxError, NotImplementedError), match="Mehler"):
        cf.derivativeBatch(C)
    assert cf.sampleOptima(C, nOptima=4, method="gumbel", uniforms=[0.2, 0.4, 0.6, 0.8]).shape == (4,)
