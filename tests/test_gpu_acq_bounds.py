"""GPU (-m gpu): the acquisition costs UCB, PI and EI of gpx_acq, their gradients and the q-batch picks held to per-candidate bounds.

Metric, references, comparators, mutants and the bound rule: tests/acq_ref.py (pinned on the CPU by tests/test_acq_host.py).

  A  the epilogue alone (gpx_dbg_acq_epilogue): made-to-order means and signed variances -- g from -38.6 to 9 at var 1, 1e-6, 1e-300
     and 4, negative / zero / infinite variances, NaN and infinite means -- each cost and each (a, b) within acq_ref.epilogue_bound
     (FIXED library constants: erfc 16 ulp, exp 3 ulp) of the longdouble value, the special values exactly the float64
     composition's, and the arg-min the first minimum among the non-NaN costs, bit for bit, whatever the chunking.
  B  gpx_acq end to end: every candidate of the four cases x {max y, median y, min y} x {UCB, PI, EI} in omega_A, device <= 8 x
     max(LAPACK, emulation b = 128) + bo_compose.costs on the device's own fills taken back; once more from the points with the
     assembly's allowance; one chunked run in a fresh child process, equal bits.
  C  gpx_acq_grad: every row in omega_G (acq_ref: the first-order effect of a relative perturbation u of every input on the row),
     device <= 8 x the comparators (bo_compose.DenseModel.grad restated on the same arrays); its costs are gpx_acq's bits; every
     row finite; d = 1 and d = 9 at n = 60 besides the cases' d = 3.
  D  the winner: gpx_acq's pick is the first arg-min of the costs it returns, and the reference's cost at that pick is within
     2 u MARGIN max(comparators) S_A of the reference's smallest cost.
  E  gpx_acq_batch (believer / constant liar, q = 6, 257 candidates with duplicates of training points and pairs 1e-7 apart):
     every row of all_costs against the longdouble replay of the device's own picks and believed values on the grown system (the
     model on X from the device's fills taken back, the picks' rows from the points), float64 comparators on the same arrays (the
     refit loop through LAPACK; the rank-one recurrence of include/gpx.h through LAPACK and through the b = 128 emulation, whose
     end-to-end mean is the device's kind of solve), masked entries NaN exactly, every pick under the regret check of D, row 0
     gpx_acq's bits.

Run with -s: every case prints device, comparators and ratio ("Acquisition accuracy", quotes them).

Measured on an MI355X (device / comparators, or device / bound):
  A  |device - longdouble| / epilogue_bound, worst over all rows and sizes:  UCB cost 0.41, b 0.05;  PI cost 0.17, a 0.23, b 0.23;
     EI cost 0.18, a 0.17, b 0.23 (the float64 composition on the same rows: 0.41 / 0.05, 0.15 / 0.23 / 0.23, 0.18 / 0.15 / 0.23).
     The device library's erfc and exp stay inside the fixed 16 and 3 ulp down to the subnormal range; no constant was widened.
  B  omega_A, tight rule, device / LAPACK / b128, range over the runs of a case:
       se-well          UCB 0.67 / 1.7 / 1.8    PI 0.23 .. 1.1 / 0.61 .. 3.1 / 0.41 .. 3.4    EI 0.32 .. 0.41 / 0.78 .. 1.1 / 0.59 .. 1.1
       se-tiny-noise    UCB 0.40 / 0.79 / 0.79  PI 0.20 .. 0.23 / 0.21 .. 0.26 / 0.19 .. 0.32  EI 0.20 .. 0.39 / 0.27 .. 0.80 / 0.32 .. 0.80
       m52-tiny-noise   UCB 4.5 / 4.8 / 6.0     PI 0.39 .. 0.99 / 0.23 .. 1.0 / 0.32 .. 1.2    EI 0.37 .. 0.64 / 0.65 .. 0.78 / 0.53 .. 0.78
       m32-per-point    UCB 5.4 / 6.3 / 8.4     PI 0.28 .. 2.5 / 0.34 .. 3.0 / 0.30 .. 5.6     EI 0.54 .. 2.2 / 0.55 .. 2.2 / 0.55 .. 4.9
     device / larger comparator 0.28 .. 1.20 of 8.  From the points, after the allowance: device 0 .. 0.04, comparators 0.14 .. 8.1.
  C  omega_G, device / larger comparator: 0.37 .. 1.31 on the cases but for EI at median y on m52-tiny-noise (4.5 against 0.92:
     4.85 of 8); d = 1: 0.44 .. 1.54, d = 9: 0.44 .. 2.79.  (The scale's solve term is a worst-case componentwise bound: on
     se-tiny-noise device and comparators alike score 2e-5 .. 2e-2.)
  D  56 picks (tight rule and from the points): 54 are the reference's own best, two (se-well, PI at median y) lie 5.4e-20 above it
     where 3.5e-13 is allowed.
  E  omega_A per row, device / refit / rank-one / rank-one b128:  m52-tiny-noise 1.9 .. 5.6 / 0.52 .. 4.3 / 0.71 .. 7.7 / 1.7 .. 6.0,
     se-tiny-noise 2.9 .. 3.3 / 0.47 .. 1.0 / 0.54 .. 0.58 / 2.1 .. 2.4: device / largest comparator 0.72 .. 1.58 of 8.  On se-tiny-noise the
     device's 3 is its end-to-end mean through explicit 128-order inverses (omega_M 2.1 in test_gpu_posterior_bounds.py), which
     the b128 comparator shares and the two LAPACK ones do not.  All 96 picks pass the regret check."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

import acq_ref as A
import kernel_reference as KR
import posterior_ref as P
import sample_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
CHUNK_CASE = "se-tiny-noise"


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


class Fit:
    """One case on the device: the fills taken back, the factor, the host's alpha (test_gpu_posterior_bounds.Fit).  `c`: a case dict
    in place of a name of posterior_ref's (then alpha is LAPACK's solve on the fill taken back)."""

    def __init__(self, dev, ctx, name, c=None):
        c = P.case(name) if c is None else c
        self.c, self.sp = c, dev.KernelSpec(P.KIND_ID[c["spec"]["kind"]], c["spec"]["d"], KR.hyp_of(c["spec"]))
        self.X, self.Z = c["X"], c["Z"]
        self.dX, self.dZ = dev.points(ctx, self.X), dev.points(ctx, self.Z)
        Kd = dev.kfill(ctx, self.sp, self.dX, nugget=c["nugget"])
        self.K = Kd.to_host()
        self.B = dev.kfill(ctx, self.sp, self.dX, Z=self.dZ).to_host()
        self.kd = dev.kdiag(ctx, self.sp, self.dZ)
        ctx.sync()
        self.L = dev.potrf(ctx, Kd)
        self.alpha = P.host_alpha(name) if name is not None else sl.cho_solve(sl.cho_factor(self.K, lower=True), c["y"])


_FITS = {}


def fit_of(dev, ctx, name):
    """(Fit, posterior reference on its arrays), once per module."""
    if name not in _FITS:
        f = Fit(dev, ctx, name)
        _FITS[name] = (f, P.reference(f.K, f.B, f.kd, alpha=f.alpha))
    return _FITS[name]


def runs_of(c):
    """[(label, acq, param)]: UCB once (its param is kappa), PI and EI at the three fBest of the case."""
    out = [("ucb", A.UCB, A.KAPPA)]
    for pn, p in A.params_of(c["y"]).items():
        out += [("pi %s" % pn, A.PI, p), ("ei %s" % pn, A.EI, p)]
    return out


# ---- A. the epilogue alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", A.EPI_SIZES)
@pytest.mark.parametrize("acqname", list(A.ACQS))
def test_epilogue_within_its_bound(dev, ctx, acqname, m):
    acq = A.ACQS[acqname]
    par = A.param_for(acq, 0.0)
    worst = {"A": 0.0, "a": 0.0, "b": 0.0}
    failures = []
    rows = A.epilogue_rows(m)
    for r, (mean, var) in enumerate(rows):
        best, best_cost, cost, coef = dev.dbg_acq_epilogue(ctx, acq, par, mean, var)
        ref = A.reference_costs(acq, par, mean, var)
        R = A.epilogue_bound(acq, par, mean, var)
        want = dict(zip("Aab", A.costs_f64(acq, par, mean, var)))
        for k, got in (("A", cost), ("a", coef[:, 0]), ("b", coef[:, 1])):
            w = A.judged(ref[k], R[k])
            q = A.bound_ratio(got, ref[k], R[k], w)
            worst[k] = max(worst[k], q)
            if not q <= 1.0:
                j = int(np.flatnonzero(w)[np.argmax(np.asarray(np.abs(got.astype(A.LD) - ref[k])[w] / R[k][w], dtype=float))])
                failures.append("%s m=%d row %d %s: |device - reference| = %.3g x bound at mean %r var %r (device %r reference %r)"
                                % (acqname, m, r, k, q, mean[j], var[j], got[j], float(ref[k][j])))
            if not A.same_pattern(got[~w], want[k][~w]):
                failures.append("%s m=%d row %d %s: special values %r, the float64 composition's %r at mean %r var %r"
                                % (acqname, m, r, k, got[~w], want[k][~w], mean[~w], var[~w]))
        SR.check_argbest_bits(np.array([best if best >= 0 else 0]), [best_cost], cost[None, :], label="%s m=%d row %d" % (acqname, m, r))
        assert (best == -1) == bool(np.all(np.isnan(cost)))
    print("\n%s m=%d (%d rows): worst |device - reference| / bound  cost %.3f  a %.3f  b %.3f" % (acqname, m, len(rows), worst["A"], worst["a"], worst["b"]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("m", A.EPI_SIZES)
def test_epilogue_argmin(dev, ctx, m):
    """The first minimum among the non-NaN costs, bit for bit: ties at candidates 1, 127, 128 and m - 1, NaN at candidate 0 and
    inside the second block, a row of nothing but NaN -> (-1, NaN), chunks of 128 equal to one launch."""
    for label, mean, var in A.argmin_rows(m):
        best, best_cost, cost, coef = dev.dbg_acq_epilogue(ctx, A.UCB, A.KAPPA, mean, var)
        best_c, best_cost_c, cost_c, coef_c = dev.dbg_acq_epilogue(ctx, A.UCB, A.KAPPA, mean, var, chunk=128)
        assert best == best_c and np.array_equal([best_cost], [best_cost_c], equal_nan=True), (m, label)
        assert np.array_equal(cost, cost_c, equal_nan=True) and np.array_equal(coef, coef_c, equal_nan=True), (m, label)
        print("m=%d %-44s -> pick %d, cost %r" % (m, label, best, best_cost))
        if np.all(np.isnan(mean)):
            assert best == -1 and np.isnan(best_cost) and np.all(np.isnan(cost)), (m, label)
            continue
        assert np.array_equal(np.isnan(cost), np.isnan(mean)), (m, label)
        SR.check_argbest_bits(np.array([best]), [best_cost], cost[None, :], label="m=%d %s" % (m, label))
    mean, var = A.epilogue_rows(257)[0]
    for acq in (A.PI, A.EI):                      # the made-to-order row, every special value in it, in chunks of 128 and 256
        one = dev.dbg_acq_epilogue(ctx, acq, 0.0, mean, var)
        for chunk in (128, 256):
            ch = dev.dbg_acq_epilogue(ctx, acq, 0.0, mean, var, chunk=chunk)
            assert one[0] == ch[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one[1:], ch[1:])), (acq, chunk)


# ---- B, D. gpx_acq end to end, and the winner --------------------------------------------------------------------------------------
def judge_costs(label, acq, par, ref, arrays, best, best_cost, costs):
    """omega_A of the device's costs against the bound, then the pick: the first arg-min of the returned costs (bits) and the regret
    check.  `arrays` = (K, B, kd, alpha) the comparators start from.  Returns the failures' messages."""
    cref = A.cost_reference(acq, par, ref)
    cmp_ = A.comparator_omegas(acq, par, cref, *arrays)
    failures = []
    try:
        A.check_bound("%s omega_A" % label, A.omega_A(costs, cref), cmp_)
    except AssertionError as e:
        failures.append(str(e))
    SR.check_argbest_bits(np.array([best]), [best_cost], costs[None, :], label=label)
    try:
        A.check_regret(label, cref, best, max(cmp_.values()))
    except AssertionError as e:
        failures.append(str(e))
    return failures


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_acq_tight_rule(dev, ctx, name):
    f, ref = fit_of(dev, ctx, name)
    failures = []
    print()
    for label, acq, par in runs_of(f.c):
        best, best_cost, costs = dev.acq(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, acq, par)
        failures += judge_costs("%s %s" % (name, label), acq, par, ref, (f.K, f.B, f.kd, f.alpha), best, best_cost, costs)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [c for c in A.CASE_NAMES if c in P.FROM_POINTS])
def test_acq_from_points_rule(dev, ctx, name):
    f, _ = fit_of(dev, ctx, name)
    c = f.c
    plans = []
    for args in ((f.dX,), (f.dX, f.dZ)):
        exact, centre = dev.kfill_plan(ctx, f.sp, *args)
        plans.append(("diff", None) if exact else ("expanded", centre))
    plans.append(("diff", None))                  # (K(Z, Z) is not formed: its slot is unused without want_cov)
    ref = P.reference_from_points(c["spec"], f.X, f.Z, c["nugget"], alpha=f.alpha, forms=tuple(p[0] for p in plans),
                                  centers=tuple(p[1] for p in plans))
    h = ref["f64"]
    failures = []
    print()
    for label, acq, par in runs_of(c):
        best, best_cost, costs = dev.acq(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, acq, par)
        failures += judge_costs("%s %s (points)" % (name, label), acq, par, ref, (h["K"], h["B"], h["kd"], f.alpha), best, best_cost, costs)
    assert not failures, "\n".join(failures)


def chunk_digest():
    """sha256 of gpx_acq's outputs on CHUNK_CASE (its own context: runs in the child as well)."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    f = Fit(dev, ctx, CHUNK_CASE)
    h = hashlib.sha256()
    for label, acq, par in runs_of(f.c):
        best, best_cost, costs = dev.acq(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, acq, par)
        for a in (np.int64(best), np.float64(best_cost), costs):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_acq_bounds as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


def test_acq_bits_do_not_depend_on_the_chunking():
    """A fresh child whose GPX_CROSS_BYTES allows 128 candidates per chunk: the 130 candidates go as 128 + 2 and give the bits of
    the one-chunk call (costs, pick and its cost, every cost kind and fBest)."""
    assert run_child("print('RESULT ' + t.chunk_digest(), flush=True)", {"GPX_CROSS_BYTES": "1"}) == chunk_digest()


# ---- C. gpx_acq_grad ---------------------------------------------------------------------------------------------------------------
def judge_grad(dev, ctx, label, f, ref, acq, par):
    c = f.c
    costs, grad = dev.acq_grad(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, acq, par)
    assert np.array_equal(costs, dev.acq(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, acq, par)[2]), label      # gpx_acq's bits
    assert grad.shape == f.Z.shape and np.all(np.isfinite(grad)), label                                   # (no reference variance is 0)
    assert np.all(ref["val"]["v"] != 0)
    gref = A.grad_reference(c["spec"], f.X, f.Z, f.K, f.B, f.alpha, acq, par, ref)
    cmp_ = A.grad_comparator_omegas(gref, c["spec"], f.X, f.Z, f.K, f.B, f.kd, f.alpha, acq, par)
    try:
        A.check_bound("%s omega_G" % label, A.omega_G(grad, gref), cmp_)
    except AssertionError as e:
        return [str(e)]
    return []


def grad_runs(c):
    out = [("ucb", A.UCB, A.KAPPA)]
    for pn in ("median y", "min y"):
        p = A.params_of(c["y"])[pn]
        out += [("pi %s" % pn, A.PI, p), ("ei %s" % pn, A.EI, p)]
    return out


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_acq_grad_rows(dev, ctx, name):
    f, ref = fit_of(dev, ctx, name)
    failures = []
    print()
    for label, acq, par in grad_runs(f.c):
        failures += judge_grad(dev, ctx, "%s %s" % (name, label), f, ref, acq, par)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d", [1, 9])
@pytest.mark.parametrize("kind", ["se", "matern32", "matern52"])
def test_acq_grad_dimension_classes(dev, ctx, kind, d):
    c = A.dims_case(kind, d)
    f = Fit(dev, ctx, None, c)
    ref = P.reference(f.K, f.B, f.kd, alpha=f.alpha)
    failures = []
    print()
    for label, acq, par in grad_runs(c):
        failures += judge_grad(dev, ctx, "%s d=%d %s" % (kind, d, label), f, ref, acq, par)
    assert not failures, "\n".join(failures)


# ---- E. gpx_acq_batch --------------------------------------------------------------------------------------------------------------
_BATCH = {}


def batch_model(dev, ctx, name):
    """The scalar-noise model of a batch case on the device and the longdouble base every replay starts from, once per module."""
    if name not in _BATCH:
        c = P.case(name)
        C = A.batch_candidates(name)
        sp = dev.KernelSpec(P.KIND_ID[c["spec"]["kind"]], c["spec"]["d"], KR.hyp_of(c["spec"]))
        dX, dC = dev.points(ctx, c["X"]), dev.points(ctx, C)
        Kd = dev.kfill(ctx, sp, dX, nugget=A.BATCH_NOISE)
        arrays = (Kd.to_host(), dev.kfill(ctx, sp, dX, Z=dC).to_host(), dev.kdiag(ctx, sp, dC))      # the device's own fills taken back
        ctx.sync()
        L = dev.potrf(ctx, Kd)
        _BATCH[name] = dict(c=c, C=C, sp=sp, dX=dX, dC=dC, L=L, alpha=dev.potrs(ctx, L, c["y"]),
                            base=A.BatchBase(c["spec"], c["X"], A.BATCH_NOISE, C, arrays=arrays))
    return _BATCH[name]


@pytest.mark.parametrize("liename", ["believer", "min y"])
@pytest.mark.parametrize("name", A.BATCH_CASES)
def test_acq_batch_rows_and_picks(dev, ctx, name, liename):
    b = batch_model(dev, ctx, name)
    c, C = b["c"], b["C"]
    lie, lie_value = (dev.LIE_BELIEVER, 0.0) if liename == "believer" else (dev.LIE_CONSTANT, float(np.min(c["y"])))
    failures = []
    print()
    for acqname, acq, par in (("ei", A.EI, float(np.max(c["y"]))), ("ucb", A.UCB, A.KAPPA)):
        for track in (0, 1):
            label = "%s %s %s track_best=%d" % (name, acqname, liename, track)
            idx, cost, lies, allc = dev.acq_batch(ctx, b["sp"], b["L"], b["dX"], b["alpha"], b["dC"], A.BATCH_NOISE, acq, par, track, lie,
                                                  lie_value, A.BATCH_Q, want_all=True)
            assert len(set(idx.tolist())) == A.BATCH_Q, label
            if lie == dev.LIE_CONSTANT:
                assert np.array_equal(lies, np.full(A.BATCH_Q, lie_value)), label
            assert np.array_equal(allc[0], dev.acq(ctx, b["sp"], b["L"], b["dX"], b["alpha"], b["dC"], acq, par)[2]), label     # gpx_acq's bits
            args = (c["spec"], c["X"], c["y"], A.BATCH_NOISE, C, idx, lies, acq, par, track)
            brefs = A.batch_reference(*args, base=b["base"])
            rows = {k: fn(*args, arrays=b["base"].arrays) for k, fn in A.BATCH_COMPARATORS.items()}
            print("  %s: picks %s" % (label, idx.tolist()))
            for t in range(A.BATCH_Q):
                assert np.array_equal(np.isnan(allc[t]), brefs[t]["masked"]), (label, t)        # masked entries NaN, no other
                SR.check_argbest_bits(idx[t:t + 1], cost[t:t + 1], allc[t:t + 1], label="%s pick %d" % (label, t))
                cmp_ = {k: A.omega_A_row(r[t], brefs[t]) for k, r in rows.items()}
                try:
                    A.check_bound("  pick %d omega_A" % t, A.omega_A_row(allc[t], brefs[t]), cmp_)
                    short, allowed = A.batch_regret(brefs[t], int(idx[t]), max(cmp_.values()))
                    assert short <= allowed, "%s pick %d = candidate %d: worse than the reference's best by %.3e > %.3e" % (label, t, idx[t], short, allowed)
                except AssertionError as e:
                    failures.append("%s: %s" % (label, e))
    assert not failures, "\n".join(failures)
