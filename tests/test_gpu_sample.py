"""GPU (-m gpu): the joint posterior sampler (gpx_psampler_*) held to the contracts of tests/sample_ref.py -- the factor by its
backward error against the device's own covariance, the draws by a longdouble replay from the device's own factor, the arg-best
exactly -- plus bit-for-bit independence of S and of the chunking, the prior, the pivot rule and the allocator's books.

The factor of a nearly singular covariance is never compared with a factor computed elsewhere (only F F^T is stable).

Measured on an MI355X, |F F^T - Chat| / ((M + 1) u sqrt(Chat_ii Chat_jj)) per case (the bound is 8, chol_stability_ref.MARGIN):
0.02 .. 0.12 on the seventeen cases with M >= 5, 0.93 at M = 1 (one square root).  Before the sampler refined its factor by one
step the same figure was 10.5 (squared exponential N = 40, M = 129, noise 1e-2) and 12.1 (Mehler N = 40, M = 128, d = 1), above
the bound: chol_potrf's 128-order leaf multiplies by explicit inverses of its diagonal blocks, and the float64 emulation of that
scheme (chol_stability_ref.chol_block_inverse) gives 18.1 and 12.6 on the same two matrices built on the host, LAPACK 0.06 and 0.08."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


class Fit(object):
    """One case on the device: points, the factor of K(X) + noise I, alpha, the default nugget 1e-10 max k(z, z)."""

    def __init__(self, dev, ctx, case):
        kind, n, m, d, noise, self.S = case
        self.c = c = SR.points_case(kind, n, m, d, noise)
        self.n, self.m = n, m
        self.sp = SR.device_spec(dev, c["spec"])
        self.dX, self.dZ = dev.points(ctx, c["X"]), dev.points(ctx, c["Z"])
        self.L = dev.potrf(ctx, dev.kfill(ctx, self.sp, self.dX, nugget=noise))
        self.alpha = dev.potrs(ctx, self.L, c["y"])
        self.nugget = 1e-10 * float(np.max(dev.kdiag(ctx, self.sp, self.dZ)))

    def sampler(self, dev, ctx, nugget=None, zero_mean=False):
        return dev.PosteriorSampler(ctx, self.sp, self.L, self.dX, np.zeros(self.n) if zero_mean else self.alpha, self.dZ,
                                    self.nugget if nugget is None else nugget)

    def factor(self, dev, ctx):
        """F itself: the draws of Xi = I from the sampler of the zero-mean model (alpha = 0: mean_j + F_jk is then F_jk exactly)."""
        s0 = self.sampler(dev, ctx, zero_mean=True)
        try:
            return np.ascontiguousarray(s0.draw(np.eye(self.m)).T)
        finally:
            s0.close()


# ---- 1, 2, 4: the factor, the mean, general draws, the arg-best ------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.SAMPLER_CASES, ids=SR.case_id)
def test_factor_mean_and_draws(dev, ctx, case):
    f = Fit(dev, ctx, case)
    m, label = f.m, SR.case_id(case)
    F = f.factor(dev, ctx)
    smp = f.sampler(dev, ctx)
    try:
        mean = smp.draw(np.zeros((1, m)))[0]
        assert np.array_equal(mean, dev.posterior(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, want_var=False)[0])   # gpx_posterior's bits
        assert np.array_equal(smp.draw(np.eye(m)), mean[None, :] + F.T)                                       # draw - mean IS F
        Chat = dev.posterior_cov(ctx, f.sp, f.L, f.dX, f.dZ)
        Chat[np.diag_indices(m)] += f.nugget
        failures = []
        try:
            SR.check_factor(F, Chat, label)
        except AssertionError as e:
            failures.append(str(e))
        xi = SR.base_samples(f.S, m)
        out = smp.draw(xi)
        SR.check_draw(out, mean, F, xi, label)
        assert np.array_equal(smp.draw(xi), out)                                                              # two calls, same bits
        for minimize in (True, False):
            idx, val, rows = smp.argbest(xi, minimize=minimize, want_samples=True)
            assert np.array_equal(rows, out)
            SR.check_argbest(idx, val, out, minimize, label)
            idx2, val2 = smp.argbest(xi, minimize=minimize)
            assert np.array_equal(idx2, idx) and np.array_equal(val2, val)
        assert not failures, "\n".join(failures)
    finally:
        smp.close()


# ---- 3: a sample's bits depend neither on S nor on the chunking ---------------------------------------------------------------------
CHUNK_CASE = SR.SAMPLER_CASES[0]      # M = 129 (two row tiles), S = 130


def chunk_digest():
    from gpexp_amd import device as dev
    ctx = dev.context()
    f = Fit(dev, ctx, CHUNK_CASE)
    smp = f.sampler(dev, ctx)
    xi = SR.base_samples(130, f.m)
    out = smp.draw(xi)
    idx, val = smp.argbest(xi)
    smp.close()
    h = hashlib.sha256()
    for a in (out, idx, val):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_child(code, extra):
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_sample as t\n%s" % (ROOT, TESTS, code)],
                       env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


def test_sample_bits_do_not_depend_on_S_or_chunking(dev, ctx):
    f = Fit(dev, ctx, CHUNK_CASE)
    smp = f.sampler(dev, ctx)
    try:
        xi = SR.base_samples(130, f.m)
        full = smp.draw(xi)
        assert np.array_equal(smp.draw(xi[:1])[0], full[0])                     # S = 1 against S = 130
        assert np.array_equal(smp.draw(xi[:3]), full[:3])
        assert np.array_equal(smp.draw(xi[[0, 129, 5]])[1], full[129])          # other company, another position
        assert np.array_equal(smp.draw(xi[:128]), full[:128])
    finally:
        smp.close()
    # GPX_CROSS_BYTES so small that S = 130 goes in two chunks (128 + 2) and the mean in chunks of 128 points
    assert run_child("print('RESULT ' + t.chunk_digest(), flush=True)", {"GPX_CROSS_BYTES": "200000"}) == chunk_digest()


# ---- 5: the prior ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m", [("se", 5), ("matern32", 129)])
def test_prior_of_far_apart_points_is_the_identity(dev, ctx, kind, m):
    """Far-apart points with signalSize 1: K = I exactly, so F = sqrt(1 + nugget) I -- to 2 u relative on the diagonal (the leaf's
    square root and one reciprocal product), exactly 0 elsewhere -- and the mean is exactly 0."""
    spec = dict(SR.kernel_spec(kind, 2), signalSize=1.0)
    Z = 1e4 * np.arange(1.0, m + 1.0)[:, None] * np.array([[1.0, -1.0]])
    nug = 1e-10
    smp = dev.PosteriorSampler(ctx, SR.device_spec(dev, spec), None, None, None, dev.points(ctx, Z), nug)
    try:
        F = smp.draw(np.eye(m)).T
        assert np.array_equal(smp.draw(np.zeros((2, m))), np.zeros((2, m)))
        assert np.all(F[~np.eye(m, dtype=bool)] == 0.0)
        assert np.max(np.abs(np.diag(F) - np.sqrt(1.0 + nug))) <= 2.0 * SR.U * np.sqrt(1.0 + nug)
    finally:
        smp.close()


ARGBEST_M = (1, 255, 256, 257)    # below, at and above the 256 threads a row is dealt to


def argbest_base_samples(m):
    """Base samples whose rows -- on the identity factor -- hold: nothing special; one value everywhere; the best value twice, at the
    two ends of the thread stride (m - 2, m - 1) and at 0 when m allows; exact zeros of both signs; a NaN in the last place; NaN only."""
    xi = np.random.default_rng(m).standard_normal((7, m))
    xi[1] = 1.5
    xi[2, [0, max(m - 2, 0), m - 1]] = -9.0
    xi[3, [max(m - 2, 0), m - 1]] = 9.0
    xi[4] = np.where(np.arange(m) % 2 == 0, 0.0, -0.0)
    xi[5, m - 1] = np.nan
    xi[6] = np.nan
    return xi


@pytest.mark.parametrize("m", ARGBEST_M)
def test_argbest_of_rows_with_ties_zeros_and_nan(dev, ctx, m):
    """The row arg-best on rows made to order: the prior of far-apart points with signalSize 1 and no nugget has K = I, so a sample
    is its base sample times the diagonal of F.  Checked on the rows the device itself returns: the first arg-best among the entries
    that are not NaN, the value there bit for bit, index 0 and NaN for a row of NaNs.  (A -0 cannot come out of the sampler --
    mean + F xi adds to +0 -- so the tie of +0 with -0 is fed in but reaches the reduction as a tie of +0 with +0.)"""
    spec = dict(SR.kernel_spec("se", 2), signalSize=1.0)
    Z = 1e4 * np.arange(1.0, m + 1.0)[:, None] * np.array([[1.0, -1.0]])
    smp = dev.PosteriorSampler(ctx, SR.device_spec(dev, spec), None, None, None, dev.points(ctx, Z), 0.0)
    try:
        xi = argbest_base_samples(m)
        for minimize in (True, False):
            idx, val, rows = smp.argbest(xi, minimize=minimize, want_samples=True)
            assert np.all(rows[1] == rows[1, 0]) and np.all(rows[4] == 0.0) and np.all(np.isnan(rows[6]))
            assert rows[2, m - 1] == rows[2, 0] == rows[2].min() and rows[3, m - 1] == rows[3, max(m - 2, 0)] == rows[3].max()
            assert np.isnan(rows[5, m - 1]) and (m < 257 or not np.any(np.isnan(rows[5, :256])))
            SR.check_argbest_bits(idx, val, rows, minimize, "m = %d, %s" % (m, "min" if minimize else "max"))
            assert idx[6] == 0 and np.isnan(val[6]) and idx[1] == 0 and idx[4] == 0
            idx2, val2 = smp.argbest(xi, minimize=minimize)
            assert np.array_equal(idx2, idx) and np.array_equal(val2, val, equal_nan=True)
    finally:
        smp.close()


# ---- 6: nugget 0 on repeated points, and the pivot policy --------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.SAMPLER_CASES[:4], ids=SR.case_id)
@pytest.mark.parametrize("drop_before", [False, True])
def test_nugget_zero_on_repeated_points_is_refused_and_the_policy_survives(dev, ctx, case, drop_before):
    """z_5 = z_2 and z_{M-1} = z_0: without a nugget the factorisation meets a pivot that is 0 in exact arithmetic.  The call
    factors with the policy (0, report) whatever the context holds, so the status is the 1-based index of a repeated point --
    6 or M -- also when a design loop left the drop policy on; and that policy is in force again afterwards: a matrix with a
    repeated point then factors with the point dropped.
    Round-to-nearest leaves a pivot that is exactly 0 a few 1e-17 on EITHER side of 0, so (0, report) refuses a repeated point
    with about an even chance per repeat, fixed for given inputs: of the 17 sampler cases with repeats 14 were refused and 3
    factored on an MI355X (their factor then holds a column of size 1e-8).  These four cases (the first shape) are refused at
    point 6, 6, 6 and 129.  The q-EI kernel's own factorisation rounds its columns outward and is certain (tests/test_gpu_qei.py)."""
    from gpexp_amd._lib import NotPositiveDefinite
    f = Fit(dev, ctx, case)
    prev = dev.potrf_policy(ctx, 1e-13 * 1.3, True) if drop_before else dev.potrf_policy(ctx, 0.0, False)
    try:
        with pytest.raises(NotPositiveDefinite) as e:
            f.sampler(dev, ctx, nugget=0.0)
        assert e.value.pivot in (6, f.m), e.value.pivot
        assert "larger jitter" in str(e.value) and "point %d" % (e.value.pivot - 1) in str(e.value)
        f.sampler(dev, ctx).close()                                             # the default nugget factors, policy or not
        twin = np.vstack([f.c["X"], f.c["X"][7:8]])
        K = dev.kfill(ctx, f.sp, dev.points(ctx, twin), nugget=0.0)
        if drop_before:
            dev.potrf(ctx, K)
            assert dev.potrf_dropped(ctx) >= 1                                  # the drop policy is still on
        else:
            try:
                dev.potrf(ctx, K)
            except NotPositiveDefinite:
                pass
            assert dev.potrf_dropped(ctx) == 0                                  # nothing dropped: (0, report) is still on
    finally:
        dev.potrf_policy(ctx, *prev)


# ---- 7: the allocator --------------------------------------------------------------------------------------------------------------------
def guarded_case():
    from gpexp_amd import device as dev
    from gpexp_amd._lib import NotPositiveDefinite
    ctx = dev.context()
    f = Fit(dev, ctx, CHUNK_CASE)
    F = f.factor(dev, ctx)
    ctx.sync()
    before = ctx.pool_stats()[1]
    smp = f.sampler(dev, ctx)
    xi = SR.base_samples(130, f.m)
    out = smp.draw(xi)
    idx, val = smp.argbest(xi)
    smp.close()
    ctx.sync()
    after = ctx.pool_stats()[1]
    try:
        f.sampler(dev, ctx, nugget=0.0)
        failed = False
    except NotPositiveDefinite:
        failed = True
    ctx.sync()
    after_failed = ctx.pool_stats()[1]
    mean = dev.posterior(ctx, f.sp, f.L, f.dX, f.alpha, f.dZ, want_var=False)[0]
    SR.check_draw(out, mean, F, xi, "guarded")
    SR.check_argbest(idx, val, out, True, "guarded")
    return "%d %d %d %d %d" % (int(ctx.lib.gpx_dbg_guard_violations(ctx.h)), before, after, after_failed, int(failed))


def test_under_allocation_guard_and_nan_fill():
    """Guard bands + NaN-filled blocks: the padding of F, Xi^T and the scratch never reaches a result, no block is overrun, and the
    pool's outstanding bytes return to their value after create / draw / free and after a failed create."""
    viol, before, after, after_failed, failed = run_child("print('RESULT ' + t.guarded_case(), flush=True)", {"GPX_ALLOC_GUARD": "2"}).split()
    assert viol == "0" and failed == "1"
    assert before == after == after_failed, (before, after, after_failed)
