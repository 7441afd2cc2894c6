"""GPU (-m gpu): the Cholesky path held to backward-error bounds on ill-conditioned K, and the pivot policy at the structural
boundaries of the factorisation.

Families, metrics and emulations: tests/chol_stability_ref.py (pinned on the CPU by tests/test_chol_stability_host.py).  K is
the DEVICE's own fill taken back with to_host(): the metrics judge the factorisation, not the assembly.  The bound on every
metric is  device <= 8 x max(LAPACK, emulation b = 128, emulation b = 1024 [, b = 16 for the leaf])  on the same matrix and the
same sampled rows; on the well-conditioned family W every metric must also stay under gamma_{n+1} (Higham Thm 10.3): a
well-conditioned K must not show the explicit-inverse penalty at all.  Run with -s: every case prints device, LAPACK and
emulation values and the ratio ("Conditioning", quotes them)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl

import chol_stability_ref as R
from helpers import rel

pytestmark = pytest.mark.gpu

# n -> path of potrf_rec / the solves (padded order): 300 (384) right-looking, in-place left solve; 2200 (2304) right-looking,
# block-inverse potrs with a ragged last block, out-of-place left solve (from 2048); 4500 (4608) the recursive split between
# POTRF_RL_MAX and two panels; 8300 (8320) potrf_blocked with look-ahead, panel solves through the 1024-order inverses
CASES = [(f, n) for f in ("S8", "M10") for n in (300, 2200, 4500, 8300)] + [(f, n) for f in ("S6s", "W") for n in (300, 2200)]
POTRI_SIZES = (300, 2200)
N_EVAL = 260        # two column tiles of the rectangular fill, one of them ragged


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def spec_of(dev, name):
    kind, hyp, _ = R.FAMILIES[name]
    return dev.KernelSpec(kind, R.D, hyp)


def lapack_results(K, y=None, Kxz=None, inverse=False):
    c = sl.cho_factor(K, lower=True, check_finite=False)
    L = np.tril(c[0])
    out = dict(L=L)
    if y is not None:
        out["alpha"] = sl.cho_solve(c, y, check_finite=False)
    if Kxz is not None:
        out["W"] = sl.solve_triangular(L, Kxz, lower=True, check_finite=False)
    if inverse:
        P = sl.lapack.dpotri(L, lower=1)[0]
        out["P"] = np.tril(P) + np.tril(P, -1).T
    return out


@pytest.mark.parametrize("name,n", CASES)
def test_backward_errors_of_factor_and_solves(dev, ctx, name, n):
    X, Z = R.family_points(name, n, extra=N_EVAL)
    sp = spec_of(dev, name)
    dX, dZ = dev.points(ctx, X), dev.points(ctx, Z)
    y = np.random.default_rng(n).standard_normal(n)
    Kd = dev.kfill(ctx, sp, dX, nugget=R.FAMILIES[name][2])
    K = Kd.to_host()
    Kxz = dev.kfill(ctx, sp, dX, Z=dZ).to_host()
    L = dev.potrf(ctx, Kd)
    Ld = L.to_host(tri=1)
    alpha = dev.potrs(ctx, L, y)
    assert np.array_equal(dev.potrs(ctx, L, y), alpha)              # second solve: the cached block inverses, same bits
    npad = (n + 127) // 128 * 128
    y_dev, a_dev = dev.padded_vector(ctx, y, npad), dev.padded_vector(ctx, np.zeros(n), npad)
    dev.potrs_dev(ctx, L, y_dev, a_dev)
    ctx.sync()
    assert np.array_equal(a_dev.to_host().ravel()[:n], alpha)       # the device-vector form: same bits
    Wd = dev.ivar(ctx, sp, L, dX, dZ, keep=True)[1].to_host()
    inverse = n in POTRI_SIZES
    Pd = dev.potri(ctx, L).to_host(tri=2) if inverse else None
    del Kd, L, y_dev, a_dev
    ctx.trim()

    rows = None if n <= 640 else R.sample_rows(n)
    ref = R.reference_values(K, lapack_results(K, y, Kxz, inverse), y, Kxz, rows, inverse)
    cap = R.gamma_chol(n) if name == "W" else None
    print("\n%s n=%d" % (name, n))
    ecw, es = R.eta(K, Ld, rows)
    got = {"eta_cw": ecw, "eta_s": es, "omega": R.omega(K, alpha, y), "omega_tri": R.omega_tri(Ld, Wd, Kxz, rows)}
    if inverse:
        got["rho_inv"] = R.rho_inv(K, Pd, rows)
    failures = []
    for metric, value in got.items():
        try:
            R.check_bound("%s %d %s" % (name, n, metric), value, ref[metric], cap=cap)
        except AssertionError as e:        # (every figure is printed before the first assertion surfaces)
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["S8", "M10", "W"])
def test_backward_error_of_the_level_batched_inverse(dev, ctx, name):
    """n = 2048 = 128 * 2^4: the branch of chol_trtri that builds the levels up to order 1024 for all diagonal blocks at once."""
    n = 2048
    X, _ = R.family_points(name, n)
    sp = spec_of(dev, name)
    Kd = dev.kfill(ctx, sp, dev.points(ctx, X), nugget=R.FAMILIES[name][2])
    K = Kd.to_host()
    L = dev.potrf(ctx, Kd)
    Pd = dev.potri(ctx, L).to_host(tri=2)
    del Kd, L
    ctx.trim()
    cols = R.sample_rows(n)
    lap = lapack_results(K, inverse=True)
    refs = {"lapack": R.rho_inv(K, lap["P"], cols)}
    for b in (128, 1024):
        refs["b%d" % b] = R.rho_inv(K, R.inverse_by_halving(R.chol_block_inverse(K, b))[1], cols)
    print()
    R.check_bound("%s %d rho_inv" % (name, n), R.rho_inv(K, Pd, cols), refs, cap=R.gamma_chol(n) if name == "W" else None)


LEAF_INPUTS = ["S8", "S6s", "M10", "graded"]


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("which", LEAF_INPUTS)
def test_leaf_alone_both_diagonal_steps(dev, ctx, which, fast):
    """One 128 x 128 leaf launch (gpx_dbg_leaf_stamps; the stamps are ignored) with the LDL^T diagonal step (fast = 1) and with the
    general one (fast = 0), which the product only runs on a block with a bad pivot.  Both must hold the bound on every input;
    they are not compared with each other (on an ill-conditioned block two correct factors differ by cond * u)."""
    if which == "graded":
        A = R.graded_block(128)
    else:
        X, _ = R.family_points(which, 128)
        Kd = dev.kfill(ctx, spec_of(dev, which), dev.points(ctx, X), nugget=R.FAMILIES[which][2])
        A = Kd.to_host()
    assert A.shape == (128, 128)
    prev = dev.potrf_policy(ctx, 0.0, False)
    try:
        M = dev.DeviceMatrix.from_host(ctx, A)
        st = (C.c_int64 * 30)()
        dev.check(ctx.lib.gpx_dbg_leaf_stamps(ctx.h, M.h, int(fast), st))
        Ld = np.tril(M.to_host()[:128, :128])
    finally:
        dev.potrf_policy(ctx, *prev)
    refs = {}
    for nm, Lr in (("lapack", lapack_results(A)["L"]), ("b16", R.chol_block_inverse(A, 16))):
        refs[nm] = R.eta(A, Lr)
    ecw, es = R.eta(A, Ld)
    print()
    failures = []
    for i, (metric, value) in enumerate((("eta_cw", ecw), ("eta_s", es))):
        try:
            R.check_bound("leaf %s fast=%d %s" % (which, fast, metric), value, {k: v[i] for k, v in refs.items()})
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---- pivot policy at the structural boundaries -----------------------------------------------------------------------
def planted_fill(dev, ctx, n, pairs):
    X, nug = R.planted("W", n, pairs)
    dX = dev.points(ctx, X)
    return dX, dev.kfill(ctx, spec_of(dev, "W"), dX, nugget=nug)


def reported_pivot(dev, ctx, n, pairs):
    from gpexp_amd._lib import NotPositiveDefinite
    dX, Kd = planted_fill(dev, ctx, n, pairs)
    prev = dev.potrf_policy(ctx, R.PIV_MIN, False)
    try:
        with pytest.raises(NotPositiveDefinite) as e:
            dev.potrf(ctx, Kd)
    finally:
        dev.potrf_policy(ctx, *prev)
        del Kd
        ctx.trim()
    return e.value.pivot


@pytest.mark.parametrize("n,q,p", [(n, q, p) for n in sorted(R.PLANTS) for q, p in R.PLANTS[n]])
def test_first_bad_pivot_is_reported_exactly(dev, ctx, n, q, p):
    R.check_pivot_report(reported_pivot(dev, ctx, n, [(q, p)]), [p])


@pytest.mark.parametrize("pairs", R.PLANTS_TWO, ids=lambda pairs: "+".join(str(p) for _, p in pairs))
def test_two_bad_pivots_report_the_smaller_index(dev, ctx, pairs):
    R.check_pivot_report(reported_pivot(dev, ctx, 8300, pairs), [p for _, p in pairs])


@pytest.mark.parametrize("n", sorted(R.PLANTS))
def test_drop_policy_equals_the_reduced_model(dev, ctx, n):
    """skip=True with all of a size's rows planted together: every one dropped and none of the padding counted (1299 is the last
    row of 1300, padded 1408), alpha exactly 0.0 there, the rest LAPACK's solve of the matrix without those rows and columns;
    mean and variance at 64 points those of the reduced model (1e-10: the reduced matrix has cond <= 1e4,
    test_chol_stability_host.py::test_planted_pivot_recipe)."""
    pairs = R.PLANTS[n]
    ps = sorted(p for _, p in pairs)
    sp = spec_of(dev, "W")
    dX, Kd = planted_fill(dev, ctx, n, pairs)
    Z = np.random.default_rng(n + 1).uniform(-1.0, 1.0, (64, R.D))
    dZ = dev.points(ctx, Z)
    K = Kd.to_host()
    Kxz = dev.kfill(ctx, sp, dX, Z=dZ).to_host()
    y = np.random.default_rng(n).standard_normal(n)
    prev = dev.potrf_policy(ctx, R.PIV_MIN, True)
    try:
        L = dev.potrf(ctx, Kd)
        dropped = dev.potrf_dropped(ctx)
    finally:
        dev.potrf_policy(ctx, *prev)
    alpha = dev.potrs(ctx, L, y)
    mean, var = dev.posterior(ctx, sp, L, dX, alpha, dZ)
    del Kd, L
    ctx.trim()
    keep = np.setdiff1d(np.arange(n), ps)
    c = sl.cho_factor(K[np.ix_(keep, keep)], lower=True, check_finite=False)
    red = sl.cho_solve(c, y[keep], check_finite=False)
    err = R.check_drop(dropped, alpha, ps, red)
    Wr = sl.solve_triangular(np.tril(c[0]), Kxz[keep], lower=True, check_finite=False)
    em, ev = rel(mean, Kxz[keep].T @ red), rel(var, R.FAMILIES["W"][1][1] - np.sum(Wr * Wr, axis=0))
    print("\ndrop n=%d: dropped %d, alpha %.2e, mean %.2e, variance %.2e (of 1e-10); smallest pivot of the reduced matrix %.3f"
          % (n, dropped, err, em, ev, np.min(np.diag(c[0])) ** 2))
    assert em <= 1e-10 and ev <= 1e-10, (em, ev)
