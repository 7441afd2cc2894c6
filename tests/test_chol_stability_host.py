"""CPU: pins the references tests/test_gpu_chol_stability.py judges the device by, before the device is judged by them.

Per matrix family and size: the inputs have the conditioning they are meant to have; LAPACK stays inside Higham's bounds in the
metrics of tests/chol_stability_ref.py (so the metrics measure what they claim); every emulation of the explicit-inverse scheme
returns a Cholesky factor; the row sampling reproduces the full-matrix value; the planted-pivot recipe plants exactly one bad
pivot.  And the checks can fail: a factor whose panel was solved in float32, a column off by 1e-11, a pivot index or a drop count
off by one are all rejected by the functions the GPU file calls.  Run with -s for the table of reference values."""
import numpy as np
import pytest
import scipy.linalg as sl

import chol_stability_ref as R

SIZES = [300, 640, 2200]


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


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_references_hold_their_bounds(name, n):
    X, Z = R.family_points(name, n, extra=260)
    K = R.host_cov(name, X)
    cond = np.linalg.cond(K)
    if name in R.ILL:
        assert cond >= 1e9, cond
    else:
        assert cond <= 1e4, cond
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n)
    kind, hyp, _ = R.FAMILIES[name]
    XZ = np.vstack([X, Z])
    Kxz = (R.host_cov(name, XZ, nugget=0.0))[:n, n:]
    rows = None if n <= 640 else R.sample_rows(n)
    lap = lapack_results(K, y, Kxz, inverse=True)
    ref = R.reference_values(K, lap, y, Kxz, rows, inverse=True, bs=(16, 128, 1024))
    print("\n%s n=%d cond=%.2e" % (name, n, cond))
    for metric, vals in ref.items():
        print("  %-10s %s" % (metric, "  ".join("%s %.3e" % kv for kv in vals.items())))
    # LAPACK inside Higham's bounds: Thm 10.3 for the factor, the gamma-type bound of Thm 10.4 for the solve
    g = R.gamma_chol(n)
    assert ref["eta_cw"]["lapack"] <= g, (ref["eta_cw"]["lapack"], g)
    assert ref["omega"]["lapack"] <= g, (ref["omega"]["lapack"], g)
    # every emulation returns a Cholesky factor of K, and on the well-conditioned family THE factor
    for b in (16, 128, 1024):
        assert ref["eta_s"]["b%d" % b] <= 1e-10, (b, ref["eta_s"]["b%d" % b])
        if name == "W":
            Lb = R.chol_block_inverse(K, b)
            assert np.max(np.abs(Lb - lap["L"])) / np.max(np.abs(lap["L"])) <= 1e-12
    if name == "W":
        a = R.solve_block_inverse(lap["L"], y, 128)
        assert np.max(np.abs(a - lap["alpha"])) / np.max(np.abs(lap["alpha"])) <= 1e-12
        Wb = R.forward_block_inverse(lap["L"], Kxz, 1024)
        assert np.max(np.abs(Wb - lap["W"])) / np.max(np.abs(lap["W"])) <= 1e-12
        Pb = R.inverse_by_halving(lap["L"])[1]
        assert np.max(np.abs(Pb - lap["P"])) / np.max(np.abs(lap["P"])) <= 1e-12


@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_row_sampling_reproduces_the_full_value(name):
    """Within 2x at n = 640, for LAPACK's factor and the 128-order emulation's, both factor metrics.  Measured: at most 1.73x
    (S6s, eta_cw of the emulation: 1.90e-13 full, 1.10e-13 sampled); LAPACK's within 1.27x.  On the SE families the componentwise
    maximum of an explicit-inverse factor is carried by a few per cent of the rows, so the sample is a lower estimate, not the
    maximum; the GPU file compares device and references on the SAME rows and does not rest on this property."""
    n = 640
    X, _ = R.family_points(name, n)
    K = R.host_cov(name, X)
    rows = R.sample_rows(n)
    assert rows.size == 51 and rows[0] == 0 and rows[-1] == n - 1 and n // 2 in rows
    fig = []
    for who, L in (("lapack", lapack_results(K)["L"]), ("b128", R.chol_block_inverse(K, 128))):
        for metric in (R.eta_cw, R.eta_s):
            full, part = metric(K, L), metric(K, L, rows)
            print("%s %s %s full %.3e sampled %.3e (%.2fx)" % (name, who, metric.__name__, full, part, full / part))
            fig.append((who, metric.__name__, full, part))
    for who, m, full, part in fig:
        assert part <= full <= 2.0 * part, (who, m, full, part)


@pytest.mark.parametrize("pairs", [[qp] for qp in R.PLANTS[1300]] + [[(1290, 1299)], R.PLANTS[1300]],
                         ids=lambda pairs: "+".join("%d-%d" % qp for qp in pairs))
def test_planted_pivot_recipe(pairs):
    """One planted row per fit (the report cases) and all of them together (the drop case), n = 1300: an unblocked L D L^T shows
    |pivot p| <= 1e-12 at every planted row, every other pivot >= 1e-2, and the matrix without the planted rows has
    cond <= 1e4 -- which is what entitles the GPU file to its 1e-10 against LAPACK on the reduced system."""
    n = 1300
    ps = [p for _, p in pairs]
    X, nug = R.planted("W", n, pairs)
    K = R.host_cov("W", X, nugget=nug)
    for q, p in pairs:
        assert np.array_equal(K[p], K[q])
    d = R.ldlt_pivots(K)
    others = np.delete(d, ps)
    print("planted %s: pivots %s, smallest other pivot %.3f" % (pairs, " ".join("%.1e" % d[p] for p in ps), others.min()))
    assert np.max(np.abs(d[ps])) <= 1e-12, d[ps]
    assert others.min() >= 1e-2, others.min()
    keep = np.setdiff1d(np.arange(n), ps)
    cond = np.linalg.cond(K[np.ix_(keep, keep)])
    assert cond <= 1e4, cond


# ---- the checks can fail ---------------------------------------------------------------------------------------------
def _refs_for_factor(name, n):
    X, _ = R.family_points(name, n)
    K = R.host_cov(name, X)
    rows = R.sample_rows(n)
    lap = lapack_results(K)
    return K, rows, lap, R.reference_values(K, lap, rows=rows)


def test_float32_panel_is_rejected():
    """Family W: in float32 the ill-conditioned families (cond 1e10 > 1 / 2^-24) break down with a negative pivot -- a NaN
    factor, which check_bound refuses as not finite; the subtle case is the factor that exists and is right to 1e-7."""
    K, rows, lap, ref = _refs_for_factor("W", 640)
    bad = R.chol_block_inverse(K, 128, panel_dtype=np.float32)
    assert R.eta_s(K, bad, rows) <= 1e-5          # still "a factor" to single precision: not garbage, subtly wrong
    for metric in ("eta_cw", "eta_s"):
        with pytest.raises(AssertionError):
            R.check_bound(metric, getattr(R, metric)(K, bad, rows), ref[metric])
        R.check_bound(metric, getattr(R, metric)(K, R.chol_block_inverse(K, 128), rows), ref[metric])   # the honest one passes
    with pytest.raises(AssertionError):
        R.check_bound("eta_cw", float("nan"), ref["eta_cw"])


@pytest.mark.parametrize("name,col", [("S8", 0), ("W", 320)])
def test_perturbed_column_is_rejected(name, col):
    """One column of the LAPACK factor off by 1e-11 relative.  On S8 it is column 0: a smooth kernel's later columns are tiny
    (that is what cond 1e10 means), and an error in them is a small backward error; on W any column carries weight."""
    K, rows, lap, ref = _refs_for_factor(name, 640)
    bad = lap["L"].copy()
    bad[:, col] *= 1.0 + 1e-11
    cap = R.gamma_chol(640) if name == "W" else None
    with pytest.raises(AssertionError):
        R.check_bound("eta_cw", R.eta_cw(K, bad, rows), ref["eta_cw"], cap=cap)
    R.check_bound("eta_cw", R.eta_cw(K, lap["L"], rows), ref["eta_cw"], cap=cap)


def test_pivot_report_off_by_one_is_rejected():
    R.check_pivot_report(1024, [1023])
    R.check_pivot_report(4091, [4100, 4090])
    for wrong in (1023, 1025):
        with pytest.raises(AssertionError):
            R.check_pivot_report(wrong, [1023])
    with pytest.raises(AssertionError):
        R.check_pivot_report(4101, [4100, 4090])


def test_drop_count_off_by_one_is_rejected():
    n, pairs = 300, [(3, 15), (100, 128), (7, 299)]
    ps = [p for _, p in pairs]
    X, nug = R.planted("W", n, pairs)
    K = R.host_cov("W", X, nugget=nug)
    keep = np.setdiff1d(np.arange(n), ps)
    y = np.random.default_rng(5).standard_normal(n)
    red = sl.cho_solve(sl.cho_factor(K[np.ix_(keep, keep)], lower=True), y[keep])
    alpha = np.zeros(n)
    alpha[keep] = red
    R.check_drop(3, alpha, ps, red)
    for wrong in (2, 4):
        with pytest.raises(AssertionError):
            R.check_drop(wrong, alpha, ps, red)
    leak = alpha.copy()
    leak[15] = 1e-300                                 # "exactly 0.0" means exactly
    with pytest.raises(AssertionError):
        R.check_drop(3, leak, ps, red)
    off = alpha.copy()
    off[keep[np.argmax(np.abs(red))]] *= 1.0 + 1e-8
    with pytest.raises(AssertionError):
        R.check_drop(3, off, ps, red)
