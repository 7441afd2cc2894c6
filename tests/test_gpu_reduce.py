"""GPU (-m gpu): the deterministic reductions of gpexp_amd/csrc/reduce.hip, one launch at a time (gpx_dbg_colreduce, gpx_dbg_rowreduce,
gpx_dbg_sum: exactly the product's launch_colreduce / launch_rowreduce / launch_sum with the product's scratch), and the two public
entry points on top of them (gpx_col_sumsq, gpx_matvec).

  exact      integer data B_ij = ((7 i + 3 j) mod 17) - 8 with integer weights: every partial sum is an integer below 2^53, so ANY order of
             summation gives the integer sum exactly and a dropped or doubled row, chunk or column cannot hide; all-ones data gives
             the row / column count
  accuracy   entries sign * 10^U(-8, 8) against np.longdouble:  |err| <= gamma(depth) * sum |terms|,  gamma(k) = k u / (1 - k u),
             depth = the longest chain of roundings a term passes through, read off the kernels (below)
  extents    rows from `rows` on (up to the padded height) and columns from `cols` on hold NaN: the result is finite; the hooks fail
             when a launch writes behind the last entry of its result
  subtract   out <- out - sum starts from the preset `out`
  bits       two calls return the same bits

DEPTHS, from reduce.hip.  colreduce_kernel: a thread owns one column of one row chunk; accumulator s0 takes chunk // 4 fused
multiply-adds (one rounding each) and the chunk % 4 rows of the tail loop, then (s0 + s1) + (s2 + s3): chunk // 4 + chunk % 4 + 2.
colreduce_final_kernel: the same shape over the nchunk partial sums: nchunk // 4 + nchunk % 4 + 2; `subtract` rounds once more.
  column form   chunk // 4 + chunk % 4 + nchunk // 4 + nchunk % 4 + 4 (+ 1)     [<= ceil(chunk / 4) + ceil(nchunk / 4) + 8]
rowreduce_kernel: a thread's s0 / s1 take ceil(cols / 512) fused multiply-adds (the weighted squares round b * w first: + 1), s0 + s1,
then 8 levels of the 256-entry tree:
  row form      ceil(cols / 512) + 9 (+ 1)
sum_kernel: ceil(n / 256) additions per thread, 8 levels:
  sum           ceil(n / 256) + 8
(chunk, nchunk) come from a restatement of `plan` that is checked against gpx_dbg_colreduce_plan for every shape."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53

COL_PCOLS = (128, 256, 384, 1152)
COL_ROWS = (1, 3, 4, 5, 6, 15, 16, 17, 19, 63, 65, 257, 300, 1000)
# 33000 x 128: 34 MB; 34816 = 2048 * 17: the 2048-chunk cap of `plan`, every chunk with one row in the tail loop; 300 x 1024: the
# skewed leading dimension (1040) of a padded matrix whose width is a multiple of 256
COL_SHAPES = [(r, p) for p in COL_PCOLS for r in COL_ROWS] + [(33000, 128), (34816, 128), (17, 1024), (300, 1024)]
ROW_COLS = (2, 128, 510, 512, 514, 1152)
ROW_ROWS = (1, 70, 300)
SUM_N = (1, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def gamma(k):
    return k * U / (1.0 - k * U)


def plan(rows, pcols):
    """(chunk, nchunk) of reduce.hip's `plan`: at most 2048 / column blocks chunks, none shorter than 16 rows but the last."""
    want = min(max(2048 // ((pcols + 255) // 256), 1), max((rows + 15) // 16, 1))
    chunk = max((rows + want - 1) // want, 1)
    return chunk, max((rows + chunk - 1) // chunk, 1)


def col_depth(rows, pcols, subtract=False):
    chunk, nchunk = plan(rows, pcols)
    return chunk // 4 + chunk % 4 + nchunk // 4 + nchunk % 4 + 4 + (1 if subtract else 0)


def row_depth(cols, weighted_squares=False):
    return (cols + 511) // 512 + 9 + (1 if weighted_squares else 0)


def int_matrix(rows, cols):
    i, j = np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    return ((7 * i + 3 * j) % 17 - 8).astype(float)


def int_weights(n):
    return ((5 * np.arange(n, dtype=np.int64)) % 7 - 3).astype(float)


def wide_matrix(rng, rows, cols):
    return rng.choice([-1.0, 1.0], (rows, cols)) * 10.0 ** rng.uniform(-8.0, 8.0, (rows, cols))


def upload(dev, ctx, H, nan_rows=0, nan_cols=0):
    """H on the device, padded, with `nan_rows` rows / `nan_cols` columns of NaN behind it (inside the padded shape)."""
    r, c = H.shape
    full = np.full((r + nan_rows, c + nan_cols), np.nan)
    full[:r, :c] = H
    return dev.DeviceMatrix.from_host(ctx, full, pad=True)


def test_shape_set_covers_every_branch_of_the_plan(dev):
    """Through gpx_dbg_colreduce_plan: nchunk mod 4 and chunk mod 4 take every value (the four accumulators and both tail loops), a
    last chunk is shorter than the others, one chunk alone, and 2048 chunks at the cap."""
    from gpexp_amd import _lib
    lib = _lib.load()
    seen_n, seen_c, short, counts = set(), set(), False, set()
    for rows, pcols in COL_SHAPES:
        n, b = C.c_int64(), C.c_int64()
        assert lib.gpx_dbg_colreduce_plan(rows, pcols, C.byref(n), C.byref(b)) == 0
        chunk, nchunk = plan(rows, pcols)
        assert n.value == nchunk and nchunk * pcols <= b.value, (rows, pcols)
        seen_n.add(nchunk % 4)
        seen_c.add(chunk % 4)
        short |= nchunk > 1 and rows % chunk != 0
        counts.add(nchunk)
    assert seen_n == {0, 1, 2, 3} and seen_c == {0, 1, 2, 3} and short
    assert 1 in counts and 2048 in counts and max(counts) == 2048


@pytest.mark.parametrize("pcols", sorted({p for _, p in COL_SHAPES}))
def test_column_reduction_is_exact_on_integers(dev, ctx, pcols):
    for rows in [r for r, p in COL_SHAPES if p == pcols]:
        H = int_matrix(rows, pcols)
        v = int_weights(rows)
        B = upload(dev, ctx, H, nan_rows=3)
        label = "%d x %d" % (rows, pcols)
        dot = dev.dbg_colreduce(ctx, B, rows, pcols, v=v)
        assert np.array_equal(dot, v @ H), label
        assert np.array_equal(dev.dbg_colreduce(ctx, B, rows, pcols, v=v), dot), label             # same bits again
        assert np.array_equal(dev.dbg_colreduce(ctx, B, rows, pcols), np.sum(H * H, axis=0)), label
        preset = 1000.0 - np.arange(pcols, dtype=float)
        assert np.array_equal(dev.dbg_colreduce(ctx, B, rows, pcols, v=v, out=preset, subtract=True), preset - v @ H), label
        assert np.array_equal(dev.dbg_colreduce(ctx, B, rows, pcols, out=preset, subtract=True), preset - np.sum(H * H, axis=0)), label
        ones = upload(dev, ctx, np.ones((rows, pcols)), nan_rows=1)
        assert np.array_equal(dev.dbg_colreduce(ctx, ones, rows, pcols), np.full(pcols, float(rows))), label
        assert np.array_equal(dev.dbg_colreduce(ctx, ones, rows, pcols, v=np.ones(rows)), np.full(pcols, float(rows))), label
        if rows > 1:      # a shorter logical height over the same matrix: the rows behind it are not read
            assert np.array_equal(dev.dbg_colreduce(ctx, B, rows - 1, pcols, v=v[:-1]), v[:-1] @ H[:-1]), label
        del B, ones
    ctx.trim()


@pytest.mark.parametrize("pcols", sorted({p for _, p in COL_SHAPES}))
def test_column_reduction_accuracy(dev, ctx, pcols):
    rng = np.random.default_rng(pcols)
    worst = 0.0
    for rows in [r for r, p in COL_SHAPES if p == pcols]:
        H = wide_matrix(rng, rows, pcols)
        v = wide_matrix(rng, rows, 1)[:, 0]
        B = upload(dev, ctx, H, nan_rows=2)
        preset = wide_matrix(rng, 1, pcols)[0]
        Hl, vl = H.astype(LD), v.astype(LD)
        cases = [
            ("dot", dev.dbg_colreduce(ctx, B, rows, pcols, v=v), np.sum(Hl * vl[:, None], axis=0), np.abs(H * v[:, None]).sum(axis=0), False),
            ("squares", dev.dbg_colreduce(ctx, B, rows, pcols), np.sum(Hl * Hl, axis=0), (H * H).sum(axis=0), False),
            ("dot, subtract", dev.dbg_colreduce(ctx, B, rows, pcols, v=v, out=preset, subtract=True),
             preset.astype(LD) - np.sum(Hl * vl[:, None], axis=0), np.abs(preset) + np.abs(H * v[:, None]).sum(axis=0), True),
            ("squares, subtract", dev.dbg_colreduce(ctx, B, rows, pcols, out=preset, subtract=True),
             preset.astype(LD) - np.sum(Hl * Hl, axis=0), np.abs(preset) + (H * H).sum(axis=0), True),
        ]
        for what, got, ref, mag, sub in cases:
            assert np.all(np.isfinite(got)), (rows, pcols, what)
            depth = col_depth(rows, pcols, sub)
            ratio = float(np.max(np.abs(got.astype(LD) - ref) / (gamma(depth) * mag)))
            worst = max(worst, ratio)
            assert ratio <= 1.0, "%d x %d %s: error %.3f of gamma(%d) sum|terms|" % (rows, pcols, what, ratio, depth)
        del B
    print("\ncolumn reduction, %d columns: largest error %.3f of its bound" % (pcols, worst))
    ctx.trim()


@pytest.mark.parametrize("cols", ROW_COLS)
def test_row_reduction(dev, ctx, cols):
    rng = np.random.default_rng(cols)
    worst = 0.0
    for rows in ROW_ROWS:
        label = "%d x %d" % (rows, cols)
        H, v = int_matrix(rows, cols), int_weights(cols)
        A = upload(dev, ctx, H, nan_cols=2)
        dot = dev.dbg_rowreduce(ctx, A, cols, v=v)
        assert np.array_equal(dot, H @ v), label
        assert np.array_equal(dev.dbg_rowreduce(ctx, A, cols, v=v), dot), label
        assert np.array_equal(dev.dbg_rowreduce(ctx, A, cols), np.sum(H * H, axis=1)), label
        assert np.array_equal(dev.dbg_rowreduce(ctx, A, cols, v=v, weighted_squares=True), (H * H) @ v), label
        ones = upload(dev, ctx, np.ones((rows, cols)), nan_cols=2)
        for got in (dev.dbg_rowreduce(ctx, ones, cols), dev.dbg_rowreduce(ctx, ones, cols, v=np.ones(cols)),
                    dev.dbg_rowreduce(ctx, ones, cols, v=np.ones(cols), weighted_squares=True)):
            assert np.array_equal(got, np.full(rows, float(cols))), label
        if cols > 2:      # a narrower logical width over the same matrix
            assert np.array_equal(dev.dbg_rowreduce(ctx, A, cols - 2, v=v[:-2]), H[:, :-2] @ v[:-2]), label
        H, v = wide_matrix(rng, rows, cols), wide_matrix(rng, 1, cols)[0]
        A = upload(dev, ctx, H, nan_cols=2)
        Hl, vl = H.astype(LD), v.astype(LD)
        for what, got, ref, mag, wsq in (
                ("dot", dev.dbg_rowreduce(ctx, A, cols, v=v), np.sum(Hl * vl[None, :], axis=1), np.abs(H * v[None, :]).sum(axis=1), False),
                ("squares", dev.dbg_rowreduce(ctx, A, cols), np.sum(Hl * Hl, axis=1), (H * H).sum(axis=1), False),
                ("weighted squares", dev.dbg_rowreduce(ctx, A, cols, v=v, weighted_squares=True),
                 np.sum(Hl * Hl * vl[None, :], axis=1), np.abs(H * H * v[None, :]).sum(axis=1), True)):
            assert np.all(np.isfinite(got)), (label, what)
            depth = row_depth(cols, wsq)
            ratio = float(np.max(np.abs(got.astype(LD) - ref) / (gamma(depth) * mag)))
            worst = max(worst, ratio)
            assert ratio <= 1.0, "%s %s: error %.3f of gamma(%d) sum|terms|" % (label, what, ratio, depth)
    print("\nrow reduction, %d columns: largest error %.3f of its bound" % (cols, worst))


@pytest.mark.parametrize("n", SUM_N)
def test_sum(dev, ctx, n):
    x = int_weights(n) * 1000.0 + np.arange(n)
    assert dev.dbg_sum(ctx, x) == float(np.sum(x.astype(np.int64)))
    assert dev.dbg_sum(ctx, np.ones(n)) == float(n)
    x = wide_matrix(np.random.default_rng(n), 1, n)[0]
    got = dev.dbg_sum(ctx, x)
    assert dev.dbg_sum(ctx, x) == got
    depth = (n + 255) // 256 + 8
    ratio = float(abs(LD(got) - np.sum(x.astype(LD))) / (gamma(depth) * np.abs(x).sum()))
    print("\nsum of %d: error %.3f of gamma(%d) sum|x|" % (n, ratio, depth))
    assert ratio <= 1.0


def test_public_col_sumsq_and_matvec(dev, ctx):
    """gpx_col_sumsq and gpx_matvec on a padded 300 x 130 matrix (384 x 256 on the device), by the same rules; entries of the host
    result behind the logical width are not touched."""
    rows, cols = 300, 130
    H, v = int_matrix(rows, cols), int_weights(cols)
    A = dev.DeviceMatrix.from_host(ctx, H, pad=True)
    assert np.array_equal(dev.col_sumsq(ctx, A, rows), np.sum(H * H, axis=0))
    assert np.array_equal(dev.col_sumsq(ctx, A, 384), np.sum(H * H, axis=0))          # the padding rows are zero
    assert np.array_equal(dev.col_sumsq(ctx, A, 17), np.sum(H[:17] * H[:17], axis=0))
    assert np.array_equal(dev.matvec(ctx, A, v), H @ v)
    ones = dev.DeviceMatrix.from_host(ctx, np.ones((rows, cols)), pad=True)
    assert np.array_equal(dev.col_sumsq(ctx, ones, rows), np.full(cols, float(rows)))
    assert np.array_equal(dev.matvec(ctx, ones, np.ones(cols)), np.full(rows, float(cols)))
    out = np.full(256, -7.25)
    dev.check(ctx.lib.gpx_col_sumsq(ctx.h, A.h, rows, out.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.array_equal(out[:cols], np.sum(H * H, axis=0)) and np.all(out[cols:] == -7.25)
    # a row of NaN behind the logical height
    Hn = H.copy()
    Hn[rows - 1] = np.nan
    An = dev.DeviceMatrix.from_host(ctx, Hn, pad=True)
    assert np.array_equal(dev.col_sumsq(ctx, An, rows - 1), np.sum(H[:-1] * H[:-1], axis=0))
    rng = np.random.default_rng(130)
    H, v = wide_matrix(rng, rows, cols), wide_matrix(rng, 1, cols)[0]
    A = dev.DeviceMatrix.from_host(ctx, H, pad=True)
    Hl = H.astype(LD)
    ss, mv = dev.col_sumsq(ctx, A, rows), dev.matvec(ctx, A, v)
    assert np.array_equal(dev.col_sumsq(ctx, A, rows), ss) and np.array_equal(dev.matvec(ctx, A, v), mv)
    r1 = float(np.max(np.abs(ss.astype(LD) - np.sum(Hl * Hl, axis=0)) / (gamma(col_depth(rows, 256)) * (H * H).sum(axis=0))))
    r2 = float(np.max(np.abs(mv.astype(LD) - np.sum(Hl * v.astype(LD)[None, :], axis=1)) / (gamma(row_depth(256)) * np.abs(H * v[None, :]).sum(axis=1))))
    print("\ncol_sumsq error %.3f, matvec error %.3f of their bounds" % (r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0
