"""Strassen's scheme applied more than once in the large NN updates of the left solve (gemm_f64.hip strassen_rec /
launch_gemm_strassen with a depth, gemm_f64_multi_kernel; chol.hip strassen_gate; GPX_STRASSEN = the maximum depth).

* without a device: a NumPy transcription of the nested scheme -- each product is handed its list of (destination, sign),
  expanded level by level through the table of the seven products -- reproduces C - A B at depth 1, 2, 3.  This pins the algebra
  and the rounding model; the native tables are pinned by the device tests;
* the driver forced to depth 2 (gpx_dbg_gemm_strassen_depth) against NumPy at the 1e-13 relative max-norm that
  tests/test_gpu_parity.py applies to every GEMM form, with and without skewed leading dimensions, with inner products on the
  64-tile and on the 128-tile path; a repeat gives the same bits;
* shapes depth 2 refuses give the bits of depth 1, shapes depth 1 refuses those of the classical product;
* the path in use: the bench workload at N = M = 32768 with the switch unset against GPX_STRASSEN=0 and GPX_STRASSEN=1 at the
  tolerances of tests/test_gpu_strassen.py (variances 1e-10 max-norm, 1e-9 element-wise, IVAR 1e-10 relative)."""
import os

import numpy as np
import pytest


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# ---- the algebra, on the host -------------------------------------------------------------------------------------------------
# products M1 .. M7 as (left operand, right operand, [(quadrant of C, sign), ...]); an operand is a list of (quadrant, sign)
# terms; quadrants 0 = X11, 1 = X12, 2 = X21, 3 = X22
PRODUCTS = [
    ([(0, 1), (3, 1)], [(0, 1), (3, 1)], [(0, 1.0), (3, 1.0)]),
    ([(2, 1), (3, 1)], [(0, 1)], [(2, 1.0), (3, -1.0)]),
    ([(0, 1)], [(1, 1), (3, -1)], [(1, 1.0), (3, 1.0)]),
    ([(3, 1)], [(2, 1), (0, -1)], [(0, 1.0), (2, 1.0)]),
    ([(0, 1), (1, 1)], [(3, 1)], [(1, 1.0), (0, -1.0)]),
    ([(2, 1), (0, -1)], [(0, 1), (1, 1)], [(3, 1.0)]),
    ([(1, 1), (3, -1)], [(2, 1), (3, 1)], [(0, 1.0)]),
]


def quadrant(X, q):
    hr, hc = X.shape[0] // 2, X.shape[1] // 2
    return X[(q >> 1) * hr:(q >> 1) * hr + hr, (q & 1) * hc:(q & 1) * hc + hc]


def operand(X, terms):
    if len(terms) == 1:
        return quadrant(X, terms[0][0])          # a raw quadrant is used where it lies
    (q0, _), (q1, s1) = terms
    return quadrant(X, q0) + quadrant(X, q1) if s1 > 0 else quadrant(X, q0) - quadrant(X, q1)


def nested(A, B, dests, depth, launches):
    """every (view of C, sign) in dests -= sign * (A B), `depth` levels deep; launches counts destinations per product"""
    if depth == 0:
        assert len(dests) <= 2 ** 3 and len({d.__array_interface__["data"][0] for d, _ in dests}) == len(dests)
        launches.append(len(dests))
        P = A @ B
        for d, s in dests:
            d -= s * P
        return
    for ta, tb, out in PRODUCTS:
        sub = [(quadrant(d, q), s * sq) for d, s in dests for q, sq in out]
        nested(operand(A, ta), operand(B, tb), sub, depth - 1, launches)


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("positive", [False, True])
def test_nested_scheme_on_the_host(depth, positive):
    rng = np.random.default_rng(100 * depth + positive)
    m, n, k = 256, 512, 384
    draw = (lambda s: rng.uniform(0.0, 1.0, s)) if positive else rng.standard_normal
    A, B, C0 = draw((m, k)), draw((k, n)), draw((m, n))
    C = C0.copy()
    launches = []
    nested(A, B, [(C, 1.0)], depth, launches)
    assert len(launches) == 7 ** depth and max(launches) == 2 ** depth
    r = rel(C, C0 - A @ B)
    print("nested scheme on the host, depth %d, positive=%d: rel = %.3e" % (depth, positive, r))
    assert r <= 1e-13


# ---- the driver, on the device ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def run_depth(dev, ctx, A, B, C0, pad, depth):
    dA = dev.DeviceMatrix.from_host(ctx, A, pad=pad)
    dB = dev.DeviceMatrix.from_host(ctx, B, pad=pad)
    dC = dev.DeviceMatrix.from_host(ctx, C0, pad=pad)
    if depth == "one":
        dev.dbg_gemm_strassen(ctx, dA, dB, dC)
    elif depth == "classical":
        dev.dbg_gemm(ctx, dA, dB, dC, 0, 1)
    else:
        dev.dbg_gemm_strassen_depth(ctx, dA, dB, dC, depth)
    return dC.to_host()


# m, n, k; pad=True skews the leading dimension of every operand whose width is a multiple of 256 from 1024 on.
# 4096 x 8192 x 2048: inner products 1024 x 2048 x 512 = 128 128-tiles -> the 64-tile kernels; 16384 x 16384 x 256: inner
# products 4096 x 4096 x 64 = 1024 128-tiles -> the 128-tile kernels (short k keeps the host product to seconds)
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,pad", [(512, 512, 64, False), (1024, 2048, 1024, False), (1024, 2048, 1024, True),
                                       (1536, 4608, 2560, True), (4096, 8192, 2048, True), (16384, 16384, 256, True),
                                       (16384, 16384, 256, False)])
def test_depth2_driver_vs_numpy(dev, ctx, m, n, k, pad):
    rng = np.random.default_rng(m + n + k + 2)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((k, n))
    C0 = rng.standard_normal((m, n))
    got = run_depth(dev, ctx, A, B, C0, pad, 2)
    want = C0 - A @ B
    assert got.shape == want.shape and np.all(np.isfinite(got))
    r = rel(got, want)
    print("strassen depth 2, %d x %d x %d pad=%d: rel = %.3e" % (m, n, k, pad, r))
    assert r <= 1e-13
    # the two-level path ran: one level rounds differently
    assert not np.array_equal(got, run_depth(dev, ctx, A, B, C0, pad, "one"))
    # the same call again on fresh data gives the same bits (fixed launch order on one stream)
    assert np.array_equal(run_depth(dev, ctx, A, B, C0, pad, 2), got)
    ctx.trim()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(768, 512, 128), (512, 1280, 128), (512, 512, 96)])
def test_depth2_refused_is_depth1(dev, ctx, m, n, k):
    """m or n not a multiple of 512, k not of 64, but admissible for one level: exactly the one-level result."""
    rng = np.random.default_rng(m * 3 + n * 5 + k)
    A, B, C0 = rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
    got = run_depth(dev, ctx, A, B, C0, False, 2)
    assert np.array_equal(got, run_depth(dev, ctx, A, B, C0, False, "one"))
    assert np.array_equal(got, run_depth(dev, ctx, A, B, C0, False, 1))
    assert not np.array_equal(got, run_depth(dev, ctx, A, B, C0, False, "classical"))
    assert rel(got, C0 - A @ B) <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(384, 512, 256), (512, 512, 48), (512, 640, 64)])
def test_depth1_refused_is_classical(dev, ctx, m, n, k):
    """shapes one level refuses: the classical product bit for bit, whatever depth is asked for; depth 0 asks for it"""
    rng = np.random.default_rng(m * 3 + n * 5 + k)
    A, B, C0 = rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
    want = run_depth(dev, ctx, A, B, C0, False, "classical")
    for depth in (0, 1, 2):
        assert np.array_equal(run_depth(dev, ctx, A, B, C0, False, depth), want)
    A, B, C0 = rng.standard_normal((512, 512)), rng.standard_normal((512, 512)), rng.standard_normal((512, 512))
    assert np.array_equal(run_depth(dev, ctx, A, B, C0, False, 0), run_depth(dev, ctx, A, B, C0, False, "classical"))


@pytest.mark.gpu
def test_depth2_in_the_solve_c4(dev, ctx):
    """The bench workload (N = 32768, d = 8, Matern-5/2, rho = 0.5, noise = 0.1, seed 32768), all M = 32768 evaluation points:
    variances and IVAR with the switch unset (two levels in the top update) and with GPX_STRASSEN=1 (one level: the arithmetic
    before this change) against GPX_STRASSEN=0."""
    N, d, noise = 32768, 8, 0.1
    rng = np.random.default_rng(32768)
    Xh = rng.uniform(-1, 1, (N, d))
    _ = np.sin(2 * np.pi * Xh.sum(1) / d) + np.sqrt(noise) * rng.standard_normal(N)   # (the workload's y: keeps the stream of draws)
    Zh = rng.uniform(-1, 1, (N, d))
    sp = dev.KernelSpec(dev.K_MATERN52, d, [0.5, 1.0])
    X, Z = dev.points(ctx, Xh), dev.points(ctx, Zh)
    K = dev.kfill(ctx, sp, X, nugget=noise)
    dev.potrf(ctx, K)
    saved = os.environ.pop("GPX_STRASSEN", None)
    res = {}
    try:
        for setting in (None, "1", "0"):
            if setting is not None:
                os.environ["GPX_STRASSEN"] = setting
            _, v = dev.posterior(ctx, sp, K, X, None, Z, want_mean=False)
            res[setting] = (v, dev.ivar(ctx, sp, K, X, Z))
            if setting is None:
                _, v2 = dev.posterior(ctx, sp, K, X, None, Z, want_mean=False)
    finally:
        if saved is None:
            os.environ.pop("GPX_STRASSEN", None)
        else:
            os.environ["GPX_STRASSEN"] = saved
    v0, iv0 = res["0"]
    assert np.array_equal(res[None][0], v2)                      # deterministic
    assert np.all(v0 > 0)
    msg = "above 1e-12 this is a bug in the scheme, not rounding"
    for setting in (None, "1"):
        v, iv = res[setting]
        assert np.all(np.isfinite(v))
        mx = rel(v, v0)
        ew = float(np.max(np.abs(v - v0) / np.abs(v0)))
        ri = abs(iv - iv0) / abs(iv0)
        print("GPX_STRASSEN=%s vs classical at C4: variances max-norm %.3e, element-wise %.3e, IVAR relative %.3e, bit-identical "
              "entries %d of %d" % (setting, mx, ew, ri, int(np.sum(v == v0)), v0.size))
        assert mx <= 1e-10, (setting, mx, msg)
        assert ew <= 1e-9, (setting, ew, msg)
        assert ri <= 1e-10, (setting, ri, msg)
        assert not np.array_equal(v, v0), "the gate admits this size: the Strassen path should have run"
    assert not np.array_equal(res[None][0], res["1"][0]), "the gate admits two levels at this size: the deeper path should have run"
    del K
    ctx.trim()
