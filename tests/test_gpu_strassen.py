"""One level of Strassen's scheme in the large NN updates of the left solve (gemm_f64.hip launch_gemm_strassen, chol.hip
trsm_left_oop_rec; switch GPX_STRASSEN, default on, 0 = classical everywhere).

* the driver, forced through gpx_dbg_gemm_strassen, against NumPy at the tolerance tests/test_gpu_parity.py applies to every GEMM
  form (1e-13 relative, max-norm; a CPU experiment with the same scheme gives 2e-15 on random operands);
* shapes the driver refuses run the classical product bit for bit;
* the path in use: the bench workload at N = M = 32768 with the switch unset against GPX_STRASSEN=0 in the same process, at the
  two tolerances tests/test_gpu_golden_r6.py applies to variances against LAPACK (1e-10 max-norm, 1e-9 element-wise), IVAR at
  1e-10 relative; a repeat reproduces the bits (fixed product order on one stream)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# m, n, k; pad=True skews the leading dimension of every operand whose width is a multiple of 256 from 1024 on
@pytest.mark.parametrize("m,n,k,pad", [(512, 1024, 512, False), (512, 1024, 512, True), (1280, 2304, 1536, True),
                                       (2048, 512, 4096, True), (256, 256, 32, False), (4096, 4608, 2048, True)])
def test_strassen_driver_vs_numpy(dev, ctx, m, n, k, pad):
    rng = np.random.default_rng(m + n + k)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((k, n))
    C0 = rng.standard_normal((m, n))
    dA = dev.DeviceMatrix.from_host(ctx, A, pad=pad)
    dB = dev.DeviceMatrix.from_host(ctx, B, pad=pad)
    dC = dev.DeviceMatrix.from_host(ctx, C0, pad=pad)
    dev.dbg_gemm_strassen(ctx, dA, dB, dC)
    got, want = dC.to_host(), C0 - A @ B
    assert got.shape == want.shape and np.all(np.isfinite(got))
    r = rel(got, want)
    print("strassen %d x %d x %d pad=%d: rel = %.3e" % (m, n, k, pad, r))
    assert r <= 1e-13
    # the same call again on fresh data gives the same bits (fixed order of the seven products)
    dC2 = dev.DeviceMatrix.from_host(ctx, C0, pad=pad)
    dev.dbg_gemm_strassen(ctx, dA, dB, dC2)
    assert np.array_equal(dC2.to_host(), got)


@pytest.mark.parametrize("m,n,k", [(384, 512, 256), (512, 512, 48), (512, 640, 64)])
def test_strassen_driver_refuses_odd_shapes(dev, ctx, m, n, k):
    """m or n not a multiple of 256, k not of 32: exactly the classical product."""
    rng = np.random.default_rng(m * 3 + n * 5 + k)
    A = rng.standard_normal((m, k))
    B = rng.standard_normal((k, n))
    C0 = rng.standard_normal((m, n))
    dA = dev.DeviceMatrix.from_host(ctx, A, pad=False)
    dB = dev.DeviceMatrix.from_host(ctx, B, pad=False)
    dC = dev.DeviceMatrix.from_host(ctx, C0, pad=False)
    dD = dev.DeviceMatrix.from_host(ctx, C0, pad=False)
    dev.dbg_gemm_strassen(ctx, dA, dB, dC)
    dev.dbg_gemm(ctx, dA, dB, dD, 0, 1)
    assert np.array_equal(dC.to_host(), dD.to_host())
    assert rel(dC.to_host(), C0 - A @ B) <= 1e-13


def test_strassen_in_the_solve_c4(dev, ctx):
    """The bench workload (N = 32768, d = 8, Matern-5/2, rho = 0.5, noise = 0.1, seed 32768), all M = 32768 evaluation points:
    the variances and the IVAR with the switch unset against GPX_STRASSEN=0.  Measured on MI355X: max-norm 1.3e-14, element-wise 5.1e-14 (the variance is a difference
    k(z,z) - |w|^2 of two numbers near 1, so its relative error is a few times that of the solve), IVAR identical to the last bit."""
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
    try:
        _, v1 = dev.posterior(ctx, sp, K, X, None, Z, want_mean=False)
        _, v2 = dev.posterior(ctx, sp, K, X, None, Z, want_mean=False)
        iv1 = dev.ivar(ctx, sp, K, X, Z)
        os.environ["GPX_STRASSEN"] = "0"
        _, v0 = dev.posterior(ctx, sp, K, X, None, Z, want_mean=False)
        iv0 = dev.ivar(ctx, sp, K, X, Z)
    finally:
        if saved is None:
            os.environ.pop("GPX_STRASSEN", None)
        else:
            os.environ["GPX_STRASSEN"] = saved
    assert np.array_equal(v1, v2)                      # deterministic
    assert np.all(np.isfinite(v1)) and np.all(v0 > 0)
    mx = rel(v1, v0)
    ew = float(np.max(np.abs(v1 - v0) / np.abs(v0)))
    ri = abs(iv1 - iv0) / abs(iv0)
    print("strassen vs classical at C4: variances max-norm %.3e, element-wise %.3e, IVAR relative %.3e, bit-identical entries %d of %d"
          % (mx, ew, ri, int(np.sum(v1 == v0)), v0.size))
    msg = "above 1e-12 this is a bug in the scheme, not rounding"
    assert mx <= 1e-10, (mx, msg)
    assert ew <= 1e-9, (ew, msg)
    assert ri <= 1e-10, (ri, msg)
    assert not np.array_equal(v1, v0), "the gate admits this size: the Strassen path should have run"
    del K
    ctx.trim()
