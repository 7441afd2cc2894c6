"""Times gpx_paths_eval (the generated-operand MFMA product) against the composed route the library offered before it for the same
numbers: gpx_kfill of K(X, Zc) into HBM plus the fp64 GEMM with V.  The composed route is timed WITHOUT the feature term (nothing
on the device generated it before), so its figure is a lower bound on what that route would cost.

    python scripts/bench_paths.py [--n 32768] [--d 8] [--features 4096] [--m 1048576] [--paths 1,16,64] [--reps 3] [--out FILE]

Per S: median wall time of a whole pass over the M points ending in a device synchronise (the fused call includes the per-path
arg-best; only S indices reach the host), the two alternated in the same process after one warm-up pass each; the operation counts
come from the shapes: generated elements (L + N) M (one cos or one exp each), MFMA flops 2 Sp (L + N) M, HBM bytes of the composed
route 2 * 8 N M (B written and read back).  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--paths", default="1,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16384, help="points per chunk of the composed route (its N x chunk buffer)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gpexp_amd import device as dev
    from gpexp_amd.paths import PathBase, spectralFrequencies
    ctx = dev.context()
    rng = np.random.default_rng(0)
    n, d, L, M = a.n, a.d, a.features, a.m
    X = rng.uniform(0.0, 1.0, (n, d))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Z = rng.uniform(0.0, 1.0, (M, d))
    noise = 1e-2
    spec = dev.KernelSpec(dev.K_SE, d, [0.5] * d + [1.0])
    dX, dZ = dev.points(ctx, X), dev.points(ctx, Z)
    t0 = time.perf_counter()
    Lf = dev.potrf(ctx, dev.kfill(ctx, spec, dX, nugget=noise))
    alpha = dev.potrs(ctx, Lf, y)
    ctx.sync()
    fit_s = time.perf_counter() - t0
    chunks = [dev.points(ctx, Z[j:j + a.chunk]) for j in range(0, M, a.chunk)]
    B = dev.DeviceMatrix.zeros(ctx, n, a.chunk, pad=True)
    Cm = dev.DeviceMatrix.zeros(ctx, 128, a.chunk, pad=True)
    res = dict(n=n, d=d, features=L, m=M, kernel="se", fit_seconds=fit_s, device=ctx.info().get("name"), cases=[])
    for S in [int(s) for s in a.paths.split(",")]:
        base = PathBase.draw(S, L, n, d, spec, rng=1)
        t0 = time.perf_counter()
        smp = dev.PathSampler(ctx, spec, Lf, dX, alpha, spectralFrequencies(spec, base.g, base.u), base.phase, base.w,
                              np.sqrt(noise) * base.xi)
        ctx.sync()
        create_s = time.perf_counter() - t0
        Vpad = np.zeros((128, n))                      # the GEMM's row tile is 128: the composed route pays for it whatever S is
        Vpad[:min(S, 128)] = smp.coefficients()[:128]
        Vd = dev.DeviceMatrix.from_host(ctx, Vpad, pad=True)

        def fused():
            t = time.perf_counter()
            smp.argbest(dZ)
            ctx.sync()
            return time.perf_counter() - t

        def composed():
            t = time.perf_counter()
            for zc in chunks:
                if zc.shape[0] == a.chunk:
                    dev.kfill_into(ctx, spec, dX, B, Z=zc)
                    dev.dbg_gemm(ctx, Vd, B, Cm, 0, 0)
            ctx.sync()
            return time.perf_counter() - t

        fused(), composed()
        tf, tc = [], []
        for _ in range(a.reps):
            tf.append(fused())
            tc.append(composed())
        Sp = (S + 15) // 16 * 16
        f, c = float(np.median(tf)), float(np.median(tc))
        res["cases"].append(dict(S=S, create_seconds=create_s, fused_seconds=f, fused_all=tf, composed_seconds=c, composed_all=tc,
                                 generated_per_second=(L + n) * M / f, fused_mfma_tflops=2.0 * Sp * (L + n) * M / f / 1e12,
                                 composed_hbm_bytes=16.0 * n * M, speedup=c / f))
        smp.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
