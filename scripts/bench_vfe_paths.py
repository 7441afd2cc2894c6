"""Times pathwise Thompson sampling on a VFE model (gpx_vfe_paths_create + one gpx_paths_eval arg-best pass) and, beside it, the
dense pathSampler at the largest training-set size whose factor the device holds.

    python scripts/bench_vfe_paths.py [--n 262144] [--nu 1024] [--d 8] [--features 1024] [--paths 64] [--m 1048576]
                                      [--dense-n 131072] [--reps 3] [--out FILE]

Per side: the fit, the create (ending in a device synchronise; the first one also builds the factors' block inverses, so a second
one is timed too) and `reps` whole arg-best passes over the M points (only S indices and values reach the host), medians.  The dense
side halves --dense-n until the allocator accepts the factor.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, ctx):
    t = time.perf_counter()
    out = fn()
    ctx.sync()
    return time.perf_counter() - t, out


def passes(smp, dZ, ctx, reps):
    timed(lambda: smp.argbest(dZ), ctx)
    return [timed(lambda: smp.argbest(dZ), ctx)[0] for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--dense-n", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gpexp_amd import device as dev
    from gpexp_amd._lib import GpxError
    from gpexp_amd.paths import PathBase, spectralFrequencies
    ctx = dev.context()
    rng = np.random.default_rng(0)
    n, nu, d, L, S, M = a.n, a.nu, a.d, a.features, a.paths, a.m
    X = rng.uniform(0.0, 1.0, (n, d))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Z = rng.uniform(0.0, 1.0, (M, d))
    noise = 1e-2
    spec = dev.KernelSpec(dev.K_MATERN52, d, [1.5, 1.2])
    dZ = dev.points(ctx, Z)
    res = dict(d=d, features=L, paths=S, m=M, kernel="matern52", device=ctx.info().get("name"))

    # ---- the VFE model ----
    dX, dS = dev.points(ctx, X), dev.points(ctx, X[rng.permutation(n)[:nu]])
    fit_s, model = timed(lambda: dev.VfeModel(ctx, spec, dX, dS, noise), ctx)
    alpha = model.solve(y)[0]
    base = PathBase.draw(S, L, 2 * nu, d, spec, rng=1)
    om = spectralFrequencies(spec, base.g, base.u)

    def create():
        return model.path_sampler(dS, alpha, om, base.phase, base.w, np.sqrt(noise) * base.xi[:, :nu], base.xi[:, nu:])
    first_s, smp = timed(create, ctx)
    smp.close()
    creates = []
    for i in range(a.reps):
        t, smp = timed(create, ctx)
        creates.append(t)
        if i + 1 < a.reps:
            smp.close()
    tp = passes(smp, dZ, ctx, a.reps)
    smp.close()
    res["vfe"] = dict(n=n, nu=nu, fit_seconds=fit_s, first_create_seconds=first_s, create_seconds=float(np.median(creates)),
                      create_all=creates, argbest_seconds=float(np.median(tp)), argbest_all=tp,
                      generated_per_second=(L + nu) * M / float(np.median(tp)))
    del model, dX

    # ---- the dense model, at the largest N whose factor fits ----
    nd = a.dense_n
    while nd >= 1024:
        try:
            dXd = dev.points(ctx, X[:nd])
            fit_s, Lf = timed(lambda: dev.potrf(ctx, dev.kfill(ctx, spec, dXd, nugget=noise)), ctx)
            break
        except (GpxError, MemoryError) as e:
            res.setdefault("dense_refused", []).append(dict(n=nd, error=str(e)[:200]))
            ctx.trim()
            nd //= 2
    al = dev.potrs(ctx, Lf, y[:nd])
    based = PathBase.draw(S, L, nd, d, spec, rng=1)

    def created():
        return dev.PathSampler(ctx, spec, Lf, dXd, al, om, based.phase, based.w, np.sqrt(noise) * based.xi)
    first_s, smp = timed(created, ctx)
    smp.close()
    create_s, smp = timed(created, ctx)
    tp = passes(smp, dZ, ctx, a.reps)
    smp.close()
    res["dense"] = dict(n=nd, fit_seconds=fit_s, first_create_seconds=first_s, create_seconds=create_s,
                        argbest_seconds=float(np.median(tp)), argbest_all=tp, generated_per_second=(L + nd) * M / float(np.median(tp)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
