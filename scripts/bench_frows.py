#!/usr/bin/env python3
"""Performance evidence for the SURVEY.md 8 f-rows and the design kernels: one JSON line per
entry point with its size, best-of-3 time, the algorithmic work and the achieved rate against the roof that bounds it.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel table (profiles/r03_frows_kernel_stats.csv).

    python scripts/bench_frows.py [--quick] [--only f1,design,mi,fitc,refit,f3,acq,loo,vfedesign,sample,qei,vfeqei] [--kernel se,matern52] [--out FILE]

--kernel: the kernels the `f1` and `design` entries are timed with, one after the other in this process (se, matern32,
matern52; default se) -- the other entries keep their own kernels.
--out: the `loo` section also appends its lines to this file (profiles/loo_frows.jsonl), the `fitc` section its two
leave-one-out lines (profiles/fitc_loo_frows.jsonl).
--sample-out: where the `sample`, `qei` and `vfeqei` sections append their lines (default profiles/sample_qei_frows.jsonl).
--vfe-out: where the `fitc` section appends its gpx_vfe_* lines (default profiles/vfe_frows.jsonl).
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpexp_amd import device as dev  # noqa: E402

PEAK_TF, PEAK_GBS = 78.6, 8000.0
ctx = dev.context()
quick = "--quick" in sys.argv
only = set(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else None
kernels = sys.argv[sys.argv.index("--kernel") + 1].split(",") if "--kernel" in sys.argv else ["se"]


def want(section):
    return only is None or section in only


def best(f, reps=3):
    ts = []
    out = None
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = f()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return out, min(ts)


def report(name, replaces, size, t, flops=None, nbytes=None, note=""):
    line = {"entry": name, "replaces": replaces, "size": size, "ms": 1e3 * t}
    if flops is not None:
        line.update(bound="mfma", algorithmic_flop=flops, achieved_tflops=flops / t / 1e12, frac=flops / t / 1e12 / PEAK_TF)
    if nbytes is not None:
        line.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / t / 1e9, frac=nbytes / t / 1e9 / PEAK_GBS)
    if note:
        line["note"] = note
    print(json.dumps(line), flush=True)
    return line


rng = np.random.default_rng(8192)
d = 8
sp = dev.KernelSpec(dev.K_SE, d, list(0.4 + 0.05 * np.arange(d)) + [1.0])


def kernel_choice(name):
    """(KernelSpec, kernel-class factory) of a --kernel name at d = 8."""
    from gpExp.kernels import KernelSquaredExponential, KernelIsoMatern
    if name == "se":
        return sp, lambda: KernelSquaredExponential(list(0.4 + 0.05 * np.arange(d)), 1.0, d)
    nu = {"matern32": 1.5, "matern52": 2.5}[name]
    k = KernelIsoMatern(0.7, 1.0, d, nu=nu)
    return k._spec(), lambda: KernelIsoMatern(0.7, 1.0, d, nu=nu)


# ---- f1: gradients of the posterior variance w.r.t. point locations (gp.py:261-341, experimentalDesign.py:168-179)
for kname in (kernels if want("f1") else []):
    ksp, make_kernel = kernel_choice(kname)
    N, M = (2048, 8192) if quick else (8192, 32768)
    Xh, Zh = rng.uniform(-1, 1, (N, d)), rng.uniform(-1, 1, (M, d))
    X, Z = dev.points(ctx, Xh), dev.points(ctx, Zh)
    L = dev.potrf(ctx, dev.kfill(ctx, ksp, X, nugget=0.1))
    _, t = best(lambda: dev.ivar_grad(ctx, ksp, L, X, Z))
    report("gpx_ivar_grad", "costFunctionGP_IVAR.derivative v1 (experimentalDesign.py:168-179)", dict(N=N, M=M, d=d, kernel=kname), t,
           flops=3.0 * N * N * M, note="ONE count, in SURVEY 8d's units (a triangular solve of an N x M block = N^2 M): beta = K^-1 K(X,Z) "
           "is two solves (2 N^2 M), S = beta beta^T as a lower SYRK is N^2 M more; tr(dK/dx S) needs S")
    _, t = best(lambda: dev.var_grad_newpt(ctx, ksp, L, X, Z))
    report("gpx_var_grad_newpt", "GP.evaluateVarianceDerivWRTnewpt (gp.py:261-280)", dict(N=N, M=M, d=d, kernel=kname), t, flops=2.0 * N * N * M)
    # one optimiser iteration of a continuous design (SLSQP, experimentalDesign.py:471-489): cost, then gradient, same design
    from gpExp.gp import GP
    from gpExp.approximation import Space
    from gpExp.experimentalDesign import costFunctionGP_IVAR
    space = Space(d, lambda size: rng.uniform(-1, 1, size), lambda p: np.ones(len(p)))
    def iteration(reuse):
        g = GP(make_kernel(), 0.1)
        g.reuseFactor = reuse
        cf = costFunctionGP_IVAR(g, N, space, mcPoints=Zh)
        cf.evaluate(Xh); cf.derivative(Xh)                      # warm: pools, block inverses
        Xq = Xh * 0.999                                         # a new design in EVERY point: one full fit, one full forward solve
        def both():
            cf.evaluate(Xq)
            return cf.derivative(Xq)
        return best(both, reps=1)[1]
    def batch_move(reuse, nb_=512):
        g = GP(make_kernel(), 0.1)
        g.reuseFactor = reuse
        cf = costFunctionGP_IVAR(g, N, space, mcPoints=Zh)
        cf.evaluate(Xh)
        ts = []
        for rep in range(3):
            Xq = Xh.copy(); Xq[-nb_:] = np.random.default_rng(rep).uniform(-1, 1, (nb_, d))
            ts.append(best(lambda: cf.evaluate(Xq), reps=1)[1])
        return min(ts)
    def batch_gradient(pinned, nb_=512):
        g = GP(make_kernel(), 0.1)
        cf = costFunctionGP_IVAR(g, N, space, mcPoints=Zh)
        cf.pinnedPoints = pinned
        cf.evaluate(Xh); cf.derivative(Xh)
        Xq = Xh.copy(); Xq[-nb_:] = np.random.default_rng(7).uniform(-1, 1, (nb_, d))
        cf.evaluate(Xq)
        return best(lambda: cf.derivative(Xq), reps=2)[1]
    t_gall, t_gfree = batch_gradient(0), batch_gradient(N - 512)
    report("design gradient of the last 512 points", "costFunctionGP_IVAR.derivative inside the batch loop (experimentalDesign.py:"
           "694-751: earlier batches pinned by equal bounds, :719-724)", dict(N=N, M=M, free=512, d=d, kernel=kname), t_gfree,
           flops=2.0 * 512 * N * M + 512.0 * 512 * M + 512.0 * N * N,
           note="beta_T = L_TT^-T W_T, S_T = (beta_T W^T) L^-1 from the kept solve, row kernel for the free points: %.1f ms for "
                "all points (kept forward solve), %.1f ms for the free ones" % (1e3 * t_gall, 1e3 * t_gfree))
    t_full, t_inc = batch_move(False), batch_move(True)
    report("design cost after moving the last 512 points", "costFunctionGP_IVAR.evaluate inside the batch loop "
           "(experimentalDesign.py:694-751: earlier batches pinned)", dict(N=N, M=M, moved=512, d=d, kernel=kname), t_inc,
           flops=2.0 * 512 * (N - 512) * M + 512.0 * 512 * M + 512.0 * N * N,
           note="refit of the moved rows (rows N^2) + W2 = L22^-1 (K(X2, Z) - L21 W1) on the kept solve; %.1f ms when every evaluation "
                "refits and solves from scratch (reuseFactor = False), %.1f ms incrementally" % (1e3 * t_full, 1e3 * t_inc))
    t_sep, t_shared = iteration(False), iteration(True)
    report("design iteration: cost + gradient", "costFunctionGP_IVAR.evaluate + .derivative at one design (experimentalDesign.py:100-117, "
           "168-179, 471-489)", dict(N=N, M=M, d=d, kernel=kname), t_shared, flops=3.0 * N * N * M + N ** 3 / 3.0,
           note="count = what one iteration needs: ONE fit (N^3/3), the forward solve once (N^2 M), backward solve and SYRK "
                "(2 N^2 M); %.1f ms when the gradient call refits and solves forward again (reuseFactor = False: two fits, "
                "4 N^2 M), %.1f ms with the kept factor and the kept forward solve" % (1e3 * t_sep, 1e3 * t_shared))
    Nv, Mv = (1024, 1024) if quick else (2048, 4096)
    Xv, Zv = dev.points(ctx, Xh[:Nv]), dev.points(ctx, Zh[:Mv])
    Lv = dev.potrf(ctx, dev.kfill(ctx, ksp, Xv, nugget=0.1))
    _, t = best(lambda: dev.var_grad(ctx, ksp, Lv, Xv, Zv), reps=2)
    report("gpx_var_grad", "GP.evaluateVarianceDerivative (gp.py:282-341)", dict(N=Nv, M=Mv, d=d, kernel=kname), t, flops=2.0 * (d + 1) * Nv * Nv * Mv,
           nbytes=8.0 * Nv * d * Mv,
           note="the (N d) x M result goes to the HOST by contract (that is what the reference returns): %.2f GB over PCIe dominate; "
                "one N x N matrix dK_l is refilled per coordinate (not d of them)" % (8.0 * Nv * d * Mv / 1e9))
    del L, Lv
# ---- a13-a15 / 8c: design kernels at C3 / C5 sizes
for kname in (kernels if want("design") else []):
    ksp = kernel_choice(kname)[0]
    N3, M3, nmc = (4096, 16384, 1024) if quick else (16384, 65536, 4096)
    rng = np.random.default_rng(16384)
    X3h, C3h, Z3h = rng.uniform(-1, 1, (N3, d)), rng.uniform(-1, 1, (M3, d)), rng.uniform(-1, 1, (nmc, d))
    X3, C3, Z3 = dev.points(ctx, X3h), dev.points(ctx, C3h), dev.points(ctx, Z3h)
    K3 = dev.potrf(ctx, dev.kfill(ctx, ksp, X3, nugget=0.1))
    _, t = best(lambda: dev.greedy_ivar_step(ctx, ksp, K3, X3, C3, Z3, 0.1))
    report("gpx_greedy_ivar_step", "costFunctionGP_IVAR.evaluate per candidate (experimentalDesign.py:79-117; SURVEY 8c composition)",
           dict(N=N3, candidates=M3, nMC=nmc, d=d, kernel=kname), t, flops=2.0 * nmc * M3 * N3 + 1.0 * N3 * N3 * (M3 + nmc),
           note="rank-one scoring of every candidate: two N x (M + nMC) triangular solves + the nMC x M x N product")
    _, t = best(lambda: dev.greedy_var(ctx, ksp, C3, 16))
    report("gpx_greedy_var", "performGreedyVarExperimentalDesign (experimentalDesign.py:787-845)", dict(candidates=M3, picks=16, d=d, kernel=kname), t,
           nbytes=8.0 * M3 * 16 * 16 / 2 + 8.0 * M3 * d * 16, note="incremental Cholesky rows; latency-bound (one launch chain per pick)")
    del K3
if want("mi"):
    d5 = 10
    sp5 = dev.KernelSpec(dev.K_SE, d5, list(0.5 + 0.03 * np.arange(d5)) + [1.0])
    Mm = 2048 if quick else 8192
    Cm = dev.points(ctx, rng.uniform(-1, 1, (Mm, d5)))
    _, t = best(lambda: dev.mi_greedy(ctx, sp5, Cm, 0.1, 8, 0))
    report("gpx_mi_greedy", "costFunctionGP_MI + performGreedyMIExperimentalDesign (experimentalDesign.py:223-285, 753-785)",
           dict(candidates=Mm, picks=8, d=d5), t, flops=Mm ** 3 / 3.0 + 2.0 * Mm ** 3 / 3.0,
           note="SURVEY 8d count: potrf M^3/3 + potri 2 M^3/3 = M^3 (round 4 charged a dense M^3 product on top that the code no "
                "longer executes); then 7 rank-one down-dates (HBM: 16 M^2 bytes each)")
# ---- f4: FITC
if want("fitc"):
    Nf = 8192 if quick else 32768
    nu = Nf // 8
    Xf = rng.uniform(-1, 1, (Nf, d))
    yf = np.sin(2 * np.pi * Xf.sum(1) / d) + np.sqrt(0.1) * rng.standard_normal(Nf)
    Xfd, Sd = dev.points(ctx, Xf), dev.points(ctx, Xf[rng.permutation(Nf)[:nu]].copy())
    m, t = best(lambda: dev.FitcModel(ctx, sp, Xfd, Sd, 0.1), reps=2)
    report("gpx_fitc_fit", "FITC branch of addNodesAndComputeCovariance (gp.py:182-210; gp_kernel_utilities.py:70-104)",
           dict(N=Nf, nu=nu, d=d), t, flops=2.0 * nu ** 3 / 3.0 + 2.0 * Nf * nu * nu,
           note="chol(Quu), Kuf, G = diag(K - Q), chol(Quu + Kuf G^-1 Kfu): two nu-order factorisations + two nu x nu x N products")
    _, t = best(lambda: m.solve(yf))
    report("gpx_fitc_solve", "GP.train with the Woodbury precision (gp.py:100-101)", dict(N=Nf, nu=nu), t, nbytes=2.0 * 8.0 * Nf * nu)
    m.lml_grad(sp, yf)                                     # warm: pools, block inverses of Lu and La
    _, t = best(lambda: m.lml_grad(sp, yf))
    report("gpx_fitc_lml_grad", "none in the reference (its FITC gradient is unrunnable); before: nparams + 1 = %d calls of "
           "gpx_fitc_fit per optimiser iterate" % (d + 3), dict(N=Nf, nu=nu, d=d, kernel="ARD-SE", nlen=d), t,
           flops=8.0 * Nf * nu * nu + 1.0 * nu ** 3,
           note="B = Quu^-1 Kuf and Y = La^-1 Ks (nu^2 N each, a triangular solve counted as in SURVEY 8d), B Ks^T, its product with "
                "Y and T = R B^T (2 nu^2 N each), one nu-order right solve; then the tiled derivative sums over R (nu x N) and T")
    m.lml_grad(sp, yf, want_inducing=True)                 # warm: the partial sums and the nu x d result
    _, t2 = best(lambda: m.lml_grad(sp, yf, want_inducing=True))
    report("gpx_fitc_lml_grad_inducing", "none in the reference (its inducing points are a frozen random subset)",
           dict(N=Nf, nu=nu, d=d, kernel="ARD-SE", nlen=d), t2, flops=8.0 * Nf * nu * nu + 1.0 * nu ** 3,
           note="gpx_fitc_lml_grad plus dL/dS (nu x d): one more row-wise weighted pass over the nu x N and nu x nu pairs and the sum "
                "of its per-segment partials; the products are those of gpx_fitc_lml_grad, so the rate is on the same count; "
                "ratio to gpx_fitc_lml_grad in this run: %.3f" % (t2 / t))
    m.loo(yf)                                              # warm: pools
    _, tl = best(lambda: m.loo(yf))
    flines = [report("gpx_fitc_loo", "N refits through GP.train (the reference has no leave-one-out call)", dict(N=Nf, nu=nu, d=d), tl,
                     flops=1.0 * Nf * nu * nu,
                     note="leave-one-out under the model's own covariance Q + G: Y = La^-1 Ks (nu^2 N), its column sums of squares, "
                          "alpha; ratio to gpx_fitc_lml_grad in this run: %.3f" % (tl / t))]
    m.loo_grad(sp, yf)                                     # warm: pools
    _, tlg = best(lambda: m.loo_grad(sp, yf))
    flines.append(report("gpx_fitc_loo_grad", "none in the reference", dict(N=Nf, nu=nu, d=d, kernel="ARD-SE", nlen=d), tlg,
                         flops=16.0 * Nf * nu * nu + 2.0 * nu ** 3,
                         note="the two solves of gpx_fitc_lml_grad (nu^2 N each) and seven nu x nu x N products (H = Y C Y^T, H Y, "
                              "B Y^T, the scaled B Y^T, C2 Y, C1 Y diag(c ginv), T = R B^T; 2 nu^2 N each), one nu^3 product; then "
                              "the tiled derivative sums over R and T; gpx_fitc_lml_grad in this run: %.2f ms, ratio %.3f"
                              % (1e3 * t, tlg / t)))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            for line in flines:
                f.write(json.dumps(line) + "\n")
    # VFE on the same shape and inducing points (gpx_vfe_*; appended to profiles/vfe_frows.jsonl).  The FITC calls it is compared
    # with are timed again here, interleaved, five repetitions each: (min, max) of both sides go into the note.
    def spread(f, reps=5):
        ts = []
        for _ in range(reps):
            ts.append(best(f, reps=1)[1])
        return min(ts), max(ts)

    mv, tvf = best(lambda: dev.VfeModel(ctx, sp, Xfd, Sd, 0.1), reps=2)
    _, tff = best(lambda: dev.FitcModel(ctx, sp, Xfd, Sd, 0.1), reps=2)
    vlines = [report("gpx_vfe_fit", "none in the reference (FITC is its only sparse model)", dict(N=Nf, nu=nu, d=d), tvf,
                     flops=2.0 * nu ** 3 / 3.0 + 2.0 * Nf * nu * nu,
                     note="gpx_fitc_fit with G = noise I and the residual trace sum_i (k_ii - Q_ii): the same two factorisations and "
                          "two nu x nu x N products; gpx_fitc_fit in this run: %.2f ms, ratio %.3f" % (1e3 * tff, tvf / tff))]
    mv.grad(sp, yf)                                        # warm: pools, block inverses of Lu and La
    (tg0, tg1), (tf0, tf1) = spread(lambda: mv.grad(sp, yf)), spread(lambda: m.lml_grad(sp, yf))
    vlines.append(report("gpx_vfe_grad", "none in the reference", dict(N=Nf, nu=nu, d=d, kernel="ARD-SE", nlen=d), tg0,
                         flops=8.0 * Nf * nu * nu + 1.0 * nu ** 3,
                         note="the two solves and three nu x nu x N products of gpx_fitc_lml_grad, R = (B alpha) alpha^T + (B Y^T) Y "
                              "by one fused rank-one pass (no diag(c) pass); five runs each: gpx_vfe_grad %.2f..%.2f ms, "
                              "gpx_fitc_lml_grad %.2f..%.2f ms, ratio of the minima %.3f"
                              % (1e3 * tg0, 1e3 * tg1, 1e3 * tf0, 1e3 * tf1, tg0 / tf0)))
    mv.grad(sp, yf, want_inducing=True)
    (ts0, ts1), (tfs0, tfs1) = (spread(lambda: mv.grad(sp, yf, want_inducing=True)),
                                spread(lambda: m.lml_grad(sp, yf, want_inducing=True)))
    vlines.append(report("gpx_vfe_grad (with dF/dS)", "none in the reference", dict(N=Nf, nu=nu, d=d, kernel="ARD-SE", nlen=d), ts0,
                         flops=8.0 * Nf * nu * nu + 1.0 * nu ** 3,
                         note="gpx_vfe_grad plus dF/dS (nu x d): the row-wise weighted pass of gpx_fitc_lml_grad_inducing; five runs "
                              "each: %.2f..%.2f ms, gpx_fitc_lml_grad_inducing %.2f..%.2f ms, ratio of the minima %.3f; ratio to "
                              "gpx_vfe_grad %.3f" % (1e3 * ts0, 1e3 * ts1, 1e3 * tfs0, 1e3 * tfs1, ts0 / tfs0, ts0 / tg0)))
    Mz = 4096 if quick else 16384
    Zd = dev.points(ctx, rng.uniform(-1, 1, (Mz, d)))
    cv, cf_ = mv.solve(yf)[0], m.solve(yf)[0]
    mv.posterior(cv, Zd); m.posterior(cf_, Zd)             # warm: pools
    (tp0, tp1), (tq0, tq1) = spread(lambda: mv.posterior(cv, Zd)), spread(lambda: m.posterior(cf_, Zd))
    fv, ff = 2.0 * nu * nu * Mz, 2.0 * nu * Nf * Mz + 1.0 * nu * nu * Mz
    vlines.append(report("gpx_vfe_posterior", "none in the reference", dict(N=Nf, nu=nu, M=Mz, d=d), tp0, flops=fv,
                         note="mean and variance: two nu x M fills, two left solves of order nu (nu^2 M each), two column sums of "
                              "squares, one weighted column sum; five runs: %.2f..%.2f ms.  gpx_fitc_posterior at the same M in this "
                              "run (one M x N fill, the M x nu x N product 2 nu N M, one right solve nu^2 M = %.3e flop): "
                              "%.2f..%.2f ms, %.1f TF/s; ratio of the minima %.4f (roofline count ratio %.4f)"
                              % (1e3 * tp0, 1e3 * tp1, ff, 1e3 * tq0, 1e3 * tq1, ff / tq0 / 1e12, tp0 / tq0, fv / ff)))
    # Bayesian-optimisation costs on the VFE model (gpx_vfe_acq / gpx_vfe_acq_grad / gpx_vfe_acq_batch) against what a user had
    # before them, timed in this run, ALTERNATING, five runs each: for the values and the arg-min the predictor, the host costs
    # (scipy.stats, as costFuncEI.evaluate forms them) and firstMinIndex; for the batch q refits on the grown data with the same
    # inducing points, each scored that way.  The gradient had no counterpart.
    import scipy.stats as spstats
    from gpexp_amd.experimentalDesign import firstMinIndex

    def alternate(f, g, reps=5):
        tf, tg = [], []
        for _ in range(reps):
            tf.append(best(f, reps=1)[1])
            tg.append(best(g, reps=1)[1])
        return (min(tf), max(tf)), (min(tg), max(tg))

    def host_ei(model, coeff, fbest, pts):
        mean, var = model.posterior(coeff, pts)
        s = np.sqrt(np.abs(var))
        g = (fbest - mean) / s
        costs = -s * (g * spstats.norm.cdf(g) + spstats.norm.pdf(g))
        return firstMinIndex(costs), costs

    fb, qb = float(np.max(yf)), 8
    mv.acq(cv, Zd, dev.ACQ_EI, fb); mv.acq_grad(cv, Zd, dev.ACQ_EI, fb)    # warm: pools
    (ta0, ta1), (th0, th1) = alternate(lambda: mv.acq(cv, Zd, dev.ACQ_EI, fb), lambda: host_ei(mv, cv, fb, Zd))
    vlines.append(report("gpx_vfe_acq", "gpx_vfe_posterior + the costs on the host (scipy.stats) + firstMinIndex",
                         dict(N=Nf, nu=nu, M=Mz, d=d, acq="EI"), ta0, flops=fv,
                         note="gpx_vfe_posterior's per-chunk step, then the cost epilogue and the arg-min on the device: M costs and "
                              "the winner reach the host instead of mean and variance; five runs each, alternating: %.2f..%.2f ms, "
                              "the predictor + host costs + firstMinIndex %.2f..%.2f ms, ratio of the minima %.3f"
                              % (1e3 * ta0, 1e3 * ta1, 1e3 * th0, 1e3 * th1, ta0 / th0)))
    tg0_, tg1_ = spread(lambda: mv.acq_grad(cv, Zd, dev.ACQ_EI, fb))
    vlines.append(report("gpx_vfe_acq_grad", "none (no gradient of a cost on a VFE model before)", dict(N=Nf, nu=nu, M=Mz, d=d, acq="EI"),
                         tg0_, flops=2.0 * fv,
                         note="the values, then both forward solves transposed and swept backward (nu^2 M each) and one fused pass "
                              "over the nu inducing points per candidate; five runs: %.2f..%.2f ms; ratio to gpx_vfe_acq in this "
                              "run %.3f" % (1e3 * tg0_, 1e3 * tg1_, tg0_ / ta0)))
    Zhost = rng.uniform(-1, 1, (Mz, d))
    Zb = dev.points(ctx, Zhost)

    def refit_batch():
        Xa, ya, picks = Xf, yf, []
        for t in range(qb):
            model = mv if t == 0 else dev.VfeModel(ctx, sp, dev.points(ctx, Xa), Sd, 0.1)
            coeff = cv if t == 0 else model.solve(ya)[0]
            mean, var = model.posterior(coeff, Zb)
            s = np.sqrt(np.abs(var))
            g = (max(fb, float(np.max(ya))) - mean) / s
            costs = -s * (g * spstats.norm.cdf(g) + spstats.norm.pdf(g))
            costs[picks] = np.nan
            j = firstMinIndex(costs)
            picks.append(j)
            Xa, ya = np.vstack((Xa, Zhost[j:j + 1])), np.append(ya, mean[j])
        return picks

    mv.acq_batch(cv, Zb, dev.ACQ_EI, fb, True, dev.LIE_BELIEVER, 0.0, qb)       # warm: pools
    picks_dev = mv.acq_batch(cv, Zb, dev.ACQ_EI, fb, True, dev.LIE_BELIEVER, 0.0, qb)[0].tolist()
    picks_ref = refit_batch()
    (tb0, tb1), (tr0, tr1) = alternate(lambda: mv.acq_batch(cv, Zb, dev.ACQ_EI, fb, True, dev.LIE_BELIEVER, 0.0, qb), refit_batch)
    vlines.append(report("gpx_vfe_acq_batch", "q refits with the same inducing points (gpx_vfe_fit + gpx_fitc_solve + gpx_vfe_posterior "
                         "+ host costs per pick)", dict(N=Nf, nu=nu, M=Mz, q=qb, d=d, acq="EI", lie="believer"), tb0,
                         flops=fv,
                         note="set-up as gpx_vfe_acq with Wa = La^-1 K(S, C) kept (2 nu^2 M flop: the count the rate is on), then per pick "
                              "ONE pass over Wa (8 nu M bytes, the weighted column reduction); five runs each, alternating: %.2f..%.2f ms, the refit "
                              "loop %.2f..%.2f ms, ratio of the minima %.4f; picks equal to the refit loop's: %s"
                              % (1e3 * tb0, 1e3 * tb1, 1e3 * tr0, 1e3 * tr1, tb0 / tr0, picks_dev == picks_ref)))
    del mv
    out_vfe =os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vfe_frows.jsonl")
    if "--vfe-out" in sys.argv:
        out_vfe = sys.argv[sys.argv.index("--vfe-out") + 1]
    with open(out_vfe, "a") as f:
        for line in vlines:
            f.write(json.dumps(line) + "\n")
# ---- f2: refit of the changed rows
if want("refit"):
    Nr = 4096 if quick else 16384
    Xr = rng.uniform(-1, 1, (Nr, d))
    Xrd = dev.points(ctx, Xr)
    Lr = dev.potrf(ctx, dev.kfill(ctx, sp, Xrd, nugget=0.1))
    keep = Nr - 512
    Xr2 = Xr.copy()
    Xr2[keep:] = rng.uniform(-1, 1, (Nr - keep, d))
    Xr2d = dev.points(ctx, Xr2)
    _, t = best(lambda: dev.refit_rows(ctx, sp, Xr2d, 0.1, Lr, keep))
    report("gpx_refit_rows", "ExperimentalDesignGreedyWithDerivatives batch loop (experimentalDesign.py:694-751)",
           dict(N=Nr, changed_rows=Nr - keep), t, flops=1.0 * (Nr - keep) * Nr * Nr,
           note="the leading %d rows of the factor are reused; only the last %d rows are re-assembled and re-solved" % (keep, Nr - keep))
# ---- f3: the hyper-parameter loop (findOptParamsLogLike / chooseParams, gp.py:498-639)
if want("f3"):
    from gpExp.kernels import KernelSquaredExponential, KernelIsoMatern
    from gpExp.gp import GP

    def f3_case(label, kern, N3, d3, maxiter):
        r3 = np.random.default_rng(N3)
        Xo = r3.uniform(-1, 1, (N3, d3))
        yo = np.sin(2 * np.pi * Xo.sum(1) / d3) + np.sqrt(0.1) * r3.standard_normal(N3)
        out = {}
        for analytic in (False, True):
            g = GP(kern(), 0.1)
            counts = dict(fits=0, grads=0)
            inner = g.loglikeParams

            def counted(pts, evals, returnDeriv=0, noiseIn=None):
                counts["fits"] += 1
                counts["grads"] += int(returnDeriv == 1)
                return inner(pts, evals, returnDeriv=returnDeriv, noiseIn=noiseIn)

            g.loglikeParams = counted
            g.loglikeParams(Xo, yo)                        # warm: pools, kernel attributes
            counts.update(fits=0, grads=0)
            ctx.sync()
            t0 = time.perf_counter()
            params, opt = g.findOptParamsLogLike(Xo, yo, maxiter=maxiter, analyticGradient=analytic)
            ctx.sync()
            out[analytic] = (time.perf_counter() - t0, dict(counts), float(opt))
        (tn, cn, on), (ta, ca, oa) = out[False], out[True]
        nhyp = len(kern().hyperParam) + 1
        # an L-BFGS-B iterate with numerical gradients = 1 + nhyp likelihood evaluations (approx_grad: forward differences)
        report("findOptParamsLogLike (%s)" % label, "GP.findOptParamsLogLike / chooseParams (gp.py:498-639)",
               dict(N=N3, d=d3, hyper_parameters=nhyp, maxfun=maxiter), ta / max(ca["grads"], 1),
               flops=N3 ** 3 / 3.0 + 2.0 * N3 ** 3 / 3.0,
               note="ms per likelihood + gradient evaluation with analyticGradient=True (one factorisation N^3/3 + the trace "
                    "through L^-1, 2 N^3/3): %d evaluations in %.2f s, optimum %.6g; numerical gradients as in the reference "
                    "(maxfun = %d likelihood evaluations = %d factorisations, about %d per L-BFGS iterate): %.2f s, %.1f ms per "
                    "factorisation, optimum %.6g" % (ca["grads"], ta, -oa, maxiter, cn["fits"], nhyp + 1, tn, 1e3 * tn / max(cn["fits"], 1), -on))

    if quick:
        f3_case("C2-lite: N=1024 d=3 iso-SE", lambda: KernelSquaredExponential([0.5], 1.0, 3), 1024, 3, 20)
    else:
        f3_case("C2: N=4096 d=3 iso-SE", lambda: KernelSquaredExponential([0.5], 1.0, 3), 4096, 3, 40)
        f3_case("N=16384 d=8 Matern-5/2", lambda: KernelIsoMatern(0.7, 1.0, 8, nu=2.5), 16384, 8, 24)
        f3_case("N=16384 d=8 ARD-SE", lambda: KernelSquaredExponential(list(0.5 + 0.05 * np.arange(8)), 1.0, 8), 16384, 8, 24)
# ---- acq: Bayesian-optimisation costs (costFuncGPUCbound / costFuncPI / costFuncEI, experimentalDesign.py:889-1003)
if want("acq"):
    from gpExp.kernels import KernelIsoMatern
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI
    import scipy.stats as spstats

    class _Space(object):
        dimension = 8

    Na, Ma = (2048, 16384) if quick else (8192, 131072)
    ra = np.random.default_rng(Na)
    Xa = ra.uniform(-1, 1, (Na, 8))
    ya = np.sin(3.0 * Xa[:, 0]) + 0.5 * np.cos(2.0 * Xa.sum(1)) + 0.05 * ra.standard_normal(Na)
    Za = ra.uniform(-1, 1, (Ma, 8))
    cf = costFuncEI(GP(KernelIsoMatern(1.5, 1.0, 8, nu=2.5), 1e-2), Xa, ya, 2, _Space())
    size = dict(N=Na, d=8, M=Ma, kernel="Matern-5/2", acq="EI")

    def values():
        return cf.evaluateBatch(Za), cf.bestCandidate(Za)

    values()
    _, t = best(values)
    report("gpx_acq (evaluateBatch + bestCandidate)", "costFuncEI.evaluate, one point per call (experimentalDesign.py:962-1003)",
           size, t, flops=2.0 * Na * Na * Ma,
           note="two passes (costs to the host, then the arg-min alone); each one is N^2 M (the forward solve)")
    _, t1 = best(lambda: cf.bestCandidate(Za))
    report("gpx_acq (bestCandidate only)", "costFuncEI.evaluate", size, t1, flops=1.0 * Na * Na * Ma)
    # max-value entropy search on the same model and candidates, K = 16 sampled optima below min y, beside the EI call above
    import copy
    from gpExp.experimentalDesign import costFuncMES
    cfm = costFuncMES(cf.gaussianProcess, Xa, ya, 2, _Space(), yStar=float(np.min(ya)) - 0.05 * np.arange(16))
    cfm.bestCandidate(Za)
    cfm1 = copy.copy(cfm)                   # the same model with K = 1: the difference is 15 more samples in the epilogue alone
    cfm1.yStar = cfm.yStar[:1]
    ts_ei, ts_mes, ts_mes1 = [], [], []
    for _ in range(3):                      # alternated, so that all see the same clocks
        ts_ei.append(best(lambda: cf.bestCandidate(Za), reps=1)[1])
        ts_mes.append(best(lambda: cfm.bestCandidate(Za), reps=1)[1])
        ts_mes1.append(best(lambda: cfm1.bestCandidate(Za), reps=1)[1])
    report("gpx_acq_mes (bestCandidate only, K = 16)", "none in the reference (no entropy search there)", dict(size, acq="MES", K=16),
           min(ts_mes), flops=1.0 * Na * Na * Ma,
           note="the posterior pass of gpx_acq with the MES epilogue (per candidate K short loops: a 73-term continued fraction "
                "below gamma = -2 sqrt 2, else erfc / exp / log); ratio to gpx_acq (EI) alternated in this process: %.3f "
                "(EI %.2f ms; K = 1: %.2f ms, so the 15 further samples of the epilogue cost %.3f ms over M candidates)"
                % (min(ts_mes) / min(ts_ei), 1e3 * min(ts_ei), 1e3 * min(ts_mes1), 1e3 * (min(ts_mes) - min(ts_mes1))))
    _, t = best(lambda: cf.derivativeBatch(Za))
    report("gpx_acq_grad (derivativeBatch)", "none in the reference (BO costs have no gradient there)", size, t,
           flops=2.0 * Na * Na * Ma + 6.0 * Na * Ma * 8,
           note="forward + backward solve 2 N^2 M, fused pass over the training points O(N M d)")
    gpa = cf.gaussianProcess
    fb = float(np.max(ya))

    def composition():
        mu, var = gpa.evaluate(Za, compvar=1)
        s = np.sqrt(var)
        g = (fb - mu) / s
        c = -s * (g * spstats.norm.cdf(g) + spstats.norm.pdf(g))
        return int(np.argmin(c))

    _, t = best(composition)
    report("composition GP.evaluate(compvar=1) + NumPy", "what a user writes today on this library", size, t,
           flops=1.0 * Na * Na * Ma)
    # q-point batch selection (selectBatch -> gpx_acq_batch) against the refit loop it replaces, half of Za, 16 picks
    Mb, qb = Ma // 2, 16
    Zb = Za[:Mb]
    sizeb = dict(N=Na, d=8, M=Mb, q=qb, kernel="Matern-5/2", acq="EI", lie="believer")
    cf.selectBatch(Zb, 2)
    _, t_one = best(lambda: cf.selectBatch(Zb, 1))
    _, t_all = best(lambda: cf.selectBatch(Zb, qb))
    _, t_bc = best(lambda: cf.bestCandidate(Zb))
    t_pick = (t_all - t_one) / (qb - 1)
    report("gpx_acq_batch set-up (selectBatch, 1 pick)", "costFuncEI(...) + bestCandidate, the first pass of the loop", sizeb, t_one,
           flops=1.0 * Na * Na * Mb, note="the posterior pass of gpx_acq with W_C = L^-1 K(X, C) kept; bestCandidate alone on the same "
           "candidates: %.2f ms; %d picks in one call: %.2f ms" % (1e3 * t_bc, qb, 1e3 * t_all))
    report("gpx_acq_batch per pick", "refit on the grown data + bestCandidate per pick", sizeb, t_pick, nbytes=8.0 * Na * Mb,
           note="(time of %d picks - time of 1 pick) / %d: one weighted column reduction over W_C + one fused pass over the "
                "candidates per pick" % (qb, qb - 1))

    def refit_loop(picks):
        Xt, yt, out = Xa, ya, []
        for _ in range(picks):
            c = costFuncEI(GP(KernelIsoMatern(1.5, 1.0, 8, nu=2.5), 1e-2), Xt, yt, 2, _Space())
            j, _ = c.bestCandidate(Zb)                      # (masking the earlier picks is host index work: left out of the timing)
            mu = c.gaussianProcess.evaluate(Zb[j:j + 1])
            Xt, yt = np.vstack((Xt, Zb[j:j + 1])), np.append(yt, mu)
            out.append(j)
        return out

    _, t = best(lambda: refit_loop(2))
    report("refit loop per pick (costFuncEI + bestCandidate)", "what a user writes today for a batch", sizeb, t / 2,
           flops=1.0 * Na * Na * Mb + Na ** 3 / 3.0,
           note="2 picks timed, per pick: one factorisation + the forward solve over all candidates; gpx_acq_batch per pick is "
                "%.1f x below it" % (t / 2 / t_pick))

# ---- loo: leave-one-out cross-validation and its hyper-parameter gradient (gpx_loo / gpx_loo_grad; none in the reference)
if want("loo"):
    from gpExp.kernels import KernelSquaredExponential, KernelIsoMatern
    Nl = 4096 if quick else 16384
    rl = np.random.default_rng(Nl)
    Xl = rl.uniform(-1, 1, (Nl, 8))
    yl = np.sin(3.0 * Xl[:, 0]) + 0.5 * np.cos(2.0 * Xl.sum(1)) + 0.1 * rl.standard_normal(Nl)
    Xd = dev.points(ctx, Xl)
    lines = []
    for kname, kern in (("Matern-5/2", KernelIsoMatern(1.5, 1.0, 8, nu=2.5)),
                        ("ARD-SE", KernelSquaredExponential(list(0.5 + 0.05 * np.arange(8)), 1.0, 8))):
        ksp = kern._spec()
        size = dict(N=Nl, d=8, kernel=kname, nlen=ksp.nlen)
        Ll = dev.potrf(ctx, dev.kfill(ctx, ksp, Xd, nugget=0.01))
        dev.loo(ctx, Ll, yl)
        _, t = best(lambda: dev.loo(ctx, Ll, yl))
        lines.append(report("gpx_loo", "N refits through GP.train (the reference has no leave-one-out call)", size, t,
                            flops=Nl ** 3 / 3.0, note="L^-1 by the halving recursion + column sums of squares + potrs"))
        dev.loo_grad(ctx, ksp, Ll, Xd, 0.01, yl)
        _, tg = best(lambda: dev.loo_grad(ctx, ksp, Ll, Xd, 0.01, yl))
        # what the gradient is composed of, through entry points that predate it: one inverse + nlen square NN products
        _, tp = best(lambda: dev.potri(ctx, Ll).free())
        A, B, Cm = (dev.DeviceMatrix.zeros(ctx, Nl, Nl) for _ in range(3))
        dev.dbg_gemm(ctx, A, B, Cm, False, False)
        _, tm = best(lambda: dev.dbg_gemm(ctx, A, B, Cm, False, False))
        for m in (A, B, Cm):
            m.free()
        base = tp + ksp.nlen * tm
        lines.append(report("gpx_loo_grad", "none in the reference", size, tg, flops=2.0 * Nl ** 3 / 3.0 + 2.0 * ksp.nlen * Nl ** 3,
                            note="composition baseline in this process: potri %.2f ms + %d x NN product %.2f ms = %.2f ms; gpx_loo_grad / "
                                 "baseline = %.3f" % (1e3 * tp, ksp.nlen, 1e3 * tm, 1e3 * base, tg / base)))
        Ll.free()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

# ---- vfedesign: IVAR design on a VFE model in the inducing space (gpx_vfe_design_*; none in the reference).  The cost is compared
# with the path that existed before it -- gpx_vfe_fit on the N design points, then gpx_vfe_posterior's variances at the M MC points and
# a host mean: what costFunctionGP_IVAR.evaluate does on a VFE model -- at the same shapes in this run, ALTERNATING, seven samples of
# ten calls each (min..max per call).  The gradient had no predecessor: its time stands against the flop model.
# --vfedesign-out: where the lines go (default profiles/vfe_design_frows.json).
if want("vfedesign"):
    from gpExp.kernels import KernelIsoMatern
    nuv, Mv, Nv, pinv = (512, 8192, 1024, 960) if quick else (1024, 32768, 4096, 4032)
    dv, bv = 8, Nv - pinv
    rv = np.random.default_rng(1024)
    kspv = KernelIsoMatern(1.5, 1.0, dv, nu=2.5)._spec()
    Xv, Zv = rv.uniform(-1, 1, (Nv, dv)), rv.uniform(-1, 1, (Mv, dv))
    Sv = Xv[rv.permutation(Nv)[:nuv]].copy()
    Xd, Sd, Zd = dev.points(ctx, Xv), dev.points(ctx, Sv), dev.points(ctx, Zv)
    Xpd, Xfd_ = dev.points(ctx, Xv[:pinv]), dev.points(ctx, Xv[pinv:])

    def per_call(f, calls=10):
        def run():
            for _ in range(calls):
                out = f()
            return out
        return run

    def samples(f, g=None, reps=7, calls=10):
        """(min, max) seconds per call of f (and of g, alternating with it)."""
        tf, tg = [], []
        for _ in range(reps):
            tf.append(best(per_call(f, calls), reps=1)[1] / calls)
            if g is not None:
                tg.append(best(per_call(g, calls), reps=1)[1] / calls)
        return ((min(tf), max(tf)), (min(tg), max(tg))) if g is not None else (min(tf), max(tf))

    def old_cost():
        return float(np.mean(dev.VfeModel(ctx, kspv, Xd, Sd, 0.05).posterior(None, Zd, want_mean=False)[1]))

    size = dict(nu=nuv, M=Mv, N=Nv, d=dv, kernel="Matern-5/2")
    dev.VfeDesign(ctx, kspv, Sd, 0.05, Zd)                    # warm: pools, code objects
    c0, c1 = samples(lambda: dev.VfeDesign(ctx, kspv, Sd, 0.05, Zd), calls=3)
    ds = dev.VfeDesign(ctx, kspv, Sd, 0.05, Zd)
    vd = [report("gpx_vfe_design_create", "none in the reference", size, c0, flops=2.0 * nuv * nuv * Mv + 7.0 * nuv ** 3 / 3.0,
                 note="chol(Quu), Gz by SYRK over the chunks of Z (2 nu^2 M), the two-sided solve for c0; %.2f..%.2f ms" % (1e3 * c0, 1e3 * c1))]
    model = nuv ** 3 * (1.0 / 3.0 + 2.0)
    old_model = 2.0 * nuv * nuv * Nv + nuv ** 3 / 3.0 + 2.0 * nuv * nuv * Mv
    for label, pinned, Xe, b in (("all %d free" % Nv, None, Xd, Nv), ("%d pinned + %d free" % (pinv, bv), Xpd, Xfd_, bv)):
        ds.pin(pinned)
        new, old = ds.eval(Xe, want_grad=False)[0], old_cost()            # warm both sides, and the values agree
        assert abs(new - old) <= 1e-8, (new, old)
        (n0, n1), (o0, o1) = samples(lambda: ds.eval(Xe, want_grad=False), old_cost)
        vd.append(report("gpx_vfe_design_eval (cost, %s)" % label, "gpx_vfe_fit + gpx_vfe_posterior + host mean", dict(size, b=b), n0,
                         flops=model + 2.0 * nuv * nuv * b,
                         note="alternating with the earlier path, seven samples of ten calls: new %.3f..%.3f ms, earlier %.3f..%.3f ms, "
                              "ratio earlier / new of the minima %.2f (flop model %.3e against %.3e: %.2f); |difference of the "
                              "values| %.1e" % (1e3 * n0, 1e3 * n1, 1e3 * o0, 1e3 * o1, o0 / n0, model + 2.0 * nuv * nuv * b,
                                                old_model, old_model / (model + 2.0 * nuv * nuv * b), abs(new - old))))
        ds.eval(Xe)
        g0, g1 = samples(lambda: ds.eval(Xe))
        rows = (6.0 * dv + 25.0) * b * nuv
        vd.append(report("gpx_vfe_design_eval (cost + gradient, %s)" % label, "none in the reference", dict(size, b=b), g0,
                         flops=model + 8.0 * nuv * nuv * b + rows,
                         note="nu^3/3 + 2 nu^3 + 2 nu^2 b for the cost, 6 nu^2 b + the row pass's (6 d + 25) b nu = %.3e more; seven samples "
                              "of ten calls: %.3f..%.3f ms; over the cost alone in this run: %.2f x" % (rows, 1e3 * g0, 1e3 * g1, g0 / n0)))
    p0, p1 = samples(lambda: ds.pin(Xpd))
    vd.append(report("gpx_vfe_design_pin", "none in the reference", dict(size, pinned=pinv), p0, flops=2.0 * nuv * nuv * pinv,
                     note="once per batch: %.3f..%.3f ms" % (1e3 * p0, 1e3 * p1)))
    path = sys.argv[sys.argv.index("--vfedesign-out") + 1] if "--vfedesign-out" in sys.argv else \
        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vfe_design_frows.json")
    with open(path, "w") as f:
        json.dump(vd, f, indent=1)
        f.write("\n")


# ---- sample / qei: joint posterior draws and Monte-Carlo q-EI against what a user can do without them: gpx_posterior_cov to the
# host, NumPy Cholesky, a NumPy product.  The two sides ALTERNATE (device, host, device, ...) and every line carries min / median /
# max of its repetitions.
def alternate(dev_f, host_f, reps):
    td, th = [], []
    for _ in range(reps):
        for f, ts in ((dev_f, td), (host_f, th)):
            ctx.sync()
            t0 = time.perf_counter()
            f()
            ctx.sync()
            ts.append(time.perf_counter() - t0)
    return td, th


def spread(ts):
    return dict(ms_min=1e3 * min(ts), ms_median=1e3 * float(np.median(ts)), ms_max=1e3 * max(ts), reps=len(ts))


def sample_report(line):
    out = sys.argv[sys.argv.index("--sample-out") + 1] if "--sample-out" in sys.argv else \
        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sample_qei_frows.jsonl")
    print(json.dumps(line), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")


if want("sample") or want("qei") or want("vfeqei"):
    from gpExp.kernels import KernelIsoMatern
    from gpExp.gp import GP
    from gpExp.experimentalDesign import costFuncEI

    class _Space8(object):
        dimension = 8

    Ns = 2048 if quick else 8192
    rs = np.random.default_rng(Ns + 1)
    Xs = rs.uniform(-1, 1, (Ns, 8))
    ys = np.sin(3.0 * Xs[:, 0]) + 0.5 * np.cos(2.0 * Xs.sum(1)) + 0.05 * rs.standard_normal(Ns)
    cfs = costFuncEI(GP(KernelIsoMatern(1.5, 1.0, 8, nu=2.5), 1e-2), Xs, ys, 2, _Space8())
    gps = cfs.gaussianProcess
    reps = 3 if quick else 5

if want("sample"):
    Ms, Ss = (1024, 64) if quick else (4096, 256)
    Zs = rs.uniform(-1, 1, (Ms, 8))
    xis = rs.standard_normal((Ss, Ms))
    jit = 1e-10

    def dev_draw():
        return gps.samplePosterior(Zs, baseSamples=xis, jitter=jit)

    def host_draw():
        mean, cov = gps.evaluate(Zs, compvar=2)
        F = np.linalg.cholesky(cov + jit * np.eye(Ms))
        return mean[None, :] + xis @ F.T

    dev_draw(), host_draw()
    td, th = alternate(dev_draw, host_draw, reps)
    size = dict(N=Ns, d=8, M=Ms, S=Ss, kernel="Matern-5/2")
    sample_report(dict(entry="gpx_psampler (samplePosterior: create + draw + free)", size=size, **spread(td),
                       note="mean, C = K(Z,Z) - W^T W, chol(C + jitter I), F Xi^T on the MFMA path; S x M doubles come back"))
    sample_report(dict(entry="host path: evaluate(compvar=2) + numpy.linalg.cholesky + product", size=size, **spread(th),
                       note="what a user can do without the sampler: M x M doubles cross to the host; median ratio host / device "
                            "%.2f" % (float(np.median(th)) / float(np.median(td)))))

if want("qei"):
    Bq, qq, Sq = (512, 8, 256) if quick else (4096, 8, 256)
    Zq = rs.uniform(-1, 1, (Bq, qq, 8))
    xiq = rs.standard_normal((Sq, qq))
    fbq = float(np.max(ys))

    def dev_qei():
        return cfs.jointEI(Zq, baseSamples=xiq, jitter=1e-10)

    def host_qei(nb=None):
        out = []
        for b in range(Bq if nb is None else nb):
            mean, cov = gps.evaluate(Zq[b], compvar=2)
            F = np.linalg.cholesky(cov + 1e-10 * np.eye(qq))
            out.append(-np.mean(np.maximum(fbq - np.min(mean[None, :] + xiq @ F.T, axis=1), 0.0)))
        return np.array(out)

    nbh = 16                                    # the host loop is timed on 16 batches and scaled: one device call per batch
    dev_qei(), host_qei(2)
    td, th = alternate(dev_qei, lambda: host_qei(nbh), reps)
    size = dict(N=Ns, d=8, B=Bq, q=qq, S=Sq, kernel="Matern-5/2")
    sample_report(dict(entry="gpx_acq_qei (jointEI)", size=size, **spread(td),
                       note="posterior chunk over all B q points + one kernel: C_b, chol in LDS, S samples per batch"))
    sample_report(dict(entry="host path per batch: evaluate(compvar=2) + NumPy", size=dict(size, B=nbh), **spread(th),
                       note="%d batches timed, one gpx_posterior_cov call each; scaled to B = %d: %.1f ms (median)"
                            % (nbh, Bq, 1e3 * float(np.median(th)) * Bq / nbh)))

# ---- vfeqei: Monte-Carlo q-EI on a VFE model (gpx_vfe_acq_qei) beside the dense jointEI on the same data, batches and base samples,
# and beside the host route a user had before it: vfePosteriorCovariance per batch, NumPy Cholesky, the sample average
if want("vfeqei"):
    Bv, qv, Sv = (512, 8, 256) if quick else (4096, 8, 256)
    np.random.seed(7)                                   # the inducing points are drawn with np.random.permutation
    cfv = costFuncEI(GP(KernelIsoMatern(1.5, 1.0, 8, nu=2.5), 1e-2, FITC=0.125, sparse="vfe"), Xs, ys, 2, _Space8())
    gpv = cfv.gaussianProcess
    Zv8 = rs.uniform(-1, 1, (Bv, qv, 8))
    xiv = rs.standard_normal((Sv, qv))
    fbv = float(np.max(ys))

    def dev_vfeqei():
        return cfv.vfeJointEI(Zv8, baseSamples=xiv, jitter=1e-10)

    def dev_denseqei():
        return cfs.jointEI(Zv8, baseSamples=xiv, jitter=1e-10)

    def host_vfeqei(nb):
        out = []
        for b in range(nb):
            mean, cov = gpv.evaluate(Zv8[b]), gpv.vfePosteriorCovariance(Zv8[b])
            F = np.linalg.cholesky(cov + 1e-10 * np.eye(qv))
            out.append(-np.mean(np.maximum(fbv - np.min(mean[None, :] + xiv @ F.T, axis=1), 0.0)))
        return np.array(out)

    nbv = 16                                    # the host loop is timed on 16 batches and scaled: two device calls per batch
    cv, ch = dev_vfeqei(), host_vfeqei(2)
    dev_denseqei()
    tv, tdn = alternate(dev_vfeqei, dev_denseqei, reps)
    tv2, thv = alternate(dev_vfeqei, lambda: host_vfeqei(nbv), reps)
    size = dict(N=Ns, nu=int(gpv.fitcnodes.shape[0]), d=8, B=Bv, q=qv, S=Sv, kernel="Matern-5/2")
    sample_report(dict(entry="gpx_vfe_acq_qei (vfeJointEI)", size=size, **spread(tv + tv2),
                       note="vfe_posterior_chunk over all B q points + one kernel: the signed Gram (k - Wu^T Wu) + Wa^T Wa, chol in LDS, "
                            "S samples per batch; against the host route on the first two batches: max |difference| %.2e"
                            % float(np.max(np.abs(cv[:2] - ch)))))
    sample_report(dict(entry="gpx_acq_qei (jointEI), dense model on the same data, batches and base samples", size=dict(size, nu=None),
                       **spread(tdn), note="alternated with the line above"))
    sample_report(dict(entry="host path per batch: evaluate + vfePosteriorCovariance + NumPy", size=dict(size, B=nbv), **spread(thv),
                       note="%d batches timed, one gpx_vfe_posterior and one gpx_vfe_posterior_cov call each; scaled to B = %d: %.1f ms "
                            "(median)" % (nbv, Bv, 1e3 * float(np.median(thv)) * Bv / nbv)))
