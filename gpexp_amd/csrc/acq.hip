// Bayesian-optimisation acquisition costs -- gfx950.
//
// Replaces costFuncGPUCbound / costFuncPI / costFuncEI.evaluate (experimentalDesign.py:889-1003), which score ONE point per call
// (a single-row GP.evaluate(compvar=1) + scipy.stats), by a pass over M candidates: the posterior of every chunk of Z exactly as
// gpx_posterior forms it (api.hip, posterior_impl: B = K(X, Zc), mean = B^T alpha, W = L^-1 B, var = k(z, z) - colsum(W^2)), then
// one epilogue that turns (mean, var) into the cost and a per-block (cost, index) partial, and one small kernel that reduces the
// partials to the FIRST arg-min among the non-NaN costs.  With mu the mean, s = sqrt(|var|) (GP.evaluate's abs, gp.py:145),
// g = (fBest - mu) / s, Phi = 0.5 erfc(-g / sqrt 2), phi the normal density:
//     UCB  A = -(mu - kappa s)       PI  A = -Phi(g)       EI  A = -s (g Phi(g) + phi(g))
//
// Gradient w.r.t. the candidate (gpx_acq_grad).  With a = dA/dmu, b = dA/dvar (from the epilogue of the same chunk):
//     UCB  a = -1          b = kappa sgn(var) / (2 s)
//     PI   a = phi / s     b = phi g sgn(var) / (2 s^2)
//     EI   a = Phi         b = -phi sgn(var) / (2 s)
// and, k(z, z) being constant for the stationary kernels,
//     grad_z A = sum_j dk(z, x_j)/dz (a alpha_j - 2 b beta_j),   beta = K^-1 K(X, z) = L^-T W.
// The backward solve reuses the forward solve W of the values; the sum over j is one fused pass over the training points per
// candidate (acq_grad_kernel).  These are the TRUE derivatives of the values returned (not the reference's SE `derivative`, which
// multiplies by signalSize twice, kernels.py:177):
//     SE        dk/dz_l = -(z_l - x_l) / cl_l^2 k
//     Matern32  dk/dz   = -sig (3 / rho^2) e^-t (z - x)             t = sqrt(3) |z - x| / rho
//     Matern52  dk/dz   = -sig (5 / (3 rho^2)) (1 + t) e^-t (z - x)  t = sqrt(5) |z - x| / rho
// all smooth at z = x.  Where var == 0 exactly, a and b are NaN, and so is the gradient row.
// The same three calls on a VFE model (gpx_vfe_acq, gpx_vfe_acq_grad, gpx_vfe_acq_batch) are at the end of this file: the cost
// formula, the epilogue, the arg-min and -- as further instantiations -- the gradient, pick and batch kernels are these.  So is the
// host code around them: AcqOut is the result side of the candidate-wise calls (scratch, epilogue launch, arg-min, copies) and
// AcqBatchState + acq_batch_picks the pick loop of the q-batch calls; acq_impl / vfe_acq_impl and acq_batch_impl /
// vfe_acq_batch_impl hold what differs -- the posterior chunk with its transposes and backward solves, and the set-up that fills
// the resident W.  Every forward solve of a cross matrix goes through chol_cross_solve (chol.hip: the one in-place / out-of-place rule).
#include "gpx_device.h"
#include <math.h>

namespace {

constexpr int ACQ_EPI = 128;   // candidates per epilogue block = one arg-min partial; chunk starts are multiples of it

// arg-min partials: VI{cost, index} under argmin_merge (gpx_device.h) -- the first minimum among the non-NaN costs, i = -1: no
// non-NaN cost seen
// cost of one candidate from its posterior mean and SIGNED variance -- the one formula of gpx_acq's epilogue and of the batch
// selection's per-pick kernel.  a = dA/dmu, b = dA/dvar (NaN where var == 0 exactly).
__device__ __forceinline__ double acq_cost(int acq, double param, double mu, double var, double* a_out, double* b_out) {
  const double s = sqrt(fabs(var));
  const double sg = var > 0.0 ? 1.0 : (var < 0.0 ? -1.0 : 0.0);
  double c, a, b;
  if (acq == GPX_ACQ_VARIANCE) {   // the variance itself (gpx_vfe_var_grad_newpt): smooth through var == 0
    *a_out = 0.0;
    *b_out = 1.0;
    return var;
  }
  if (acq == GPX_ACQ_UCB) {
    c = -(mu - param * s);
    a = -1.0;
    b = param * sg / (2.0 * s);
  } else {
    const double g = (param - mu) / s;
    const double Phi = 0.5 * erfc(-g * M_SQRT1_2);
    const double phi = exp(-0.5 * g * g) * 0.39894228040143267794;   // 1 / sqrt(2 pi)
    if (acq == GPX_ACQ_PI) {
      c = -Phi;
      a = phi / s;
      b = phi * g * sg / (2.0 * s * s);
    } else {
      c = -s * (g * Phi + phi);
      a = Phi;
      b = -phi * sg / (2.0 * s);
    }
  }
  if (var == 0.0) a = b = __builtin_nan("");
  *a_out = a;
  *b_out = b;
  return c;
}

// ---- max-value entropy search (gpx_acq_mes; Wang & Jegelka 2017) -----------------------------------------------------------------
// K samples y*_k of the optimum VALUE (sign = +1: sampled minima, gamma_k = (mu - y*_k) / s; sign = -1: sampled maxima,
// gamma_k = (y*_k - mu) / s), lambda = phi / Phi:
//     h(gamma)  = gamma lambda / 2 - log Phi(gamma)            h'(gamma) = -(lambda / 2) (1 + gamma (gamma + lambda))
//     A = -(1/K) sum_k h(gamma_k)      a = dA/dmu = -(sign / (K s)) sum_k h'      b = dA/dvar = (sgn(var) / (2 K s^2)) sum_k h' gamma_k
// summed in the order k = 0 .. K-1.  Composed from erfc, exp and log, h loses the digits of two terms of size gamma^2 / 2 that
// cancel and h' those of 1 + gamma (gamma + lambda) -> 2 / gamma^2, and both are NaN below gamma = -38.5 where Phi underflows.
// With t = -gamma / sqrt 2 >= MES_T0 the continued fraction
//     1 / (sqrt(pi) erfcx(t)) = t + (1/2) / (t + 1 / (t + (3/2) / (t + ..)))  =  t + D,   D = (1/2) / (t + C2),
//     C2 = 1 / (t + (3/2) / (t + 2 / (t + ..)))
// gives lambda = sqrt 2 (t + D), h = -t D + log(2 sqrt(pi) (t + D)) with t D = (1 - w) / 2, and 1 + gamma (gamma + lambda) = w =
// C2 / (t + C2): nothing cancels, no exponential is taken, and |gamma| = 1e150 is served.  MES_CF_TERMS = the largest partial
// numerator index kept (k / 2, k = 3 .. MES_CF_TERMS below C2): the fewest for which the truncation of D and of C2 at t = MES_T0 is
// below u / 8 (tests/test_acq_mes_host.py pins both against mpmath).  Below MES_T0 (and for gamma > 0, through the upper tail Q
// and log1p(-Q)) the composition with an exactly formed gamma^2 / 2; its cancellation is bounded by that of gamma = -sqrt 2 MES_T0.
// (T0 = 3 would need 41 terms only, but the composition below it then loses 2 T0^2 times the library's error in h and gamma^4 / 2
// times in h': 2000 u in h' at gamma = -4 on the device.  DESIGN.md section 2, "Acquisition accuracy".)
// Beyond gamma = 40 phi and Q are zero in every double: h = h' = 0 (the formulas' own values, without inf * 0).
constexpr double MES_T0 = 2.0;
constexpr int MES_CF_TERMS = 73;

__device__ __forceinline__ void mes_h(double g, double* h_out, double* hp_out) {
  const double t = -g * M_SQRT1_2;
  double h, hp;
  if (t >= MES_T0) {
    double f = t;
    for (int k = MES_CF_TERMS; k >= 3; --k) f = t + (0.5 * k) / f;
    const double C2 = 1.0 / f, den = t + C2;
    const double w = C2 / den, td = t + 0.5 / den;
    h = log(3.54490770181103205460 * td) - 0.5 * (1.0 - w);   // 2 sqrt(pi)
    hp = -(M_SQRT1_2 * td) * w;
  } else if (g <= 40.0) {
    const double p = g * g, e = fma(g, g, -p);                 // gamma^2 = p + e exactly
    const double E = exp(-0.5 * p);
    const double phi = fma(-0.5 * e, E, E) * 0.39894228040143267794;   // 1 / sqrt(2 pi)
    const double Q = 0.5 * erfc(fabs(g) * M_SQRT1_2);          // the tail beyond |gamma|
    double lam;
    if (g <= 0.0) {
      lam = phi / Q;
      h = 0.5 * g * lam - log(Q);
    } else {
      lam = phi / (1.0 - Q);
      h = 0.5 * g * lam - log1p(-Q);
    }
    hp = -0.5 * lam * (1.0 + g * (g + lam));
  } else if (g > 40.0) {
    h = 0.0;
    hp = 0.0;
  } else {
    h = hp = __builtin_nan("");
  }
  *h_out = h;
  *hp_out = hp;
}

// the y* of a MES call on the device (K doubles), beside the scalar `param` of the three closed forms; y == NULL: not a MES call
struct MesArg {
  const double* y = nullptr;
  int K = 0;
  double sign = 1.0;
};

// acq_cost's counterpart: cost and (a, b) of one candidate from its posterior mean and SIGNED variance
__device__ __forceinline__ double mes_cost(const MesArg& ms, double mu, double var, double* a_out, double* b_out) {
  const double s = sqrt(fabs(var));
  const double sg = var > 0.0 ? 1.0 : (var < 0.0 ? -1.0 : 0.0);
  double sh = 0.0, shp = 0.0, shg = 0.0;
  for (int k = 0; k < ms.K; ++k) {
    const double g = (ms.sign > 0.0 ? mu - ms.y[k] : ms.y[k] - mu) / s;
    double h, hp;
    mes_h(g, &h, &hp);
    sh += h;
    shp += hp;
    shg += hp * g;
  }
  const double Kd = (double)ms.K;
  double a = -(ms.sign / (Kd * s)) * shp;
  double b = (sg / (2.0 * Kd * s * s)) * shg;
  if (var == 0.0) a = b = __builtin_nan("");
  *a_out = a;
  *b_out = b;
  return -(sh / Kd);
}

// values epilogue of one chunk [j0, j0 + mc): var = kd - ssq (ssq == NULL: kd IS the signed variance -- the VFE predictor's), the
// cost (written to cost[j0 + j]), the gradient coefficients (a, b) per candidate of the chunk (coef, nullable) and one arg-min
// partial per block at part_*[j0 / ACQ_EPI + blockIdx.x].  MES: mes_cost on `ms` in place of acq_cost (the three closed forms never
// enter it: their instantiation is the kernel as it was).
template <bool MES>
__global__ __launch_bounds__(ACQ_EPI) void acq_epilogue_kernel(int acq, double param, MesArg ms, const double* __restrict__ mean,
                                                               const double* __restrict__ kd, const double* __restrict__ ssq,
                                                               int64_t mc, int64_t j0, double* __restrict__ cost,
                                                               double* __restrict__ coef, double* __restrict__ part_c,
                                                               int64_t* __restrict__ part_i) {
  __shared__ double sc[ACQ_EPI];
  __shared__ int64_t si[ACQ_EPI];
  const int64_t j = (int64_t)blockIdx.x * ACQ_EPI + threadIdx.x;
  VI v{0.0, -1};
  if (j < mc) {
    double a, b;
    const double var = ssq ? kd[j] - ssq[j] : kd[j];
    const double c = MES ? mes_cost(ms, mean[j], var, &a, &b) : acq_cost(acq, param, mean[j], var, &a, &b);
    cost[j0 + j] = c;
    if (coef) {
      coef[2 * j] = a;
      coef[2 * j + 1] = b;
    }
    if (c == c) v = VI{c, j0 + j};
  }
  const VI r = block_arg_reduce(v, sc, si, blockDim.x, argmin_merge);
  if (threadIdx.x == 0) {
    part_c[j0 / ACQ_EPI + blockIdx.x] = r.v;
    part_i[j0 / ACQ_EPI + blockIdx.x] = r.i;
  }
}

// the partials of all chunks -> out_c[0], out_i[0] (one workgroup; each thread folds a strided slice in index order first)
__global__ __launch_bounds__(256) void acq_argmin_kernel(const double* __restrict__ part_c, const int64_t* __restrict__ part_i,
                                                         int64_t np_, double* __restrict__ out_c, int64_t* __restrict__ out_i) {
  __shared__ double sc[256];
  __shared__ int64_t si[256];
  VI v{0.0, -1};
  for (int64_t p = threadIdx.x; p < np_; p += 256) v = argmin_merge(v, VI{part_c[p], part_i[p]});
  const VI r = block_arg_reduce(v, sc, si, blockDim.x, argmin_merge);
  if (threadIdx.x == 0) {
    out_c[0] = r.i < 0 ? __builtin_nan("") : r.v;
    out_i[0] = r.i;
  }
}

// grad[m][l] = dA_m / dz_m[l] for the candidates of one chunk: one workgroup per candidate, one pass over the training points,
// fixed-order tree reduction per coordinate.  betaT: row m = beta[:, m] (row stride ldt), coef[2m], coef[2m+1] = (a, b).
// Per pair the radial factor f(r) (radial_pair, gpx_device.h) multiplies (x_j - z) -- the derivative is linear in the coordinate
// difference for the three kernels -- and the kernel's constant is applied once at the end:
//     SE   f = k(z, x_j),              const_l = 1 / cl_l^2 = scale_l^2
//     M32  f = e^-t,                   const   = sig scale^2
//     M52  f = (1 + t) e^-t,           const   = sig scale^2 / 3
// TWO (gpx_vfe_acq_grad): X = the inducing points, alpha = beta_u, and the weight of b is gamma = betaT - betaT2, the difference of
// the two transposed backward solves (Quu^-1 k_u and A^-1 k_u, row m each), taken here: gamma is never stored.
template <int KIND, int DMAX, bool TWO>
__global__ __launch_bounds__(256) void acq_grad_kernel(KParams kp, const double* __restrict__ X, int64_t n,
                                                       const double* __restrict__ Zc, const double* __restrict__ betaT,
                                                       const double* __restrict__ betaT2, int64_t ldt,
                                                       const double* __restrict__ alpha, const double* __restrict__ coef,
                                                       double* __restrict__ out) {
  __shared__ double red[256];
  const int64_t mm = blockIdx.x;
  const int d = kp.d, t = threadIdx.x;
  const double ca = coef[2 * mm], cb = -2.0 * coef[2 * mm + 1];
  double zs[DMAX], s1[DMAX];
#pragma unroll
  for (int l = 0; l < DMAX; ++l) {
    zs[l] = l < d ? Zc[mm * d + l] : 0.0;
    s1[l] = 0.0;
  }
  const double* __restrict__ bt = betaT + mm * ldt;
  const double* __restrict__ bt2 = TWO ? betaT2 + mm * ldt : nullptr;
  for (int64_t j = t; j < n; j += 256) {
    double diff[DMAX];
    const double f = radial_pair<KIND, DMAX>(kp, X + j * d, zs, diff);   // diff = x_j - z
    const double bj = TWO ? bt[j] - bt2[j] : bt[j];
    const double w = fma(ca, alpha[j], cb * bj) * f;
#pragma unroll
    for (int l = 0; l < DMAX; ++l) s1[l] = fma(w, diff[l], s1[l]);
  }
#pragma unroll
  for (int l = 0; l < DMAX; ++l) {
    if (l < d) {   // (uniform)
      double c = kp.scale[l] * kp.scale[l];
      if (KIND == GPX_K_MATERN32) c *= kp.sig;
      if (KIND == GPX_K_MATERN52) c *= kp.sig / 3.0;
      block_sum_256(red, c * s1[l]);
      if (t == 0) out[mm * d + l] = red[0];
      __syncthreads();
    }
  }
}

// betaT2 == NULL: the dense instantiation; else the VFE one (TWO)
int launch_acq_grad(gpx_ctx* ctx, const KParams& kp, const double* X, int64_t n, const double* Zc, int64_t mc,
                    const double* betaT, const double* betaT2, int64_t ldt, const double* alpha, const double* coef,
                    double* out) {
#define GPX_CALL(K_, DM_)                                                                                                     \
  do {                                                                                                                        \
    if (betaT2)                                                                                                               \
      hipLaunchKernelGGL((acq_grad_kernel<K_, DM_, true>), dim3((unsigned)mc), dim3(256), 0, ctx->stream, kp, X, n, Zc, betaT, \
                         betaT2, ldt, alpha, coef, out);                                                                      \
    else                                                                                                                      \
      hipLaunchKernelGGL((acq_grad_kernel<K_, DM_, false>), dim3((unsigned)mc), dim3(256), 0, ctx->stream, kp, X, n, Zc, betaT, \
                         betaT2, ldt, alpha, coef, out);                                                                      \
  } while (0)
  GPX_RADIAL_DISPATCH(kp.kind, kp.d, GPX_CALL);
#undef GPX_CALL
  GPX_HIP(hipGetLastError());
  return 0;
}

// the device copy of a call's y* (from its Scratch; the copy is queued: `spec->ystar` is the caller's and outlives the call)
int mes_upload(gpx_ctx* ctx, Scratch& sc, const MesSpec* spec, MesArg* out) {
  double* dy = nullptr;
  GPX_TRY(sc.get(spec->K * 8, &dy));
  GPX_HIP(hipMemcpyAsync(dy, spec->ystar, (size_t)spec->K * 8, hipMemcpyHostToDevice, ctx->stream));
  out->y = dy;
  out->K = (int)spec->K;
  out->sign = (double)spec->sign;
  return 0;
}

// The result side of the candidate-wise calls, dense (acq_impl) and VFE (vfe_acq_impl): the costs of all M candidates, one arg-min
// partial per ACQ_EPI of them, the winner's slots and -- for a gradient -- the (a, b) of one chunk and the M x d result.
struct AcqOut {
  int64_t M = 0, d = 0, nparts = 0;
  double *cost = nullptr, *part_c = nullptr, *best_c = nullptr, *coef = nullptr, *grad = nullptr;
  int64_t *part_i = nullptr, *best_i = nullptr;
  MesArg mes;   // (set by mes_upload for acq == GPX_ACQ_MES)

  int take(Scratch& sc, int64_t M_, int64_t mc_alloc, int64_t d_, bool want_grad) {
    M = M_;
    d = d_;
    nparts = (M + ACQ_EPI - 1) / ACQ_EPI;
    GPX_TRY(sc.get(M * 8, &cost));
    GPX_TRY(sc.get(nparts * 8, &part_c));
    GPX_TRY(sc.get(nparts * 8, &part_i));
    GPX_TRY(sc.get(8, &best_c));
    GPX_TRY(sc.get(8, &best_i));
    if (want_grad) {
      GPX_TRY(sc.get(2 * mc_alloc * 8, &coef));
      GPX_TRY(sc.get(M * d * 8, &grad));
    }
    return 0;
  }
  // the chunk [j0, j0 + mc): ssq == NULL: kd IS the signed variance (the VFE predictor's); prof_bytes: the caller's own bracket
  int epilogue(gpx_ctx* ctx, int acq, double param, const double* mean, const double* kd, const double* ssq, int64_t mc, int64_t j0,
               double prof_bytes) {
    ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, prof_bytes);
    const dim3 grid((unsigned)((mc + ACQ_EPI - 1) / ACQ_EPI));
    if (acq == GPX_ACQ_MES)
      hipLaunchKernelGGL(acq_epilogue_kernel<true>, grid, dim3(ACQ_EPI), 0, ctx->stream, acq, param, mes, mean, kd, ssq, mc, j0, cost,
                         coef, part_c, part_i);
    else
      hipLaunchKernelGGL(acq_epilogue_kernel<false>, grid, dim3(ACQ_EPI), 0, ctx->stream, acq, param, mes, mean, kd, ssq, mc, j0, cost,
                         coef, part_c, part_i);
    GPX_HIP(hipGetLastError());
    return 0;
  }
  // the arg-min over all chunks (when wanted) and the copies to the host, queued: the caller's Scratch waits for them
  int finish(gpx_ctx* ctx, double* cost_host, int64_t* best, double* best_cost, double* grad_host) {
    if (best || best_cost) {
      ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 16.0 * (double)nparts);
      hipLaunchKernelGGL(acq_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)part_c, (const int64_t*)part_i,
                         nparts, best_c, best_i);
      GPX_HIP(hipGetLastError());
      if (best) GPX_HIP(hipMemcpyAsync(best, best_i, 8, hipMemcpyDeviceToHost, ctx->stream));
      if (best_cost) GPX_HIP(hipMemcpyAsync(best_cost, best_c, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (cost_host) GPX_HIP(hipMemcpyAsync(cost_host, cost, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (grad_host) GPX_HIP(hipMemcpyAsync(grad_host, grad, (size_t)(M * d * 8), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
  }
};

// Shared body of gpx_acq / gpx_acq_grad.  cost_host (M), grad_host (M x d) nullable; best / best_cost nullable.
int acq_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha, const gpx_mat* Z,
             int acq, double param, double* cost_host, int64_t* best, double* best_cost, double* grad_host,
             const MesSpec* mes = nullptr) {
  const int64_t n = L->rows, np = L->prows, M = Z->rows, d = kp.d;
  const bool grad = grad_host != nullptr;
  const ChunkRange cr(M, gpx_eval_chunk(np));
  const int64_t bytesT = (grad && np >= 4096) ? cr.mc_alloc * chol_binv_order(np) * 8 : 0;
  double *pBt = nullptr, *pT = nullptr;
  PosteriorWork w(np, cr.mc_alloc, true);   // the same solve as posterior_impl
  AcqOut out;
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(w.take(sc, true, true));
  if (grad && !w.oop()) GPX_TRY(sc.get(w.bytesB, &pBt));
  if (bytesT) GPX_TRY(sc.get(bytesT, &pT));
  GPX_TRY(out.take(sc, M, cr.mc_alloc, d, grad));
  if (mes) GPX_TRY(mes_upload(ctx, sc, mes, &out.mes));
  GPX_TRY(w.upload_alpha(ctx, alpha, n));
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, j0 = c.j0;
    const double* Zc = Z->p + j0 * d;
    // gpx_posterior's own per-chunk step: the values equal GP.evaluate's
    GPX_TRY(w.run(ctx, kp, L, X, Zc, mc));
    GPX_TRY(out.epilogue(ctx, acq, param, w.mean, w.kd, w.ssq, mc, j0, 8.0 * 5.0 * (double)mc));
    if (!grad) continue;
    // beta^T = W^T L^-1 (mcp x np, row stride np) in the buffer W does not occupy (B is consumed by the out-of-place solve)
    double* Bt = w.oop() ? w.B : pBt;
    GPX_TRY(launch_transpose(ctx, w.solution(), np, mcp, gpx_skew_ld(mcp), Bt, np));
    if (pT) GPX_TRY(chol_trsm_right_n_leading(ctx, const_cast<gpx_mat*>(L), np, Bt, np, mcp, pT));
    else GPX_TRY(chol_trsm_right_n(ctx, L->p, L->ld, L->aux, Bt, np, mcp, np));
    ProfScope ps(ctx, GPX_PROF_GREEDY, (double)n * (double)mc * (6.0 * (double)d + 25.0),
                 8.0 * ((double)n * (double)mc + (double)n * d));
    GPX_TRY(launch_acq_grad(ctx, kp, X->p, n, Zc, mc, Bt, nullptr, np, w.alpha, out.coef, out.grad + j0 * d));
  }
  return out.finish(ctx, cost_host, best, best_cost, grad_host);
}

// the acquisition entries' own checks in front of the shared prologue
int acq_args(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
             const gpx_mat* Z, int acq, KParams* kp, const MesSpec* mes = nullptr) {
  GPX_ARG(ctx && L && X && Z && alpha, "NULL argument");
  if (mes) GPX_TRY(mes_args(mes));   // (the gpx_acq_mes* entries: acq is theirs, GPX_ACQ_MES)
  else GPX_ARG(acq == GPX_ACQ_UCB || acq == GPX_ACQ_PI || acq == GPX_ACQ_EI, "acq must be GPX_ACQ_UCB, GPX_ACQ_PI or GPX_ACQ_EI");
  return gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Z, nullptr, "point sets must be unpadded (n x d)", kp);
}

// ---- q-point batch selection with resident state (gpx_acq_batch) ------------------------------------------------------------
// Conditioning the model on one more (hallucinated) observation at candidate s is a rank-one change of everything the cost
// needs.  State: W_C = L^-1 K(X, C) (np x Mp, resident), mu, v (signed variance), the rows U[t] of the earlier picks.  Per pick
//     delta = v_s + noise,  y_s = mu_s (believer) or the caller's constant,
//     u_j   = (k(c_s, c_j) - W_C[:, s]^T W_C[:, j] - sum_{r<t} U[r][s] U[r][j]) / sqrt(delta),   U[t] = u,
//     mu_j += u_j (y_s - mu_s) / sqrt(delta),   v_j -= u_j^2,   param = max(param, y_s) when track_best
// which is the posterior of the model refitted on X + picks, y + lies with the same scalar noise.  The only pass of size N x M is
// the weighted column reduction h = W_C[:, s]^T W_C (launch_colreduce, fixed order); acq_batch_kernel does the rest in one pass
// over the candidates.  A pivot with delta <= 1e-13 k(c_s, c_s) adds no information (greedy_row_kernel's rule): u = 0.

// scalars of the current pick, written by acq_pick_kernel, read by acq_batch_kernel
enum { SC_DELTA = 0, SC_MU = 1, SC_LIE = 2, SC_PARAM = 3, SC_LIVE = 4, SC_N = 8 };

// pick `cur` = candidate s: its column of W_C (w, np), its coordinates along the earlier picks (uc, cur), the pick's scalars,
// and the mask.  Reads mu / v / U only: the state is changed by the NEXT acq_batch_kernel.
// VFE (gpx_vfe_acq_batch): Wc = Wa (nup rows), v = t, delta = noise + t_s -- never tiny, the pick is always live; kd is not read.
template <bool VFE>
__global__ __launch_bounds__(256) void acq_pick_kernel(const double* __restrict__ Wc, int64_t ld, int64_t np, int64_t s,
                                                       const double* __restrict__ U, int64_t ldu, int cur,
                                                       const double* __restrict__ mu, const double* __restrict__ v,
                                                       const double* __restrict__ kd, double noise, int lie, double lie_value,
                                                       int track_best, double* __restrict__ sc, double* __restrict__ uc,
                                                       double* __restrict__ w, int* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < np) w[i] = Wc[i * ld + s];
  if (i < cur) uc[i] = U[i * ldu + s];
  if (i == 0) {
    const double delta = VFE ? noise + v[s] : v[s] + noise, mus = mu[s];
    const double ys = lie == GPX_LIE_BELIEVER ? mus : lie_value;
    sc[SC_DELTA] = delta;
    sc[SC_MU] = mus;
    sc[SC_LIE] = ys;
    if (track_best && ys > sc[SC_PARAM]) sc[SC_PARAM] = ys;
    sc[SC_LIVE] = VFE || delta > 1e-13 * kd[s] ? 1.0 : 0.0;
    mask[s] = 1;
  }
}

// One pass over the candidates: (upd) condition mu, v on the pick `cur` = candidate s and store its row U[cur]; then the costs
// under the mask (NaN for a picked candidate) and one arg-min partial per block.  Only j < M is touched: the padding columns of
// W_C / U never enter a result.
// VFE (gpx_vfe_acq_batch): hdot = Wa[:, s]^T Wa enters with the opposite sign and alone (no k(c_s, c_j): the observation acts through
// the inducing variables), v holds t_j = |Wa[:, j]|^2 and the variance scored is rfix[j] + t_j.
// MES: mes_cost on `ms` (the y* held fixed from pick to pick) in place of acq_cost, as in acq_epilogue_kernel.
template <bool VFE, bool MES>
__global__ __launch_bounds__(ACQ_EPI) void acq_batch_kernel(KParams kp, int acq, MesArg ms, const double* __restrict__ Cp, int64_t M,
                                                            int upd, int64_t s, int cur, const double* __restrict__ sc,
                                                            const double* __restrict__ uc, const double* __restrict__ hdot,
                                                            double* __restrict__ U, int64_t ldu, double* __restrict__ mu,
                                                            double* __restrict__ v, const double* __restrict__ rfix,
                                                            const int* __restrict__ mask,
                                                            double* __restrict__ cost, double* __restrict__ part_c,
                                                            int64_t* __restrict__ part_i) {
  __shared__ double shc[ACQ_EPI];
  __shared__ int64_t shi[ACQ_EPI];
  const int64_t j = (int64_t)blockIdx.x * ACQ_EPI + threadIdx.x;
  VI best{0.0, -1};
  if (j < M) {
    double m = mu[j], var = v[j];
    if (upd) {
      double u = 0.0;
      if (sc[SC_LIVE] != 0.0) {   // (uniform)
        const double rs = 1.0 / sqrt(sc[SC_DELTA]);
        double acc = VFE ? hdot[j] : kpair(kp, Cp + s * kp.d, Cp + j * kp.d) - hdot[j];
        for (int r = 0; r < cur; ++r) acc = fma(-uc[r], U[(int64_t)r * ldu + j], acc);
        u = acc * rs;
        m = fma(u, (sc[SC_LIE] - sc[SC_MU]) * rs, m);
        var = fma(-u, u, var);
        mu[j] = m;
        v[j] = var;
      }
      U[(int64_t)cur * ldu + j] = u;
    }
    double a, b;
    const double vs = VFE ? rfix[j] + var : var;
    double c = MES ? mes_cost(ms, m, vs, &a, &b) : acq_cost(acq, sc[SC_PARAM], m, vs, &a, &b);
    if (mask[j]) c = __builtin_nan("");
    cost[j] = c;
    if (c == c) best = VI{c, j};
  }
  const VI r = block_arg_reduce(best, shc, shi, blockDim.x, argmin_merge);
  if (threadIdx.x == 0) {
    part_c[blockIdx.x] = r.v;
    part_i[blockIdx.x] = r.i;
  }
}

// The state of the pick loop, dense (acq_batch_impl) and VFE (vfe_acq_batch_impl), beside the resident W the caller fills: the
// rows U of the earlier picks, mu, v (dense: the signed variance; VFE: t), rfix (VFE only: r), hd (a column sum of squares of the
// set-up, then h of every pick), kd = k(c, c), the costs with their arg-min partials and winner slots, the scalars of the pick, its
// coordinates uc along the earlier picks, its column w of W, the mask, and the partial sums of the column reductions.
struct AcqBatchState {
  int64_t M = 0, Mp = 0, nparts = 0;
  double *U = nullptr, *mu = nullptr, *v = nullptr, *rfix = nullptr, *hd = nullptr, *kd = nullptr, *part = nullptr;
  double *cost = nullptr, *part_c = nullptr, *best_c = nullptr, *sc = nullptr, *uc = nullptr, *w = nullptr;
  int64_t *part_i = nullptr, *best_i = nullptr;
  int* mask = nullptr;
  MesArg mes;         // (set by mes_upload for acq == GPX_ACQ_MES)
  double sc0[SC_N];   // (lives as long as the call: the copy of the scalars is queued from it)

  // prows: the padded row count of W (np, or nup on a VFE model)
  int take(Scratch& s, int64_t M_, int64_t prows, int64_t q, bool vfe) {
    M = M_;
    Mp = gpx_round_up(M, GPX_TILE);
    nparts = (M + ACQ_EPI - 1) / ACQ_EPI;
    const int64_t bytesM = Mp * 8;
    GPX_TRY(s.get(q * Mp * 8, &U));
    GPX_TRY(s.get(bytesM, &mu));
    GPX_TRY(s.get(bytesM, &v));
    if (vfe) GPX_TRY(s.get(bytesM, &rfix));
    GPX_TRY(s.get(bytesM, &kd));
    GPX_TRY(s.get(bytesM, &hd));
    GPX_TRY(s.get(colreduce_partial_elems(prows, Mp) * 8 + 8, &part));
    GPX_TRY(s.get(M * 8, &cost));
    GPX_TRY(s.get(nparts * 8, &part_c));
    GPX_TRY(s.get(nparts * 8, &part_i));
    GPX_TRY(s.get(8, &best_c));
    GPX_TRY(s.get(8, &best_i));
    GPX_TRY(s.get(SC_N * 8, &sc));
    GPX_TRY(s.get(q * 8, &uc));
    GPX_TRY(s.get((prows > q ? prows : q) * 8, &w));
    GPX_TRY(s.get(Mp * 4, &mask));
    return 0;
  }
  // nothing picked yet, param as the caller gave it: queued before the set-up
  int init(gpx_ctx* ctx, double param) {
    for (int i = 0; i < SC_N; ++i) sc0[i] = 0.0;
    sc0[SC_PARAM] = param;
    GPX_HIP(hipMemsetAsync(mask, 0, (size_t)Mp * 4, ctx->stream));
    GPX_HIP(hipMemcpyAsync(sc, sc0, sizeof(sc0), hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
};

// The q picks on a state whose set-up is done (mu, v, rfix, kd filled; W = the resident rows x M matrix, row stride ld, prows
// padded rows).  `who` opens the error text.
template <bool VFE>
int acq_batch_picks(gpx_ctx* ctx, const KParams& kp, int acq, const gpx_mat* Cm, AcqBatchState& st, const double* W, int64_t ld,
                    int64_t rows, int64_t prows, double noise, int track_best, int lie, double lie_value, int64_t q,
                    int64_t* out_idx, double* out_cost, double* out_lie, double* all_costs, const char* who) {
  const int64_t M = st.M, Mp = st.Mp;
  const dim3 gEpi((unsigned)st.nparts), gPick((unsigned)(((prows > q ? prows : q) + 255) / 256));
  int64_t s = -1;
  for (int64_t t = 0; t < q; ++t) {
    {
      ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 8.0 * (double)M * (6.0 + (double)t));
      if (acq == GPX_ACQ_MES)
        hipLaunchKernelGGL((acq_batch_kernel<VFE, true>), gEpi, dim3(ACQ_EPI), 0, ctx->stream, kp, acq, st.mes, (const double*)Cm->p,
                           M, t > 0 ? 1 : 0, s, (int)(t - 1), (const double*)st.sc, (const double*)st.uc, (const double*)st.hd, st.U,
                           Mp, st.mu, st.v, (const double*)st.rfix, (const int*)st.mask, st.cost, st.part_c, st.part_i);
      else
        hipLaunchKernelGGL((acq_batch_kernel<VFE, false>), gEpi, dim3(ACQ_EPI), 0, ctx->stream, kp, acq, st.mes, (const double*)Cm->p,
                           M, t > 0 ? 1 : 0, s, (int)(t - 1), (const double*)st.sc, (const double*)st.uc, (const double*)st.hd, st.U,
                           Mp, st.mu, st.v, (const double*)st.rfix, (const int*)st.mask, st.cost, st.part_c, st.part_i);
      hipLaunchKernelGGL(acq_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)st.part_c,
                         (const int64_t*)st.part_i, st.nparts, st.best_c, st.best_i);
    }
    double c = 0.0;
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipMemcpyAsync(&s, st.best_i, 8, hipMemcpyDeviceToHost, ctx->stream));
    GPX_HIP(hipMemcpyAsync(&c, st.best_c, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (all_costs) GPX_HIP(hipMemcpyAsync(all_costs + t * M, st.cost, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    GPX_HIP(hipStreamSynchronize(ctx->stream));
    if (s < 0 || s >= M) {
      gpx_set_error("%s: pick %lld of %lld: no candidate has a non-NaN cost", who, (long long)(t + 1), (long long)q);
      return -1;
    }
    out_idx[t] = s;
    if (out_cost) out_cost[t] = c;
    if (t + 1 == q && !out_lie) break;
    hipLaunchKernelGGL(acq_pick_kernel<VFE>, gPick, dim3(256), 0, ctx->stream, W, ld, prows, s, (const double*)st.U, Mp, (int)t,
                       (const double*)st.mu, (const double*)st.v, VFE ? (const double*)nullptr : (const double*)st.kd, noise, lie,
                       lie_value, track_best, st.sc, st.uc, st.w, st.mask);
    GPX_HIP(hipGetLastError());
    if (out_lie) GPX_HIP(hipMemcpyAsync(out_lie + t, st.sc + SC_LIE, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (t + 1 == q) break;
    GPX_TRY(launch_colreduce(ctx, W, ld, rows, Mp, st.w, st.hd, st.part));
  }
  return 0;
}

int acq_batch_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha, const gpx_mat* Cm,
                   double noise, int acq, double param, int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx,
                   double* out_cost, double* out_lie, double* all_costs, const MesSpec* mes = nullptr) {
  const int64_t n = L->rows, np = L->prows, M = Cm->rows, d = kp.d;
  const int64_t Mp = gpx_round_up(M, GPX_TILE), ld = gpx_skew_ld(Mp);
  // the solve of gpx_acq (chol_cross_solve), the cross matrix chunk by chunk into the resident W_C
  const bool oop = chol_cross_oop(np);
  const int64_t mcmax = gpx_round_up(gpx_eval_chunk(np), GPX_TILE);
  const int64_t mcw = Mp < mcmax ? Mp : mcmax, ldb = gpx_skew_ld(mcw);
  double *Wc = nullptr, *pB = nullptr, *pal = nullptr;
  AcqBatchState st;
  Scratch sc(ctx);
  GPX_TRY(sc.get(np * ld * 8, &Wc));
  if (oop) GPX_TRY(sc.get(np * ldb * 8, &pB));
  GPX_TRY(gpx_upload_padded(ctx, sc, alpha, n, np, &pal));
  GPX_TRY(st.take(sc, M, np, q, false));
  if (mes) GPX_TRY(mes_upload(ctx, sc, mes, &st.mes));
  GPX_TRY(st.init(ctx, param));
  // ---- set-up: the posterior pass with W kept.  Not gpx_posterior_chunk: the solve lands in the resident W_C with ITS row
  // stride, and the squares are reduced once over all of W_C (into hd).  Its own step rule, not ChunkRange's: the walk is over
  // the PADDED columns (mcw at a time, every chunk a multiple of 128 wide) ----
  for (int64_t j0 = 0; j0 < Mp; j0 += mcw) {
    const int64_t mcp = (Mp - j0) < mcw ? (Mp - j0) : mcw;
    const int64_t mc = (M - j0) < mcp ? (M - j0) : mcp;
    double* B = oop ? pB : Wc + j0;
    const int64_t ldc = oop ? gpx_skew_ld(mcp) : ld;
    GPX_TRY(launch_kfill(ctx, kp, X->p, n, Cm->p + j0 * d, mc, 0, nullptr, 0, 0.0, B, np, mcp, ldc));
    GPX_TRY(launch_colreduce(ctx, B, ldc, n, mcp, pal, st.mu + j0, st.part));
    GPX_TRY(chol_cross_solve(ctx, L, B, ldc, oop ? Wc + j0 : nullptr, ld, mcp));
  }
  GPX_TRY(launch_colreduce(ctx, Wc, ld, n, Mp, nullptr, st.hd, st.part));
  GPX_TRY(launch_kdiag(ctx, kp, Cm->p, M, st.kd));
  GPX_TRY(launch_vec_sub(ctx, st.kd, st.hd, M, st.v));
  return acq_batch_picks<false>(ctx, kp, acq, Cm, st, Wc, ld, n, np, noise, track_best, lie, lie_value, q, out_idx, out_cost,
                                out_lie, all_costs, "acq batch");
}

}  // namespace

// (gpx_internal.h) acq_argmin_kernel for the arg-min partials of another file (sample.hip: one partial per q-EI workgroup)
int launch_acq_argmin(gpx_ctx* ctx, const double* part_c, const int64_t* part_i, int64_t nparts, double* out_c, int64_t* out_i) {
  ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 16.0 * (double)nparts);
  hipLaunchKernelGGL(acq_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, part_c, part_i, nparts, out_c, out_i);
  GPX_HIP(hipGetLastError());
  return 0;
}

// (gpx_internal.h) the y* rules of the gpx_acq_mes* and gpx_vfe_acq_mes* entries
int mes_args(const MesSpec* mes) {
  GPX_ARG(mes->ystar != nullptr, "ystar is NULL");
  GPX_ARG(mes->K >= 1 && mes->K <= GPX_MES_MAX_K, "K (the number of sampled optima in ystar) must be between 1 and GPX_MES_MAX_K");
  GPX_ARG(mes->sign == 1 || mes->sign == -1, "sign must be +1 (ystar holds sampled minima) or -1 (sampled maxima)");
  for (int64_t k = 0; k < mes->K; ++k)
    if (!__builtin_isfinite(mes->ystar[k])) {
      gpx_set_error("%s:%d bad argument: ystar[%lld] is not finite: every sampled optimum must be", __FILE__, __LINE__, (long long)k);
      return -1;
    }
  return 0;
}

// ---- the same three calls on a VFE model (gpx_vfe_acq, gpx_vfe_acq_grad, gpx_vfe_acq_batch; argument checks: fitc.hip) -------------
// Notation of fitc.hip: S the nu inducing points, Quu = K(S,S) + noise I = Lu Lu^T, A = Quu + Kuf Kfu / noise = La La^T,
// beta_u = Quu^-1 Kuf alpha, k_u(z) = K(S, z);  mean = k_u^T beta_u,  var = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2.
//
// Values: vfe_posterior_chunk (gpx_vfe_posterior's own per-chunk step), then AcqOut's epilogue on the signed variance it leaves
// (ssq == NULL) and its arg-min.  Gradient, with (a, b) from that epilogue:
//     gamma(z) = Quu^-1 k_u - A^-1 k_u,     grad_z A = sum_u dk(z, s_u)/dz (a beta_u[u] - 2 b gamma(z)[u])
// The two forward solves of the values stay (Wu = Lu^-1 k_u, Wa = La^-1 k_u: FOUR nu x chunk buffers instead of two or three), each
// is transposed and swept backward from the right (Wu^T Lu^-1, Wa^T La^-1: acq_impl's pattern, the nu-axis contiguous per
// candidate; chol_trsm_right_n at every order -- no branch of its own at order 4096), and acq_grad_kernel<.., TWO> reads both
// rows and takes their difference in its one pass over the inducing points.
int vfe_acq_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                 double* cost_host, int64_t* best, double* best_cost, double* grad_host, const MesSpec* mes) {
  FitcView fv;
  fitc_view(f, &fv);
  const int64_t nu = fv.nu, nup = fv.nup, M = Z->rows, d = fv.kp->d;
  const bool grad = grad_host != nullptr;
  KParams kpz = *fv.kp;   // the candidates may reach beyond the training domain
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Z));
  const ChunkRange cr(M, gpx_eval_chunk(nup));
  double *T1 = nullptr, *T2 = nullptr;
  VfePosteriorWork w(nup, cr.mc_alloc, true);
  AcqOut out;
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(w.take(sc, true));
  const bool oop = w.oop();
  if (grad) {   // two more blocks: the targets of the transpositions, or (out of place) the second one Wa's own
    if (!oop) GPX_TRY(sc.get(w.bytesB, &T1));
    GPX_TRY(sc.get(w.bytesB, &T2));
    if (oop) w.Wa = T2;
  }
  GPX_TRY(out.take(sc, M, cr.mc_alloc, d, grad));
  if (mes) GPX_TRY(mes_upload(ctx, sc, mes, &out.mes));
  GPX_TRY(w.beta(ctx, f, coeff, sc));   // (GPX_ACQ_VARIANCE: no coeff, no mean; its weight a is 0)
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, j0 = c.j0, ldb = gpx_skew_ld(mcp);
    const double* Zc = Z->p + j0 * d;
    // values only: both out-of-place solutions land in the one buffer, as in gpx_vfe_posterior
    GPX_TRY(w.run(ctx, f, kpz, S, Zc, mc));
    GPX_TRY(out.epilogue(ctx, acq, param, w.pm, w.pv, nullptr, mc, j0, 8.0 * 4.0 * (double)mc));
    if (!grad) continue;
    // (Quu^-1 k_u)^T = Wu^T Lu^-1 and (A^-1 k_u)^T = Wa^T La^-1 (mcp x nup, row stride nup), in the two buffers the forward
    // solutions do not occupy
    double *Tu = oop ? w.B1 : T1, *Ta = oop ? w.B2 : T2;
    GPX_TRY(launch_transpose(ctx, w.solU(), nup, mcp, ldb, Tu, nup));
    GPX_TRY(chol_trsm_right_n(ctx, fv.Lu->p, fv.Lu->ld, fv.Lu->aux, Tu, nup, mcp, nup));
    GPX_TRY(launch_transpose(ctx, w.solA(), nup, mcp, ldb, Ta, nup));
    GPX_TRY(chol_trsm_right_n(ctx, fv.La->p, fv.La->ld, fv.La->aux, Ta, nup, mcp, nup));
    ProfScope ps(ctx, GPX_PROF_GREEDY, (double)nu * (double)mc * (6.0 * (double)d + 26.0),
                 8.0 * (2.0 * (double)nu * (double)mc + (double)nu * d));
    GPX_TRY(launch_acq_grad(ctx, kpz, S->p, nu, Zc, mc, Tu, Ta, nup, w.bu, out.coef, out.grad + j0 * d));
  }
  return out.finish(ctx, cost_host, best, best_cost, grad_host);
}

// q-point batch on a VFE model whose inducing points and hyper-parameters stay fixed.  One more observation at c_s changes A to
// A + k_u(c_s) k_u(c_s)^T / noise and nothing else (Quu, and with it r_j = k(c_j,c_j) - |Lu^-1 k_u(c_j)|^2, stays), so the refit is a
// rank-one recurrence in the inducing space.  State: Wa = La^-1 K(S, C) (nup x Mp, the only matrix kept), mu, r, t_j = |Wa[:, j]|^2,
// the rows U[t].  Per pick
//     v_j = r_j + t_j;   delta = noise + t_s  (NOT v_s + noise);   y_s = mu_s (believer) or the caller's constant
//     u_j = (Wa[:, s]^T Wa[:, j] - sum_{r<t} U[r][s] U[r][j]) / sqrt(delta),   U[t] = u
//     mu_j += u_j (y_s - mu_s) / sqrt(delta),   t_j -= u_j^2,   param = max(param, y_s) when track_best
// delta >= noise > 0 (gpx_vfe_fit refuses noise <= 0): the tiny-pivot rule of the dense path (delta <= 1e-13 k(c_s, c_s): u = 0) has
// no counterpart here, every pick conditions.  The only nu x M pass per pick is h = Wa[:, s]^T Wa (launch_colreduce, fixed order);
// acq_batch_picks<true> (the dense loop, with acq_pick_kernel<true> / acq_batch_kernel<true>) does the rest.  The set-up walks the candidates in gpx_vfe_acq's chunks with
// gpx_vfe_acq's launches, so row 0 of the costs holds its bits; the Lu solve of a chunk is transient (one nup x chunk buffer; out of
// place it lands in the chunk's columns of Wa, which the La solve then overwrites).
int vfe_acq_batch_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Cm, int acq,
                       double param, int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx, double* out_cost,
                       double* out_lie, double* all_costs, const MesSpec* mes) {
  FitcView fv;
  fitc_view(f, &fv);
  const int64_t nu = fv.nu, nup = fv.nup, M = Cm->rows, d = fv.kp->d;
  const int64_t Mp = gpx_round_up(M, GPX_TILE), ld = gpx_skew_ld(Mp);
  KParams kpz = *fv.kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Cm));
  const bool oop = chol_cross_oop(nup);
  const ChunkRange cr(M, gpx_eval_chunk(nup));
  const int64_t ldb = gpx_skew_ld(cr.mc_alloc);
  double *pW, *pB, *bu;
  AcqBatchState st;   // v = t, rfix = r, hd = |Lu^-1 k_u|^2 at the set-up
  Scratch sc(ctx);
  GPX_TRY(sc.get(nup * ld * 8, &pW));
  GPX_TRY(sc.get(nup * ldb * 8, &pB));
  GPX_TRY(st.take(sc, M, nup, q, true));
  if (mes) GPX_TRY(mes_upload(ctx, sc, mes, &st.mes));
  GPX_TRY(vfe_beta_u(ctx, f, coeff, sc, &bu));
  GPX_TRY(st.init(ctx, param));
  // ---- set-up: gpx_vfe_acq's chunks.  Not vfe_posterior_chunk: the La solve lands in the resident Wa with ITS row stride; the Lu
  // solve is transient (in place in pB; out of place in the chunk's columns of Wa, which the La solve then overwrites) ----
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, j0 = c.j0, ldc = gpx_skew_ld(mcp);
    const double* Cc = Cm->p + j0 * d;
    double* Wc = pW + j0;
    GPX_TRY(launch_kfill(ctx, kpz, S->p, nu, Cc, mc, 0, nullptr, 0, 0.0, pB, nup, mcp, ldc));
    GPX_TRY(launch_colreduce(ctx, pB, ldc, nu, mcp, bu, st.mu + j0, st.part));
    GPX_TRY(chol_cross_solve(ctx, fv.Lu, pB, ldc, oop ? Wc : nullptr, ld, mcp));
    GPX_TRY(launch_colreduce(ctx, oop ? Wc : pB, oop ? ld : ldc, nu, mcp, nullptr, st.hd + j0, st.part));
    // the second fill: the right-hand side of the La solve -- out of place again in pB, in place in Wa's own columns
    double* B2 = oop ? pB : Wc;
    GPX_TRY(launch_kfill(ctx, kpz, S->p, nu, Cc, mc, 0, nullptr, 0, 0.0, B2, nup, mcp, oop ? ldc : ld));
    GPX_TRY(chol_cross_solve(ctx, fv.La, B2, oop ? ldc : ld, oop ? Wc : nullptr, ld, mcp));
    GPX_TRY(launch_colreduce(ctx, Wc, ld, nu, mcp, nullptr, st.v + j0, st.part));
    GPX_TRY(launch_kdiag(ctx, *fv.kp, Cc, mc, st.kd + j0));
  }
  GPX_TRY(launch_vec_sub(ctx, st.kd, st.hd, M, st.rfix));
  return acq_batch_picks<true>(ctx, kpz, acq, Cm, st, pW, ld, nu, nup, fv.noise, track_best, lie, lie_value, q, out_idx, out_cost,
                               out_lie, all_costs, "vfe acq batch");
}

extern "C" {

int gpx_acq(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
            const gpx_mat* Z, int acq, double param, double* cost, int64_t* best, double* best_cost) {
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Z, acq, &kp));
  if (Z->rows == 0) {
    if (best) *best = -1;
    if (best_cost) *best_cost = __builtin_nan("");
    return 0;
  }
  return acq_impl(ctx, kp, L, X, alpha, Z, acq, param, cost, best, best_cost, nullptr);
}

int gpx_acq_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const double* alpha, const gpx_mat* Z, int acq, double param, double* cost, double* grad) {
  GPX_ARG(grad != nullptr, "grad is NULL");
  GPX_ARG(kind == GPX_K_SE || kind == GPX_K_MATERN32 || kind == GPX_K_MATERN52,
          "acquisition gradients exist for the stationary kernels (SE, Matern 3/2, Matern 5/2) only: the Mehler kernel's "
          "prior variance depends on the point");
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Z, acq, &kp));
  if (Z->rows == 0) return 0;
  return acq_impl(ctx, kp, L, X, alpha, Z, acq, param, cost, nullptr, nullptr, grad);
}

int gpx_acq_batch(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                  const double* alpha, const gpx_mat* C, double noise, int acq, double param, int track_best, int lie,
                  double lie_value, int64_t q, int64_t* out_idx, double* out_cost, double* out_lie, double* all_costs) {
  GPX_ARG(out_idx != nullptr, "out_idx is NULL");
  GPX_ARG(lie == GPX_LIE_BELIEVER || lie == GPX_LIE_CONSTANT, "lie must be GPX_LIE_BELIEVER or GPX_LIE_CONSTANT");
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, C, acq, &kp));
  GPX_ARG(q >= 1, "need at least one pick");
  GPX_ARG(q <= C->rows, "more picks than candidates");
  GPX_ARG(noise >= 0.0, "noise variance must not be negative");
  return acq_batch_impl(ctx, kp, L, X, alpha, C, noise, acq, param, track_best != 0, lie, lie_value, q, out_idx, out_cost, out_lie,
                        all_costs);
}

// ---- max-value entropy search: the three calls above with mes_cost on the caller's K sampled optima in place of acq_cost ---------
int gpx_acq_mes(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
                const gpx_mat* Z, const double* ystar, int64_t K, int sign, double* cost, int64_t* best, double* best_cost) {
  const MesSpec mes{ystar, K, sign};
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Z, GPX_ACQ_MES, &kp, &mes));
  if (Z->rows == 0) {
    if (best) *best = -1;
    if (best_cost) *best_cost = __builtin_nan("");
    return 0;
  }
  return acq_impl(ctx, kp, L, X, alpha, Z, GPX_ACQ_MES, 0.0, cost, best, best_cost, nullptr, &mes);
}

int gpx_acq_mes_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const double* alpha, const gpx_mat* Z, const double* ystar, int64_t K, int sign, double* cost, double* grad) {
  GPX_ARG(grad != nullptr, "grad is NULL");
  GPX_ARG(kind == GPX_K_SE || kind == GPX_K_MATERN32 || kind == GPX_K_MATERN52,
          "acquisition gradients exist for the stationary kernels (SE, Matern 3/2, Matern 5/2) only: the Mehler kernel's "
          "prior variance depends on the point");
  const MesSpec mes{ystar, K, sign};
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Z, GPX_ACQ_MES, &kp, &mes));
  if (Z->rows == 0) return 0;
  return acq_impl(ctx, kp, L, X, alpha, Z, GPX_ACQ_MES, 0.0, cost, nullptr, nullptr, grad, &mes);
}

int gpx_acq_mes_batch(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                      const double* alpha, const gpx_mat* C, double noise, const double* ystar, int64_t K, int sign, int lie,
                      double lie_value, int64_t q, int64_t* out_idx, double* out_cost, double* out_lie, double* all_costs) {
  GPX_ARG(out_idx != nullptr, "out_idx is NULL");
  GPX_ARG(lie == GPX_LIE_BELIEVER || lie == GPX_LIE_CONSTANT, "lie must be GPX_LIE_BELIEVER or GPX_LIE_CONSTANT");
  const MesSpec mes{ystar, K, sign};
  KParams kp;
  GPX_TRY(acq_args(ctx, kind, d, hyp, nhyp, L, X, alpha, C, GPX_ACQ_MES, &kp, &mes));
  GPX_ARG(q >= 1, "need at least one pick");
  GPX_ARG(q <= C->rows, "more picks than candidates");
  GPX_ARG(noise >= 0.0, "noise variance must not be negative");
  return acq_batch_impl(ctx, kp, L, X, alpha, C, noise, GPX_ACQ_MES, 0.0, 0, lie, lie_value, q, out_idx, out_cost, out_lie, all_costs,
                        &mes);
}

}  // extern "C"

// test hook (gpx_debug.h): AcqOut's epilogue chunk by chunk and its arg-min on host vectors of means and SIGNED variances (ssq ==
// NULL, the VFE predictor's form).  Every device buffer the two kernels write carries DBG_BAND words of a sentinel behind its last
// entry; a launch that writes there fails the call.
namespace {

constexpr int64_t DBG_BAND = 32;
constexpr int64_t DBG_SENTINEL = 0x5A5AA5A5C3C33C3CLL;   // (as a double: 2.6e127, no value an epilogue makes)

template <typename T>
int dbg_banded(gpx_ctx* ctx, Scratch& sc, int64_t count, T** p) {
  static_assert(sizeof(T) == 8, "eight-byte words");
  std::vector<int64_t> h((size_t)(count + DBG_BAND), DBG_SENTINEL);
  GPX_TRY(sc.get((count + DBG_BAND) * 8, p));
  GPX_HIP(hipMemcpyAsync(*p, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));   // (h goes out of scope)
  return 0;
}

int dbg_band_intact(gpx_ctx* ctx, const void* p, int64_t count) {
  int64_t h[DBG_BAND];
  GPX_HIP(hipMemcpyAsync(h, (const int64_t*)p + count, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < DBG_BAND; ++i)
    GPX_ARG(h[i] == DBG_SENTINEL, "the acquisition epilogue or its arg-min wrote behind the last entry of a result");
  return 0;
}

}  // namespace

// the body of both hooks; mes != NULL: gpx_dbg_acq_mes_epilogue's (acq = GPX_ACQ_MES)
static int dbg_acq_epilogue_impl(gpx_ctx* ctx, int acq, double param, const MesSpec* mes, const double* mean, const double* var,
                                 int64_t m, int64_t chunk, double* cost, double* coef, int64_t* best, double* best_cost) {
  GPX_ARG(ctx && mean && var && cost && best && best_cost, "NULL argument");
  if (mes) GPX_TRY(mes_args(mes));
  else GPX_ARG(acq == GPX_ACQ_UCB || acq == GPX_ACQ_PI || acq == GPX_ACQ_EI, "acq must be GPX_ACQ_UCB, GPX_ACQ_PI or GPX_ACQ_EI");
  GPX_ARG(m >= 1, "need at least one candidate");
  GPX_ARG(chunk >= 0 && chunk % ACQ_EPI == 0, "chunk must be 0 (one launch) or a multiple of 128");
  const int64_t step = chunk > 0 && chunk < m ? chunk : m;
  double *dmean = nullptr, *dvar = nullptr;
  AcqOut out;
  Scratch sc(ctx);
  out.M = m;
  out.nparts = (m + ACQ_EPI - 1) / ACQ_EPI;
  GPX_TRY(sc.get(m * 8, &dmean));
  GPX_TRY(sc.get(m * 8, &dvar));
  GPX_TRY(dbg_banded(ctx, sc, m, &out.cost));
  GPX_TRY(dbg_banded(ctx, sc, out.nparts, &out.part_c));
  GPX_TRY(dbg_banded(ctx, sc, out.nparts, &out.part_i));
  GPX_TRY(dbg_banded(ctx, sc, 1, &out.best_c));
  GPX_TRY(dbg_banded(ctx, sc, 1, &out.best_i));
  if (coef) GPX_TRY(dbg_banded(ctx, sc, 2 * step, &out.coef));
  if (mes) GPX_TRY(mes_upload(ctx, sc, mes, &out.mes));
  GPX_HIP(hipMemcpyAsync(dmean, mean, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
  GPX_HIP(hipMemcpyAsync(dvar, var, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
  for (int64_t j0 = 0; j0 < m; j0 += step) {
    const int64_t mc = m - j0 < step ? m - j0 : step;
    GPX_TRY(out.epilogue(ctx, acq, param, dmean + j0, dvar + j0, nullptr, mc, j0, 8.0 * 4.0 * (double)mc));
    if (coef) GPX_HIP(hipMemcpyAsync(coef + 2 * j0, out.coef, (size_t)(2 * mc) * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  GPX_TRY(out.finish(ctx, cost, best, best_cost, nullptr));
  GPX_TRY(dbg_band_intact(ctx, out.cost, m));
  GPX_TRY(dbg_band_intact(ctx, out.part_c, out.nparts));
  GPX_TRY(dbg_band_intact(ctx, out.part_i, out.nparts));
  GPX_TRY(dbg_band_intact(ctx, out.best_c, 1));
  GPX_TRY(dbg_band_intact(ctx, out.best_i, 1));
  if (coef) GPX_TRY(dbg_band_intact(ctx, out.coef, 2 * step));
  return 0;
}

extern "C" int gpx_dbg_acq_epilogue(gpx_ctx* ctx, int acq, double param, const double* mean, const double* var, int64_t m,
                                    int64_t chunk, double* cost, double* coef, int64_t* best, double* best_cost) {
  return dbg_acq_epilogue_impl(ctx, acq, param, nullptr, mean, var, m, chunk, cost, coef, best, best_cost);
}

extern "C" int gpx_dbg_acq_mes_epilogue(gpx_ctx* ctx, const double* ystar, int64_t K, int sign, const double* mean, const double* var,
                                        int64_t m, int64_t chunk, double* cost, double* coef, int64_t* best, double* best_cost) {
  const MesSpec mes{ystar, K, sign};
  return dbg_acq_epilogue_impl(ctx, GPX_ACQ_MES, 0.0, &mes, mean, var, m, chunk, cost, coef, best, best_cost);
}
