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

// values epilogue of one chunk [j0, j0 + mc): var = kd - ssq, the cost (written to cost[j0 + j]), the gradient coefficients
// (a, b) per candidate of the chunk (coef, nullable) and one arg-min partial per block at part_*[j0 / ACQ_EPI + blockIdx.x].
__global__ __launch_bounds__(ACQ_EPI) void acq_epilogue_kernel(int acq, double param, const double* __restrict__ mean,
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
    const double c = acq_cost(acq, param, mean[j], kd[j] - ssq[j], &a, &b);
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
template <int KIND, int DMAX>
__global__ __launch_bounds__(256) void acq_grad_kernel(KParams kp, const double* __restrict__ X, int64_t n,
                                                       const double* __restrict__ Zc, const double* __restrict__ betaT,
                                                       int64_t ldt, const double* __restrict__ alpha,
                                                       const double* __restrict__ coef, double* __restrict__ out) {
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
  for (int64_t j = t; j < n; j += 256) {
    double diff[DMAX];
    const double f = radial_pair<KIND, DMAX>(kp, X + j * d, zs, diff);   // diff = x_j - z
    const double w = fma(ca, alpha[j], cb * bt[j]) * f;
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

int launch_acq_grad(gpx_ctx* ctx, const KParams& kp, const double* X, int64_t n, const double* Zc, int64_t mc,
                    const double* betaT, int64_t ldt, const double* alpha, const double* coef, double* out) {
#define GPX_CALL(K_, DM_)                                                                                                 \
  hipLaunchKernelGGL((acq_grad_kernel<K_, DM_>), dim3((unsigned)mc), dim3(256), 0, ctx->stream, kp, X, n, Zc, betaT, ldt, \
                     alpha, coef, out)
  GPX_RADIAL_DISPATCH(kp.kind, kp.d, GPX_CALL);
#undef GPX_CALL
  GPX_HIP(hipGetLastError());
  return 0;
}

// Shared body of gpx_acq / gpx_acq_grad.  cost_host (M), grad_host (M x d) nullable; best / best_cost nullable.
int acq_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha, const gpx_mat* Z,
             int acq, double param, double* cost_host, int64_t* best, double* best_cost, double* grad_host) {
  const int64_t n = L->rows, np = L->prows, M = Z->rows, d = kp.d;
  const bool grad = grad_host != nullptr;
  const int64_t mcmax = gpx_eval_chunk(np);
  const int64_t mc_alloc = gpx_round_up(M < mcmax ? M : mcmax, GPX_TILE);
  // the same solve as posterior_impl: from 2048 training points out of place through the block inverses
  const bool oop = np >= 2048;
  const int64_t ldb_alloc = gpx_skew_ld(mc_alloc);
  const int64_t bytesB = np * ldb_alloc * 8, bytes_out = mc_alloc * 8;
  const int64_t bytes_part = colreduce_partial_elems(np, mc_alloc) * 8 + 8;
  const int64_t nparts = (M + ACQ_EPI - 1) / ACQ_EPI;
  const int64_t bytesT = (grad && np >= 4096) ? mc_alloc * chol_binv_order(np) * 8 : 0;
  double *pB = nullptr, *pW = nullptr, *pT = nullptr, *pal = nullptr, *pmean = nullptr, *pout = nullptr, *ppart = nullptr;
  double *pkd = nullptr, *pcost = nullptr, *pcoef = nullptr, *pgrad = nullptr, *ppc = nullptr, *pbc = nullptr;
  int64_t *ppi = nullptr, *pbi = nullptr;
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(sc.get(bytesB, &pB));
  if (oop || grad) GPX_TRY(sc.get(bytesB, &pW));
  if (bytesT) GPX_TRY(sc.get(bytesT, &pT));
  GPX_TRY(sc.get(np * 8, &pal));
  GPX_TRY(sc.get(bytes_out, &pmean));
  GPX_TRY(sc.get(bytes_out, &pout));
  GPX_TRY(sc.get(bytes_out, &pkd));
  GPX_TRY(sc.get(bytes_part, &ppart));
  GPX_TRY(sc.get(M * 8, &pcost));
  GPX_TRY(sc.get(nparts * 8, &ppc));
  GPX_TRY(sc.get(nparts * 8, &ppi));
  GPX_TRY(sc.get(8, &pbc));
  GPX_TRY(sc.get(8, &pbi));
  if (grad) {
    GPX_TRY(sc.get(2 * bytes_out, &pcoef));
    GPX_TRY(sc.get(M * d * 8, &pgrad));
  }
  GPX_HIP(hipMemsetAsync(pal, 0, (size_t)np * 8, ctx->stream));
  GPX_HIP(hipMemcpyAsync(pal, alpha, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  for (int64_t j0 = 0; j0 < M; j0 += mcmax) {
    const int64_t mc = (M - j0) < mcmax ? (M - j0) : mcmax;
    const int64_t mcp = gpx_round_up(mc, GPX_TILE);
    double* B = pB;
    const double* Zc = Z->p + j0 * d;
    const int64_t ldb = gpx_skew_ld(mcp);
    // gpx_posterior's own per-chunk step: the values equal GP.evaluate's
    GPX_TRY(gpx_posterior_chunk(ctx, kp, L, X, Zc, mc, B, oop ? pW : nullptr, pal, pmean, nullptr, pout, pkd, ppart));
    double* Wsol = oop ? pW : B;
    {
      ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 8.0 * 5.0 * (double)mc);
      hipLaunchKernelGGL(acq_epilogue_kernel, dim3((unsigned)((mc + ACQ_EPI - 1) / ACQ_EPI)), dim3(ACQ_EPI), 0, ctx->stream, acq,
                         param, (const double*)pmean, (const double*)pkd, (const double*)pout, mc, j0, pcost, pcoef, ppc, ppi);
      GPX_HIP(hipGetLastError());
    }
    if (!grad) continue;
    // beta^T = W^T L^-1 (mcp x np, row stride np) in the buffer W does not occupy (B is consumed by the out-of-place solve)
    double* Bt = Wsol == B ? pW : B;
    GPX_TRY(launch_transpose(ctx, Wsol, np, mcp, ldb, Bt, np));
    if (pT) GPX_TRY(chol_trsm_right_n_leading(ctx, const_cast<gpx_mat*>(L), np, Bt, np, mcp, pT));
    else GPX_TRY(chol_trsm_right_n(ctx, L->p, L->ld, L->aux, Bt, np, mcp, np));
    ProfScope ps(ctx, GPX_PROF_GREEDY, (double)n * (double)mc * (6.0 * (double)d + 25.0),
                 8.0 * ((double)n * (double)mc + (double)n * d));
    GPX_TRY(launch_acq_grad(ctx, kp, X->p, n, Zc, mc, Bt, np, pal, pcoef, pgrad + j0 * d));
  }
  if (best || best_cost) {
    ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 16.0 * (double)nparts);
    hipLaunchKernelGGL(acq_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)ppc, (const int64_t*)ppi, nparts,
                       pbc, pbi);
    GPX_HIP(hipGetLastError());
    if (best) GPX_HIP(hipMemcpyAsync(best, pbi, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (best_cost) GPX_HIP(hipMemcpyAsync(best_cost, pbc, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (cost_host) GPX_HIP(hipMemcpyAsync(cost_host, pcost, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (grad_host) GPX_HIP(hipMemcpyAsync(grad_host, pgrad, (size_t)(M * d * 8), hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// the acquisition entries' own checks in front of the shared prologue
int acq_args(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
             const gpx_mat* Z, int acq, KParams* kp) {
  GPX_ARG(ctx && L && X && Z && alpha, "NULL argument");
  GPX_ARG(acq == GPX_ACQ_UCB || acq == GPX_ACQ_PI || acq == GPX_ACQ_EI, "acq must be GPX_ACQ_UCB, GPX_ACQ_PI or GPX_ACQ_EI");
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

__global__ __launch_bounds__(256) void acq_batch_v_kernel(const double* __restrict__ kd, const double* __restrict__ ss, int64_t M,
                                                          double* __restrict__ v) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < M) v[j] = kd[j] - ss[j];
}

// pick `cur` = candidate s: its column of W_C (w, np), its coordinates along the earlier picks (uc, cur), the pick's scalars,
// and the mask.  Reads mu / v / U only: the state is changed by the NEXT acq_batch_kernel.
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
    const double delta = v[s] + noise, mus = mu[s];
    const double ys = lie == GPX_LIE_BELIEVER ? mus : lie_value;
    sc[SC_DELTA] = delta;
    sc[SC_MU] = mus;
    sc[SC_LIE] = ys;
    if (track_best && ys > sc[SC_PARAM]) sc[SC_PARAM] = ys;
    sc[SC_LIVE] = delta > 1e-13 * kd[s] ? 1.0 : 0.0;
    mask[s] = 1;
  }
}

// One pass over the candidates: (upd) condition mu, v on the pick `cur` = candidate s and store its row U[cur]; then the costs
// under the mask (NaN for a picked candidate) and one arg-min partial per block.  Only j < M is touched: the padding columns of
// W_C / U never enter a result.
__global__ __launch_bounds__(ACQ_EPI) void acq_batch_kernel(KParams kp, int acq, const double* __restrict__ Cp, int64_t M,
                                                            int upd, int64_t s, int cur, const double* __restrict__ sc,
                                                            const double* __restrict__ uc, const double* __restrict__ hdot,
                                                            double* __restrict__ U, int64_t ldu, double* __restrict__ mu,
                                                            double* __restrict__ v, const int* __restrict__ mask,
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
        double acc = kpair(kp, Cp + s * kp.d, Cp + j * kp.d) - hdot[j];
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
    double c = acq_cost(acq, sc[SC_PARAM], m, var, &a, &b);
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

int acq_batch_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha, const gpx_mat* Cm,
                   double noise, int acq, double param, int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx,
                   double* out_cost, double* out_lie, double* all_costs) {
  const int64_t n = L->rows, np = L->prows, M = Cm->rows, d = kp.d;
  const int64_t Mp = gpx_round_up(M, GPX_TILE), ld = gpx_skew_ld(Mp);
  // the solve of gpx_acq: in place below 2048 training points, above out of place through the block inverses, the cross matrix
  // chunk by chunk into the resident W_C
  const bool oop = np >= 2048;
  const int64_t mcmax = gpx_round_up(gpx_eval_chunk(np), GPX_TILE);
  const int64_t mcw = Mp < mcmax ? Mp : mcmax, ldb = gpx_skew_ld(mcw);
  const int64_t bytesW = np * ld * 8, bytesB = oop ? np * ldb * 8 : 0, bytesU = q * Mp * 8, bytesM = Mp * 8;
  const int64_t bytes_part = colreduce_partial_elems(np, Mp) * 8 + 8;
  const int64_t nparts = (M + ACQ_EPI - 1) / ACQ_EPI;
  const int64_t bytes_w = (np > q ? np : q) * 8;
  double *pW = nullptr, *pB = nullptr, *pU = nullptr, *pal = nullptr, *pmu = nullptr, *pv = nullptr, *pkd = nullptr, *pss = nullptr;
  double *ppart = nullptr, *pcost = nullptr, *ppc = nullptr, *pbc = nullptr, *psc = nullptr, *puc = nullptr, *pw = nullptr;
  int64_t *ppi = nullptr, *pbi = nullptr;
  int* pmask = nullptr;
  Scratch sc(ctx);
  const dim3 gEpi((unsigned)nparts), gM((unsigned)((M + 255) / 256));
  const dim3 gPick((unsigned)(((np > q ? np : q) + 255) / 256));
  GPX_TRY(sc.get(bytesW, &pW));
  if (oop) GPX_TRY(sc.get(bytesB, &pB));
  GPX_TRY(sc.get(bytesU, &pU));
  GPX_TRY(sc.get(np * 8, &pal));
  GPX_TRY(sc.get(bytesM, &pmu));
  GPX_TRY(sc.get(bytesM, &pv));
  GPX_TRY(sc.get(bytesM, &pkd));
  GPX_TRY(sc.get(bytesM, &pss));    // |W_C[:, j]|^2 at the set-up, then h of every pick
  GPX_TRY(sc.get(bytes_part, &ppart));
  GPX_TRY(sc.get(M * 8, &pcost));
  GPX_TRY(sc.get(nparts * 8, &ppc));
  GPX_TRY(sc.get(nparts * 8, &ppi));
  GPX_TRY(sc.get(8, &pbc));
  GPX_TRY(sc.get(8, &pbi));
  GPX_TRY(sc.get(SC_N * 8, &psc));
  GPX_TRY(sc.get(q * 8, &puc));
  GPX_TRY(sc.get(bytes_w, &pw));
  GPX_TRY(sc.get(Mp * 4, &pmask));
  double sc0[SC_N] = {0.0, 0.0, 0.0, param, 0.0, 0.0, 0.0, 0.0};
  GPX_HIP(hipMemsetAsync(pal, 0, (size_t)np * 8, ctx->stream));
  GPX_HIP(hipMemcpyAsync(pal, alpha, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  GPX_HIP(hipMemsetAsync(pmask, 0, (size_t)Mp * 4, ctx->stream));
  GPX_HIP(hipMemcpyAsync(psc, sc0, sizeof(sc0), hipMemcpyHostToDevice, ctx->stream));
  double *Wc = pW, *U = pU, *mu = pmu, *v = pv, *hd = pss;
  // ---- set-up: the posterior pass with W kept.  Not gpx_posterior_chunk: the solve lands in the resident W_C with ITS row
  // stride, and the squares are reduced once over all of W_C ----
  for (int64_t j0 = 0; j0 < Mp; j0 += mcw) {
    const int64_t mcp = (Mp - j0) < mcw ? (Mp - j0) : mcw;
    const int64_t mc = (M - j0) < mcp ? (M - j0) : mcp;
    double* B = oop ? pB : Wc + j0;
    const int64_t ldc = oop ? gpx_skew_ld(mcp) : ld;
    GPX_TRY(launch_kfill(ctx, kp, X->p, n, Cm->p + j0 * d, mc, 0, nullptr, 0, 0.0, B, np, mcp, ldc));
    GPX_TRY(launch_colreduce(ctx, B, ldc, n, mcp, pal, mu + j0, ppart));
    if (oop) GPX_TRY(chol_trsm_left_oop(ctx, const_cast<gpx_mat*>(L), B, ldc, Wc + j0, ld, mcp));
    else GPX_TRY(chol_trsm_left(ctx, L->p, L->ld, L->aux, B, ldc, np, mcp));
  }
  GPX_TRY(launch_colreduce(ctx, Wc, ld, n, Mp, nullptr, hd, ppart));
  GPX_TRY(launch_kdiag(ctx, kp, Cm->p, M, pkd));
  hipLaunchKernelGGL(acq_batch_v_kernel, gM, dim3(256), 0, ctx->stream, (const double*)pkd, (const double*)hd, M, v);
  GPX_HIP(hipGetLastError());
  // ---- the picks ----
  int64_t s = -1;
  for (int64_t t = 0; t < q; ++t) {
    {
      ProfScope ps(ctx, GPX_PROF_GREEDY, 0.0, 8.0 * (double)M * (6.0 + (double)t));
      hipLaunchKernelGGL(acq_batch_kernel, gEpi, dim3(ACQ_EPI), 0, ctx->stream, kp, acq, (const double*)Cm->p, M, t > 0 ? 1 : 0,
                         s, (int)(t - 1), (const double*)psc, (const double*)puc, (const double*)hd, U, Mp, mu, v,
                         (const int*)pmask, pcost, ppc, ppi);
      hipLaunchKernelGGL(acq_argmin_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)ppc, (const int64_t*)ppi, nparts,
                         pbc, pbi);
    }
    double c = 0.0;
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipMemcpyAsync(&s, pbi, 8, hipMemcpyDeviceToHost, ctx->stream));
    GPX_HIP(hipMemcpyAsync(&c, pbc, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (all_costs) GPX_HIP(hipMemcpyAsync(all_costs + t * M, pcost, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    GPX_HIP(hipStreamSynchronize(ctx->stream));
    if (s < 0 || s >= M) {
      gpx_set_error("acq batch: pick %lld of %lld: no candidate has a non-NaN cost", (long long)(t + 1), (long long)q);
      return -1;
    }
    out_idx[t] = s;
    if (out_cost) out_cost[t] = c;
    if (t + 1 == q && !out_lie) break;
    hipLaunchKernelGGL(acq_pick_kernel, gPick, dim3(256), 0, ctx->stream, (const double*)Wc, ld, np, s, (const double*)U, Mp,
                       (int)t, (const double*)mu, (const double*)v, (const double*)pkd, noise, lie, lie_value, track_best,
                       psc, puc, pw, pmask);
    GPX_HIP(hipGetLastError());
    if (out_lie) GPX_HIP(hipMemcpyAsync(out_lie + t, psc + SC_LIE, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (t + 1 == q) break;
    GPX_TRY(launch_colreduce(ctx, Wc, ld, n, Mp, pw, hd, ppart));
  }
  return 0;
}

}  // namespace

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

}  // extern "C"
