// Pathwise posterior sampling (Matheron's rule; Wilson et al. 2020) -- gfx950.
//
// A posterior draw is a FUNCTION: a random-feature draw of the prior plus a kernel-basis update from the resident factor,
//     f~_s(z) = sum_j c_sj cos(omega_j . z + b_j),   c = sqrt(2 sig / L) w                       (prior path, L features)
//     V       = alpha - (K + noise I)^-1 (f~(X) + eps)                                           (update weights, S x N)
//     f_s(z)  = f~_s(z) + sum_i v_si k(x_i, z)                                                   (posterior path)
// so it can be evaluated at any number of points afterwards, in chunks, and differentiated.  The sampler's two rules hold here
// too: no random numbers are made on the device (omega, b, w and eps come from the caller, so a result is a deterministic
// function of its arguments), and only the stationary kernels are served (the frequencies are draws of their spectral density,
// made on the host).
//
// Resident state (gpx_paths): G, R x (d + 1), the GENERATORS -- rows [0, Lp) hold (omega_j, b_j), rows [Lp, Lp + Np) hold (x_i, 0) --
// and Ct, R x Sp, the COEFFICIENTS transposed -- rows [0, Lp) hold c, rows [Lp, Lp + Np) hold V -- with Lp, Np the counts rounded
// up to PT_R and Sp = S rounded up to 16, all padding 0.  Nothing N x N and nothing N x M.
//
// paths_eval_kernel, the hot path: out[s][m] = sum_r Ct[r][s] g(r, m) as ONE product on v_mfma_f64_16x16x4_f64 whose large operand
// g (cos(omega_r . z_m + b_r) over the features, then k(x_r, z_m) over the training points) is GENERATED IN REGISTERS and never
// stored.  In that instruction's B layout lane l holds B[k = l >> 4][col = l & 15]: a wave owns 16 points, lane l keeps the
// coordinates of point (l & 15) in registers and per step evaluates exactly one g(r0 + (l >> 4), m) -- its B operand.  The A
// operand is the 16-path x 4-r slab of Ct, staged through LDS in tiles of PT_R rows (row stride PT_CS = 80 doubles: the k groups
// of a half-wave's read fall on disjoint bank halves); a generated g is reused by all (up to four) 16-path blocks of the
// workgroup's 64 paths, which is what amortises the exp / cos.  k is formed from coordinate differences, (x - z) scale first, as
// kpair does: no centring and no exact-form gate.
// Determinism: the accumulator of (s, m) -- C/D map of the f64 instruction: row = (lane >> 4) + 4 reg, col = lane & 15 -- takes the
// WHOLE range of r in ascending steps of 4 inside one wave: no split, no atomics; a step's four products depend on row s of Ct
// and on z_m alone.  So a value's bits depend neither on S, nor on the other paths or points of the call, nor on the chunking of
// Z.  Padding contributes +0 exactly: padded coefficients are 0 and a padded generator row is all zeros (cos(0) = 1, k(0, z) <=
// sig), pad lanes evaluate at z = 0 -- nothing there is NaN or Inf -- and their results are not stored.
//
// paths_grad_kernel: one workgroup per point, thread t takes r = t, t + 256, ... in ascending order, block_sum_256 adds the 256
// partial sums in a fixed tree.  The kernel derivative is radial_pair's factor times the coordinate difference: nothing divides
// by the distance, and at z = x_i the term is exactly 0.
//
// VFE models (gpx_vfe_paths_create; the entry and its argument checks are in fitc.hip, where the struct is).  Nothing in the two
// kernels knows that the point block holds TRAINING points: a path of the variational posterior is the same resident object with the
// nu inducing points S in the point block and other weights (decoupled sampling, Wilson et al. 2020, section 4.2).  With Quu = K(S,S)
// + noise I = Lu Lu^T (the inducing variables are u = f(S) + eps), A = Quu + Kuf Kfu / noise = La La^T and beta_u = Quu^-1 Kuf alpha,
// Matheron's rule on (f, u) with u ~ q(u) = N(Quu beta_u, Quu A^-1 Quu) gives
//     V = 1 beta_u^T - (F~_S + eps_u) Quu^-1 + Xi2 La^-1                   (S_paths x nu;  F~_S[s][u] = f~_s(s_u), eps_u = sqrt(noise) Xi1)
// -- zero draws: the predictor's mean; exact prior in place of the features: covariance k - k_u^T Quu^-1 k_u' + k_u^T A^-1 k_u', the
// predictor's.  The build is on the device for all paths at once: f~ at S by launch_paths_eval over the feature rows, eps_u added,
// both sweeps against Lu and the one against La as blocked RIGHT solves on the (S_paths padded to 128) x nup matrices
// (chol_trsm_right, chol_trsm_right_n: O(nu^2) per path, nothing of size N), and vfe_paths_setv_kernel writes V into Ct.  No atomics;
// a path's weights depend on its own row of the draws alone.
#include "gpx_device.h"
#include <math.h>
#include <vector>

struct gpx_paths {
  int64_t S, Sp, nfeat, Lp, n, Np;
  KParams kp;
  double* G;    // (Lp + Np) x (d + 1)
  double* Ct;   // (Lp + Np) x Sp
  int64_t G_bytes, Ct_bytes;
};

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int PT_R = 32;    // rows of G / Ct per LDS tile (the feature block and the point block are padded to it)
constexpr int PT_M = 64;    // points per workgroup: 16 per wave
constexpr int PT_S = 64;    // paths per workgroup: up to four 16-path blocks share one generated operand
constexpr int PT_CS = 80;   // row stride of the coefficient tile in LDS

template <int KIND, int DMAX>
__global__ __launch_bounds__(256) void paths_eval_kernel(KParams kp, const double* __restrict__ G, const double* __restrict__ Ct,
                                                         int64_t Sp, int64_t Lp, int64_t R, const double* __restrict__ Z,
                                                         int64_t mc, int64_t S, double* __restrict__ out, int64_t ldo) {
  __shared__ double Cs[PT_R * PT_CS];
  __shared__ double Gs[PT_R * (DMAX + 1)];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 15, kq = lane >> 4, d = kp.d, gs = d + 1;
  const int64_t s0 = (int64_t)blockIdx.y * PT_S;
  const int ncol = (Sp - s0) < PT_S ? (int)(Sp - s0) : PT_S;   // a multiple of 16
  const int nsb = ncol >> 4;
  const int64_t m = (int64_t)blockIdx.x * PT_M + wave * 16 + col;
  double z[DMAX];
#pragma unroll
  for (int l = 0; l < DMAX; ++l) z[l] = (l < d && m < mc) ? Z[m * d + l] : 0.0;
  d4 acc[4];
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) acc[sb] = d4{0.0, 0.0, 0.0, 0.0};
  for (int64_t r0 = 0; r0 < R; r0 += PT_R) {
    __syncthreads();   // the previous tile is consumed
    for (int e = t; e < PT_R * ncol; e += 256) {
      const int r = e / ncol, c = e - r * ncol;
      Cs[r * PT_CS + c] = Ct[(r0 + r) * Sp + s0 + c];
    }
    for (int e = t; e < PT_R * gs; e += 256) {
      const int r = e / gs, c = e - r * gs;
      Gs[r * (DMAX + 1) + c] = G[(r0 + r) * gs + c];
    }
    __syncthreads();
    const bool feat = r0 < Lp;   // (uniform: Lp is a multiple of PT_R)
    for (int rr = 0; rr < PT_R; rr += 4) {
      const double* __restrict__ g = Gs + (rr + kq) * (DMAX + 1);
      double a = 0.0, b;
      if (feat) {
#pragma unroll
        for (int l = 0; l < DMAX; ++l)
          if (l < d) a = fma(g[l], z[l], a);
        b = cos(a + g[d]);
      } else {
#pragma unroll
        for (int l = 0; l < DMAX; ++l)
          if (l < d) {
            const double e = (g[l] - z[l]) * kp.scale[l];
            a = fma(e, e, a);
          }
        if (KIND == GPX_K_SE) {
          b = kp.sig * exp(-0.5 * a);
        } else {
          const double tt = sqrt(a);
          b = KIND == GPX_K_MATERN32 ? kp.sig * (1.0 + tt) * exp(-tt) : kp.sig * (1.0 + tt + a * (1.0 / 3.0)) * exp(-tt);
        }
      }
      const double* __restrict__ ca = Cs + (rr + kq) * PT_CS + col;
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
        if (sb < nsb) acc[sb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[sb * 16], b, acc[sb], 0, 0, 0);
    }
  }
  if (m < mc) {
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t s = s0 + sb * 16 + kq + 4 * v;   // the f64 C/D map: row = (lane >> 4) + 4 reg
        if (sb < nsb && s < S) out[s * ldo + m] = acc[sb][v];
      }
  }
}

// F[s][i] += eps[s][i]  (F: row stride ld; eps: S x n)
__global__ __launch_bounds__(256) void paths_addeps_kernel(double* __restrict__ F, int64_t ld, const double* __restrict__ eps,
                                                           int64_t n, int64_t S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) F[s * ld + i] += eps[s * n + i];
}

// V = alpha - sol, into the point block of Ct (sol: S rows of stride ld)
__global__ __launch_bounds__(256) void paths_setv_kernel(const double* __restrict__ sol, int64_t ld, const double* __restrict__ alpha,
                                                         int64_t n, int64_t S, double* __restrict__ Ct, int64_t Sp, int64_t Lp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) Ct[(Lp + i) * Sp + s] = alpha[i] - sol[s * ld + i];
}

// out (S x n) = the point block of Ct, transposed
__global__ __launch_bounds__(256) void paths_getv_kernel(const double* __restrict__ Ct, int64_t Sp, int64_t Lp, int64_t n, int64_t S,
                                                         double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) out[s * n + i] = Ct[(Lp + i) * Sp + s];
}

// One workgroup per point p of path s = path[p]: value and gradient of f_s at z_p.
//   d/dz_l of the feature term: -c_sj sin(omega_j . z + b_j) omega_jl;   of the kernel term: v_si f (x_i - z)_l scale_l^2 [sig, sig / 3]
// with f = radial_pair's factor (SE: k itself; Matern 3/2: e^-t; Matern 5/2: (1 + t) e^-t).
template <int KIND, int DMAX>
__global__ __launch_bounds__(256) void paths_grad_kernel(KParams kp, const double* __restrict__ G, const double* __restrict__ Ct,
                                                         int64_t Sp, int64_t Lp, int64_t nfeat, int64_t n,
                                                         const double* __restrict__ Zp, const int64_t* __restrict__ path,
                                                         double* __restrict__ val, double* __restrict__ grad) {
  __shared__ double red[256];
  const int t = threadIdx.x, d = kp.d, gs = d + 1;
  const int64_t p = blockIdx.x, s = path[p];
  double zs[DMAX], gf[DMAX], gk[DMAX];
#pragma unroll
  for (int l = 0; l < DMAX; ++l) {
    zs[l] = l < d ? Zp[p * d + l] : 0.0;
    gf[l] = 0.0;
    gk[l] = 0.0;
  }
  double v = 0.0;
  for (int64_t j = t; j < nfeat; j += 256) {
    const double* __restrict__ g = G + j * gs;
    const double c = Ct[j * Sp + s];
    double a = 0.0;
#pragma unroll
    for (int l = 0; l < DMAX; ++l)
      if (l < d) a = fma(g[l], zs[l], a);
    a += g[d];
    double sn, cs;
    sincos(a, &sn, &cs);
    v = fma(c, cs, v);
    const double w = -c * sn;
#pragma unroll
    for (int l = 0; l < DMAX; ++l)
      if (l < d) gf[l] = fma(w, g[l], gf[l]);
  }
  for (int64_t i = t; i < n; i += 256) {
    double diff[DMAX];
    const double f = radial_pair<KIND, DMAX>(kp, G + (Lp + i) * gs, zs, diff);   // diff = x_i - z
    const double vi = Ct[(Lp + i) * Sp + s];
    double k = f;
    if (KIND != GPX_K_SE) {
      double r2 = 0.0;
#pragma unroll
      for (int l = 0; l < DMAX; ++l) {
        const double e = diff[l] * kp.scale[l];   // (diff is 0 from d on)
        r2 = fma(e, e, r2);
      }
      const double tt = sqrt(r2);
      k = KIND == GPX_K_MATERN32 ? kp.sig * (1.0 + tt) * exp(-tt) : kp.sig * (1.0 + tt + r2 * (1.0 / 3.0)) * exp(-tt);
    }
    v = fma(vi, k, v);
    const double w = vi * f;
#pragma unroll
    for (int l = 0; l < DMAX; ++l) gk[l] = fma(w, diff[l], gk[l]);
  }
#pragma unroll
  for (int l = 0; l < DMAX; ++l) {
    if (l < d) {   // (uniform)
      double c = kp.scale[l] * kp.scale[l];
      if (KIND == GPX_K_MATERN32) c *= kp.sig;
      if (KIND == GPX_K_MATERN52) c *= kp.sig / 3.0;
      block_sum_256(red, fma(c, gk[l], gf[l]));
      if (t == 0) grad[p * d + l] = red[0];
      __syncthreads();
    }
  }
  if (val) {   // (uniform)
    block_sum_256(red, v);
    if (t == 0) val[p] = red[0];
  }
}

// out (S rows of stride ldo) = the paths at the mc points Zc, with the generator rows [0, R) (R = Lp: the prior part alone)
int launch_paths_eval(gpx_ctx* ctx, const gpx_paths* ps, int64_t R, const double* Zc, int64_t mc, double* out, int64_t ldo) {
  const dim3 grid((unsigned)((mc + PT_M - 1) / PT_M), (unsigned)((ps->Sp + PT_S - 1) / PT_S));
  ProfScope pf(ctx, GPX_PROF_KCROSS, 2.0 * (double)ps->Sp * (double)R * (double)mc, 8.0 * (double)ps->S * (double)mc);
#define GPX_PATHS_EVAL(K_, D_)                                                                                                   \
  hipLaunchKernelGGL((paths_eval_kernel<K_, D_>), grid, dim3(256), 0, ctx->stream, ps->kp, (const double*)ps->G,                 \
                     (const double*)ps->Ct, ps->Sp, ps->Lp, R, Zc, mc, ps->S, out, ldo)
  GPX_RADIAL_DISPATCH(ps->kp.kind, ps->kp.d, GPX_PATHS_EVAL);
#undef GPX_PATHS_EVAL
  GPX_HIP(hipGetLastError());
  return 0;
}

const char* const kPointsMsg = "point sets must be unpadded (n x d)";

// What the two constructors share: G and Ct of a new object (its shape fields set), all 0, with the feature block uploaded -- G
// rows [0, Lp) = (omega_j, b_j), Ct rows [0, Lp) = c = sqrt(2 sig / L) w.  hG, hC: the caller's (empty) host images, which must
// outlive the queued copies.
int paths_begin(gpx_ctx* ctx, gpx_paths* ps, const double* omega, const double* phase, const double* w, std::vector<double>& hG,
                std::vector<double>& hC) {
  const int d = ps->kp.d;
  const int64_t S = ps->S, Sp = ps->Sp, nfeat = ps->nfeat, Lp = ps->Lp, gs = d + 1, R = Lp + ps->Np;
  hG.assign((size_t)(Lp * gs), 0.0);
  hC.assign((size_t)(Lp * Sp), 0.0);
  const double amp = sqrt(2.0 * ps->kp.sig / (double)nfeat);
  for (int64_t j = 0; j < nfeat; ++j) {
    for (int l = 0; l < d; ++l) hG[(size_t)(j * gs + l)] = omega[j * d + l];
    hG[(size_t)(j * gs + d)] = phase[j];
    for (int64_t s = 0; s < S; ++s) hC[(size_t)(j * Sp + s)] = amp * w[s * nfeat + j];
  }
  GPX_TRY(gpx_dev_alloc(ctx, R * gs * 8, &ps->G));
  ps->G_bytes = R * gs * 8;
  GPX_TRY(gpx_dev_alloc(ctx, R * Sp * 8, &ps->Ct));
  ps->Ct_bytes = R * Sp * 8;
  GPX_HIP(hipMemsetAsync(ps->G, 0, (size_t)ps->G_bytes, ctx->stream));
  GPX_HIP(hipMemsetAsync(ps->Ct, 0, (size_t)ps->Ct_bytes, ctx->stream));
  GPX_HIP(hipMemcpyAsync(ps->G, hG.data(), hG.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  GPX_HIP(hipMemcpyAsync(ps->Ct, hC.data(), hC.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// T (Sq x ld, Sq = S padded to 128) <- the S x n host draws, 0 elsewhere (a NULL host array: all 0)
int paths_stage_rows(gpx_ctx* ctx, const double* host, int64_t S, int64_t n, double* T, int64_t Sq, int64_t ld) {
  GPX_HIP(hipMemsetAsync(T, 0, (size_t)(Sq * ld * 8), ctx->stream));
  if (host)
    GPX_HIP(hipMemcpy2DAsync(T, (size_t)ld * 8, host, (size_t)n * 8, (size_t)n * 8, (size_t)S, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// V = 1 bu^T - T + Q into the point block of Ct (T, Q: S rows of stride ld; bu: n)
__global__ __launch_bounds__(256) void vfe_paths_setv_kernel(const double* __restrict__ T, const double* __restrict__ Q, int64_t ld,
                                                             const double* __restrict__ bu, int64_t n, int64_t S,
                                                             double* __restrict__ Ct, int64_t Sp, int64_t Lp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double b = bu[i];
  for (int64_t s = blockIdx.y; s < S; s += gridDim.y) Ct[(Lp + i) * Sp + s] = (b - T[s * ld + i]) + Q[s * ld + i];
}

}  // namespace

// (gpx_internal.h; the header comment has the formulas)
int vfe_paths_create_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* Sm, const double* coeff, const double* omega,
                          const double* phase, int64_t nfeat, const double* w, const double* eps_u, const double* xi_q, int64_t S,
                          gpx_paths** out) {
  FitcView v;
  fitc_view(f, &v);
  const KParams& kp = *v.kp;
  const int d = kp.d;
  const int64_t nu = v.nu, nup = v.nup, gs = d + 1;
  const int64_t Sp = gpx_round_up(S, 16), Sq = gpx_round_up(S, GPX_TILE), Lp = gpx_round_up(nfeat, PT_R), Np = gpx_round_up(nu, PT_R);
  const int64_t ld = gpx_skew_ld(nup);
  std::vector<double> hG, hC;   // (declared first, as in gpx_paths_create)
  Held<gpx_paths, gpx_paths_free> ps(ctx, new gpx_paths{S, Sp, nfeat, Lp, nu, Np, kp, nullptr, nullptr, 0, 0});
  GPX_TRY(paths_begin(ctx, ps.get(), omega, phase, w, hG, hC));
  GPX_HIP(hipMemcpy2DAsync(ps->G + Lp * gs, (size_t)gs * 8, Sm->p, (size_t)Sm->ld * 8, (size_t)d * 8, (size_t)nu,
                           hipMemcpyDeviceToDevice, ctx->stream));
  double *T, *Q, *F, *bu;
  Scratch sc(ctx);
  GPX_TRY(sc.get(Sq * ld * 8, &T));
  GPX_TRY(sc.get(Sq * ld * 8, &Q));
  GPX_TRY(sc.get(S * nu * 8, &F));
  GPX_TRY(vfe_beta_u(ctx, f, coeff, sc, &bu));
  GPX_TRY(paths_stage_rows(ctx, eps_u, S, nu, T, Sq, ld));
  GPX_TRY(paths_stage_rows(ctx, xi_q, S, nu, Q, Sq, ld));
  // T = f~(S) + eps_u: the prior paths at S by the evaluation kernel itself (generator rows [0, Lp) only), added to the staged draw
  GPX_TRY(launch_paths_eval(ctx, ps.get(), Lp, Sm->p, nu, F, nu));
  const dim3 grid((unsigned)((nu + 255) / 256), (unsigned)(S < 1024 ? S : 1024));
  hipLaunchKernelGGL(paths_addeps_kernel, grid, dim3(256), 0, ctx->stream, T, ld, (const double*)F, nu, S);
  GPX_HIP(hipGetLastError());
  // T <- T Lu^-T Lu^-1 = T Quu^-1;  Q <- Xi2 La^-1 (row s: (La^-T xi2_s)^T).  The padding of both stays 0: the factors' is the identity.
  GPX_TRY(chol_trsm_right(ctx, v.Lu->p, v.Lu->ld, v.Lu->aux, T, ld, Sq, nup));
  GPX_TRY(chol_trsm_right_n(ctx, v.Lu->p, v.Lu->ld, v.Lu->aux, T, ld, Sq, nup));
  GPX_TRY(chol_trsm_right_n(ctx, v.La->p, v.La->ld, v.La->aux, Q, ld, Sq, nup));
  hipLaunchKernelGGL(vfe_paths_setv_kernel, grid, dim3(256), 0, ctx->stream, (const double*)T, (const double*)Q, ld,
                     (const double*)bu, nu, S, ps->Ct, Sp, Lp);
  GPX_HIP(hipGetLastError());
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  *out = ps.release();
  return 0;
}

extern "C" {

int gpx_paths_free(gpx_ctx* ctx, gpx_paths* ps) {
  if (!ps) return 0;
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  (void)hipStreamSynchronize(ctx->stream);
  if (ps->G) gpx_dev_release(ctx, ps->G, ps->G_bytes);
  if (ps->Ct) gpx_dev_release(ctx, ps->Ct, ps->Ct_bytes);
  delete ps;
  return 0;
}

int gpx_paths_shape(const gpx_paths* ps, int64_t* S, int64_t* nfeat, int64_t* n) {
  GPX_ARG(ps != nullptr, "paths is NULL");
  if (S) *S = ps->S;
  if (nfeat) *nfeat = ps->nfeat;
  if (n) *n = ps->n;
  return 0;
}

int gpx_paths_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const double* alpha, const double* omega, const double* phase, int64_t nfeat, const double* w,
                     const double* eps, int64_t S, gpx_paths** out) {
  GPX_ARG(ctx && omega && phase && w && out, "NULL argument");
  GPX_ARG(kind == GPX_K_SE || kind == GPX_K_MATERN32 || kind == GPX_K_MATERN52,
          "paths: stationary kernels only (squared exponential, Matern 3/2, Matern 5/2)");
  bool prior;
  GPX_TRY(gpx_model_or_prior(L, X, alpha, "paths: L, X and alpha are given together, or all three NULL (prior paths)", &prior));
  GPX_ARG(nfeat >= 1, "paths: needs at least one feature");
  GPX_ARG(S >= 1, "paths: needs at least one path");
  KParams kp;
  if (prior) GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  else GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, nullptr, nullptr, kPointsMsg, &kp));
  const int64_t n = prior ? 0 : L->rows, gs = d + 1;
  const int64_t Sp = gpx_round_up(S, 16), Lp = gpx_round_up(nfeat, PT_R), Np = gpx_round_up(n, PT_R);
  // host images of the feature block (declared first: the holder and the scratch below synchronise before these go)
  std::vector<double> hG, hC;
  Held<gpx_paths, gpx_paths_free> ps(ctx, new gpx_paths{S, Sp, nfeat, Lp, n, Np, kp, nullptr, nullptr, 0, 0});
  GPX_TRY(paths_begin(ctx, ps.get(), omega, phase, w, hG, hC));
  if (!prior) {
    const int64_t np = L->prows;
    GPX_HIP(hipMemcpy2DAsync(ps->G + Lp * gs, (size_t)gs * 8, X->p, (size_t)X->ld * 8, (size_t)d * 8, (size_t)n,
                             hipMemcpyDeviceToDevice, ctx->stream));
    double *Fx, *pal, *deps = nullptr, *pscr;
    Scratch sc(ctx);
    GPX_TRY(sc.get(S * np * 8, &Fx));
    GPX_TRY(sc.get(np * 8, &pal));
    GPX_TRY(sc.get(chol_potrs_scratch_bytes(np), &pscr));
    if (eps) GPX_TRY(sc.get(S * n * 8, &deps));
    GPX_HIP(hipMemsetAsync(Fx, 0, (size_t)(S * np * 8), ctx->stream));
    GPX_HIP(hipMemcpyAsync(pal, alpha, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    // the prior paths at X by the evaluation kernel itself (the update weights do not take part: generator rows [0, Lp) only)
    GPX_TRY(launch_paths_eval(ctx, ps.get(), Lp, X->p, n, Fx, np));
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(S < 1024 ? S : 1024));
    if (eps) {
      GPX_HIP(hipMemcpyAsync(deps, eps, (size_t)(S * n * 8), hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(paths_addeps_kernel, grid, dim3(256), 0, ctx->stream, Fx, np, (const double*)deps, n, S);
      GPX_HIP(hipGetLastError());
    }
    // (K + noise I)^-1 (f~(X) + eps), right-hand side by right-hand side: gpx_potrs_dev's solve on each padded row
    for (int64_t s = 0; s < S; ++s) GPX_TRY(chol_potrs(ctx, const_cast<gpx_mat*>(L), Fx + s * np, pscr));
    hipLaunchKernelGGL(paths_setv_kernel, grid, dim3(256), 0, ctx->stream, (const double*)Fx, np, (const double*)pal, n, S,
                       ps->Ct, Sp, Lp);
    GPX_HIP(hipGetLastError());
  }
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  *out = ps.release();
  return 0;
}

int gpx_paths_eval(gpx_ctx* ctx, const gpx_paths* ps, const gpx_mat* Z, double* out, int sign, int64_t* best_idx,
                   double* best_val) {
  GPX_ARG(ctx && ps && Z, "NULL argument");
  GPX_ARG(sign == 0 || sign == 1 || sign == -1, "paths: sign must be +1 (minimum), -1 (maximum) or 0 (no pick)");
  GPX_ARG(sign == 0 || best_idx, "paths: a pick needs best_idx");
  GPX_ARG(out || sign != 0, "paths: neither values nor a pick asked for");
  const int d = ps->kp.d;
  GPX_ARG(Z->cols == d && Z->pcols == d, kPointsMsg);
  GPX_ARG(Z->rows >= 1, "paths: needs at least one point");
  KParams kz = ps->kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kz, Z));   // (refuses a non-finite coordinate; the centre it computes is not used here)
  const int64_t M = Z->rows, S = ps->S, R = ps->Lp + ps->Np;
  const ChunkRange cr(M, gpx_eval_chunk(ps->Sp));
  {
    double *outd, *dval = nullptr;
    int64_t* didx = nullptr;
    Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
    GPX_TRY(sc.get(S * cr.widest * 8, &outd));
    if (sign != 0) {
      GPX_TRY(sc.get(S * 8, &didx));
      GPX_TRY(sc.get(S * 8, &dval));
    }
    for (const ChunkRange::Step c : cr) {
      const int64_t m0 = c.j0, mc = c.mc;
      GPX_TRY(launch_paths_eval(ctx, ps, R, Z->p + m0 * d, mc, outd, mc));
      if (out)
        GPX_HIP(hipMemcpy2DAsync(out + m0, (size_t)M * 8, outd, (size_t)mc * 8, (size_t)mc * 8, (size_t)S, hipMemcpyDeviceToHost,
                                 ctx->stream));
      if (sign != 0) {
        ProfScope pf(ctx, GPX_PROF_GREEDY, 0.0, 8.0 * (double)S * (double)mc);
        GPX_TRY(launch_row_argbest(ctx, outd, S, mc, mc, m0, sign, m0 == 0 ? 1 : 0, didx, dval));
      }
    }
    if (sign != 0) {
      GPX_HIP(hipMemcpyAsync(best_idx, didx, (size_t)S * 8, hipMemcpyDeviceToHost, ctx->stream));
      if (best_val) GPX_HIP(hipMemcpyAsync(best_val, dval, (size_t)S * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  if (sign != 0) gpx_row_argbest_nan(S, best_idx, best_val);
  return 0;
}

int gpx_paths_grad(gpx_ctx* ctx, const gpx_paths* ps, const gpx_mat* Zp, const int64_t* path, double* val, double* grad) {
  GPX_ARG(ctx && ps && Zp && path && grad, "NULL argument");
  const int d = ps->kp.d;
  GPX_ARG(Zp->cols == d && Zp->pcols == d, kPointsMsg);
  GPX_ARG(Zp->rows >= 1, "paths: needs at least one point");
  const int64_t P = Zp->rows;
  for (int64_t p = 0; p < P; ++p) GPX_ARG(path[p] >= 0 && path[p] < ps->S, "paths: a path index is outside [0, S)");
  KParams kz = ps->kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kz, Zp));
  int64_t* dpath;
  double *dgrad, *dvalp = nullptr;
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(sc.get(P * 8, &dpath));
  GPX_TRY(sc.get(P * d * 8, &dgrad));
  if (val) GPX_TRY(sc.get(P * 8, &dvalp));
  GPX_HIP(hipMemcpyAsync(dpath, path, (size_t)P * 8, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope pf(ctx, GPX_PROF_GREEDY, 2.0 * (double)P * (double)(ps->nfeat + ps->n) * (double)(d + 1), 0.0);
#define GPX_PATHS_GRAD(K_, D_)                                                                                                   \
  hipLaunchKernelGGL((paths_grad_kernel<K_, D_>), dim3((unsigned)P), dim3(256), 0, ctx->stream, ps->kp, (const double*)ps->G,    \
                     (const double*)ps->Ct, ps->Sp, ps->Lp, ps->nfeat, ps->n, (const double*)Zp->p, (const int64_t*)dpath,       \
                     dvalp, dgrad)
    GPX_RADIAL_DISPATCH(ps->kp.kind, d, GPX_PATHS_GRAD);
#undef GPX_PATHS_GRAD
    GPX_HIP(hipGetLastError());
  }
  GPX_HIP(hipMemcpyAsync(grad, dgrad, (size_t)(P * d * 8), hipMemcpyDeviceToHost, ctx->stream));
  if (val) GPX_HIP(hipMemcpyAsync(val, dvalp, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

int gpx_paths_coeff(gpx_ctx* ctx, const gpx_paths* ps, double* v) {
  GPX_ARG(ctx && ps && v, "NULL argument");
  if (ps->n == 0) return 0;   // prior paths: V is empty
  double* dv;
  Scratch sc(ctx);
  GPX_TRY(sc.get(ps->S * ps->n * 8, &dv));
  const dim3 grid((unsigned)((ps->n + 255) / 256), (unsigned)(ps->S < 1024 ? ps->S : 1024));
  hipLaunchKernelGGL(paths_getv_kernel, grid, dim3(256), 0, ctx->stream, (const double*)ps->Ct, ps->Sp, ps->Lp, ps->n, ps->S, dv);
  GPX_HIP(hipGetLastError());
  GPX_HIP(hipMemcpyAsync(v, dv, (size_t)(ps->S * ps->n * 8), hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

}  // extern "C"
