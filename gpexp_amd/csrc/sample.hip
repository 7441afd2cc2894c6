// Joint posterior sampling and Monte-Carlo q-EI -- gfx950.
//
// The reference draws functions in GP.generateSamples (gp.py:343-371: SVD of the prior covariance, numpy.random inside); these
// entry points draw from the POSTERIOR at M points jointly, pick per draw (Thompson sampling) and score whole q-batches by joint
// expected improvement.  Two rules carry the file:
//   * no random numbers are made here: every call takes the standard-normal base samples Xi from the caller, so a result is a
//     deterministic function of its arguments (two calls agree bit for bit) and the q-EI of different batches is compared on
//     COMMON random numbers;
//   * the covariance is made positive definite by a NUGGET on its diagonal, C + nugget I, and factored with the pivot policy
//     (0, report): no pivot is dropped, a pivot <= 0 is returned as a status > 0 (the drop rule of gpx_greedy_var would divide
//     through pivots that are rounding noise of K(Z,Z) - W^T W).
//
// Sampler (gpx_psampler_*).  mean_j = k_j^T alpha by gpx_posterior's own chunk step; C = K(Z,Z) - W^T W by the sequence of
// gpx_posterior_cov (before the nugget C holds the bits that call returns); F = chol(C + nugget I) through chol_potrf, then
// psampler_finish_kernel writes the strict upper triangle and the identity extension of the padding as 0, and ONE step of
// refinement follows, F <- F + F Phi(F^-1 (Chat - F F^T) F^-T): the leaf of chol_potrf multiplies by explicit inverses of its
// diagonal blocks, which on a covariance whose spectrum reaches down to the nugget leaves |F F^T - Chat| up to 12 (M + 1) u
// sqrt(Chat_ii Chat_jj) (LAPACK: 0.06; measured); the step costs two triangular solves and two products.  The product
// Y = F Xi^T runs on the MFMA path with tri = 1, which reads whole diagonal tiles.  Per element that kernel accumulates in
// ascending k whatever tile size the launch picks; the tile size only moves the END of a row tile's k range, and what lies
// between the two ends is the zero part of F, which adds +0 exactly -- so a sample's bits depend neither on S nor on the chunking
// nor on the other samples of the call.  psampler_epilogue_kernel adds the mean and turns Y (M x S) into sample-major rows;
// launch_row_argbest (reduce.hip) reduces a row to its first minimum / maximum (the smaller index wins a tie).
//
// On a VFE model (gpx_vfe_psampler_create, gpx_vfe_posterior_cov: entries in fitc.hip, bodies here) the mean is taken by
// vfe_posterior_chunk's sequence (gpx_vfe_posterior's bits) and C = (K(Z,Z) - Wu^T Wu) + Wa^T Wa, Wu = Lu^-1 K(S,Z), Wa = La^-1 K(S,Z),
// by posterior_cov_into's steps once per factor under the cross-solve rule (vfe_posterior_cov_into); everything from the nugget on
// is psampler_factor, the one tail both constructors call; here it also MEASURES the residual after the refinement step and repeats
// the step while it is above half the factor contract (`verify`; the dense constructor keeps its one step and its bits).
//
// q-EI (gpx_acq_qei).  cost_b = -(1/S) sum_s max(0, fBest - min_j (mu_bj + (F_b xi_s)_j)), F_b = chol(C_b + nugget I).  The means
// and W = L^-1 K(X, Zb) come from gpx_posterior_chunk, chunked over WHOLE batches; qei_kernel does the rest.  A workgroup owns a
// span of G = 32 / q consecutive batches (G q <= 32 contiguous doubles per row of W: one 256-byte line at most) and
//   1. forms the q (q + 1) / 2 entries of every C_b: rows of W pass through LDS in tiles of 64; entry p is split into nsl row
//      slices (row r belongs to slice r mod nsl), each slice is one fma chain in ascending r, the slices are added in slice order;
//   2. factors C_b + nugget I in LDS, right-looking, a team of T threads per batch, column by column (the column is rounded outward
//      by at most one step, so that a point repeated bit for bit is CERTAIN to meet a pivot <= 0 when the nugget is 0);
//   3. runs the S samples: team thread u takes the samples u, u + T, ..., sums its values PAIRWISE (a binary-counter stack), and
//      the team's T sums go through a halving tree: a summation tree of depth <= ceil(log2 S), no atomics.
// G, T and nsl depend on q alone and every batch is worked with the same arithmetic wherever it sits: permuting the batches
// permutes the costs bit for bit.  A batch whose factorisation meets a pivot <= 0 gets cost NaN and is counted; the arg-min is
// the first minimum among the non-NaN costs (argmin_merge), one partial per workgroup, reduced by gpx_acq's own kernel.
//
// On a VFE model (gpx_vfe_acq_qei: entry in fitc.hip, body vfe_qei_impl here) the means, Wu = Lu^-1 K(S, Zb) and Wa = La^-1 K(S, Zb)
// come from vfe_posterior_chunk and step 1 runs twice, qei_kernel<.., true>: C_b = (k - Wu_b^T Wu_b) + Wa_b^T Wa_b, a SIGNED Gram of two
// factors, each sum by the rule of step 1 over the nu inducing rows; steps 2 and 3 are the same code.  QeiRun holds what the two
// drivers share.
#include "gpx_device.h"
#include <math.h>
#include <vector>

struct gpx_psampler {
  int64_t m, mp;
  gpx_mat* F;          // mp x mp: chol(C + nugget I), strict upper triangle and padding 0
  double* mean;        // mp doubles, 0 on the padding
  int64_t mean_bytes;
};

namespace {

// the context's pivot policy set to (0, report) for a scope; the caller's policy comes back on every exit
struct PolicyScope {
  gpx_ctx* ctx;
  double piv_min;
  int piv_skip;
  explicit PolicyScope(gpx_ctx* c) : ctx(c), piv_min(c->piv_min), piv_skip(c->piv_skip) {
    c->piv_min = 0.0;
    c->piv_skip = 0;
  }
  PolicyScope(const PolicyScope&) = delete;
  PolicyScope& operator=(const PolicyScope&) = delete;
  ~PolicyScope() {
    ctx->piv_min = piv_min;
    ctx->piv_skip = piv_skip;
  }
};

__global__ __launch_bounds__(256) void psampler_nugget_kernel(double* __restrict__ F, int64_t ld, int64_t m, double nugget) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) F[i * ld + i] += nugget;
}

// the factored matrix made a plain lower-triangular operand: 0 above the diagonal and on the whole padding (the unit diagonal of
// the identity extension included).  One thread per element of the mp x mp storage (row = blockIdx.x).
__global__ __launch_bounds__(256) void psampler_finish_kernel(double* __restrict__ F, int64_t ld, int64_t m, int64_t mp) {
  const int64_t j = (int64_t)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
  if (j < mp && (j > i || i >= m || j >= m)) F[i * ld + j] = 0.0;
}

// One step of refinement of the factor, F <- F + F Phi(F^-1 R F^-T) with R = Chat - F F^T (the first-order solution of
// (F + E)(F + E)^T = Chat): Phi keeps the strict lower triangle of its symmetric argument and half of its diagonal.  In place on G.
__global__ __launch_bounds__(256) void psampler_phi_kernel(double* __restrict__ G, int64_t ld, int64_t mp) {
  const int64_t j = (int64_t)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
  if (j < mp) G[i * ld + j] = j > i ? 0.0 : (j == i ? 0.5 * G[i * ld + j] : G[i * ld + j]);
}

// F += Y on the lower triangle of the m x m block
__global__ __launch_bounds__(256) void psampler_addlower_kernel(double* __restrict__ F, int64_t ldf, const double* __restrict__ Y,
                                                                int64_t ldy, int64_t m) {
  const int64_t j = (int64_t)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
  if (i < m && j <= i) F[i * ldf + j] += Y[i * ldy + j];
}

// Xt (mp x scp, row stride scp) = the transpose of the sc x m chunk of base samples, 0 on the padding; 32 x 32 tiles
__global__ __launch_bounds__(256) void psampler_xi_kernel(const double* __restrict__ xi, int64_t sc, int64_t m,
                                                          double* __restrict__ Xt, int64_t scp) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t s0 = (int64_t)blockIdx.x * 32, k0 = (int64_t)blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) tile[r][tx] = (s0 + r < sc && k0 + tx < m) ? xi[(s0 + r) * m + k0 + tx] : 0.0;
  __syncthreads();
  for (int r = ty; r < 32; r += 8) Xt[(k0 + r) * scp + s0 + tx] = tile[tx][r];
}

// out[s][j] = mean[j] + Y[j][s] for the sc samples of the chunk (Y: mp x scp): the transpose into sample-major rows
__global__ __launch_bounds__(256) void psampler_epilogue_kernel(const double* __restrict__ Y, int64_t scp,
                                                                const double* __restrict__ mean, int64_t sc, int64_t m,
                                                                double* __restrict__ out) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t s0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) tile[r][tx] = Y[(j0 + r) * scp + s0 + tx];   // (inside the padded storage)
  __syncthreads();
  const double mj = j0 + tx < m ? mean[j0 + tx] : 0.0;
  for (int r = ty; r < 32; r += 8)
    if (s0 + r < sc && j0 + tx < m) out[(s0 + r) * m + j0 + tx] = mj + tile[tx][r];
}

// rmax[i] = max_j |R[i][j]| / sqrt(C[i][i] C[j][j]) over j < m: one workgroup per row i < m (the backward error of a factor, entry by
// entry in the measure the factor contract is stated in; a maximum, so no order matters)
__global__ __launch_bounds__(256) void psampler_resid_kernel(const double* __restrict__ R, int64_t ldr, const double* __restrict__ C,
                                                             int64_t ldc, int64_t m, double* __restrict__ rmax) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t i = blockIdx.x;
  const double cii = C[i * ldc + i];
  double v = 0.0;
  for (int64_t j = t; j < m; j += 256) {
    const double q = fabs(R[i * ldr + j]) / sqrt(cii * C[j * ldc + j]);
    v = q > v ? q : v;
  }
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] = red[t + w] > red[t] ? red[t + w] : red[t];
    __syncthreads();
  }
  if (t == 0) rmax[i] = red[0];
}

// One step of refinement from the residual R = Chat - F F^T in pR (consumed):  G = F^-1 R F^-T (the leaf inverses of the
// factorisation serve both solves);  F += F Phi(G).  pY: mp x mp of scratch.
int psampler_refine(gpx_ctx* ctx, gpx_mat* F, const double* invd, double* pR, double* pY, int64_t m, int64_t mp) {
  const dim3 gridM((unsigned)mp, (unsigned)((mp + 255) / 256));
  GPX_TRY(chol_trsm_left(ctx, F->p, F->ld, invd, pR, mp, mp, mp));
  GPX_TRY(chol_trsm_right(ctx, F->p, F->ld, invd, pR, mp, mp, mp));
  hipLaunchKernelGGL(psampler_phi_kernel, gridM, dim3(256), 0, ctx->stream, pR, mp, mp);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_gemm_tri(ctx, F->p, F->ld, pR, mp, pY, mp, mp, mp, mp, false, false, false, 1));
  hipLaunchKernelGGL(psampler_addlower_kernel, gridM, dim3(256), 0, ctx->stream, F->p, F->ld, (const double*)pY, mp, m);
  GPX_HIP(hipGetLastError());
  return 0;
}

constexpr int PSAMPLER_MAX_EXTRA = 4;   // refinement steps `verify` may add to the first

// The tail of both constructors (gpx_psampler_create, gpx_vfe_psampler_create): ps->F holds the covariance C on entry (mp x mp, the
// padding 0) and chol(C + nugget I), finished and refined, on return.  Runs under the caller's PolicyScope; a pivot <= 0 is returned
// (> 0) with the message that names the point.  Synchronises the stream.
// verify: after the refinement step the residual is MEASURED on the device, max_ij |Chat - F F^T|_ij / sqrt(Chat_ii Chat_jj), and while
// it is above 4 (M + 1) u -- half the factor contract's 8 (M + 1) u -- the step is repeated, PSAMPLER_MAX_EXTRA times at most.  One step
// is first order in G = F^-1 R F^-T, and on a covariance of low numerical rank whose other eigenvalues are the nugget (many points on a
// line under a squared exponential: condition 1e11, several tiles) the explicit leaf inverses of chol_potrf leave an R for which G is
// not small: the step then leaves a residual of the order |G|^2, which the next step takes as its R (the iteration is Newton's,
// the later steps' solves use the first factor's leaf inverses: an inexact Newton step).  Costs one more mp^2 buffer and one product
// per check.  The dense constructor passes false: its launches and its bits stay what they were.
int psampler_factor(gpx_ctx* ctx, gpx_psampler* ps, Scratch& sc, double nugget, bool verify) {
  const int64_t m = ps->m, mp = ps->mp;
  gpx_mat* F = ps->F;
  double* invd;
  GPX_TRY(sc.get(mp * GPX_TILE * 8, &invd));
  hipLaunchKernelGGL(psampler_nugget_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, F->p, F->ld, m, nugget);
  GPX_HIP(hipGetLastError());
  // Chat is kept for one step of refinement: chol_potrf's leaf multiplies by explicit inverses of its diagonal blocks, and on a
  // covariance whose spectrum reaches down to the nugget that leaves |F F^T - Chat| an order above what a plain Cholesky leaves
  double *pR, *pY, *pC = nullptr, *rmax = nullptr;
  GPX_TRY(sc.get(mp * mp * 8, &pR));
  GPX_TRY(sc.get(mp * mp * 8, &pY));
  GPX_TRY(gpx_copy2d(ctx, F->p, F->ld, pR, mp, mp, mp));
  if (verify) {
    GPX_TRY(sc.get(mp * mp * 8, &pC));
    GPX_TRY(sc.get(mp * 8, &rmax));
    GPX_TRY(gpx_copy2d(ctx, F->p, F->ld, pC, mp, mp, mp));
  }
  GPX_TRY(chol_potrf(ctx, F->p, F->ld, mp, invd, m));
  int info = 0;
  GPX_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipDeviceSynchronize());   // (the blocked factorisation of a large C uses three streams)
  if (info != 0) {
    gpx_set_error("psampler: C + nugget I is not positive definite (pivot %d <= 0, nugget %g): the point repeats an earlier one "
                  "or lies on a training point of a noise-free model; a larger nugget factors it", info, nugget);
    return info;
  }
  hipLaunchKernelGGL(psampler_finish_kernel, dim3((unsigned)mp, (unsigned)((mp + 255) / 256)), dim3(256), 0, ctx->stream, F->p,
                     F->ld, m, mp);
  GPX_HIP(hipGetLastError());
  // R = Chat - F F^T;  G = F^-1 R F^-T;  F += F Phi(G)
  GPX_TRY(launch_gemm(ctx, F->p, F->ld, F->p, F->ld, pR, mp, mp, mp, mp, true, true, false));
  GPX_TRY(psampler_refine(ctx, F, invd, pR, pY, m, mp));
  if (verify) {
    std::vector<double> h((size_t)m);
    const double cap = 4.0 * (double)(m + 1) * 0x1p-53;
    for (int extra = 0; extra < PSAMPLER_MAX_EXTRA; ++extra) {
      GPX_TRY(gpx_copy2d(ctx, pC, mp, pR, mp, mp, mp));
      GPX_TRY(launch_gemm(ctx, F->p, F->ld, F->p, F->ld, pR, mp, mp, mp, mp, true, true, false));
      hipLaunchKernelGGL(psampler_resid_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, (const double*)pR, mp,
                         (const double*)pC, mp, m, rmax);
      GPX_HIP(hipGetLastError());
      GPX_HIP(hipMemcpyAsync(h.data(), rmax, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipStreamSynchronize(ctx->stream));
      double worst = 0.0;
      for (int64_t i = 0; i < m; ++i) worst = h[(size_t)i] > worst ? h[(size_t)i] : worst;
      if (worst <= cap) break;
      GPX_TRY(psampler_refine(ctx, F, invd, pR, pY, m, mp));
    }
  }
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// C += D on the mp x mp storage (D: row stride mp)
__global__ __launch_bounds__(256) void vfe_cov_add_kernel(double* __restrict__ C, int64_t ldc, const double* __restrict__ D,
                                                          int64_t mp) {
  const int64_t j = (int64_t)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
  if (j < mp) C[i * ldc + j] += D[i * mp + j];
}

// C (mp x mp, row stride ldc; mp = Z's rows padded to 128) = (K(Z,Z) - Wu^T Wu) + Wa^T Wa with Wu = Lu^-1 K(S,Z), Wa = La^-1 K(S,Z):
// the full covariance of the variational posterior -- vfe_posterior_chunk's variance on the diagonal, in its order of operations.
// posterior_cov_into's steps once per factor: fill, the cross-solve rule, transpose, its GEMM; nothing N x M.  kpz: the model's
// kernel re-centred on S and Z.
int vfe_posterior_cov_into(gpx_ctx* ctx, const FitcView& v, const KParams& kpz, const gpx_mat* S, const gpx_mat* Z, Scratch& sc,
                           double* C, int64_t ldc) {
  const int64_t nu = v.nu, nup = v.nup, m = Z->rows, mp = gpx_round_up(m, GPX_TILE), ldb = gpx_skew_ld(mp);
  const bool oop = chol_cross_oop(nup);
  double *B, *W = nullptr, *Wt, *D;
  GPX_TRY(sc.get(nup * ldb * 8, &B));
  if (oop) GPX_TRY(sc.get(nup * ldb * 8, &W));
  GPX_TRY(sc.get(mp * nup * 8, &Wt));
  GPX_TRY(sc.get(mp * mp * 8, &D));
  GPX_TRY(launch_kfill(ctx, kpz, Z->p, m, Z->p, m, 1, nullptr, 0, 0.0, C, mp, mp, ldc));
  for (int which = 0; which < 2; ++which) {
    GPX_TRY(launch_kfill(ctx, kpz, S->p, nu, Z->p, m, 0, nullptr, 0, 0.0, B, nup, mp, ldb));   // (each solve consumes it)
    GPX_TRY(chol_cross_solve(ctx, which == 0 ? v.Lu : v.La, B, ldb, W, ldb, mp));
    GPX_TRY(launch_transpose(ctx, oop ? W : B, nup, mp, ldb, Wt, nup));
    if (which == 0) {
      GPX_TRY(launch_gemm(ctx, Wt, nup, Wt, nup, C, ldc, mp, mp, nup, true, true, false));
    } else {
      GPX_TRY(launch_gemm(ctx, Wt, nup, Wt, nup, D, mp, mp, mp, nup, true, false, false));
      hipLaunchKernelGGL(vfe_cov_add_kernel, dim3((unsigned)mp, (unsigned)((mp + 255) / 256)), dim3(256), 0, ctx->stream, C, ldc,
                         (const double*)D, mp);
      GPX_HIP(hipGetLastError());
    }
  }
  return 0;
}

// draw / argbest: S samples in chunks whose work matrices stay under the cross-matrix budget
int psampler_run(gpx_ctx* ctx, const gpx_psampler* ps, const double* xi, int64_t S, int sign, double* samples, int64_t* out_idx,
                 double* out_val) {
  const int64_t m = ps->m, mp = ps->mp;
  // per sample: a column of Xt and of Y (mp each), a row of the staged Xi and of the result (m each)
  const ChunkRange cr(S, gpx_chunk_len((int64_t)16 << 30, (2 * mp + 2 * m) * 8));
  const int64_t sc_alloc = cr.widest, scp_alloc = cr.mc_alloc;
  double *stage, *Xt, *Y, *outd, *dval = nullptr;
  int64_t* didx = nullptr;
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(sc.get(sc_alloc * m * 8, &stage));
  GPX_TRY(sc.get(mp * scp_alloc * 8, &Xt));
  GPX_TRY(sc.get(mp * scp_alloc * 8, &Y));
  GPX_TRY(sc.get(sc_alloc * m * 8, &outd));
  if (out_idx) {
    GPX_TRY(sc.get(sc_alloc * 8, &didx));
    GPX_TRY(sc.get(sc_alloc * 8, &dval));
  }
  for (const ChunkRange::Step c : cr) {
    const int64_t s0 = c.j0, scn = c.mc, scp = c.mcp;
    GPX_HIP(hipMemcpyAsync(stage, xi + s0 * m, (size_t)(scn * m * 8), hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)(scp / 32), (unsigned)(mp / 32));
    hipLaunchKernelGGL(psampler_xi_kernel, grid, dim3(256), 0, ctx->stream, (const double*)stage, scn, m, Xt, scp);
    GPX_HIP(hipGetLastError());
    GPX_TRY(launch_gemm_tri(ctx, ps->F->p, ps->F->ld, Xt, scp, Y, scp, mp, scp, mp, false, false, false, 1));
    hipLaunchKernelGGL(psampler_epilogue_kernel, grid, dim3(256), 0, ctx->stream, (const double*)Y, scp, (const double*)ps->mean,
                       scn, m, outd);
    GPX_HIP(hipGetLastError());
    if (samples) GPX_HIP(hipMemcpyAsync(samples + s0 * m, outd, (size_t)(scn * m * 8), hipMemcpyDeviceToHost, ctx->stream));
    if (out_idx) {
      ProfScope pf(ctx, GPX_PROF_GREEDY, 0.0, 8.0 * (double)scn * (double)m);
      GPX_TRY(launch_row_argbest(ctx, outd, scn, m, m, 0, sign, 1, didx, dval));   // (one chunk covers the whole row)
      GPX_HIP(hipMemcpyAsync(out_idx + s0, didx, (size_t)scn * 8, hipMemcpyDeviceToHost, ctx->stream));
      if (out_val) GPX_HIP(hipMemcpyAsync(out_val + s0, dval, (size_t)scn * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  return 0;
}

// ---- q-EI ---------------------------------------------------------------------------------------------------------------------
constexpr int QEI_TR = 64;        // rows of W per LDS tile
constexpr int QEI_TS = 33;        // its row stride (odd: the row slices of one column fall on different banks)
constexpr int QEI_ITEMS = 3;      // (entry, slice) items a thread can own: G npair nsl <= 768 (q = 32: 528 entries, one slice)
constexpr int QEI_LEVELS = 32;    // levels of the pairwise-sum stack: any S below 2^31

struct QeiPlan {
  int G, T, nsl, npair;
};
QeiPlan qei_plan(int q) {
  QeiPlan p;
  p.G = 32 / q;
  p.npair = q * (q + 1) / 2;
  p.T = 1;
  while (2 * p.T * p.G <= 256) p.T *= 2;
  p.nsl = 1;
  while (2 * p.nsl * p.G * p.npair <= 256) p.nsl *= 2;
  return p;
}

// One Gram pass of qei_kernel over one factor W (n rows used, row stride ldw; the workgroup's columns [c0, c0 + ncols)): on return
// part[p nsl + sl] holds slice sl of entry p -- sum over the rows r = sl (mod nsl), r < n, of W[r][ci] W[r][cj], one fma chain in
// ascending r -- and the workgroup is synchronised.  Rows pass through `tile` in tiles of QEI_TR; rows >= n are never read.
__device__ __forceinline__ void qei_gram_pass(const double* __restrict__ W, int64_t ldw, int64_t n, int64_t c0, int ncols, int gb,
                                              int q, const QeiPlan& pl, double* __restrict__ tile, double* __restrict__ part,
                                              const unsigned char* __restrict__ pi_, const unsigned char* __restrict__ pj_) {
  const int t = threadIdx.x, nsl = pl.nsl, npair = pl.npair;
  const int nitems = pl.G * npair * nsl;
  double acc[QEI_ITEMS];
#pragma unroll
  for (int k = 0; k < QEI_ITEMS; ++k) acc[k] = 0.0;
  for (int64_t r0 = 0; r0 < n; r0 += QEI_TR) {
    const int rows = (n - r0) < QEI_TR ? (int)(n - r0) : QEI_TR;
    __syncthreads();   // the previous tile is consumed (first pass: the tables are written; second: the slices are added up)
    for (int e = t; e < rows * ncols; e += 256) {
      const int r = e / ncols, c = e - r * ncols;
      tile[r * QEI_TS + c] = W[(r0 + r) * ldw + c0 + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QEI_ITEMS; ++k) {
      const int it = t + 256 * k;
      if (it >= nitems) continue;
      const int p = it / nsl, sl = it - p * nsl, g = p / npair;
      if (g >= gb) continue;
      const int pp = p - g * npair, ci = g * q + pi_[pp], cj = g * q + pj_[pp];
      double a = acc[k];
      for (int r = sl; r < rows; r += nsl) a = fma(tile[r * QEI_TS + ci], tile[r * QEI_TS + cj], a);
      acc[k] = a;
    }
  }
#pragma unroll
  for (int k = 0; k < QEI_ITEMS; ++k)
    if (t + 256 * k < nitems) part[t + 256 * k] = acc[k];
  __syncthreads();
}

// One workgroup = the batches [gb0, gb0 + G) of the chunk (fewer at the chunk's end).  W: the chunk's solved cross matrix (n rows
// used, row stride ldw), batch b its columns [b q, (b + 1) q); Zc / mean: the chunk's points and posterior means; b0: the chunk's
// first batch in the call (cost, the partials' indices and the debug blocks are addressed by the global batch).
// VFE: the signed two-factor Gram of a variational model, C_b = (k - Wu^T Wu) + Wa^T Wa with W = Wu = Lu^-1 K(S, Zb) and W2 = Wa =
// La^-1 K(S, Zb) (same stride, n = nu rows each): two passes of the one tile loop, first Wu then Wa, `tile` and `part` reused;
// after the first A = k - su, after the second A += sa -- vfe_posterior_chunk's pv = (kd - su) + sa, entry by entry.  The dense
// instantiation ignores W2 and is the kernel it was.
template <int QMAX, bool VFE>
__global__ __launch_bounds__(256) void qei_kernel(KParams kp, const double* __restrict__ W, const double* __restrict__ W2, int64_t ldw,
                                                  int64_t n, const double* __restrict__ Zc, const double* __restrict__ mean, int q,
                                                  QeiPlan pl, int64_t nb, int64_t b0, const double* __restrict__ xi, int64_t S,
                                                  double fBest, double nugget, double* __restrict__ cost,
                                                  double* __restrict__ part_c, int64_t* __restrict__ part_i, int* __restrict__ nbad,
                                                  double* __restrict__ dbgC, double* __restrict__ dbgF) {
  __shared__ double tile[QEI_TR * QEI_TS];
  __shared__ double part[256 * QEI_ITEMS];
  __shared__ double A[32 * 32];          // G blocks of q x q
  __shared__ double mu[32], cl[32];
  __shared__ double red[256];
  __shared__ int bad[32];
  __shared__ unsigned char pi_[528], pj_[528];
  const int t = threadIdx.x, G = pl.G, T = pl.T, nsl = pl.nsl, npair = pl.npair, d = kp.d;
  const int64_t gb0 = (int64_t)blockIdx.x * G;
  const int gb = (nb - gb0) < G ? (int)(nb - gb0) : G;
  const int ncols = gb * q, qq = q * q;
  const int64_t c0 = gb0 * q;
  for (int p = t; p < npair; p += 256) {   // entry p of the lower triangle, row-major: (i, j), j <= i
    int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    while (i * (i + 1) / 2 > p) --i;
    pi_[p] = (unsigned char)i;
    pj_[p] = (unsigned char)(p - i * (i + 1) / 2);
  }
  if (t < 32) {
    mu[t] = t < ncols ? mean[c0 + t] : 0.0;
    bad[t] = 0;
  }
  // ---- 1. W_b^T W_b, entry by entry ----
  qei_gram_pass(W, ldw, n, c0, ncols, gb, q, pl, tile, part, pi_, pj_);
  for (int p = t; p < G * npair; p += 256) {
    const int g = p / npair;
    if (g >= gb) continue;
    const int pp = p - g * npair, i = pi_[pp], j = pj_[pp];
    double s = part[p * nsl];
    for (int sl = 1; sl < nsl; ++sl) s += part[p * nsl + sl];
    const double v = kpair(kp, Zc + (c0 + g * q + i) * d, Zc + (c0 + g * q + j) * d) - s;
    A[g * qq + i * q + j] = v;
    A[g * qq + j * q + i] = v;
  }
  if (VFE) {
    qei_gram_pass(W2, ldw, n, c0, ncols, gb, q, pl, tile, part, pi_, pj_);   // (its first barrier: `part` and A are settled)
    for (int p = t; p < G * npair; p += 256) {
      const int g = p / npair;
      if (g >= gb) continue;
      const int pp = p - g * npair, i = pi_[pp], j = pj_[pp];
      double s = part[p * nsl];
      for (int sl = 1; sl < nsl; ++sl) s += part[p * nsl + sl];
      const double v = A[g * qq + i * q + j] + s;
      A[g * qq + i * q + j] = v;
      A[g * qq + j * q + i] = v;
    }
  }
  __syncthreads();
  if (dbgC)
    for (int e = t; e < gb * qq; e += 256) dbgC[(b0 + gb0) * qq + e] = A[e];
  __syncthreads();
  if (t < ncols) {
    const int g = t / q, i = t - g * q;
    A[g * qq + i * q + i] += nugget;
  }
  __syncthreads();
  // ---- 2. right-looking Cholesky in LDS: a team of T threads per batch, all teams in step ----
  const int team = t / T, u = t - team * T;
  const bool active = team < gb;
  double* Ag = A + (active ? team : 0) * qq;
  for (int k = 0; k < q; ++k) {
    const double piv = Ag[k * q + k];
    if (active && u == 0 && !(piv > 0.0)) bad[team] = 1;
    // Rounded OUTWARD, one step at most: rt <= sqrt(piv) and |l_ik| >= |a_ik| / rt.  In exact arithmetic a point that repeats an
    // earlier one bit for bit meets a pivot of exactly 0, and round-to-nearest leaves it a few 1e-17 on either side of 0 by chance.
    // With this rule it is certain to be <= 0: the two rows are equal bitwise at the earlier point's step (a_ik = piv = c), so
    // l >= c / rt >= sqrt(c), c - l^2 <= 0 exactly, and the steps after it only subtract squares.
    double rt = sqrt(piv);
    if (fma(rt, rt, -piv) > 0.0) rt = nextafter(rt, 0.0);
    __syncthreads();
    if (active)
      for (int i = k + u; i < q; i += T) {
        const double a = Ag[i * q + k];
        double l = a / rt;
        const double over = fma(l, rt, -a);   // the sign of l rt - a, exactly
        if (a > 0.0 ? over < 0.0 : over > 0.0) l = nextafter(l, a > 0.0 ? __builtin_inf() : -__builtin_inf());
        Ag[i * q + k] = i == k ? rt : l;
      }
    __syncthreads();
    if (active)
      for (int e = u; e < qq; e += T) {
        const int i = e / q, j = e - i * q;
        if (j > k && i >= j) Ag[e] = fma(-Ag[i * q + k], Ag[j * q + k], Ag[e]);
      }
    __syncthreads();
  }
  if (active)
    for (int e = u; e < qq; e += T)
      if (e - (e / q) * q > e / q) Ag[e] = 0.0;
  __syncthreads();
  if (dbgF)
    for (int e = t; e < gb * qq; e += 256) dbgF[(b0 + gb0) * qq + e] = A[e];
  // ---- 3. the samples: pairwise sums per thread, a halving tree per team ----
  double tot = 0.0;
  if (active) {
    double st[QEI_LEVELS];
#pragma unroll
    for (int l = 0; l < QEI_LEVELS; ++l) st[l] = 0.0;
    const double* __restrict__ mg = mu + team * q;
    int64_t cnt = 0;
    for (int64_t s = u; s < S; s += T, ++cnt) {
      const double* __restrict__ xs = xi + s * q;
      double f[QMAX];
#pragma unroll
      for (int j = 0; j < QMAX; ++j) f[j] = 0.0;
#pragma unroll
      for (int k = 0; k < QMAX; ++k) {
        if (k < q) {
          const double xk = xs[k];
#pragma unroll
          for (int j = k; j < QMAX; ++j)
            if (j < q) f[j] = fma(Ag[j * q + k], xk, f[j]);
        }
      }
      double mn = __builtin_inf();
#pragma unroll
      for (int j = 0; j < QMAX; ++j)
        if (j < q) {
          const double v = mg[j] + f[j];
          mn = v < mn ? v : mn;
        }
      const double dlt = fBest - mn;
      double a = dlt < 0.0 ? 0.0 : dlt;
      // push: the binary counter `cnt` says which levels are full
      bool go = true;
#pragma unroll
      for (int l = 0; l < QEI_LEVELS; ++l) {
        if (go) {
          if ((cnt >> l) & 1) {
            a = st[l] + a;
          } else {
            st[l] = a;
            go = false;
          }
        }
      }
    }
    bool first = true;
#pragma unroll
    for (int l = 0; l < QEI_LEVELS; ++l) {
      if ((cnt >> l) & 1) {
        tot = first ? st[l] : st[l] + tot;
        first = false;
      }
    }
  }
  red[t] = tot;
  __syncthreads();
  for (int h = T / 2; h > 0; h >>= 1) {
    if (u < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (active && u == 0) {
    const double c = bad[team] ? __builtin_nan("") : -(red[t] / (double)S);
    cost[b0 + gb0 + team] = c;
    cl[team] = c;
  }
  __syncthreads();
  if (t == 0) {
    VI best{0.0, -1};
    int nbd = 0;
    for (int g = 0; g < gb; ++g) {
      nbd += bad[g];
      if (cl[g] == cl[g]) best = argmin_merge(best, VI{cl[g], b0 + gb0 + g});
    }
    part_c[blockIdx.x] = best.v;
    part_i[blockIdx.x] = best.i;
    nbad[blockIdx.x] = nbd;
  }
}

// What gpx_acq_qei and gpx_vfe_acq_qei share around qei_kernel: the chunking over whole batches, the call's buffers, the launch of
// one chunk and the final reduction with its copies.  np: the padded order of the factor(s) the chunk is solved against.
struct QeiRun {
  const int64_t q, B, S;
  const QeiPlan pl;
  int64_t bc, ngroups, g0 = 0;   // batches per chunk, workgroups of the call, workgroups launched so far
  double *dxi = nullptr, *dcost = nullptr, *part_c = nullptr, *best_c = nullptr, *dC = nullptr, *dF = nullptr;
  int64_t *part_i = nullptr, *best_i = nullptr;
  int* dbad = nullptr;

  // whole batches per chunk (whole workgroup spans while the chunk holds one): its own step rule, not ChunkRange's
  QeiRun(int64_t np, int64_t q_, int64_t B_, int64_t S_) : q(q_), B(B_), S(S_), pl(qei_plan((int)q_)) {
    bc = gpx_eval_chunk(np) / q;
    if (bc >= pl.G) bc = bc / pl.G * pl.G;
    if (bc > B) bc = B;
    ngroups = (bc + pl.G - 1) / pl.G * ((B + bc - 1) / bc);
  }
  int64_t mc_alloc() const { return gpx_round_up(bc * q, GPX_TILE); }
  int take(gpx_ctx* ctx, Scratch& sc, const double* xi, bool dbg) {
    GPX_TRY(sc.get(S * q * 8, &dxi));
    GPX_TRY(sc.get(B * 8, &dcost));
    GPX_TRY(sc.get(ngroups * 8, &part_c));
    GPX_TRY(sc.get(ngroups * 8, &part_i));
    GPX_TRY(sc.get(ngroups * 4, &dbad));
    GPX_TRY(sc.get(8, &best_c));
    GPX_TRY(sc.get(8, &best_i));
    if (dbg) {
      GPX_TRY(sc.get(B * q * q * 8, &dC));
      GPX_TRY(sc.get(B * q * q * 8, &dF));
    }
    GPX_HIP(hipMemcpyAsync(dxi, xi, (size_t)(S * q * 8), hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
  // the chunk of nb batches from batch b0: W (and Wa on a VFE model: the signed Gram) with n rows used and row stride ldw
  template <bool VFE>
  int launch(gpx_ctx* ctx, const KParams& kp, const double* W, const double* Wa, int64_t ldw, int64_t n, const double* Zc,
             const double* pmean, int64_t nb, int64_t b0, double fBest, double nugget) {
    const int64_t groups = (nb + pl.G - 1) / pl.G;
#define GPX_QEI(QM_)                                                                                                            \
  hipLaunchKernelGGL((qei_kernel<QM_, VFE>), dim3((unsigned)groups), dim3(256), 0, ctx->stream, kp, W, Wa, ldw, n, Zc, pmean,   \
                     (int)q, pl, nb, b0, (const double*)dxi, S, fBest, nugget, dcost, part_c + g0, part_i + g0, dbad + g0, dC, dF)
    if (q <= 1) GPX_QEI(1);
    else if (q <= 2) GPX_QEI(2);
    else if (q <= 4) GPX_QEI(4);
    else if (q <= 8) GPX_QEI(8);
    else if (q <= 16) GPX_QEI(16);
    else GPX_QEI(32);
#undef GPX_QEI
    GPX_HIP(hipGetLastError());
    g0 += groups;
    return 0;
  }
  int finish(gpx_ctx* ctx, double* cost_host, int64_t* best, double* best_cost, int64_t* n_bad, double* dbg_C, double* dbg_F) {
    if (best || best_cost) {
      GPX_TRY(launch_acq_argmin(ctx, part_c, part_i, g0, best_c, best_i));
      if (best) GPX_HIP(hipMemcpyAsync(best, best_i, 8, hipMemcpyDeviceToHost, ctx->stream));
      if (best_cost) GPX_HIP(hipMemcpyAsync(best_cost, best_c, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (cost_host) GPX_HIP(hipMemcpyAsync(cost_host, dcost, (size_t)B * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dbg_C) {
      GPX_HIP(hipMemcpyAsync(dbg_C, dC, (size_t)(B * q * q * 8), hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipMemcpyAsync(dbg_F, dF, (size_t)(B * q * q * 8), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (n_bad) {
      std::vector<int> hbad((size_t)g0, 0);
      GPX_HIP(hipMemcpyAsync(hbad.data(), dbad, (size_t)g0 * 4, hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipStreamSynchronize(ctx->stream));
      int64_t s = 0;
      for (int64_t g = 0; g < g0; ++g) s += hbad[(size_t)g];
      *n_bad = s;
    }
    return 0;
  }
};

// Shared body of gpx_acq_qei and gpx_dbg_qei_blocks (dbg_*: host B x q, B x q x q, B x q x q; all three or none).
int qei_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha, const gpx_mat* Zb, int64_t q,
             const double* xi, int64_t S, double fBest, double nugget, double* cost_host, int64_t* best, double* best_cost,
             int64_t* n_bad, double* dbg_mean, double* dbg_C, double* dbg_F) {
  const int64_t n = L->rows, np = L->prows, B = Zb->rows / q, d = kp.d;
  QeiRun r(np, q, B, S);
  PosteriorWork w(np, r.mc_alloc(), true);
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(w.take(sc, true, true));
  GPX_TRY(r.take(ctx, sc, xi, dbg_C != nullptr));
  GPX_TRY(w.upload_alpha(ctx, alpha, n));
  for (int64_t b0 = 0; b0 < B; b0 += r.bc) {
    const int64_t nb = (B - b0) < r.bc ? (B - b0) : r.bc, mc = nb * q;
    const int64_t ldb = gpx_skew_ld(gpx_round_up(mc, GPX_TILE));
    const double* Zc = Zb->p + b0 * q * d;
    // gpx_posterior's own per-chunk step: the means are GP.evaluate's, W the solve every variance comes from
    GPX_TRY(w.run(ctx, kp, L, X, Zc, mc, dbg_mean ? dbg_mean + b0 * q : nullptr));
    ProfScope ps(ctx, GPX_PROF_GREEDY, (double)nb * ((double)n * (double)(q * (q + 1)) + (double)S * (double)(q * (q + 1))),
                 8.0 * (double)n * (double)mc);
    GPX_TRY(r.launch<false>(ctx, kp, w.solution(), nullptr, ldb, n, Zc, w.mean, nb, b0, fBest, nugget));
  }
  return r.finish(ctx, cost_host, best, best_cost, n_bad, dbg_C, dbg_F);
}

int qei_args(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
             const gpx_mat* Zb, int64_t q, double nugget, KParams* kp) {
  GPX_ARG(ctx && L && X && alpha && Zb, "NULL argument");
  GPX_ARG(q >= 1 && q <= GPX_QEI_MAX_Q, "q-EI: the batch size q must be in 1 .. GPX_QEI_MAX_Q (32)");
  GPX_ARG(nugget >= 0.0, "q-EI: the nugget must not be negative");
  GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Zb, nullptr, "point sets must be unpadded (n x d)", kp));
  GPX_ARG(Zb->rows >= q && Zb->rows % q == 0, "q-EI: the rows of Zb must be a positive multiple of q (consecutive q rows form one batch)");
  return 0;
}

}  // namespace

// The bodies of gpx_vfe_posterior_cov and gpx_vfe_psampler_create, behind fitc.hip's argument checks (gpx_internal.h)
int vfe_posterior_cov_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* cov) {
  FitcView v;
  fitc_view(f, &v);
  KParams kpz = *v.kp;   // the evaluation points may reach beyond the training domain
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Z));
  const int64_t m = Z->rows, mp = gpx_round_up(m, GPX_TILE);
  Scratch sc(ctx);
  double* pK;
  GPX_TRY(sc.get(mp * mp * 8, &pK));
  GPX_TRY(vfe_posterior_cov_into(ctx, v, kpz, S, Z, sc, pK, mp));
  GPX_HIP(hipMemcpy2DAsync(cov, (size_t)m * 8, pK, (size_t)mp * 8, (size_t)m * 8, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int vfe_psampler_create_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double nugget,
                             gpx_psampler** out) {
  FitcView v;
  fitc_view(f, &v);
  KParams kpz = *v.kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Z));
  const int64_t m = Z->rows, mp = gpx_round_up(m, GPX_TILE), d = kpz.d;
  PolicyScope policy(ctx);   // a design loop may have left the drop policy on
  Held<gpx_psampler, gpx_psampler_free> ps(ctx, new gpx_psampler{m, mp, nullptr, nullptr, 0});
  GPX_TRY(gpx_mat_new(ctx, m, m, 1, &ps->F));
  GPX_TRY(gpx_dev_alloc(ctx, mp * 8, &ps->mean));
  ps->mean_bytes = mp * 8;
  Scratch sc(ctx);
  {
    // the mean: gpx_vfe_posterior's chunks and launches (the bits it returns), each chunk straight into the resident vector
    const ChunkRange cr(m, gpx_eval_chunk(v.nup));
    VfePosteriorWork w(v.nup, cr.mc_alloc, false);
    GPX_TRY(w.take(sc, false));
    GPX_TRY(w.beta(ctx, f, coeff, sc));
    for (const ChunkRange::Step c : cr) {
      w.pm = ps->mean + c.j0;
      GPX_TRY(w.run(ctx, f, kpz, S, Z->p + c.j0 * d, c.mc));
    }
  }
  GPX_TRY(vfe_posterior_cov_into(ctx, v, kpz, S, Z, sc, ps->F->p, ps->F->ld));
  GPX_TRY(psampler_factor(ctx, ps.get(), sc, nugget, true));
  *out = ps.release();
  return 0;
}

// The body of gpx_vfe_acq_qei and gpx_dbg_vfe_qei_blocks (dbg_*: all three or none), qei_impl on a VFE model: the means and both
// solutions come from vfe_posterior_chunk (gpx_vfe_posterior's bits), chunked over whole batches under gpx_eval_chunk(nup), and
// qei_kernel<.., true> forms C_b = (k - Wu^T Wu) + Wa^T Wa from the nu used rows of each.  Wa has a block of its own: from the order
// at which the solves run out of place both would land in the one buffer and only the La solution would survive.
int vfe_qei_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q, const double* xi,
                 int64_t nS, double fBest, double nugget, double* cost_host, int64_t* best, double* best_cost, int64_t* n_bad,
                 double* dbg_mean, double* dbg_C, double* dbg_F) {
  FitcView v;
  fitc_view(f, &v);
  KParams kpz = *v.kp;   // re-centred on S and the WHOLE of Zb: the chunking cannot move a fill
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Zb));
  const int64_t nu = v.nu, B = Zb->rows / q, d = kpz.d;
  QeiRun r(v.nup, q, B, nS);
  VfePosteriorWork w(v.nup, r.mc_alloc(), true);
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  GPX_TRY(w.take(sc, true));
  if (w.oop()) GPX_TRY(sc.get(w.bytesB, &w.Wa));
  GPX_TRY(r.take(ctx, sc, xi, dbg_C != nullptr));
  GPX_TRY(w.beta(ctx, f, coeff, sc));
  for (int64_t b0 = 0; b0 < B; b0 += r.bc) {
    const int64_t nb = (B - b0) < r.bc ? (B - b0) : r.bc, mc = nb * q;
    const int64_t ldb = gpx_skew_ld(gpx_round_up(mc, GPX_TILE));
    const double* Zc = Zb->p + b0 * q * d;
    GPX_TRY(w.run(ctx, f, kpz, S, Zc, mc));
    if (dbg_mean) GPX_HIP(hipMemcpyAsync(dbg_mean + b0 * q, w.pm, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
    ProfScope ps(ctx, GPX_PROF_GREEDY, (double)nb * (2.0 * (double)nu + (double)nS) * (double)(q * (q + 1)),
                 8.0 * 2.0 * (double)nu * (double)mc);
    GPX_TRY(r.launch<true>(ctx, kpz, w.solU(), w.solA(), ldb, nu, Zc, w.pm, nb, b0, fBest, nugget));
  }
  return r.finish(ctx, cost_host, best, best_cost, n_bad, dbg_C, dbg_F);
}

extern "C" {

int gpx_psampler_free(gpx_ctx* ctx, gpx_psampler* ps) {
  if (!ps) return 0;
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  (void)hipStreamSynchronize(ctx->stream);
  if (ps->F) (void)gpx_mat_free(ctx, ps->F);
  if (ps->mean) gpx_dev_release(ctx, ps->mean, ps->mean_bytes);
  delete ps;
  return 0;
}

int gpx_psampler_shape(const gpx_psampler* ps, int64_t* m) {
  GPX_ARG(ps != nullptr, "sampler is NULL");
  if (m) *m = ps->m;
  return 0;
}

int gpx_psampler_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                        const double* alpha, const gpx_mat* Z, double nugget, gpx_psampler** out) {
  GPX_ARG(ctx && Z && out, "NULL argument");
  bool prior;
  GPX_TRY(gpx_model_or_prior(L, X, alpha, "psampler: L, X and alpha are given together, or all three NULL (the prior)", &prior));
  GPX_ARG(nugget >= 0.0, "psampler: the nugget must not be negative");
  GPX_ARG(Z->rows >= 1, "psampler: needs at least one point");
  KParams kp;
  if (prior) {
    GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
    GPX_ARG(Z->cols == d && Z->pcols == d, "point sets must be unpadded (n x d)");
    GPX_TRY(gpx_kparams_sets(ctx, &kp, Z));
  } else {
    GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Z, nullptr, "point sets must be unpadded (n x d)", &kp));
  }
  const int64_t m = Z->rows, mp = gpx_round_up(m, GPX_TILE);
  PolicyScope policy(ctx);   // a design loop may have left the drop policy on
  Held<gpx_psampler, gpx_psampler_free> ps(ctx, new gpx_psampler{m, mp, nullptr, nullptr, 0});
  GPX_TRY(gpx_mat_new(ctx, m, m, 1, &ps->F));
  GPX_TRY(gpx_dev_alloc(ctx, mp * 8, &ps->mean));
  ps->mean_bytes = mp * 8;
  gpx_mat* F = ps->F;
  Scratch sc(ctx);
  if (prior) {
    GPX_HIP(hipMemsetAsync(ps->mean, 0, (size_t)mp * 8, ctx->stream));
    GPX_TRY(launch_kfill(ctx, kp, Z->p, m, Z->p, m, 1, nullptr, 0, 0.0, F->p, mp, mp, F->ld));
  } else {
    // the mean: gpx_posterior's chunks and launches (the bits it returns)
    const ChunkRange cr(m, gpx_eval_chunk(L->prows));
    PosteriorWork w(L->prows, cr.mc_alloc, false);
    GPX_TRY(w.take(sc, true, false, false));
    GPX_TRY(w.upload_alpha(ctx, alpha, L->rows));
    for (const ChunkRange::Step c : cr) GPX_TRY(w.run(ctx, kp, L, X, Z->p + c.j0 * d, c.mc, nullptr, ps->mean + c.j0));
    GPX_TRY(posterior_cov_into(ctx, kp, L, X, Z, sc, F->p, F->ld));
  }
  GPX_TRY(psampler_factor(ctx, ps.get(), sc, nugget, false));
  *out = ps.release();
  return 0;
}

int gpx_psampler_draw(gpx_ctx* ctx, const gpx_psampler* ps, const double* xi, int64_t S, double* out) {
  GPX_ARG(ctx && ps && xi && out, "NULL argument");
  GPX_ARG(S >= 1, "psampler: needs at least one sample");
  return psampler_run(ctx, ps, xi, S, 1, out, nullptr, nullptr);
}

int gpx_psampler_argbest(gpx_ctx* ctx, const gpx_psampler* ps, const double* xi, int64_t S, int sign, int64_t* out_idx,
                         double* out_val, double* samples) {
  GPX_ARG(ctx && ps && xi && out_idx, "NULL argument");
  GPX_ARG(S >= 1, "psampler: needs at least one sample");
  GPX_ARG(sign == 1 || sign == -1, "psampler: sign must be +1 (minimum) or -1 (maximum)");
  GPX_TRY(psampler_run(ctx, ps, xi, S, sign, samples, out_idx, out_val));   // (synchronised: its Scratch is gone)
  gpx_row_argbest_nan(S, out_idx, out_val);
  return 0;
}

int gpx_acq_qei(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
                const gpx_mat* Zb, int64_t q, const double* xi, int64_t S, double fBest, double nugget, double* cost, int64_t* best,
                double* best_cost, int64_t* n_bad) {
  KParams kp;
  GPX_TRY(qei_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Zb, q, nugget, &kp));
  GPX_ARG(xi != nullptr, "q-EI: xi is NULL");
  GPX_ARG(S >= 1 && S < ((int64_t)1 << 31), "q-EI: needs at least one base sample (and fewer than 2^31)");
  return qei_impl(ctx, kp, L, X, alpha, Zb, q, xi, S, fBest, nugget, cost, best, best_cost, n_bad, nullptr, nullptr, nullptr);
}

// debug (gpx_debug.h): the blocks qei_kernel works on -- gpx_acq_qei's launches with one zero base sample
int gpx_dbg_qei_blocks(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                       const double* alpha, const gpx_mat* Zb, int64_t q, double nugget, double* mean, double* Cb, double* Fb) {
  KParams kp;
  GPX_TRY(qei_args(ctx, kind, d, hyp, nhyp, L, X, alpha, Zb, q, nugget, &kp));
  GPX_ARG(mean && Cb && Fb, "NULL argument");
  const std::vector<double> xi0((size_t)q, 0.0);
  return qei_impl(ctx, kp, L, X, alpha, Zb, q, xi0.data(), 1, 0.0, nugget, nullptr, nullptr, nullptr, nullptr, mean, Cb, Fb);
}

}  // extern "C"
