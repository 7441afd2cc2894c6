// IVAR design on a VFE model, in the inducing space -- gfx950 (none in the reference: it has no VFE).
//
// Notation of fitc.hip: S the nu inducing points, k_u(.) = K(S, .), Quu = K(S,S) + noise I = Lu Lu^T, and for design points X
//     A = Quu + sum_i k_u(x_i) k_u(x_i)^T / noise = La La^T,       var(z) = k(z,z) - |Lu^-1 k_u(z)|^2 + |La^-1 k_u(z)|^2.
// The design enters through the nu x nu matrix A only, the M Monte-Carlo points Z through ONE nu x nu Gram matrix
//     Gz = K(S,Z) K(Z,S) / M,        kbar = mean_z k(z,z),
// so the integrated variance and its gradient w.r.t. the free design points are
//     IVAR(X)         = kbar - tr(Lu^-1 Gz Lu^-T) + tr(La^-1 Gz La^-T)
//     dIVAR/dx_i[l]   = -(2 / noise) sum_u H[u][i] dk(x_i, s_u)/dx_i[l],     H = A^-1 Gz A^-1 k_u(X)
// An optimiser iterate costs O(nu^3 + nu^2 b) for b free points: independent of M and -- with the leading points pinned into A0 = Quu
// + K(S,Xp) K(Xp,S) / noise -- of the pinned count.
//
// gpx_vfe_design_create keeps Lu, Gz, A0 = Quu (three nu x nu matrices) and the scalars kbar and c0 = tr(Lu^-1 Gz Lu^-T).  Gz is
// accumulated over chunks of Z (one nu x chunk fill under GPX_CROSS_BYTES, as gpx_vfe_posterior) by the fp64-MFMA SYRK, the chunks in
// index order, then scaled and mirrored (vfd_sym_kernel).  gpx_vfe_design_eval, with P = K(S,Xf) (nu x b) and P^T (its own fill):
//     A  = A0 + P P^T / noise        SYRK into La's storage, then vfd_sym_kernel in place (lower triangle + mirror)
//     La = chol(A)                   fitc_factor: chol_potrf with the context's pivot policy
//     Y1 = La^-1 Gz La^-T            a copy of Gz, chol_cross_solve (from order 2048 out of place through the block inverses),
//                                    chol_trsm_right;   tr Y1: diagonal gather + launch_sum (fixed order)
//     V^T = P^T La^-T,   H^T = (V^T Y1) La^-1        chol_trsm_right, one b x nu x nu product, chol_trsm_right_n: A^-1 Gz A^-1 is never
//                                    formed, and H comes out as the b x nu weights the row pass wants
//     grad = -(2 / noise) rows of fitc_wgrad_rows(Xf, S, H^T)       fitc.hip's row pass of dL/dS: the TRUE derivative table
// Flops: nu^3 / 3 (factor) + 2 nu^3 (two-sided solve) + 2 nu^2 b (SYRK); with the gradient 6 nu^2 b more (two solves, one product)
// and the row pass's (6 d + 25) b nu.  Memory: three resident nu x nu matrices, two more per eval (La, Y1; a third from order 2048),
// two nu x b buffers, one nu x chunk at create.  No atomics; every reduction in an order that depends on the shapes only: two calls
// with the same arguments return the same bits.
//
// gpx_vfe_var_grad: the literal (N d) x M matrix d var(z_j)/dx_k[l] = -(2 / noise) E[k][j] D_l[k][j] on a fitted VFE model, with
// C = A^-1 K(S,Z) (both sweeps from the right on its transpose), E = K(X,S) C, D_l = (dK(X,S)/dx[l]) C: per chunk of Z one GEMM for E
// and, per coordinate, one rectangular derivative fill (vfd_dkfill_kernel), one GEMM and one finish pass (vfd_vg_finish_kernel).  It
// is bound by the copy of its result to the host, as gpx_var_grad.
#include "gpx_device.h"
#include <math.h>
#include <vector>

struct gpx_vfe_design {
  KParams kp;   // the kernel, centred on S
  int64_t nu, nup, m, pinned;
  double noise, kbar, c0;
  gpx_mat *S, *Lu, *Gz, *A0;
};

namespace {

constexpr int ST = 16;   // tile of vfd_sym_kernel: 16 x 16 elements per workgroup of 256

// out = (BASE ? base : 0) + T / den on the lower triangle (row >= column) of an n x n matrix, mirrored into the upper one: the
// symmetric scaled add A = A0 + P P^T / noise (den = noise) and the scale-and-mirror of Gz (den = -M, base = NULL).  One
// workgroup per 16 x 16 tile on or below the diagonal (blockIdx.x <= blockIdx.y; the others leave at once); the mirror image goes
// through LDS so that both stores run along rows.  Only the lower triangle of base and T is read, so out may be either of them.
template <bool BASE>
__global__ __launch_bounds__(256) void vfd_sym_kernel(const double* base, int64_t ldb, const double* T, int64_t ldt, double den,
                                                      int64_t n, double* out, int64_t ldo) {
  __shared__ double tile[ST][ST + 1];
  const int bj = blockIdx.x, bi = blockIdx.y;
  if (bj > bi) return;
  const int tx = threadIdx.x & (ST - 1), ty = threadIdx.x / ST;
  const int64_t i = (int64_t)bi * ST + ty, j = (int64_t)bj * ST + tx;
  double v = 0.0;
  if (i < n && j <= i) {
    v = T[i * ldt + j] / den;
    if (BASE) v += base[i * ldb + j];
    out[i * ldo + j] = v;
  }
  tile[ty][tx] = v;
  __syncthreads();
  // element (ty, tx) of the mirrored tile (bj, bi) is element (tx, ty) of this one
  const int64_t mi = (int64_t)bj * ST + ty, mj = (int64_t)bi * ST + tx;
  if (mi < n && mj < n && mj > mi) out[mi * ldo + mj] = tile[tx][ty];
}

int launch_sym(gpx_ctx* ctx, const double* base, int64_t ldb, const double* T, int64_t ldt, double den, int64_t n, double* out,
               int64_t ldo) {
  const unsigned t = (unsigned)((n + ST - 1) / ST);
  ProfScope ps(ctx, GPX_PROF_REDUCE, (double)n * n, 8.0 * (base ? 2.0 : 1.5) * (double)n * n);
  if (base)
    hipLaunchKernelGGL(vfd_sym_kernel<true>, dim3(t, t), dim3(256), 0, ctx->stream, base, ldb, T, ldt, den, n, out, ldo);
  else
    hipLaunchKernelGGL(vfd_sym_kernel<false>, dim3(t, t), dim3(256), 0, ctx->stream, base, ldb, T, ldt, den, n, out, ldo);
  GPX_HIP(hipGetLastError());
  return 0;
}

// *d_tr (device) = tr(L^-1 G L^-T) over the first nu diagonal entries, summed in a fixed order; returns the buffer that holds
// L^-1 G L^-T (nup x nup, row stride ld): Y, or W when the left solve ran out of place (W != NULL).  dg: nup doubles of scratch.
int two_sided(gpx_ctx* ctx, gpx_mat* L, const gpx_mat* G, double* Y, double* W, int64_t ld, int64_t nu, double* dg, double* d_tr,
              double** sol_out) {
  const int64_t nup = L->prows;
  GPX_TRY(gpx_copy2d(ctx, G->p, G->ld, Y, ld, nup, nup));
  double* sol = W ? W : Y;
  GPX_TRY(chol_cross_solve(ctx, L, Y, ld, W, ld, nup));
  GPX_TRY(chol_trsm_right(ctx, L->p, L->ld, L->aux, sol, ld, nup, nup));
  {
    ProfScope ps(ctx, GPX_PROF_REDUCE, (double)nu, 16.0 * (double)nu);
    GPX_TRY(launch_diag(ctx, sol, ld, nu, dg));
    GPX_TRY(launch_sum(ctx, dg, nu, d_tr));
  }
  if (sol_out) *sol_out = sol;
  return 0;
}

// Quu = K(S,S) + noise I into K (nup x nup; identity on the padding)
int fill_quu(gpx_ctx* ctx, const gpx_vfe_design* ds, gpx_mat* K) {
  return launch_kfill(ctx, ds->kp, ds->S->p, ds->nu, ds->S->p, ds->nu, 1, nullptr, 1, ds->noise, K->p, ds->nup, ds->nup, K->ld);
}

// dst (nup x nup) = base + K(S,Xq) K(Xq,S) / noise;  T: a nup x nup work matrix of dst's row stride (may be dst itself, not base)
int add_gram(gpx_ctx* ctx, const gpx_vfe_design* ds, const KParams& kp, const gpx_mat* Xq, double* P, int64_t ldp, const gpx_mat* base,
             double* T, gpx_mat* dst) {
  const int64_t nup = ds->nup, qp = gpx_round_up(Xq->rows, GPX_TILE);
  GPX_TRY(launch_kfill(ctx, kp, ds->S->p, ds->nu, Xq->p, Xq->rows, 0, nullptr, 0, 0.0, P, nup, qp, ldp));
  GPX_TRY(launch_gemm(ctx, P, ldp, P, ldp, T, dst->ld, nup, nup, qp, true, false, true));
  return launch_sym(ctx, base->p, base->ld, T, dst->ld, ds->noise, nup, dst->p, dst->ld);
}

// D[k][u] = dk(x_k, s_u)/dx_k[l] (TRUE derivative: -c_l f (x_k[l] - s_u[l]), the table of acq.hip) for k < n, u < nu; zeros on the
// padding (rows < np, columns < nup), masked by index.  Workgroup = 256 columns of one row.
template <int KIND, int DMAX>
__global__ __launch_bounds__(256) void vfd_dkfill_kernel(KParams kp, const double* __restrict__ X, int64_t n, const double* __restrict__ S,
                                                         int64_t nu, int64_t nup, int l, double* __restrict__ D, int64_t ld) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (u >= nup) return;
  double v = 0.0;
  if (k < n && u < nu) {
    double p[DMAX], diff[DMAX];
#pragma unroll
    for (int q = 0; q < DMAX; ++q) p[q] = q < kp.d ? S[u * kp.d + q] : 0.0;
    const double f = radial_pair<KIND, DMAX>(kp, X + k * kp.d, p, diff);   // diff = x_k - s_u
    double c = kp.scale[l] * kp.scale[l];
    if (KIND == GPX_K_MATERN32) c *= kp.sig;
    if (KIND == GPX_K_MATERN52) c *= kp.sig / 3.0;
    double dl = 0.0;
#pragma unroll
    for (int q = 0; q < DMAX; ++q)
      if (q == l) dl = diff[q];
    v = -c * f * dl;
  }
  D[k * ld + u] = v;
}

int launch_dkfill(gpx_ctx* ctx, const KParams& kp, const gpx_mat* X, const gpx_mat* S, int64_t np, int64_t nup, int l, double* D,
                  int64_t ld) {
  const dim3 grid((unsigned)((nup + 255) / 256), (unsigned)np);
  ProfScope ps(ctx, GPX_PROF_KCROSS, 0.0, 8.0 * (double)np * nup);
#define GPX_CALL(K_, DM_) \
  hipLaunchKernelGGL((vfd_dkfill_kernel<K_, DM_>), grid, dim3(256), 0, ctx->stream, kp, X->p, X->rows, S->p, S->rows, nup, l, D, ld)
  GPX_RADIAL_DISPATCH(kp.kind, kp.d, GPX_CALL);
#undef GPX_CALL
  GPX_HIP(hipGetLastError());
  return 0;
}

// O[(k d + l) ldo + j] = s E[k][j] D[k][j] for k < n, j < mc: row block l of the chunk's result
__global__ __launch_bounds__(256) void vfd_vg_finish_kernel(const double* __restrict__ E, const double* __restrict__ D, int64_t ldm,
                                                            int64_t mc, int d, int l, double s, double* __restrict__ O, int64_t ldo) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (j >= mc) return;
  O[(k * d + l) * ldo + j] = s * E[k * ldm + j] * D[k * ldm + j];
}

int design_free(gpx_ctx* ctx, gpx_vfe_design* ds) {
  if (!ds) return 0;
  (void)hipStreamSynchronize(ctx->stream);
  if (ds->S) gpx_mat_free(ctx, ds->S);
  if (ds->Lu) gpx_mat_free(ctx, ds->Lu);
  if (ds->Gz) gpx_mat_free(ctx, ds->Gz);
  if (ds->A0) gpx_mat_free(ctx, ds->A0);
  delete ds;
  return 0;
}

}  // namespace

// (gpx_internal.h; the header comment has the formulas)
int vfe_var_grad_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* X, const gpx_mat* S, const gpx_mat* Z, double* out) {
  FitcView fv;
  fitc_view(f, &fv);
  const int64_t n = fv.n, nu = fv.nu, np = fv.np, nup = fv.nup, M = Z->rows;
  const int d = fv.kp->d;
  KParams kpx = *fv.kp, kpz = *fv.kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kpx, X, S));
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Z));
  const int64_t ldn = gpx_skew_ld(nup);
  const ChunkRange cr(M, gpx_eval_chunk(np * (d + 2) + nup));   // E, D and the d row blocks of the result, and C^T
  const int64_t mc_alloc = cr.mc_alloc, ldm = gpx_skew_ld(mc_alloc);
  Scratch tmp(ctx);   // its scope exit is the synchronisation the host result waits for
  double *Kxs, *Dk, *Ct, *E, *D, *O;
  GPX_TRY(tmp.get(np * ldn * 8, &Kxs));
  GPX_TRY(tmp.get(np * ldn * 8, &Dk));
  GPX_TRY(tmp.get(mc_alloc * ldn * 8, &Ct));
  GPX_TRY(tmp.get(np * ldm * 8, &E));
  GPX_TRY(tmp.get(np * ldm * 8, &D));
  GPX_TRY(tmp.get(n * d * ldm * 8, &O));
  GPX_TRY(launch_kfill(ctx, kpx, X->p, n, S->p, nu, 0, nullptr, 0, 0.0, Kxs, np, nup, ldn));
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, j0 = c.j0;
    // C^T = K(Zc,S) La^-T La^-1 (mcp x nup)
    GPX_TRY(launch_kfill(ctx, kpz, Z->p + j0 * d, mc, S->p, nu, 0, nullptr, 0, 0.0, Ct, mcp, nup, ldn));
    GPX_TRY(chol_trsm_right(ctx, fv.La->p, fv.La->ld, fv.La->aux, Ct, ldn, mcp, nup));
    GPX_TRY(chol_trsm_right_n(ctx, fv.La->p, fv.La->ld, fv.La->aux, Ct, ldn, mcp, nup));
    GPX_TRY(launch_gemm(ctx, Kxs, ldn, Ct, ldn, E, ldm, np, mcp, nup, true, false, false));
    for (int l = 0; l < d; ++l) {
      GPX_TRY(launch_dkfill(ctx, kpx, X, S, np, nup, l, Dk, ldn));
      GPX_TRY(launch_gemm(ctx, Dk, ldn, Ct, ldn, D, ldm, np, mcp, nup, true, false, false));
      ProfScope ps(ctx, GPX_PROF_REDUCE, 2.0 * (double)n * mc, 24.0 * (double)n * mc);
      hipLaunchKernelGGL(vfd_vg_finish_kernel, dim3((unsigned)((mc + 255) / 256), (unsigned)n), dim3(256), 0, ctx->stream,
                         (const double*)E, (const double*)D, ldm, mc, d, l, -2.0 / fv.noise, O, ldm);
      GPX_HIP(hipGetLastError());
    }
    GPX_HIP(hipMemcpy2DAsync(out + j0, (size_t)M * 8, O, (size_t)ldm * 8, (size_t)mc * 8, (size_t)(n * d), hipMemcpyDeviceToHost,
                             ctx->stream));
    if (!cr.last(c)) GPX_HIP(hipStreamSynchronize(ctx->stream));   // the next chunk overwrites O
  }
  return 0;
}

extern "C" {

int gpx_vfe_design_free(gpx_ctx* ctx, gpx_vfe_design* ds) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  return design_free(ctx, ds);
}

int gpx_vfe_design_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* S, double noise,
                          const gpx_mat* Z, gpx_vfe_design** out) {
  GPX_ARG(ctx && S && Z && out, "NULL argument");
  GPX_ARG(noise > 0.0, "vfe_design: the noise variance must be positive (it is the whole of G and the nugget of Quu)");
  GPX_ARG(S->rows >= 1 && Z->rows >= 1, "vfe_design: at least one inducing point and one Monte-Carlo point are required");
  GPX_ARG(S->cols == d && S->pcols == d && Z->cols == d && Z->pcols == d,
          "vfe_design: S and Z must be unpadded (nu x d) and (M x d) point sets");
  Held<gpx_vfe_design, design_free> ds(ctx, new gpx_vfe_design());
  ds->S = ds->Lu = ds->Gz = ds->A0 = nullptr;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &ds->kp));
  GPX_TRY(gpx_mat_clone(ctx, S, &ds->S));
  GPX_TRY(gpx_kparams_sets(ctx, &ds->kp, ds->S));
  const int64_t nu = S->rows, M = Z->rows;
  ds->nu = nu;
  ds->m = M;
  ds->pinned = 0;
  ds->noise = noise;
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, &ds->Lu));
  const int64_t nup = ds->nup = ds->Lu->prows, ldn = ds->Lu->ld;
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, &ds->Gz));
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, &ds->A0));
  GPX_TRY(fill_quu(ctx, ds.get(), ds->Lu));
  GPX_TRY(fitc_factor(ctx, ds->Lu, "K(inducing, inducing) + noise"));
  GPX_TRY(fill_quu(ctx, ds.get(), ds->A0));
  // Gz = sum over the chunks of K(S,Zc) K(Zc,S), in index order: launch_gemm accumulates as C - A B^T, so the sum is built negated
  // from zero and the scale is -1 / M
  KParams kpz = ds->kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, ds->S, Z));
  const ChunkRange cr(M, gpx_eval_chunk(nup));
  const bool oop = chol_cross_oop(nup);
  MatHold Y(ctx), W(ctx);
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, Y.put()));
  if (oop) GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, W.put()));
  Scratch tmp(ctx);
  double *B, *kd, *dg;
  GPX_TRY(tmp.get(nup * gpx_skew_ld(cr.mc_alloc) * 8, &B));
  GPX_TRY(tmp.get(M * 8, &kd));
  GPX_TRY(tmp.get((nup + 8) * 8, &dg));
  GPX_HIP(hipMemsetAsync(ds->Gz->p, 0, (size_t)ds->Gz->bytes, ctx->stream));
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, ldb = gpx_skew_ld(mcp);
    GPX_TRY(launch_kfill(ctx, kpz, ds->S->p, nu, Z->p + c.j0 * d, mc, 0, nullptr, 0, 0.0, B, nup, mcp, ldb));
    GPX_TRY(launch_gemm(ctx, B, ldb, B, ldb, ds->Gz->p, ldn, nup, nup, mcp, true, true, true));
  }
  GPX_TRY(launch_sym(ctx, nullptr, 0, ds->Gz->p, ldn, -(double)M, nup, ds->Gz->p, ldn));
  // kbar and c0
  GPX_TRY(launch_kdiag(ctx, ds->kp, Z->p, M, kd));
  GPX_TRY(launch_sum(ctx, kd, M, dg + nup));
  GPX_TRY(two_sided(ctx, ds->Lu, ds->Gz, Y->p, oop ? W->p : nullptr, ldn, nu, dg, dg + nup + 1, nullptr));
  double h[2];
  GPX_HIP(hipMemcpyAsync(h, dg + nup, 16, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  ds->kbar = h[0] / (double)M;
  ds->c0 = h[1];
  *out = ds.release();
  return 0;
}

int gpx_vfe_design_pin(gpx_ctx* ctx, gpx_vfe_design* ds, const gpx_mat* Xp) {
  GPX_ARG(ctx && ds, "NULL argument");
  const int d = ds->kp.d;
  GPX_ARG(!Xp || Xp->rows == 0 || (Xp->cols == d && Xp->pcols == d), "vfe_design_pin: Xp must be an unpadded (p x d) point set");
  GPX_TRY(fill_quu(ctx, ds, ds->A0));
  ds->pinned = 0;
  if (!Xp || Xp->rows == 0) return 0;
  KParams kp = ds->kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kp, ds->S, Xp));
  const int64_t pp = gpx_round_up(Xp->rows, GPX_TILE), ldp = gpx_skew_ld(pp);
  MatHold T(ctx);
  GPX_TRY(gpx_mat_new(ctx, ds->nu, ds->nu, 1, T.put()));
  Scratch tmp(ctx);
  double* P;
  GPX_TRY(tmp.get(ds->nup * ldp * 8, &P));
  GPX_TRY(add_gram(ctx, ds, kp, Xp, P, ldp, ds->A0, T->p, ds->A0));
  ds->pinned = Xp->rows;
  return 0;
}

int gpx_vfe_design_eval(gpx_ctx* ctx, const gpx_vfe_design* ds, const gpx_mat* Xf, double* cost, double* grad) {
  GPX_ARG(ctx && ds && Xf && cost, "NULL argument");
  const int d = ds->kp.d;
  GPX_ARG(Xf->rows >= 1, "vfe_design_eval: at least one free design point is required");
  GPX_ARG(Xf->cols == d && Xf->pcols == d, "vfe_design_eval: Xf must be an unpadded (b x d) point set");
  GPX_ARG(!grad || ds->kp.kind == GPX_K_SE || ds->kp.kind == GPX_K_MATERN32 || ds->kp.kind == GPX_K_MATERN52,
          "vfe_design_eval: the gradient exists for the squared exponential and the isotropic Materns only, not for the Mehler "
          "kernel (the cost does: pass grad = NULL)");
  const int64_t nu = ds->nu, nup = ds->nup, ldn = ds->A0->ld, b = Xf->rows, bp = gpx_round_up(b, GPX_TILE), ldp = gpx_skew_ld(bp);
  KParams kp = ds->kp;
  GPX_TRY(gpx_kparams_sets(ctx, &kp, ds->S, Xf));
  const bool oop = chol_cross_oop(nup);
  MatHold La(ctx), Y(ctx), W(ctx);
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, La.put()));
  GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, Y.put()));
  if (oop) GPX_TRY(gpx_mat_new(ctx, nu, nu, 1, W.put()));
  Scratch tmp(ctx);
  // P (nup x ldp) is dead after the SYRK: its storage then holds V^T Y1 and H^T (bp x ldn)
  const int64_t pbytes = (nup * ldp > bp * ldn ? nup * ldp : bp * ldn) * 8;
  double *P, *dg;
  GPX_TRY(tmp.get(pbytes, &P));
  GPX_TRY(tmp.get((nup + 8) * 8, &dg));
  GPX_TRY(add_gram(ctx, ds, kp, Xf, P, ldp, ds->A0, La->p, La.get()));
  GPX_TRY(fitc_factor(ctx, La.get(), "Quu + K(S,X) K(X,S) / noise"));
  double* Y1 = nullptr;
  GPX_TRY(two_sided(ctx, La.get(), ds->Gz, Y->p, oop ? W->p : nullptr, ldn, nu, dg, dg + nup, &Y1));
  double tr = 0.0;
  GPX_HIP(hipMemcpyAsync(&tr, dg + nup, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (!grad) {
    GPX_HIP(hipStreamSynchronize(ctx->stream));
    *cost = ds->kbar - ds->c0 + tr;
    return 0;
  }
  double *Pt, *ppart, *gout;
  GPX_TRY(tmp.get(bp * ldn * 8, &Pt));
  GPX_TRY(tmp.get(fitc_wgrad_partial_elems(b, nu, d) * 8, &ppart));
  GPX_TRY(tmp.get(b * d * 8, &gout));
  GPX_TRY(launch_kfill(ctx, kp, Xf->p, b, ds->S->p, nu, 0, nullptr, 0, 0.0, Pt, bp, nup, ldn));
  GPX_TRY(chol_trsm_right(ctx, La->p, La->ld, La->aux, Pt, ldn, bp, nup));                  // V^T = P^T La^-T
  GPX_TRY(launch_gemm(ctx, Pt, ldn, Y1, ldn, P, ldn, bp, nup, nup, false, false, false));   // V^T Y1
  GPX_TRY(chol_trsm_right_n(ctx, La->p, La->ld, La->aux, P, ldn, bp, nup));                 // H^T
  GPX_TRY(fitc_wgrad_rows(ctx, kp, Xf, ds->S, P, ldn, ppart, gout));
  GPX_HIP(hipMemcpyAsync(grad, gout, (size_t)(b * d) * 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  *cost = ds->kbar - ds->c0 + tr;
  const double s = -2.0 / ds->noise;
  for (int64_t i = 0; i < b * d; ++i) grad[i] *= s;
  return 0;
}

int gpx_vfe_design_shape(const gpx_vfe_design* ds, int64_t* nu, int64_t* m, int64_t* pinned) {
  GPX_ARG(ds != nullptr, "vfe design state is NULL");
  if (nu) *nu = ds->nu;
  if (m) *m = ds->m;
  if (pinned) *pinned = ds->pinned;
  return 0;
}

}  // extern "C"
