// Leave-one-out cross-validation from the factor, with its hyper-parameter gradient -- gfx950.  The reference has no
// counterpart (a user of it refits N times through GP.train); Rasmussen & Williams 5.4.2.
//
// Zero prior mean, K including the nugget D = diag(noise); P = K^-1, alpha = P y, p_i = P_ii:
//   mu_i = y_i - alpha_i / p_i,  var_i = 1 / p_i        predictive distribution of the OBSERVATION y_i given all the others
//   L_LOO = sum_i [ 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log 2 pi ]
//   dL_LOO / d theta = sum_i ( alpha_i a_i - 1/2 (1 + alpha_i^2 / p_i) q_i ) / p_i
//       with W = P dK/d theta,  a_i = (W alpha)_i,  q_i = sum_l W_il P_il  (= [P dK P]_ii, P being symmetric)
//
//  gpx_loo       needs diag(P) only: L^-1 by the halving recursion (chol_trtri, N^3/3), p_i = column sum of squares of L^-1
//                (launch_colreduce), alpha by chol_potrs, one finishing kernel, launch_sum.  No N x N K^-1, no symmetric product.
//  gpx_loo_grad  full symmetric P (gpx_potri_impl, 2 N^3 / 3).  Per LENGTH-type parameter (d for SE, one rho for Matern): a tiled
//                fill writes dK (8 N^2 bytes), W = P dK is one fp64-MFMA product (2 N^3) in row slabs, a fused row kernel reads
//                the rows of W and P once for both dots (16 N^2 bytes).  signalSize and noise need no product:
//                  noise (dK = I):          a = P alpha,                         q_i = sum_l P_il^2
//                  signalSize (dK = K0/s):  P K0 = I - P D  ->  a = (alpha - P (D o alpha)) / s,  q_i = (p_i - sum_l P_il^2 D_l) / s
//                i.e. row reductions over P (launch_rowreduce); with a scalar nugget the signalSize sums are the noise sums scaled.
//
// Every reduction is a fixed-shape tree (no floating-point atomics): two calls agree bit for bit.
//
// PADDING.  The factor's storage is padded to a multiple of 128 with an IDENTITY extension (gpx.h): rows / columns >= n of L are
// unit vectors, so L^-1 = [L11^-1 0; 0 I] and P = [K^-1 0; 0 I] there -- finite, and exactly 0 off the diagonal.  Nothing below
// relies on more than FINITE: the column reduction of L^-1 stops at row n, the row reductions over P run over the first n rows
// with weight vectors that are exactly 0 from n on (a mask of ones for the unweighted sum of squares), dK has exact zeros in its
// padding (so padded rows of P cannot enter W = P dK), and the fused row kernel reads columns < n only.
#include "gpx_internal.h"
#include <math.h>
#include <vector>

namespace {

constexpr int TS = 64;

// One row's term of the gradient sum from its two row quantities.
__device__ __forceinline__ double loo_term(double al, double p, double a, double q) {
  return (al * a - 0.5 * (1.0 + al * al / p) * q) / p;
}

// mu, var (each nullable) and the log predictive probability of every point; p_i = pd[i * pstride] (a vector, or the diagonal of P)
__global__ __launch_bounds__(256) void loo_finish_kernel(int64_t n, const double* __restrict__ y, const double* __restrict__ alpha,
                                                         const double* __restrict__ pd, int64_t pstride, double* __restrict__ mean,
                                                         double* __restrict__ var, double* __restrict__ lp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p = pd[i * pstride], al = alpha[i];
  if (mean) mean[i] = y[i] - al / p;
  if (var) var[i] = 1.0 / p;
  lp[i] = 0.5 * log(p) - 0.5 * al * al / p - 0.9189385332046727418;  // 1/2 log 2 pi
}

// Full symmetric dK/d theta_q WITHOUT its 1 / theta_q (the host divides the finished sum), over the padded np x np storage (row
// stride ld), 64 x 64 tiles, exact zeros in the padding.  Conventions of lml_pair (hyper.hip): coordinate differences first, then
// scaled; acc = the scaled squared distance.
//   SE, length q:   K0 e_q^2,  e_q = (x_q - x'_q) / cl_q
//   Matern 3/2:     rho dk/d rho = s t^2 e^-t;      5/2:  s t^2 (1 + t) e^-t / 3
// (a - b) = -(b - a) exactly and the sum runs in the same order, so the two triangles agree bit for bit.
__global__ __launch_bounds__(256) void loo_dkfill_kernel(KParams kp, const double* __restrict__ X, int64_t n, int q,
                                                         double* __restrict__ out, int64_t ld) {
  extern __shared__ double sm[];
  const int d = kp.d;
  double* As = sm;           // [TS][d] raw coords of the row points
  double* Bs = sm + TS * d;  // [TS][d] of the column points
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * TS, j0 = (int64_t)blockIdx.x * TS;
  for (int idx = t; idx < TS * d; idx += 256) {
    int p = idx / d, k = idx - p * d;
    int64_t gi = i0 + p, gj = j0 + p;
    As[idx] = gi < n ? X[gi * d + k] : 0.0;
    Bs[idx] = gj < n ? X[gj * d + k] : 0.0;
  }
  __syncthreads();
  const int tx = t & 31, ty = t >> 5;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int r = ty + 8 * a;
    const int64_t gi = i0 + r;
    double v[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cc = 2 * tx + c;
      const int64_t gj = j0 + cc;
      v[c] = 0.0;
      if (gi < n && gj < n) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
          const double e = (As[r * d + k] - Bs[cc * d + k]) * kp.scale[k];
          acc = fma(e, e, acc);
        }
        if (kp.kind == GPX_K_SE) {
          const double e = (As[r * d + q] - Bs[cc * d + q]) * kp.scale[q];
          v[c] = kp.sig * exp(-0.5 * acc) * (e * e);
        } else {
          const double tt = sqrt(acc), ex = kp.sig * exp(-tt);
          v[c] = kp.kind == GPX_K_MATERN32 ? acc * ex : acc * (1.0 + tt) * ex * (1.0 / 3.0);
        }
      }
    }
    *reinterpret_cast<double2*>(out + gi * ld + j0 + 2 * tx) = make_double2(v[0], v[1]);
  }
}

// One workgroup per row i = r0 + blockIdx.x (< n) of a slab of W = P dK: reads the rows of W and P once, forms
// q_i = sum_l W_il P_il and a_i = sum_l W_il alpha_l over the columns l < n (every thread a fixed strided subset, fixed-shape trees
// over the 256 partial sums) and writes the row's term of the gradient sum.  alpha: zero padded to an even length >= n.
__global__ __launch_bounds__(256) void loo_rowdots_kernel(const double* __restrict__ W, int64_t ldw, const double* __restrict__ P,
                                                          int64_t ldp, int64_t r0, int64_t n, const double* __restrict__ alpha,
                                                          double* __restrict__ out) {
  __shared__ double redq[256];
  __shared__ double reda[256];
  const int t = threadIdx.x;
  const int64_t i = r0 + blockIdx.x;
  const double* w = W + (int64_t)blockIdx.x * ldw;
  const double* p = P + i * ldp;
  double q0 = 0.0, q1 = 0.0, a0 = 0.0, a1 = 0.0;
  for (int64_t c = 2 * t; c < n; c += 512) {
    double2 wv = *reinterpret_cast<const double2*>(w + c);
    double2 pv = *reinterpret_cast<const double2*>(p + c);
    const double2 av = *reinterpret_cast<const double2*>(alpha + c);
    if (c + 1 >= n) wv.y = pv.y = 0.0;  // odd n: the second column of the last pair is padding
    q0 = fma(wv.x, pv.x, q0);
    q1 = fma(wv.y, pv.y, q1);
    a0 = fma(wv.x, av.x, a0);
    a1 = fma(wv.y, av.y, a1);
  }
  redq[t] = q0 + q1;
  reda[t] = a0 + a1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      redq[t] += redq[t + s];
      reda[t] += reda[t + s];
    }
    __syncthreads();
  }
  if (t == 0) out[i] = loo_term(alpha[i], p[i], reda[0], redq[0]);
}

// The same term for the parameters whose row quantities are row reductions over P:
//   a_i = ca0 alpha_i + ca1 av_i,   q_i = cq0 p_i + cq1 qv_i     (p_i = the diagonal of P)
__global__ __launch_bounds__(256) void loo_rowterm_kernel(int64_t n, const double* __restrict__ alpha, const double* __restrict__ P,
                                                          int64_t ldp, const double* __restrict__ av, double ca0, double ca1,
                                                          const double* __restrict__ qv, double cq0, double cq1,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p = P[i * (ldp + 1)], al = alpha[i];
  out[i] = loo_term(al, p, fma(ca0, al, ca1 * av[i]), fma(cq0, p, cq1 * qv[i]));
}

// v[i] = a[i] * b[i] (b nullable: a copy), i < n
__global__ __launch_bounds__(256) void loo_vecmul_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                         double* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = b ? a[i] * b[i] : a[i];
}

__global__ __launch_bounds__(256) void loo_ones_kernel(int64_t n, double* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = 1.0;
}

inline dim3 blocks256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// dv (np doubles) <- alpha = K^-1 y: y zero padded, solved in place
int loo_alpha(gpx_ctx* ctx, const gpx_mat* L, const double* y, double* dy, double* dv, double* potrs_scratch) {
  const int64_t n = L->rows, np = L->prows;
  GPX_TRY(gpx_fill_padded(ctx, dy, y, n, np));
  GPX_HIP(hipMemcpyAsync(dv, dy, (size_t)np * 8, hipMemcpyDeviceToDevice, ctx->stream));
  return chol_potrs(ctx, const_cast<gpx_mat*>(L), dv, potrs_scratch);  // caches the block inverses in L, as gpx_potrs does
}

}  // namespace

extern "C" {

int gpx_loo(gpx_ctx* ctx, const gpx_mat* L, const double* y, double* mean, double* var, double* logp) {
  GPX_ARG(ctx && L && y && logp, "NULL argument");
  GPX_ARG(L->factored && L->aux, "matrix has not been factored by gpx_potrf");
  const int64_t n = L->rows, np = L->prows;
  GPX_ARG(n >= 1 && L->cols == n, "the factor must be square");
  Scratch sc(ctx);
  double *pI, *ptmp, *pdy, *pal, *pps, *pp, *ppart, *pm, *pv, *plp;
  GPX_TRY(sc.get(np * np * 8, &pI));
  GPX_TRY(sc.get((np / 2 + 64) * (np / 2 + 64) * 8, &ptmp));
  GPX_TRY(sc.get(np * 8, &pdy));
  GPX_TRY(sc.get(np * 8, &pal));
  GPX_TRY(sc.get(chol_potrs_scratch_bytes(np), &pps));
  GPX_TRY(sc.get(np * 8, &pp));
  GPX_TRY(sc.get(colreduce_partial_elems(n, np) * 8, &ppart));
  GPX_TRY(sc.get(n * 8, &pm));
  GPX_TRY(sc.get(n * 8, &pv));
  GPX_TRY(sc.get(n * 8, &plp));
  GPX_TRY(loo_alpha(ctx, L, y, pdy, pal, pps));
  GPX_TRY(chol_trtri(ctx, L, pI, ptmp));  // L^-1, zero above the diagonal
  // p_j = sum over the rows i < n of (L^-1)_ij^2 (rows >= n are the identity extension: see PADDING)
  GPX_TRY(launch_colreduce(ctx, pI, np, n, np, nullptr, pp, ppart));
  {
    ProfScope ps(ctx, GPX_PROF_REDUCE, 0.0, 48.0 * (double)n);
    hipLaunchKernelGGL(loo_finish_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, (const double*)pdy, (const double*)pal,
                       (const double*)pp, (int64_t)1, mean ? pm : nullptr, var ? pv : nullptr, plp);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, plp, n, ctx->d_scal));
  if (mean) GPX_HIP(hipMemcpyAsync(mean, pm, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (var) GPX_HIP(hipMemcpyAsync(var, pv, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipMemcpyAsync(logp, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_loo_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const double* nugget, int64_t nugget_len, const double* y, int64_t slab_rows, double* logp, double* grad) {
  GPX_ARG(ctx && L && X && y && logp && grad, "NULL argument");
  GPX_ARG(kind == GPX_K_SE || kind == GPX_K_MATERN32 || kind == GPX_K_MATERN52,
          "loo_grad: hyper-parameter derivatives exist for the squared exponential and the isotropic Materns (as gpx_lml_grad); "
          "gpx_loo itself takes every kernel");
  KParams kp;
  GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, nullptr, nullptr, "X does not match the factor", &kp));
  const int64_t n = L->rows, np = L->prows;
  GPX_ARG(n >= 1 && L->cols == n, "the factor must be square");
  GPX_ARG(nugget_len == 0 || nugget_len == 1 || nugget_len == n, "nugget_len must be 0, 1 or N");
  GPX_ARG(nugget_len == 0 || nugget != nullptr, "nugget is NULL");
  GPX_ARG(slab_rows >= 0 && slab_rows % GPX_TILE == 0, "slab_rows must be 0 (auto) or a multiple of 128");
  const int nlen = kind == GPX_K_SE ? d : 1;
  const double sig = hyp[nlen];
  // a per-point nugget of length 1 is the scalar (n == 1)
  const bool per_point = nugget_len > 1;
  const double nscal = nugget_len == 1 ? nugget[0] : 0.0;
  MatHold P(ctx);
  GPX_TRY(gpx_potri_impl(ctx, L, P.put(), 1));  // both triangles: the rows of P are read whole
  Scratch sc(ctx);
  double *pdy, *pal, *pps, *pone, *pD = nullptr, *pDal = nullptr, *pav, *pqv, *pterm, *plp, *out, *pdK = nullptr;
  void* pW = nullptr;
  GPX_TRY(sc.get(np * 8, &pdy));
  GPX_TRY(sc.get(np * 8, &pal));
  GPX_TRY(sc.get(chol_potrs_scratch_bytes(np), &pps));
  GPX_TRY(sc.get(np * 8, &pone));
  GPX_TRY(sc.get(np * 8, &pav));
  GPX_TRY(sc.get(np * 8, &pqv));
  GPX_TRY(sc.get(np * 8, &pterm));
  GPX_TRY(sc.get(np * 8, &plp));
  GPX_TRY(sc.get((nlen + 3) * 8, &out));  // [0, nlen): lengths, nlen: signalSize, nlen + 1: noise, nlen + 2: L_LOO
  const double* al = pal;
  GPX_TRY(loo_alpha(ctx, L, y, pdy, pal, pps));
  // ---- value: p_i from the diagonal of P
  {
    ProfScope ps(ctx, GPX_PROF_REDUCE, 0.0, 32.0 * (double)n);
    hipLaunchKernelGGL(loo_finish_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, (const double*)pdy, al, (const double*)P->p,
                       P->ld + 1, (double*)nullptr, (double*)nullptr, plp);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, plp, n, out + nlen + 2));
  // ---- noise: a = P alpha, q_i = sum_l P_il^2 (weights: ones below n, zeros from n on)
  GPX_HIP(hipMemsetAsync(pone, 0, (size_t)np * 8, ctx->stream));
  hipLaunchKernelGGL(loo_ones_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, pone);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_rowreduce(ctx, P->p, P->ld, n, np, al, pav, 0));
  GPX_TRY(launch_rowreduce(ctx, P->p, P->ld, n, np, pone, pqv, 1));
  hipLaunchKernelGGL(loo_rowterm_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, al, (const double*)P->p, P->ld,
                     (const double*)pav, 0.0, 1.0, (const double*)pqv, 0.0, 1.0, pterm);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, pterm, n, out + nlen + 1));
  // ---- signalSize: P K0 = I - P D.  Scalar nugget: the noise sums scaled; per point: two more row reductions
  if (per_point) {
    GPX_TRY(sc.get(np * 8, &pD));
    GPX_TRY(sc.get(np * 8, &pDal));
    GPX_HIP(hipMemsetAsync(pD, 0, (size_t)np * 8, ctx->stream));
    GPX_HIP(hipMemsetAsync(pDal, 0, (size_t)np * 8, ctx->stream));
    GPX_HIP(hipMemcpyAsync(pD, nugget, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(loo_vecmul_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, (const double*)pD, al, pDal);
    GPX_HIP(hipGetLastError());
    GPX_TRY(launch_rowreduce(ctx, P->p, P->ld, n, np, pDal, pav, 0));
    GPX_TRY(launch_rowreduce(ctx, P->p, P->ld, n, np, pD, pqv, 1));
  }
  {
    const double c = per_point ? 1.0 : nscal;
    hipLaunchKernelGGL(loo_rowterm_kernel, blocks256(n), dim3(256), 0, ctx->stream, n, al, (const double*)P->p, P->ld,
                       (const double*)pav, 1.0 / sig, -c / sig, (const double*)pqv, 1.0 / sig, -c / sig, pterm);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, pterm, n, out + nlen));
  // ---- lengths: dK, W = P dK in row slabs, fused row dots.  dK and W take the row stride np: their blocks then have the size
  // of the two N x N work matrices gpx_potri_impl has just handed back to the pool
  GPX_TRY(sc.get(np * np * 8, &pdK));
  int64_t slab = slab_rows == 0 || slab_rows > np ? np : slab_rows;
  if (slab_rows == 0) {
    // auto: the whole matrix when it fits, otherwise the largest slab the free memory admits (after the pool has been given
    // back: gpx_dev_alloc trims it before it gives up).  Not GPX_TRY: a refused size is retried smaller, and when nothing fits
    // gpx_dev_alloc's own out-of-memory text stands, which the Python side recognises
    if (gpx_dev_alloc(ctx, slab * np * 8, &pW) != 0) {
      pW = nullptr;
      size_t fr = 0, tot = 0;
      GPX_HIP(hipMemGetInfo(&fr, &tot));
      slab = (int64_t)((double)fr * 0.9 / (8.0 * (double)np)) / GPX_TILE * GPX_TILE;
      if (slab > np) slab = np;
      while (slab >= GPX_TILE && gpx_dev_alloc(ctx, slab * np * 8, &pW) != 0) {
        pW = nullptr;
        slab = slab / 2 / GPX_TILE * GPX_TILE;
      }
      if (!pW) return -2;
    }
    sc.adopt(pW, slab * np * 8);
  } else {
    GPX_TRY(sc.get(slab * np * 8, &pW));
  }
  for (int q = 0; q < nlen; ++q) {
    {
      ProfScope ps(ctx, GPX_PROF_KFILL, 0.0, 8.0 * (double)np * np);
      const size_t sh = (size_t)(2 * TS * d) * sizeof(double);
      hipLaunchKernelGGL(loo_dkfill_kernel, dim3((unsigned)(np / TS), (unsigned)(np / TS)), dim3(256), sh, ctx->stream, kp,
                         X->p, n, q, pdK, np);
    }
    GPX_HIP(hipGetLastError());
    for (int64_t r0 = 0; r0 < n; r0 += slab) {
      const int64_t m = r0 + slab <= np ? slab : np - r0;          // rows of W in this slab (a multiple of 128)
      const int64_t rows = r0 + m <= n ? m : n - r0;               // of them real points
      GPX_TRY(launch_gemm(ctx, P->p + r0 * P->ld, P->ld, pdK, np, (double*)pW, np, m, np, np, false, false, false));
      ProfScope ps(ctx, GPX_PROF_REDUCE, 4.0 * (double)rows * n, 16.0 * (double)rows * n);
      hipLaunchKernelGGL(loo_rowdots_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const double*)pW, np,
                         (const double*)P->p, P->ld, r0, n, al, pterm);
    }
    GPX_HIP(hipGetLastError());
    GPX_TRY(launch_sum(ctx, pterm, n, out + q));
  }
  std::vector<double> h((size_t)nlen + 3);
  GPX_HIP(hipMemcpyAsync(h.data(), out, (size_t)(nlen + 3) * 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  // dK/d cl_k = K0 e_k^2 / cl_k;  dK/d rho = (rho dk/d rho) / rho
  for (int k = 0; k < nlen; ++k) grad[k] = h[(size_t)k] / hyp[k];
  grad[nlen] = h[(size_t)nlen];
  grad[nlen + 1] = h[(size_t)nlen + 1];
  *logp = h[(size_t)nlen + 2];
  return 0;
}

}  // extern "C"
