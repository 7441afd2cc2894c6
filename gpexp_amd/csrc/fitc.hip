// f4: FITC sparse approximation -- gfx950.
//
// Replaces the reference's dense construction (gp.py:182-210, 401-426; gp_kernel_utilities.py:70-104), which forms the
// N x N matrices Q = Kfu Quu^-1 Kuf, K, G = diag(K - Q), and the Woodbury precision
//     P = Gi - Gi Kfu (Quu + Kuf Gi Kfu)^-1 Kuf Gi,          Gi = diag(1 / (g + 1e-12)),
// and then runs the dense N x N prediction loops on P.  Here nothing N x N is ever formed on the product path: with
// nu inducing points the model is  Lu = chol(Quu),  Kuf (nu x N),  W = Lu^-1 Kuf,  g = diag(K) - colsum(W^2),
// Ks = -Kuf Gi,  La = chol(Quu + Kuf Gi Kfu)  -- all built from the kfill / potrf / TRSM / GEMM / reduction kernels of
// the dense path -- and
//     P y      = Gi (y - Kfu A^-1 Kuf Gi y)                                   (two reductions + one nu x nu solve)
//     log|Q+G| = sum log g + log|A| - log|Quu|                                (determinant lemma)
//     var(z)   = k(z,z) - sum_i Gi_i k_zi^2 + |La^-1 Kuf Gi k_z|^2           (one NT GEMM + one right TRSM per chunk)
// Quu and K both carry the nugget, exactly as the reference builds them.  gpx_fitc_dense materialises Q + G and P for
// the reference's `covarianceMatrix` / `precisionMatrix` attributes (small N only; parity tests).
//
// gpx_fitc_lml_grad: the hyper-parameter gradient of that likelihood (none in the reference: its own is unrunnable).  With
// B = Quu^-1 Kuf, alpha = P y, M = alpha alpha^T - P (N x N, never formed), m = diag M, Y = La^-1 Ks:
//     m_i = alpha_i^2 - Gi_i + |Y[:, i]|^2
//     R   = B (M - diag m) = (B alpha) alpha^T + (B Ks^T La^-T) Y - B diag(Gi + m)        (nu x N)
//     T   = R B^T                                                                        (nu x nu, symmetric)
//     dL/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) + sum_i m_i dk(x_i,x_i) ],   dL/d noise = 1/2 [ sum m - tr T ]
// Two nu x nu x N solves (B through Lu, Y through La) and three nu x nu x N products (B Ks^T, its product with Y, R B^T) on the
// fp64-MFMA GEMM; the sums against dKuf and dK(S,S) come from ONE tiled kernel (fitc_wsum_kernel) that recomputes the
// derivative of every pair from the point coordinates and stores none of the d derivative matrices.  Working memory:
// THREE nu x N buffers (B^T then the solve's input then R; B; Y) and TWO nu x nu ones (B Ks^T, T), plus vectors and the
// per-tile partial sums.
//
// gpx_fitc_lml_grad_inducing: the same call also returns dL/dS, the gradient w.r.t. the inducing-point LOCATIONS (the pseudo-inputs
// of Snelson & Ghahramani; nothing here assumes S is a subset of X).  Moving s_u changes row u of Kuf and row and column u of
// K(S,S); the diagonals k(s_u,s_u), k(x_i,x_i) and the nugget inside Quu do not depend on S.  So, with the R and T above,
//     dL/ds_u[l] = sum_i R[u][i] dk(s_u, x_i)/ds_u[l] - sum_v 1/2 (T[u][v] + T[v][u]) dk(s_u, s_v)/ds_u[l]
// with the TRUE point derivatives of acq.hip's table (zero and smooth at coincident points: S a subset of X needs no special case;
// the v = u term vanishes).  T is symmetric up to round-off (~1e-15 of its largest entry), and row u of T is used for both halves.
// No further solve or product: one row-wise weighted pass over the nu x N and the nu x nu pairs (fitc_wgrad_kernel, launched
// twice), of the size of the two fitc_wsum_kernel passes, and a small kernel that adds its per-segment partials in index order.
// Scratch grows by those partials (segments x nu x d) and the nu x d result; nothing of size nu x N x d exists.
//
// gpx_fitc_loo / gpx_fitc_loo_grad: leave-one-out cross-validation UNDER THE MODEL'S OWN PRIOR of the observations, N(0, Q + G) (the
// covariance the likelihood above scores; P is its precision), and the hyper-parameter gradient of its log predictive probability.
// p(y_i | y_-i) is the Gaussian conditional of N(0, Q + G) -- FITC refitted on X \ {x_i} with the same inducing points, y_i
// predicted through Q -- and NOT gpx_fitc_posterior at x_i after such a refit, which keeps the reference's true k(z, X) against P.
// With ssq_i = |Y[:, i]|^2 (P = Gi - Y^T Y):
//     p_i = P_ii = ginv_i - ssq_i,   mean_i = y_i - alpha_i / p_i,   var_i = 1 / p_i,   L = sum_i [1/2 log p_i - alpha_i^2 / (2 p_i)] - N/2 log 2 pi
// gpx_fitc_loo is the set-up the gradients share (alpha, Y by one nu x nu x N solve, ssq by one column reduction) and one
// element-wise kernel; the terms of L are formed and summed as gpx_loo does (loo.hip).  The gradient is dL = 1/2 tr(M dKt) with
//     r = alpha / p,  b = P r,  c_i = (1 + alpha_i^2 / p_i) / p_i,  C = diag(c),     M = alpha b^T + b alpha^T - P C P,  m = diag M
// (M symmetric, N x N, never formed), and from R = B (M - diag m) on it IS gpx_fitc_lml_grad: T = R B^T, the two weighted passes, tr T
// and the host assembly are one body (fitc_grad_tail), as is the set-up (fitc_work_begin).  Upstream of R only nu-sized objects:
//     C1 = B Y^T,   H = Y C Y^T,   C2 = (B diag(ginv o c)) Y^T - C1 H                                            (nu x nu each)
//     B P C P       = B diag(ginv^2 o c) - (C1 Y) diag(c o ginv) - C2 Y
//     diag(P C P)_i = ginv_i^2 c_i - 2 ginv_i c_i ssq_i + sum_k Y_ki (H Y)_ki
//     R             = C2 Y + C1 (Y diag(c o ginv)) + (B alpha) b^T + (B b) alpha^T - B diag(ginv^2 o c + m)
// Seven nu x nu x N products through launch_gemm (H, H Y, C1, the scaled B Y^T, C2 Y, C1 (Y diag(c o ginv)) -- subtracted into C2 Y's
// result with Y scaled by -(c o ginv) in place, launch_gemm accumulating as C - A B --, T) and one nu^3 (C1 H), beside the two
// solves: about twice gpx_fitc_lml_grad.  The column sums sum_k Y_ki (H Y)_ki go through launch_colreduce (the product times Y entry
// by entry, weights of one), b through launch_rowreduce + launch_colreduce; the new kernels are element-wise (fitc_loo_terms_kernel,
// fitc_loo_mdiag_kernel, fitc_loo_r_kernel, scale_cols_to_kernel): padding written as zeros, masked by index, two columns per thread
// where fitc_r_kernel does so.  No atomics; every reduction in a fixed order.  Working memory: THREE nu x N buffers (the consumed
// copy / Y C / H Y / the scaled B / R in turn; B; Y) and THREE nu x nu ones (C1, C2, H then T), vectors and the per-tile partial
// sums; gpx_fitc_loo: two nu x N buffers and vectors.  Nothing N x N.  p_i <= 0 or not finite: no test, as gpx_loo -- the
// arithmetic's NaN (log) or negative variance comes back.
//
// gpx_vfe_*: Titsias' variational free energy on the same struct.  A VFE model is a gpx_fitc whose G is the CONSTANT noise I
// (g = noise, ginv = 1 / noise exactly, no 1e-12 guard; Quu keeps the nugget: inducing variables u = f(S) + eps), flagged `vfe`,
// with one more scalar trres = sum_i (k(x_i,x_i) - Q_ii) reduced in a fixed order at fit time.  Solve, log-determinant, dense and
// free work on it as they are; with Kt = Q + noise I, P = Kt^-1, alpha = P y:
//     F = -1/2 y^T alpha - 1/2 log det Kt - N/2 log 2 pi - trres / (2 noise)
//     R = B (M + I / noise) = (B alpha) alpha^T + (B Y^T) Y      (no diagonal correction),      T = R B^T
//     dF/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) - (N / noise) dk(x,x) ],   dF/d noise = 1/2 [ tr M - tr T ] + trres / (2 noise^2)
//     dF/ds_u as dL/ds_u above;   tr M = sum_i (alpha_i^2 - 1 / noise + ssq_i)
// -- fitc_work_begin, C1 = B Ks^T La^-T, C1 Y, one fused rank-one pass (vfe_r_kernel) and fitc_grad_tail, whose noise entry takes its
// scalar from a slot of its own: the three products and two solves of gpx_fitc_lml_grad, without its diag(c) pass.  Predictor (the
// optimal variational posterior; k_u = K(S, z), nothing N x M):
//     mean(z) = k_u^T beta_u,  beta_u = Quu^-1 (Kuf alpha);      var(z) = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2
// per chunk of candidates (gpx_eval_chunk, the dense predictor's budget) one nu x M fill (two with the variance: each solve consumes
// its right-hand side), two left solves of order nu (chol_cross_solve, the dense predictor's rule), two column sums of squares,
// one weighted column sum and vfe_var_kernel; one device-to-host copy per output per chunk.
// That per-chunk step is vfe_posterior_chunk, shared with the acquisition costs on a VFE model (gpx_vfe_acq, gpx_vfe_acq_grad: their
// bodies and gpx_vfe_acq_batch's are in acq.hip beside the kernels they share with the dense calls; the entries and their argument
// checks are here, where the struct is).
// Sampling from that predictor's distribution is offered the same way: gpx_vfe_paths_create (decoupled paths, V = 1 beta_u^T -
// (F~_S + eps_u) Quu^-1 + Xi2 La^-1; body in paths.hip), gpx_vfe_posterior_cov (K(Z,Z) - Wu^T Wu + Wa^T Wa, the predictor's variance
// on its diagonal) and gpx_vfe_psampler_create (the exact joint sampler on it; bodies in sample.hip) have their entries and argument
// checks here -- a VFE model, its own S, for the paths a stationary kernel -- and reach the model through fitc_view and vfe_beta_u.
#include "gpx_device.h"
#include <math.h>
#include <stdlib.h>
#include <vector>

struct gpx_fitc {
  KParams kp;
  int64_t n, nu, np, nup;
  double noise;
  gpx_mat* Lu;   // chol(Quu)                       nup x nup
  gpx_mat* Kuf;  // K(S, X)                         nup x np
  gpx_mat* W;    // Lu^-1 Kuf                       nup x np
  gpx_mat* Ks;   // -Kuf diag(ginv)                 nup x np
  gpx_mat* La;   // chol(Quu + Kuf Gi Kfu)          nup x nup
  double* g;     // diag(K - Q), 1 on the padding   np (device)
  double* ginv;  // 1 / (g + 1e-12), 0 on padding   np (device)
  double sumlogg;
  int vfe;       // 1: a VFE model (gpx_vfe_fit): g = noise, ginv = 1 / noise, no guard
  double trres;  // VFE: sum_i (k(x_i,x_i) - Q_ii), fixed order; 0 for FITC
};

namespace {

// g[i] = kd[i] + noise - qd[i], ginv[i] = 1/(g[i] + 1e-12) for i < n; padding: g = 1, ginv = 0
__global__ void fitc_g_kernel(const double* __restrict__ kd, const double* __restrict__ qd, double noise, int64_t n,
                              int64_t np, double* __restrict__ g, double* __restrict__ ginv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  if (i < n) {
    const double v = kd[i] + noise - qd[i];
    g[i] = v;
    ginv[i] = 1.0 / (v + 1e-12);
  } else {
    g[i] = 1.0;
    ginv[i] = 0.0;
  }
}

// VFE: g[i] = noise, ginv[i] = 1 / noise (no guard), res[i] = kd[i] - qd[i] for i < n; padding: g = 1, ginv = 0, res = 0
__global__ void vfe_g_kernel(const double* __restrict__ kd, const double* __restrict__ qd, double noise, int64_t n, int64_t np,
                             double* __restrict__ g, double* __restrict__ ginv, double* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const bool in = i < n;
  g[i] = in ? noise : 1.0;
  ginv[i] = in ? 1.0 / noise : 0.0;
  res[i] = in ? kd[i] - qd[i] : 0.0;
}

// out[r][c] = -in[r][c] * s[c]
__global__ __launch_bounds__(256) void scale_cols_neg_kernel(const double* __restrict__ in, int64_t ldi,
                                                             const double* __restrict__ s, double* __restrict__ out,
                                                             int64_t ldo, int64_t cols) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  const double2 v = *reinterpret_cast<const double2*>(in + r * ldi + c);
  const double2 w = *reinterpret_cast<const double2*>(s + c);
  *reinterpret_cast<double2*>(out + r * ldo + c) = double2{-v.x * w.x, -v.y * w.y};
}

__global__ void log_sum_kernel(const double* __restrict__ g, int64_t n, double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t i = t; i < n; i += 256) s += log(g[i]);
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) out[0] = red[0];
}

// t[i] = ginv[i] * (y[i] - t[i])
__global__ void fitc_coeff_kernel(const double* __restrict__ ginv, const double* __restrict__ y, double* __restrict__ t,
                                  int64_t np) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < np) t[i] = ginv[i] * (y[i] - t[i]);
}

__global__ void negate_kernel(double* __restrict__ x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = -x[i];
}

int factor_in_place(gpx_ctx* ctx, gpx_mat* K, const char* what) {
  if (!K->aux) {
    K->aux_bytes = K->prows * GPX_TILE * 8;
    void* p;
    GPX_TRY(gpx_dev_alloc(ctx, K->aux_bytes, &p));
    K->aux = (double*)p;
  }
  GPX_TRY(chol_potrf(ctx, K->p, K->ld, K->prows, K->aux, K->rows));
  int info = 0;
  GPX_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  K->binv_ib = 0;  // block inverses (chol_potrs) belong to the previous contents
  K->factored = (info == 0);
  if (info != 0) {
    gpx_set_error("fitc: %s is not positive definite (pivot %d <= 0)", what, info);
    return info;
  }
  return 0;
}

void fitc_release(gpx_ctx* ctx, gpx_fitc* f) {
  if (!f) return;
  (void)hipStreamSynchronize(ctx->stream);
  if (f->Lu) gpx_mat_free(ctx, f->Lu);
  if (f->Kuf) gpx_mat_free(ctx, f->Kuf);
  if (f->W) gpx_mat_free(ctx, f->W);
  if (f->Ks) gpx_mat_free(ctx, f->Ks);
  if (f->La) gpx_mat_free(ctx, f->La);
  if (f->g) gpx_dev_release(ctx, f->g, f->np * 8);
  if (f->ginv) gpx_dev_release(ctx, f->ginv, f->np * 8);
  delete f;
}

// Bt[m][i] *= s[i] (row-major m x cols, row stride ld)
__global__ __launch_bounds__(256) void scale_cols_kernel(double* __restrict__ Bt, int64_t ld, const double* __restrict__ s,
                                                         int64_t cols) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  double2 v = *reinterpret_cast<double2*>(Bt + r * ld + c);
  const double2 w = *reinterpret_cast<const double2*>(s + c);
  v.x *= w.x;
  v.y *= w.y;
  *reinterpret_cast<double2*>(Bt + r * ld + c) = v;
}

// ---- hyper-parameter gradient ----------------------------------------------------------------------------------------------
constexpr int TS = 64;

// The weighted derivative sums over a RECTANGULAR pair of point sets: rows u < na are the points A, columns i < nb the points B,
// Mw (row stride ld, storage of at least round_up(na, 64) x round_up(nb, 64)) the weights.  partial[tile][q]:
//   q < nd:  sum Mw_ui K0_ui e_q(u, i)^2  (SE, nd = d; e_q = (a_q - b_q) / cl_q)   or   sum Mw_ui rho dk_ui/d rho  (Matern, nd = 1)
//   q = nd:  sum Mw_ui K0_ui
// K0 = the covariance without a nugget.  As lmlgrad_kernel (hyper.hip): a 64 x 64 tile per workgroup, raw coordinates of both sets
// in LDS, differences first and then scaled, every thread 8 rows x 2 adjacent columns (one 16-byte load of Mw per row), the
// tile's sums through lml_tile_term / lml_tile_store (gpx_device.h: wave shuffles and 4 LDS words per sum).  Rows >= na and columns >= nb are masked BY INDEX: what the padding of Mw holds is read
// and dropped.  K0 is recomputed, for the squared exponential too, although Kuf holds it: one exp is ~30 fp64 operations beside
// the ~6 d of the distance and the sums, a second operand would double the kernel's 8 bytes per pair, K(S,S) is not kept at
// all (Lu overwrote it).  By operation count the two passes are a few per cent of the call's products; not timed on their own.
__global__ __launch_bounds__(256) void fitc_wsum_kernel(KParams kp, const double* __restrict__ A, int64_t na,
                                                        const double* __restrict__ B, int64_t nb,
                                                        const double* __restrict__ Mw, int64_t ld,
                                                        double* __restrict__ partial) {
  extern __shared__ double sm[];
  const int d = kp.d;
  double* As = sm;               // [TS][d] raw coords of the row points
  double* Bs = sm + TS * d;      // [TS][d] of the column points
  double* red = Bs + TS * d;     // [4] per-wave partials
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * TS, j0 = (int64_t)blockIdx.x * TS;
  for (int idx = t; idx < TS * d; idx += 256) {
    int p = idx / d, k = idx - p * d;
    int64_t gi = i0 + p, gj = j0 + p;
    As[idx] = gi < na ? A[gi * d + k] : 0.0;
    Bs[idx] = gj < nb ? B[gj * d + k] : 0.0;
  }
  __syncthreads();
  const int tx = t & 31, ty = t >> 5;
  double tk[16];  // Mw_ui * K0_ui of this thread's 8 rows x 2 columns
  double drho = 0.0;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int r = ty + 8 * a;
    const int64_t gi = i0 + r;
    const double2 mv = *reinterpret_cast<const double2*>(Mw + gi * ld + j0 + 2 * tx);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cc = 2 * tx + c;
      const int64_t gj = j0 + cc;
      double v = 0.0;
      if (gi < na && gj < nb) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
          const double e = (As[r * d + k] - Bs[cc * d + k]) * kp.scale[k];
          acc = fma(e, e, acc);
        }
        const double w = c == 0 ? mv.x : mv.y;
        double kv, dv;
        lml_pair(kp, acc, &kv, &dv);
        v = w * kv;
        drho = fma(w, dv, drho);
      }
      tk[a * 2 + c] = v;
    }
  }
  const int nd = lml_nd(kp.kind, d);
  for (int q = 0; q <= nd; ++q)
    lml_tile_store(lml_tile_term(kp, q, nd, As, Bs, tk, drho, tx, ty), red,
                   partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (nd + 1) + q);
}

// m[i] = alpha_i^2 - ginv_i + ssq_i (= M_ii) and c[i] (nullable) = alpha_i^2 + ssq_i (= ginv_i + m_i) for i < n; both 0 on the padding
__global__ __launch_bounds__(256) void fitc_mdiag_kernel(const double* __restrict__ alpha, const double* __restrict__ ginv,
                                                         const double* __restrict__ ssq, int64_t n, int64_t np,
                                                         double* __restrict__ m, double* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const double v = i < n ? fma(alpha[i], alpha[i], ssq[i]) : 0.0;
  if (c) c[i] = v;
  m[i] = i < n ? v - ginv[i] : 0.0;
}

// R[u][i] += ba[u] alpha[i] - B[u][i] c[i]  (rows = blockIdx.y, two columns per thread; `cols` even)
__global__ __launch_bounds__(256) void fitc_r_kernel(double* __restrict__ R, int64_t ldr, const double* __restrict__ B, int64_t ldb,
                                                     const double* __restrict__ ba, const double* __restrict__ alpha,
                                                     const double* __restrict__ c, int64_t cols) {
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (j >= cols) return;
  double2 v = *reinterpret_cast<double2*>(R + r * ldr + j);
  const double2 b = *reinterpret_cast<const double2*>(B + r * ldb + j);
  const double2 al = *reinterpret_cast<const double2*>(alpha + j);
  const double2 cv = *reinterpret_cast<const double2*>(c + j);
  const double bu = ba[r];
  v.x += fma(bu, al.x, -b.x * cv.x);
  v.y += fma(bu, al.y, -b.y * cv.y);
  *reinterpret_cast<double2*>(R + r * ldr + j) = v;
}

// VFE: R[u][i] += ba[u] alpha[i]  (R holds (B Y^T) Y; rows = blockIdx.y, two columns per thread; `cols` even), as fitc_r_kernel
// without its diagonal term.  alpha is 0 on the padding columns, so they keep the product's zeros.
__global__ __launch_bounds__(256) void vfe_r_kernel(double* __restrict__ R, int64_t ldr, const double* __restrict__ ba,
                                                    const double* __restrict__ alpha, int64_t cols) {
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (j >= cols) return;
  double2 v = *reinterpret_cast<double2*>(R + r * ldr + j);
  const double2 al = *reinterpret_cast<const double2*>(alpha + j);
  const double bu = ba[r];
  v.x = fma(bu, al.x, v.x);
  v.y = fma(bu, al.y, v.y);
  *reinterpret_cast<double2*>(R + r * ldr + j) = v;
}

// VFE predictor epilogue: var[j] = kd[j] - su[j] + sa[j] (signed), j < mc
__global__ __launch_bounds__(256) void vfe_var_kernel(const double* __restrict__ kd, const double* __restrict__ su,
                                                      const double* __restrict__ sa, int64_t mc, double* __restrict__ var) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < mc) var[j] = (kd[j] - su[j]) + sa[j];
}

// ---- leave-one-out: the element-wise and column-wise kernels (the header comment has the formulas) --------------------------------
// From alpha, ginv and ssq, for i < n:  p = ginv - ssq (= P_ii),  r = alpha / p,  c = (1 + alpha^2 / p) / p,  gc = ginv c,  ngc = -gc,
// the predictions mean = y - alpha / p, var = 1 / p, and the point's term lp of L_LOO exactly as loo_finish_kernel (loo.hip) forms
// it.  r, c, gc, ngc, mean, var are each nullable (gpx_fitc_loo wants the predictions, the gradient wants the vectors); what is
// written is written over all np entries, 0 from n on (masked by index: p is 0 there).
__global__ __launch_bounds__(256) void fitc_loo_terms_kernel(const double* __restrict__ alpha, const double* __restrict__ ginv,
                                                             const double* __restrict__ ssq, const double* __restrict__ y, int64_t n,
                                                             int64_t np, double* __restrict__ r, double* __restrict__ c,
                                                             double* __restrict__ gc, double* __restrict__ ngc,
                                                             double* __restrict__ mean, double* __restrict__ var,
                                                             double* __restrict__ lp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const bool in = i < n;
  const double gi = ginv[i], al = alpha[i];
  const double p = in ? gi - ssq[i] : 1.0;
  const double cc = in ? (1.0 + al * al / p) / p : 0.0;
  if (r) r[i] = in ? al / p : 0.0;
  if (c) c[i] = cc;
  if (gc) gc[i] = in ? gi * cc : 0.0;
  if (ngc) ngc[i] = in ? -(gi * cc) : 0.0;
  if (mean) mean[i] = in ? y[i] - al / p : 0.0;
  if (var) var[i] = in ? 1.0 / p : 0.0;
  lp[i] = in ? 0.5 * log(p) - 0.5 * al * al / p - 0.9189385332046727418 : 0.0;  // 1/2 log 2 pi
}

// From t = Y^T (Y r) and hy_i = sum_k Y_ki (H Y)_ki, for i < n:
//   b = ginv r - t (= P r),   m = 2 alpha b - (ginv^2 c - 2 ginv c ssq + hy) (= M_ii),   e = ginv^2 c + m;   all 0 on the padding
__global__ __launch_bounds__(256) void fitc_loo_mdiag_kernel(const double* __restrict__ alpha, const double* __restrict__ ginv,
                                                             const double* __restrict__ ssq, const double* __restrict__ r,
                                                             const double* __restrict__ c, const double* __restrict__ t,
                                                             const double* __restrict__ hy, int64_t n, int64_t np,
                                                             double* __restrict__ b, double* __restrict__ m, double* __restrict__ e) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  double bv = 0.0, mv = 0.0, ev = 0.0;
  if (i < n) {
    const double gi = ginv[i], g2c = gi * gi * c[i];
    bv = fma(gi, r[i], -t[i]);
    mv = 2.0 * alpha[i] * bv - (g2c - 2.0 * gi * c[i] * ssq[i] + hy[i]);
    ev = g2c + mv;
  }
  b[i] = bv;
  m[i] = mv;
  e[i] = ev;
}

// R[u][i] += ba[u] b[i] + bb[u] alpha[i] - B[u][i] e[i]  (rows = blockIdx.y, two columns per thread; `cols` even), as fitc_r_kernel
__global__ __launch_bounds__(256) void fitc_loo_r_kernel(double* __restrict__ R, int64_t ldr, const double* __restrict__ B, int64_t ldb,
                                                         const double* __restrict__ ba, const double* __restrict__ bb,
                                                         const double* __restrict__ alpha, const double* __restrict__ b,
                                                         const double* __restrict__ e, int64_t cols) {
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (j >= cols) return;
  double2 v = *reinterpret_cast<double2*>(R + r * ldr + j);
  const double2 bm = *reinterpret_cast<const double2*>(B + r * ldb + j);
  const double2 al = *reinterpret_cast<const double2*>(alpha + j);
  const double2 bv = *reinterpret_cast<const double2*>(b + j);
  const double2 ev = *reinterpret_cast<const double2*>(e + j);
  const double u1 = ba[r], u2 = bb[r];
  v.x += fma(u1, bv.x, fma(u2, al.x, -bm.x * ev.x));
  v.y += fma(u1, bv.y, fma(u2, al.y, -bm.y * ev.y));
  *reinterpret_cast<double2*>(R + r * ldr + j) = v;
}

// out[r][c] = in[r][c] * (s ? s[c] : 1) * (other ? other[r][c] : 1)  (rows = blockIdx.y, two columns per thread; `cols` even;
// `other` has in's row stride; out may be `in` itself, hence no __restrict__ on the two)
__global__ __launch_bounds__(256) void scale_cols_to_kernel(const double* in, int64_t ldi, const double* __restrict__ s,
                                                            const double* __restrict__ other, double* out, int64_t ldo,
                                                            int64_t cols) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  double2 v = *reinterpret_cast<const double2*>(in + r * ldi + c);
  if (s) {
    const double2 w = *reinterpret_cast<const double2*>(s + c);
    v.x *= w.x;
    v.y *= w.y;
  }
  if (other) {
    const double2 o = *reinterpret_cast<const double2*>(other + r * ldi + c);
    v.x *= o.x;
    v.y *= o.y;
  }
  *reinterpret_cast<double2*>(out + r * ldo + c) = v;
}

__global__ void fill_kernel(double* __restrict__ x, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}

// the sums of fitc_wsum_kernel for the na x nb weights Mw into out[nd + 1] (device); ppart: (tiles of Mw) x (nd + 1) doubles
int fitc_wsums(gpx_ctx* ctx, const KParams& kp, const gpx_mat* A, const gpx_mat* B, const double* Mw, int64_t ld, double* ppart,
               double* out) {
  const int64_t na = A->rows, nb = B->rows, tr = gpx_round_up(na, TS) / TS, tc = gpx_round_up(nb, TS) / TS;
  const int nq = lml_nd(kp.kind, kp.d) + 1;
  ProfScope ps(ctx, GPX_PROF_REDUCE, 0.0, 8.0 * (double)na * nb);
  const size_t sh = (size_t)(2 * TS * kp.d + 4) * sizeof(double);
  hipLaunchKernelGGL(fitc_wsum_kernel, dim3((unsigned)tc, (unsigned)tr), dim3(256), sh, ctx->stream, kp, A->p, na, B->p, nb, Mw, ld,
                     ppart);
  GPX_HIP(hipGetLastError());
  return launch_tile_sums(ctx, ppart, tr * tc, nq, out);
}

// ---- gradient w.r.t. the inducing-point locations -----------------------------------------------------------------------------
// Rows of a strip whose running sums one thread holds at a time: all 8 of its rows up to DMAX = 4, beyond that as many as keep the
// sums at 32 doubles per thread (the strip is then walked in 8 / rows passes over the segment's column tiles).
constexpr int wgrad_rows(int dmax) { return dmax <= 4 ? 8 : 32 / dmax; }

// column tiles of 64 per segment of a row strip, for weights of na x nb: a function of the shape alone (the sums must not depend
// on the device), at least 2 tiles, and few enough that strips x segments reaches 1024 workgroups where the shape has them --
// nu = 4096 has 64 strips, so against N = 32768 it gets 16 segments of 32 tiles.
int64_t wgrad_tiles_per_segment(int64_t na, int64_t nb) {
  const int64_t strips = gpx_round_up(na, TS) / TS, tc = gpx_round_up(nb, TS) / TS;
  const int64_t want = (1024 + strips - 1) / strips;
  const int64_t tps = (tc + want - 1) / want;
  return tps < 2 ? 2 : tps;
}
int64_t wgrad_segments(int64_t na, int64_t nb) {
  const int64_t tc = gpx_round_up(nb, TS) / TS, tps = wgrad_tiles_per_segment(na, nb);
  return (tc + tps - 1) / tps;
}

// The row-wise weighted sums of the point derivative over a RECTANGULAR pair of point sets (rows u < na: the points A, columns
// c < nb: the points B, weights Mw as for fitc_wsum_kernel):
//     partial[seg][u][l] = sum over the columns c of segment `seg` of Mw[u][c] f(r_uc) (a_u[l] - b_c[l])
// f = the radial factor of radial_pair (gpx_device.h); the kernel's constant and the sign are applied once, by
// fitc_wgrad_sum_kernel.  Workgroup (blockIdx.x, blockIdx.y) = (segment, strip of 64 rows): the strip's raw coordinates stay in
// LDS, the segment's column tiles [blockIdx.x tps, ...) pass through LDS one at a time.  Thread (tx, ty) = (t & 31, t >> 5) holds
// the columns 2 tx + c of the tile in registers and the rows ty + 8 a: one 16-byte load of Mw per row, differences first and then
// scaled, d running sums per row kept across the tiles.  At the end the 32 threads of a row add their sums by shuffles in a fixed
// order and tx = 0 writes the row's d partials.  Rows >= na and columns >= nb are masked BY INDEX (a select, not a product: the
// padding of Mw may hold NaN); their coordinates are staged as zeros, so f is finite there.
template <int KIND, int DMAX>
__global__ __launch_bounds__(256) void fitc_wgrad_kernel(KParams kp, const double* __restrict__ A, int64_t na,
                                                         const double* __restrict__ B, int64_t nb,
                                                         const double* __restrict__ Mw, int64_t ld, int64_t tc, int64_t tps,
                                                         double* __restrict__ partial) {
  extern __shared__ double sm[];
  constexpr int RP = wgrad_rows(DMAX);
  const int d = kp.d;
  double* As = sm;            // [TS][d] raw coords of the row points
  double* Bs = sm + TS * d;   // [TS][d] of the column points of the current tile
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int64_t i0 = (int64_t)blockIdx.y * TS;
  const int64_t t0 = (int64_t)blockIdx.x * tps, t1 = t0 + tps < tc ? t0 + tps : tc;
  for (int idx = t; idx < TS * d; idx += 256) {
    const int64_t gi = i0 + idx / d;
    As[idx] = gi < na ? A[gi * d + idx % d] : 0.0;
  }
  for (int pass = 0; pass < 8 / RP; ++pass) {
    double acc[RP][DMAX];
#pragma unroll
    for (int a = 0; a < RP; ++a)
#pragma unroll
      for (int l = 0; l < DMAX; ++l) acc[a][l] = 0.0;
    for (int64_t jt = t0; jt < t1; ++jt) {
      const int64_t j0 = jt * TS;
      __syncthreads();   // the previous tile has been read by everyone (before the first tile: As is complete)
      for (int idx = t; idx < TS * d; idx += 256) {
        const int64_t gj = j0 + idx / d;
        Bs[idx] = gj < nb ? B[gj * d + idx % d] : 0.0;
      }
      __syncthreads();
      double pc[2][DMAX];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int l = 0; l < DMAX; ++l) pc[c][l] = l < d ? Bs[(2 * tx + c) * d + l] : 0.0;
#pragma unroll
      for (int a = 0; a < RP; ++a) {
        const int r = ty + 8 * (pass * RP + a);
        const int64_t gi = i0 + r;
        const double2 mv = *reinterpret_cast<const double2*>(Mw + gi * ld + j0 + 2 * tx);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          double diff[DMAX];
          const double f = radial_pair<KIND, DMAX>(kp, As + r * d, pc[c], diff);   // diff = a_u - b_c
          const double w = (gi < na && j0 + 2 * tx + c < nb) ? (c == 0 ? mv.x : mv.y) * f : 0.0;
#pragma unroll
          for (int l = 0; l < DMAX; ++l) acc[a][l] = fma(w, diff[l], acc[a][l]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < RP; ++a) {
      const int64_t gi = i0 + ty + 8 * (pass * RP + a);
#pragma unroll
      for (int l = 0; l < DMAX; ++l) {
        if (l < d) {   // (uniform)
          double s = acc[a][l];
          for (int off = 16; off > 0; off >>= 1) s += __shfl_down(s, off, 32);
          if (tx == 0 && gi < na) partial[((int64_t)blockIdx.x * na + gi) * d + l] = s;
        }
      }
    }
  }
}

// out[u][l] (i = u d + l < count) from the partials of fitc_wgrad_kernel, the segments added in index order, with the constant
// that turns (factor * difference) into the TRUE derivative dk(u, p)/du_l = -c_l f (u_l - p_l) (the table of acq.hip):
// c_l = scale_l^2 (SE), sig scale^2 (Matern 3/2), sig scale^2 / 3 (Matern 5/2).  subtract = 0: out = -c sum;  1: out -= -c sum.
__global__ __launch_bounds__(256) void fitc_wgrad_sum_kernel(KParams kp, const double* __restrict__ partial, int64_t nseg,
                                                             int64_t count, int subtract, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int l = (int)(i % kp.d);
  double s = 0.0;
  for (int64_t g = 0; g < nseg; ++g) s += partial[g * count + i];
  double c = kp.scale[l] * kp.scale[l];
  if (kp.kind == GPX_K_MATERN32) c *= kp.sig;
  if (kp.kind == GPX_K_MATERN52) c *= kp.sig / 3.0;
  out[i] = subtract ? fma(c, s, out[i]) : -c * s;
}

// out[na x d] (device) = (subtract ? out - : ) sum_c Mw[u][c] dk(a_u, b_c)/da_u;  ppart: wgrad_segments(na, nb) x na x d doubles
int fitc_wgrad(gpx_ctx* ctx, const KParams& kp, const gpx_mat* A, const gpx_mat* B, const double* Mw, int64_t ld, double* ppart,
               int subtract, double* out) {
  const int64_t na = A->rows, nb = B->rows, tr = gpx_round_up(na, TS) / TS, tc = gpx_round_up(nb, TS) / TS;
  const int64_t tps = wgrad_tiles_per_segment(na, nb), nseg = wgrad_segments(na, nb), count = na * kp.d;
  ProfScope ps(ctx, GPX_PROF_REDUCE, (double)na * nb * (6.0 * kp.d + 25.0), 8.0 * (double)na * nb);
  const size_t sh = (size_t)(2 * TS * kp.d) * sizeof(double);
  const dim3 grid((unsigned)nseg, (unsigned)tr);
#define GPX_CALL(K_, DM_)                                                                                                    \
  hipLaunchKernelGGL((fitc_wgrad_kernel<K_, DM_>), grid, dim3(256), sh, ctx->stream, kp, A->p, na, B->p, nb, Mw, ld, tc, tps, \
                     ppart)
  GPX_RADIAL_DISPATCH(kp.kind, kp.d, GPX_CALL);
#undef GPX_CALL
  GPX_HIP(hipGetLastError());
  hipLaunchKernelGGL(fitc_wgrad_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, kp,
                     (const double*)ppart, nseg, count, subtract, out);
  GPX_HIP(hipGetLastError());
  return 0;
}

// dt (np doubles, device) <- alpha = P y:  u = Kuf Gi y = -(Ks y);  w = A^-1 u;  t = Kfu w;  alpha = Gi (y - t), 0 on the padding.
// dy (np): y, zero padded.  du (nup), part (colreduce partials for nup x np), ps (chol_potrs_scratch_bytes(nup)): scratch.
int fitc_alpha(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* dy, double* du, double* dt, double* part, double* ps) {
  GPX_TRY(gpx_fill_padded(ctx, dy, y, f->n, f->np));
  GPX_HIP(hipMemsetAsync(du, 0, (size_t)f->nup * 8, ctx->stream));
  GPX_TRY(launch_rowreduce(ctx, f->Ks->p, f->Ks->ld, f->nu, f->np, dy, du));
  hipLaunchKernelGGL(negate_kernel, dim3((unsigned)((f->nup + 255) / 256)), dim3(256), 0, ctx->stream, du, f->nup);
  // both sweeps against chol(A) through its explicit 1024-order block inverses (cached in La by the first solve): the
  // leaf-level sweeps stream every 512-row diagonal block through one workgroup (0.80 ms of the 1.4 ms at nu = 4096)
  GPX_TRY(chol_potrs(ctx, f->La, du, ps));
  GPX_TRY(launch_colreduce(ctx, f->Kuf->p, f->Kuf->ld, f->nu, f->np, du, dt, part));
  hipLaunchKernelGGL(fitc_coeff_kernel, dim3((unsigned)((f->np + 255) / 256)), dim3(256), 0, ctx->stream, f->ginv, dy, dt,
                     f->np);
  GPX_HIP(hipGetLastError());
  return 0;
}

// log det(Q + G) = sum log g + log det A - log det Quu.  Blocking.
int fitc_logdet(gpx_ctx* ctx, const gpx_fitc* f, double* out) {
  double la = 0.0, lu = 0.0;
  GPX_TRY(launch_logdet(ctx, f->La->p, f->La->ld, f->nu, ctx->d_scal));
  GPX_HIP(hipMemcpyAsync(&la, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  GPX_TRY(launch_logdet(ctx, f->Lu->p, f->Lu->ld, f->nu, ctx->d_scal));
  GPX_HIP(hipMemcpyAsync(&lu, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  *out = f->sumlogg + la - lu;
  return 0;
}

// y^T alpha, summed on the host in index order
double fitc_quad(const double* y, const double* coeff, int64_t n) {
  double s = 0.0;
  for (int64_t i = 0; i < n; ++i) s += y[i] * coeff[i];
  return s;
}

}  // namespace

int64_t fitc_n(const gpx_fitc* f) { return f->n; }
int64_t fitc_np(const gpx_fitc* f) { return f->np; }
int64_t fitc_nup(const gpx_fitc* f) { return f->nup; }
int fitc_is_vfe(const gpx_fitc* f) { return f->vfe; }
void fitc_view(const gpx_fitc* f, FitcView* v) { *v = FitcView{&f->kp, f->n, f->nu, f->np, f->nup, f->noise, f->Lu, f->La}; }
// what vfe_design.hip shares with the model: the factorisation with its pivot report, and the row pass of dL/dS
int fitc_factor(gpx_ctx* ctx, gpx_mat* K, const char* what) { return factor_in_place(ctx, K, what); }
int64_t fitc_wgrad_partial_elems(int64_t na, int64_t nb, int d) { return wgrad_segments(na, nb) * na * d; }
int fitc_wgrad_rows(gpx_ctx* ctx, const KParams& kp, const gpx_mat* A, const gpx_mat* B, const double* Mw, int64_t ld, double* ppart,
                    double* out) {
  return fitc_wgrad(ctx, kp, A, B, Mw, ld, ppart, 0, out);
}

// beta_u = Quu^-1 (Kuf alpha): one row reduction over Kuf and both sweeps against chol(Quu); 0 on the padding
int vfe_beta_u(gpx_ctx* ctx, const gpx_fitc* f, const double* coeff, Scratch& tmp, double** bu_out) {
  const int64_t np = f->np, nup = f->nup;
  double *dc, *bu, *ps;
  GPX_TRY(gpx_upload_padded(ctx, tmp, coeff, f->n, np, &dc));
  GPX_TRY(tmp.get(nup * 8, &bu));
  GPX_TRY(tmp.get(chol_potrs_scratch_bytes(nup), &ps));
  GPX_HIP(hipMemsetAsync(bu, 0, (size_t)nup * 8, ctx->stream));
  GPX_TRY(launch_rowreduce(ctx, f->Kuf->p, f->Kuf->ld, f->nu, np, dc, bu));
  GPX_TRY(chol_potrs(ctx, f->Lu, bu, ps));
  *bu_out = bu;
  return 0;
}

// (gpx_internal.h: the contract)
int vfe_posterior_chunk(gpx_ctx* ctx, const gpx_fitc* f, const KParams& kpz, const gpx_mat* S, const double* Zc, int64_t mc,
                        double* B1, double* B2, double* Wu, double* Wa, const double* bu, double* pm, double* su, double* sa,
                        double* kd, double* pv, double* part) {
  const int64_t nu = f->nu, nup = f->nup;
  const int64_t mcp = gpx_round_up(mc, GPX_TILE), ldb = gpx_skew_ld(mcp);
  GPX_TRY(launch_kfill(ctx, kpz, S->p, nu, Zc, mc, 0, nullptr, 0, 0.0, B1, nup, mcp, ldb));
  if (bu) GPX_TRY(launch_colreduce(ctx, B1, ldb, nu, mcp, bu, pm, part));
  if (!B2) return 0;
  // each solve consumes its right-hand side: a second fill (cheaper than a copy, as in the fit)
  GPX_TRY(launch_kfill(ctx, kpz, S->p, nu, Zc, mc, 0, nullptr, 0, 0.0, B2, nup, mcp, ldb));
  GPX_TRY(chol_cross_solve(ctx, f->Lu, B1, ldb, Wu, ldb, mcp));
  GPX_TRY(launch_colreduce(ctx, Wu ? Wu : B1, ldb, nu, mcp, nullptr, su, part));
  GPX_TRY(chol_cross_solve(ctx, f->La, B2, ldb, Wa, ldb, mcp));   // (Wu and Wa: both or neither)
  GPX_TRY(launch_colreduce(ctx, Wa ? Wa : B2, ldb, nu, mcp, nullptr, sa, part));
  GPX_TRY(launch_kdiag(ctx, f->kp, Zc, mc, kd));
  hipLaunchKernelGGL(vfe_var_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)kd,
                     (const double*)su, (const double*)sa, mc, pv);
  GPX_HIP(hipGetLastError());
  return 0;
}

// beta^T = (P B)^T for B = np x mcp right-hand sides (row stride mcp; K(X, Z) of one chunk of evaluation points) under the
// Woodbury precision P = Gi - Ks^T A^-1 Ks (Ks = -Kuf Gi, A = La La^T): the point-derivative routines of the reference read
// `precisionMatrix`, which for a FITC model is exactly this P (gp.py:194-206, 275, 322).  Nothing N x N is formed:
//   Bt = B^T (mcp x np);  U = Bt Ks^T (mcp x nup);  U <- U La^-T La^-1 = (A^-1 Ks B)^T;  Bt <- Bt Gi - U Ks.
// Bt: mcp x np doubles (row stride np) = the result; U: mcp x nup doubles of scratch.
int fitc_solve_beta_t(gpx_ctx* ctx, const gpx_fitc* f, const double* B, int64_t mcp, double* Bt, double* U) {
  const int64_t np = f->np, nup = f->nup;
  GPX_TRY(launch_transpose(ctx, B, np, mcp, mcp, Bt, np));
  GPX_TRY(launch_gemm(ctx, Bt, np, f->Ks->p, f->Ks->ld, U, nup, mcp, nup, np, true, false, false));
  GPX_TRY(chol_trsm_right(ctx, f->La->p, f->La->ld, f->La->aux, U, nup, mcp, nup));
  GPX_TRY(chol_trsm_right_n(ctx, f->La->p, f->La->ld, f->La->aux, U, nup, mcp, nup));
  dim3 grid((unsigned)((np / 2 + 255) / 256), (unsigned)mcp);
  hipLaunchKernelGGL(scale_cols_kernel, grid, dim3(256), 0, ctx->stream, Bt, np, f->ginv, np);
  GPX_TRY(launch_gemm(ctx, U, nup, f->Ks->p, f->Ks->ld, Bt, np, mcp, np, nup, false, true, false));
  GPX_HIP(hipGetLastError());
  return 0;
}

namespace {

#define FITC_ARG(cond, what, msg)                                                              \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      gpx_set_error("%s:%d bad argument: %s: %s", __FILE__, __LINE__, what, msg);              \
      return -1;                                                                               \
    }                                                                                          \
  } while (0)

// The FITC-only entries refuse a VFE model, the gpx_vfe_* entries a FITC one; `instead` names the call to use
#define FITC_KIND(f, want_vfe, what, instead)                                                                              \
  FITC_ARG(((f)->vfe != 0) == (want_vfe), what,                                                                            \
           (want_vfe) ? "the model is a FITC model (gpx_fitc_fit), not a VFE model: " instead                              \
                      : "the model is a VFE model (gpx_vfe_fit), not a FITC model: " instead)

// The argument rules the hyper-parameter gradients share (gpx_fitc_lml_grad*, gpx_fitc_loo_grad; `what` names the entry in the
// message): a kernel with hyper-parameter derivatives, the one the model was fitted with, and the model's own X and S.
int fitc_grad_args(const gpx_fitc* f, const char* what, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                   const gpx_mat* S, KParams* kp) {
  FITC_ARG(kind == GPX_K_SE || kind == GPX_K_MATERN32 || kind == GPX_K_MATERN52, what,
           "hyper-parameter derivatives exist for the squared exponential and the isotropic Materns (as gpx_lml_grad); "
           "the Mehler kernel has none");
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, kp));
  bool same = kind == f->kp.kind && d == f->kp.d && kp->sig == f->kp.sig;
  for (int k = 0; same && k < d; ++k) same = kp->scale[k] == f->kp.scale[k];
  FITC_ARG(same, what, "(kind, d, hyp) is not the kernel the model was fitted with");
  FITC_ARG(X->cols == d && X->pcols == d && X->rows == f->n && S->cols == d && S->pcols == d && S->rows == f->nu, what,
           "X and S must be the unpadded (n x d) nodes and (nu x d) inducing points of the model");
  FITC_ARG(f->W->ld == f->Ks->ld && f->Kuf->ld == f->Ks->ld, what, "the model's nu x N matrices differ in row stride");
  return 0;
}

// Work buffers of the calls that start from alpha, Y = La^-1 Ks and its column sums of squares (gpx_fitc_loo), and of the
// gradients, which add B = Quu^-1 Kuf and end in the common tail from R on (fitc_grad_tail).  All from the caller's Scratch.
struct FitcWork {
  int64_t ldk, ldt;
  int nq;
  bool own_nsum;      // the noise entry's scalar comes from out[2 nq + 3] instead of sum m (VFE: tr M beside the constant -N / noise)
  double noise_add;   // added to the noise entry (VFE: trres / (2 noise^2))
  double *dy, *du, *al, *part, *ps, *ssq, *b1, *Y;              // every call
  double *ba, *dg, *Bm, *C1, *T, *ppart, *out, *gpart, *gs;     // gradients (gpart, gs: with dL/dS only)
};

// Takes the buffers and queues the common set-up:  al = alpha = P y,  Y = La^-1 Ks,  ssq_i = |Y[:, i]|^2;  with `grad` also
// Bm = B = Quu^-1 Kuf and the buffers of the tail (nq = sums per weighted pass; want_s: those of dL/dS).  b1 is free afterwards.
int fitc_work_begin(gpx_ctx* ctx, const gpx_fitc* f, const double* y, bool grad, int nq, int d, bool want_s, Scratch& tmp,
                    FitcWork* w) {
  const int64_t n = f->n, nu = f->nu, np = f->np, nup = f->nup;
  const int64_t ldk = w->ldk = f->Ks->ld, ldt = w->ldt = gpx_skew_ld(nup);
  w->nq = nq;
  w->own_nsum = false;
  w->noise_add = 0.0;
  w->gpart = w->gs = nullptr;
  const int64_t big = grad && np * ldt > nup * ldk ? np * ldt : nup * ldk;
  GPX_TRY(tmp.get(np * 8, &w->dy));
  GPX_TRY(tmp.get(nup * 8, &w->du));
  GPX_TRY(tmp.get(np * 8, &w->al));
  GPX_TRY(tmp.get(colreduce_partial_elems(nup, np) * 8 + 8, &w->part));
  GPX_TRY(tmp.get(chol_potrs_scratch_bytes(nup), &w->ps));
  GPX_TRY(tmp.get(np * 8, &w->ssq));
  GPX_TRY(tmp.get(big * 8, &w->b1));
  GPX_TRY(tmp.get(nup * ldk * 8, &w->Y));
  if (grad) {
    const int64_t tiles = (nup / TS) * ((np > nup ? np : nup) / TS);   // of R (nup x np) or of T (nup x nup), whichever has more
    GPX_TRY(tmp.get(nup * 8, &w->ba));
    GPX_TRY(tmp.get(nup * 8, &w->dg));
    GPX_TRY(tmp.get(nup * ldk * 8, &w->Bm));
    GPX_TRY(tmp.get(nup * ldt * 8, &w->C1));
    GPX_TRY(tmp.get(nup * ldt * 8, &w->T));
    GPX_TRY(tmp.get(tiles * nq * 8, &w->ppart));
    // [0, nq): sums against R; [nq, 2 nq): against T; then sum m, tr T, the sum of the leave-one-out terms, and the noise
    // entry's own scalar (own_nsum)
    GPX_TRY(tmp.get((2 * nq + 4) * 8, &w->out));
    if (want_s) {   // the per-segment partials of fitc_wgrad (weights R or T, whichever has more segments) and the nu x d result
      const int64_t sr = wgrad_segments(nu, n), st = wgrad_segments(nu, nu);
      GPX_TRY(tmp.get((sr > st ? sr : st) * nu * d * 8, &w->gpart));
      GPX_TRY(tmp.get(nu * d * 8, &w->gs));
    }
  }
  GPX_TRY(fitc_alpha(ctx, f, y, w->dy, w->du, w->al, w->part, w->ps));
  if (grad) {
    // B = Quu^-1 Kuf = Lu^-T W through its transpose: B^T = W^T Lu^-1
    GPX_TRY(launch_transpose(ctx, f->W->p, nup, np, ldk, w->b1, ldt));
    GPX_TRY(chol_trsm_right_n(ctx, f->Lu->p, f->Lu->ld, f->Lu->aux, w->b1, ldt, np, nup));
    GPX_TRY(launch_transpose(ctx, w->b1, np, nup, ldt, w->Bm, ldk));
  }
  // Y = La^-1 Ks through La's block inverses (the solve consumes its right-hand side: a copy)
  GPX_TRY(gpx_copy2d(ctx, f->Ks->p, ldk, w->b1, ldk, nup, np));
  GPX_TRY(chol_trsm_left_oop(ctx, f->La, w->b1, ldk, w->Y, ldk, np));
  GPX_TRY(launch_colreduce(ctx, w->Y, ldk, nu, np, nullptr, w->ssq, w->part));
  return 0;
}

// The common tail of the gradients, from R = B (M - diag m) in w.b1 and sum m in w.out[2 nq] (w.own_nsum: the scalar of the noise
// entry in w.out[2 nq + 3], otherwise sum m serves there too):  T = R B^T, the weighted sums against
// dKuf and dK(S,S), tr T, dL/dS, the copies and the host assembly.  grad[nlen + 2] and grad_s[nu x d] (host) are each nullable.
// (xsrc, xdst, xcount): one more device-to-host copy queued with the others (alpha for the marginal likelihood's value).
int fitc_grad_tail(gpx_ctx* ctx, const gpx_fitc* f, const KParams& kp, const FitcWork& w, const double* hyp, const gpx_mat* X,
                   const gpx_mat* S, double* grad, double* grad_s, const double* xsrc, double* xdst, int64_t xcount,
                   double* loo_value) {
  const int64_t nu = f->nu, np = f->np, nup = f->nup, ldk = w.ldk, ldt = w.ldt;
  const int nq = w.nq, nd = nq - 1, d = kp.d;
  double *b1 = w.b1, *T = w.T, *out = w.out;
  // T = R B^T;  the sums against dKuf (weights R) and dK(S,S) (weights T: the same kernel with both point sets = S -- T is
  // nu x nu, so the symmetric half that lml_trace would save is nothing, and one kernel serves both);  tr T
  GPX_TRY(launch_gemm(ctx, b1, ldk, w.Bm, ldk, T, ldt, nup, nup, np, true, false, false));
  if (grad) {
    GPX_TRY(fitc_wsums(ctx, kp, S, X, b1, ldk, w.ppart, out));
    GPX_TRY(fitc_wsums(ctx, kp, S, S, T, ldt, w.ppart, out + nq));
    GPX_TRY(launch_diag(ctx, T, ldt, nu, w.dg));
    GPX_TRY(launch_sum(ctx, w.dg, nu, out + 2 * nq + 1));
  }
  // dL/ds_u = sum_i R[u][i] dk(s_u, x_i)/ds_u - sum_v T[u][v] dk(s_u, s_v)/ds_u: moving s_u changes row u of Kuf and row and column
  // u of K(S,S) (T is symmetric, so row u serves for both; the v = u term is zero); the diagonals and the nugget do not move
  if (grad_s) {
    GPX_TRY(fitc_wgrad(ctx, kp, S, X, b1, ldk, w.gpart, 0, w.gs));
    GPX_TRY(fitc_wgrad(ctx, kp, S, S, T, ldt, w.gpart, 1, w.gs));
  }
  // (the copies land in locals or in the caller's buffers: the stream is drained before any error return, so none is pending then)
  std::vector<double> h((size_t)(2 * nq + 4));
  const hipError_t eh = grad ? hipMemcpyAsync(h.data(), out, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  const hipError_t ea = xdst ? hipMemcpyAsync(xdst, xsrc, (size_t)xcount * 8, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  const hipError_t eg = grad_s ? hipMemcpyAsync(grad_s, w.gs, (size_t)(nu * d) * 8, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  GPX_HIP(eh);
  GPX_HIP(ea);
  GPX_HIP(eg);
  GPX_HIP(es);
  if (grad) {
    const double* hr = h.data();
    const double* ht = h.data() + nq;
    const double msum = h[(size_t)2 * nq], trT = h[(size_t)2 * nq + 1];
    // dK/d cl_k = K0 e_k^2 / cl_k;  dK/d rho = (rho dk/d rho) / rho;  dK/d signalSize = K0 / s and dk(x,x)/d signalSize = 1
    for (int k = 0; k < nd; ++k) grad[k] = 0.5 * (2.0 * hr[k] - ht[k]) / hyp[k];
    grad[nd] = 0.5 * ((2.0 * hr[nd] - ht[nd]) / hyp[nd] + msum);
    grad[nd + 1] = w.own_nsum ? 0.5 * (h[(size_t)2 * nq + 3] - trT) + w.noise_add : 0.5 * (msum - trT);
    if (loo_value) *loo_value = h[(size_t)2 * nq + 2];
  }
  return 0;
}

// Shared body of gpx_fitc_lml_grad / gpx_fitc_lml_grad_inducing (header comment: the formulas, the products and the buffers).
// logp, grad[nlen + 2] and grad_s[nu x d] (all host) are each nullable here; the entries decide what is required.
int fitc_lml_grad_impl(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                       const gpx_mat* S, const double* y, double* logp, double* grad, double* grad_s) {
  KParams kp;
  FITC_KIND(f, false, "fitc_lml_grad", "call gpx_vfe_grad");
  GPX_TRY(fitc_grad_args(f, "fitc_lml_grad", kind, d, hyp, nhyp, X, S, &kp));
  const int64_t n = f->n, nu = f->nu, np = f->np, nup = f->nup;
  const int nq = lml_nd(kind, d) + 1;
  Scratch tmp(ctx);
  FitcWork w;
  double *mv, *cv;
  GPX_TRY(tmp.get(np * 8, &mv));
  GPX_TRY(tmp.get(np * 8, &cv));
  GPX_TRY(fitc_work_begin(ctx, f, y, true, nq, d, grad_s != nullptr, tmp, &w));
  const int64_t ldk = w.ldk, ldt = w.ldt;
  double *al = w.al, *b1 = w.b1, *Bm = w.Bm, *C1 = w.C1, *ba = w.ba;
  // m, c = Gi + m
  hipLaunchKernelGGL(fitc_mdiag_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)al,
                     (const double*)f->ginv, (const double*)w.ssq, n, np, mv, cv);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, mv, n, w.out + 2 * nq));
  // R = (B alpha) alpha^T + (B Ks^T La^-T) Y - B diag(c), over the consumed copy
  GPX_HIP(hipMemsetAsync(ba, 0, (size_t)nup * 8, ctx->stream));
  GPX_TRY(launch_rowreduce(ctx, Bm, ldk, nu, np, al, ba));
  GPX_TRY(launch_gemm(ctx, Bm, ldk, f->Ks->p, ldk, C1, ldt, nup, nup, np, true, false, false));
  GPX_TRY(chol_trsm_right(ctx, f->La->p, f->La->ld, f->La->aux, C1, ldt, nup, nup));
  GPX_TRY(launch_gemm(ctx, C1, ldt, w.Y, ldk, b1, ldk, nup, np, nup, false, false, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, 4.0 * (double)nup * np, 24.0 * (double)nup * np);
    hipLaunchKernelGGL(fitc_r_kernel, dim3((unsigned)((np / 2 + 255) / 256), (unsigned)nup), dim3(256), 0, ctx->stream, b1, ldk,
                       (const double*)Bm, ldk, (const double*)ba, (const double*)al, (const double*)cv, np);
  }
  GPX_HIP(hipGetLastError());
  std::vector<double> hal(logp ? (size_t)n : 0);
  GPX_TRY(fitc_grad_tail(ctx, f, kp, w, hyp, X, S, grad, grad_s, al, logp ? hal.data() : nullptr, n, nullptr));
  if (logp) {
    double logdet;
    GPX_TRY(fitc_logdet(ctx, f, &logdet));
    *logp = -0.5 * fitc_quad(y, hal.data(), n) - 0.5 * logdet - 0.5 * (double)n * 1.8378770664093454836;  // log 2 pi
  }
  return 0;
}

// gpx_fitc_loo_grad (header comment: the formulas, the products and the buffers).  After the common set-up b1 is worked five times
// over (Y C, H Y, B diag(ginv c), then R), H shares T's storage (it is dead before the tail forms T), and Y itself is scaled in
// place once nothing reads it unscaled any more.
int fitc_loo_grad_impl(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                       const gpx_mat* S, const double* y, double* logp, double* grad) {
  KParams kp;
  FITC_KIND(f, false, "fitc_loo_grad", "it has no leave-one-out objective; its objective is gpx_vfe_bound / gpx_vfe_grad");
  GPX_TRY(fitc_grad_args(f, "fitc_loo_grad", kind, d, hyp, nhyp, X, S, &kp));
  const int64_t n = f->n, nu = f->nu, np = f->np, nup = f->nup;
  const int nq = lml_nd(kind, d) + 1;
  Scratch tmp(ctx);
  FitcWork w;
  double *rv, *cv, *gc, *ngc, *lp, *yr, *tv, *hy, *ones, *bv, *mv, *ev, *bb, *C2;
  GPX_TRY(tmp.get(np * 8, &rv));
  GPX_TRY(tmp.get(np * 8, &cv));
  GPX_TRY(tmp.get(np * 8, &gc));
  GPX_TRY(tmp.get(np * 8, &ngc));
  GPX_TRY(tmp.get(np * 8, &lp));
  GPX_TRY(tmp.get(nup * 8, &yr));
  GPX_TRY(tmp.get(np * 8, &tv));
  GPX_TRY(tmp.get(np * 8, &hy));
  GPX_TRY(tmp.get(nup * 8, &ones));
  GPX_TRY(tmp.get(np * 8, &bv));
  GPX_TRY(tmp.get(np * 8, &mv));
  GPX_TRY(tmp.get(np * 8, &ev));
  GPX_TRY(tmp.get(nup * 8, &bb));
  GPX_TRY(fitc_work_begin(ctx, f, y, true, nq, d, false, tmp, &w));
  const int64_t ldk = w.ldk, ldt = w.ldt;
  GPX_TRY(tmp.get(nup * ldt * 8, &C2));
  double *al = w.al, *b1 = w.b1, *Bm = w.Bm, *Y = w.Y, *C1 = w.C1, *H = w.T, *ba = w.ba;
  const dim3 gvec((unsigned)((np + 255) / 256)), gmat((unsigned)((np / 2 + 255) / 256), (unsigned)nup);
  // p, r, c and the value
  hipLaunchKernelGGL(fitc_loo_terms_kernel, gvec, dim3(256), 0, ctx->stream, (const double*)al, (const double*)f->ginv,
                     (const double*)w.ssq, (const double*)w.dy, n, np, rv, cv, gc, ngc, (double*)nullptr, (double*)nullptr, lp);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, lp, n, w.out + 2 * nq + 2));
  // t = Y^T (Y r)
  GPX_TRY(launch_rowreduce(ctx, Y, ldk, nu, np, rv, yr));
  GPX_TRY(launch_colreduce(ctx, Y, ldk, nu, np, yr, tv, w.part));
  // H = (Y C) Y^T;  hy_i = sum_k Y_ki (H Y)_ki: the product, times Y entry by entry, summed down the columns
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, (double)nup * np, 16.0 * (double)nup * np);
    hipLaunchKernelGGL(scale_cols_to_kernel, gmat, dim3(256), 0, ctx->stream, (const double*)Y, ldk, (const double*)cv,
                       (const double*)nullptr, b1, ldk, np);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_gemm(ctx, b1, ldk, Y, ldk, H, ldt, nup, nup, np, true, false, false));
  GPX_TRY(launch_gemm(ctx, H, ldt, Y, ldk, b1, ldk, nup, np, nup, false, false, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, (double)nup * np, 24.0 * (double)nup * np);
    hipLaunchKernelGGL(scale_cols_to_kernel, gmat, dim3(256), 0, ctx->stream, (const double*)b1, ldk, (const double*)nullptr,
                       (const double*)Y, b1, ldk, np);
  }
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((nup + 255) / 256)), dim3(256), 0, ctx->stream, ones, nup, 1.0);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_colreduce(ctx, b1, ldk, nu, np, ones, hy, w.part));
  // b = P r, m = diag M, e = ginv^2 c + m
  hipLaunchKernelGGL(fitc_loo_mdiag_kernel, gvec, dim3(256), 0, ctx->stream, (const double*)al, (const double*)f->ginv,
                     (const double*)w.ssq, (const double*)rv, (const double*)cv, (const double*)tv, (const double*)hy, n, np, bv, mv,
                     ev);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, mv, n, w.out + 2 * nq));
  // B alpha, B b
  GPX_HIP(hipMemsetAsync(ba, 0, (size_t)nup * 8, ctx->stream));
  GPX_HIP(hipMemsetAsync(bb, 0, (size_t)nup * 8, ctx->stream));
  GPX_TRY(launch_rowreduce(ctx, Bm, ldk, nu, np, al, ba));
  GPX_TRY(launch_rowreduce(ctx, Bm, ldk, nu, np, bv, bb));
  // C1 = B Y^T;  C2 = (B diag(ginv c)) Y^T - C1 H
  GPX_TRY(launch_gemm(ctx, Bm, ldk, Y, ldk, C1, ldt, nup, nup, np, true, false, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, (double)nup * np, 16.0 * (double)nup * np);
    hipLaunchKernelGGL(scale_cols_to_kernel, gmat, dim3(256), 0, ctx->stream, (const double*)Bm, ldk, (const double*)gc,
                       (const double*)nullptr, b1, ldk, np);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_gemm(ctx, b1, ldk, Y, ldk, C2, ldt, nup, nup, np, true, false, false));
  GPX_TRY(launch_gemm(ctx, C1, ldt, H, ldt, C2, ldt, nup, nup, nup, false, true, false));
  // -B P C P = C2 Y + C1 (Y diag(ginv c)) - B diag(ginv^2 c): the first product, then Y <- -Y diag(ginv c) in place and the second
  // product subtracted from the first (launch_gemm accumulates as C - A B);  R = that + (B alpha) b^T + (B b) alpha^T - B diag(m)
  GPX_TRY(launch_gemm(ctx, C2, ldt, Y, ldk, b1, ldk, nup, np, nup, false, false, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, (double)nup * np, 16.0 * (double)nup * np);
    hipLaunchKernelGGL(scale_cols_kernel, gmat, dim3(256), 0, ctx->stream, Y, ldk, (const double*)ngc, np);
  }
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_gemm(ctx, C1, ldt, Y, ldk, b1, ldk, nup, np, nup, false, true, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, 6.0 * (double)nup * np, 24.0 * (double)nup * np);
    hipLaunchKernelGGL(fitc_loo_r_kernel, gmat, dim3(256), 0, ctx->stream, b1, ldk, (const double*)Bm, ldk, (const double*)ba,
                       (const double*)bb, (const double*)al, (const double*)bv, (const double*)ev, np);
  }
  GPX_HIP(hipGetLastError());
  return fitc_grad_tail(ctx, f, kp, w, hyp, X, S, grad, nullptr, nullptr, nullptr, 0, logp);
}

// F from alpha (host) and the model: the one place the VFE value is put together (gpx_vfe_bound and gpx_vfe_grad: the same bits)
int vfe_value(gpx_ctx* ctx, const gpx_fitc* f, const double* y, const double* alpha, double* bound) {
  double logdet;
  GPX_TRY(fitc_logdet(ctx, f, &logdet));
  *bound = -0.5 * fitc_quad(y, alpha, f->n) - 0.5 * logdet - 0.5 * (double)f->n * 1.8378770664093454836   // log 2 pi
           - 0.5 * f->trres / f->noise;
  return 0;
}

// gpx_vfe_grad (header comment: the formulas).  fitc_lml_grad_impl without the diagonal of M: R = (B alpha) alpha^T + (B Y^T) Y.
int vfe_grad_impl(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                  const gpx_mat* S, const double* y, double* bound, double* grad, double* grad_s) {
  KParams kp;
  FITC_KIND(f, true, "vfe_grad", "call gpx_fitc_lml_grad / gpx_fitc_lml_grad_inducing");
  GPX_TRY(fitc_grad_args(f, "vfe_grad", kind, d, hyp, nhyp, X, S, &kp));
  const int64_t n = f->n, nu = f->nu, np = f->np, nup = f->nup;
  const int nq = lml_nd(kind, d) + 1;
  Scratch tmp(ctx);
  FitcWork w;
  double* mv;
  GPX_TRY(tmp.get(np * 8, &mv));
  GPX_TRY(fitc_work_begin(ctx, f, y, true, nq, d, grad_s != nullptr, tmp, &w));
  const int64_t ldk = w.ldk, ldt = w.ldt;
  double *al = w.al, *b1 = w.b1, *Bm = w.Bm, *C1 = w.C1, *ba = w.ba;
  // the two scalars of the tail: sum_i m_i dk(x_i,x_i) with the constant m_i = -1 / noise, and tr M for the noise entry
  w.own_nsum = true;
  w.noise_add = 0.5 * f->trres / (f->noise * f->noise);
  hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, ctx->stream, w.out + 2 * nq, (int64_t)1, -(double)n / f->noise);
  hipLaunchKernelGGL(fitc_mdiag_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)al,
                     (const double*)f->ginv, (const double*)w.ssq, n, np, mv, (double*)nullptr);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, mv, n, w.out + 2 * nq + 3));
  // R = (B alpha) alpha^T + (B Ks^T La^-T) Y, over the consumed copy
  GPX_HIP(hipMemsetAsync(ba, 0, (size_t)nup * 8, ctx->stream));
  GPX_TRY(launch_rowreduce(ctx, Bm, ldk, nu, np, al, ba));
  GPX_TRY(launch_gemm(ctx, Bm, ldk, f->Ks->p, ldk, C1, ldt, nup, nup, np, true, false, false));
  GPX_TRY(chol_trsm_right(ctx, f->La->p, f->La->ld, f->La->aux, C1, ldt, nup, nup));
  GPX_TRY(launch_gemm(ctx, C1, ldt, w.Y, ldk, b1, ldk, nup, np, nup, false, false, false));
  {
    ProfScope pr(ctx, GPX_PROF_REDUCE, 2.0 * (double)nup * np, 16.0 * (double)nup * np);
    hipLaunchKernelGGL(vfe_r_kernel, dim3((unsigned)((np / 2 + 255) / 256), (unsigned)nup), dim3(256), 0, ctx->stream, b1, ldk,
                       (const double*)ba, (const double*)al, np);
  }
  GPX_HIP(hipGetLastError());
  std::vector<double> hal(bound ? (size_t)n : 0);
  GPX_TRY(fitc_grad_tail(ctx, f, kp, w, hyp, X, S, grad, grad_s, al, bound ? hal.data() : nullptr, n, nullptr));
  if (bound) GPX_TRY(vfe_value(ctx, f, y, hal.data(), bound));
  return 0;
}

}  // namespace

extern "C" {

int gpx_fitc_free(gpx_ctx* ctx, gpx_fitc* f) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  fitc_release(ctx, f);
  return 0;
}

// Shared body of gpx_fitc_fit / gpx_vfe_fit (vfe: G = noise I and the residual trace; header comment)
static int fitc_fit_impl(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                         double noise, bool vfe, gpx_fitc** out) {
  GPX_ARG(ctx && X && S && out, "NULL argument");
  Held<gpx_fitc, gpx_fitc_free> f(ctx, new gpx_fitc());
  f->Lu = f->Kuf = f->W = f->Ks = f->La = nullptr;
  f->g = f->ginv = nullptr;
  f->vfe = vfe ? 1 : 0;
  f->trres = 0.0;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &f->kp));
  if (!(X->cols == d && X->pcols == d && S->cols == d && S->pcols == d && S->rows > 0 && X->rows > 0)) {
    gpx_set_error("fitc: X and the inducing points must be non-empty unpadded (n x d) point sets");
    return -1;
  }
  GPX_TRY(gpx_kparams_sets(ctx, &f->kp, X, S));
  const KParams& kp = f->kp;
  f->n = X->rows;
  f->nu = S->rows;
  f->noise = noise;
  Scratch tmp(ctx);
  // Lu = chol(K(S,S) + noise I)
  GPX_TRY(gpx_mat_new(ctx, f->nu, f->nu, 1, &f->Lu));
  f->nup = f->Lu->prows;
  GPX_TRY(launch_kfill(ctx, kp, S->p, f->nu, S->p, f->nu, 1, nullptr, 1, noise, f->Lu->p, f->nup, f->nup, f->Lu->ld));
  GPX_TRY(factor_in_place(ctx, f->Lu, "K(inducing, inducing) + noise"));
  // Kuf, W = Lu^-1 Kuf
  GPX_TRY(gpx_mat_new(ctx, f->nu, f->n, 1, &f->Kuf));
  f->np = f->Kuf->pcols;
  GPX_TRY(gpx_mat_new(ctx, f->nu, f->n, 1, &f->W));
  GPX_TRY(gpx_mat_new(ctx, f->nu, f->n, 1, &f->Ks));
  GPX_TRY(launch_kfill(ctx, kp, S->p, f->nu, X->p, f->n, 0, nullptr, 0, 0.0, f->Kuf->p, f->nup, f->np, f->Kuf->ld));
  // (out of place through Lu's 1024-order block inverses, every product K >= 1024 on 128-tiles: 7.9 ms against 9.3 for the
  // in-place leaf recursion at nu = 4096, N = 32768.  The solve consumes its right-hand side: a second fill of Kuf into Ks --
  // which is only written further down -- costs 0.19 ms, the copy it replaces 0.61.)
  GPX_TRY(launch_kfill(ctx, kp, S->p, f->nu, X->p, f->n, 0, nullptr, 0, 0.0, f->Ks->p, f->nup, f->np, f->Ks->ld));
  GPX_TRY(chol_trsm_left_oop(ctx, f->Lu, f->Ks->p, f->Ks->ld, f->W->p, f->W->ld, f->np));
  // g = diag(K) + noise - colsum(W^2)
  double *qd, *kd, *part;
  GPX_TRY(tmp.get(f->np * 8, &qd));
  GPX_TRY(tmp.get(f->np * 8, &kd));
  GPX_TRY(tmp.get(colreduce_partial_elems(f->nup, f->np) * 8 + 8, &part));
  GPX_TRY(gpx_dev_alloc(ctx, f->np * 8, &f->g));
  GPX_TRY(gpx_dev_alloc(ctx, f->np * 8, &f->ginv));
  GPX_TRY(launch_colreduce(ctx, f->W->p, f->W->ld, f->nu, f->np, nullptr, qd, part));
  GPX_TRY(launch_kdiag(ctx, kp, X->p, f->n, kd));
  if (vfe) {
    // G = noise I;  trres = sum_i (k_ii - Q_ii) over the residuals in index order (launch_sum: one workgroup, fixed tree).  (Both
    // copies land in the model, which is released only behind a stream synchronisation.)
    double* res;
    GPX_TRY(tmp.get(f->np * 8 + 8, &res));
    hipLaunchKernelGGL(vfe_g_kernel, dim3((unsigned)((f->np + 255) / 256)), dim3(256), 0, ctx->stream, kd, qd, noise, f->n, f->np,
                       f->g, f->ginv, res);
    GPX_HIP(hipGetLastError());
    GPX_TRY(launch_sum(ctx, res, f->n, res + f->np));
    GPX_HIP(hipMemcpyAsync(&f->trres, res + f->np, 8, hipMemcpyDeviceToHost, ctx->stream));
    f->sumlogg = (double)f->n * log(noise);
  } else {
    hipLaunchKernelGGL(fitc_g_kernel, dim3((unsigned)((f->np + 255) / 256)), dim3(256), 0, ctx->stream, kd, qd, noise,
                       f->n, f->np, f->g, f->ginv);
    hipLaunchKernelGGL(log_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, f->g, f->n, ctx->d_scal);
    GPX_HIP(hipMemcpyAsync(&f->sumlogg, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  // Ks = -Kuf Gi;  A = Quu + Kuf Gi Kfu = Quu - Ks Kuf^T;  La = chol(A)
  {
    dim3 grid((unsigned)((f->np / 2 + 255) / 256), (unsigned)f->nup);
    hipLaunchKernelGGL(scale_cols_neg_kernel, grid, dim3(256), 0, ctx->stream, f->Kuf->p, f->Kuf->ld, f->ginv, f->Ks->p,
                       f->Ks->ld, f->np);
  }
  GPX_TRY(gpx_mat_new(ctx, f->nu, f->nu, 1, &f->La));
  GPX_TRY(launch_kfill(ctx, kp, S->p, f->nu, S->p, f->nu, 1, nullptr, 1, noise, f->La->p, f->nup, f->nup, f->La->ld));
  // nu x nu under a k range of N: as slices of the k range when C alone cannot fill the chip with 128-tiles (gemm_f64.hip,
  // launch_gemm_ksplit: 11.2 -> 9.0 ms at nu = 4096, N = 32768; 1024 or 4096 tiles wanted instead of 2048: no faster)
  {
    const int64_t t128 = (f->nup / 128) * (f->nup / 128 + 1) / 2;
    int64_t parts = 1;
    while (parts < 16 && t128 * parts < 2048 && f->np % (2 * parts * 16) == 0 && f->np / (2 * parts) >= 4096) parts *= 2;
    double* P = nullptr;
    if (parts > 1 && tmp.get(parts * f->nup * f->nup * 8, &P) != 0) parts = 1;   // (no room for the partials: one launch)
    if (parts > 1)
      GPX_TRY(launch_gemm_ksplit(ctx, f->Ks->p, f->Ks->ld, f->Kuf->p, f->Kuf->ld, f->La->p, f->La->ld, f->nup, f->nup, f->np, true,
                                 parts, P));
    else
      GPX_TRY(launch_gemm(ctx, f->Ks->p, f->Ks->ld, f->Kuf->p, f->Kuf->ld, f->La->p, f->La->ld, f->nup, f->nup, f->np, true, true,
                          true));
  }
  GPX_TRY(factor_in_place(ctx, f->La, "Quu + Kuf G^-1 Kfu"));
  GPX_HIP(hipGetLastError());
  *out = f.release();
  return 0;
}

int gpx_fitc_fit(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                 double noise, gpx_fitc** out) {
  return fitc_fit_impl(ctx, kind, d, hyp, nhyp, X, S, noise, false, out);
}

// a gpx_fitc whose G is noise I, flagged as a VFE model, with trres = sum_i (k(x_i,x_i) - Q_ii)
int gpx_vfe_fit(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                double noise, gpx_fitc** out) {
  GPX_ARG(noise > 0.0, "vfe: the noise variance must be positive (it is the whole of G and the nugget of Quu)");
  return fitc_fit_impl(ctx, kind, d, hyp, nhyp, X, S, noise, true, out);
}

int gpx_fitc_shape(const gpx_fitc* f, int64_t* n, int64_t* nu) {
  GPX_ARG(f != nullptr, "fitc model is NULL");
  if (n) *n = f->n;
  if (nu) *nu = f->nu;
  return 0;
}

// coeff = P y (host arrays of length n); quad = y^T P y
int gpx_fitc_solve(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* coeff, double* quad) {
  GPX_ARG(ctx && f && y && coeff, "NULL argument");
  Scratch tmp(ctx);
  double *dy, *du, *dt, *part, *ps;
  GPX_TRY(tmp.get(f->np * 8, &dy));
  GPX_TRY(tmp.get(f->nup * 8, &du));
  GPX_TRY(tmp.get(f->np * 8, &dt));
  GPX_TRY(tmp.get(colreduce_partial_elems(f->nup, f->np) * 8 + 8, &part));
  GPX_TRY(tmp.get(chol_potrs_scratch_bytes(f->nup), &ps));
  GPX_TRY(fitc_alpha(ctx, f, y, dy, du, dt, part, ps));
  GPX_HIP(hipMemcpyAsync(coeff, dt, (size_t)f->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  if (quad) *quad = fitc_quad(y, coeff, f->n);
  return 0;
}

// log det(Q + G) = sum log g + log det A - log det Quu
int gpx_fitc_logdet(gpx_ctx* ctx, const gpx_fitc* f, double* out) {
  GPX_ARG(ctx && f && out, "NULL argument");
  return fitc_logdet(ctx, f, out);
}

// *logp (nullable) = the log marginal likelihood of y, grad[nlen + 2] = its derivatives [lengths..., signalSize, noise variance]
// (header comment: the formula, the products and the buffers)
int gpx_fitc_lml_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                      const gpx_mat* S, const double* y, double* logp, double* grad) {
  GPX_ARG(ctx && f && X && S && y && grad, "NULL argument");
  return fitc_lml_grad_impl(ctx, f, kind, d, hyp, nhyp, X, S, y, logp, grad, nullptr);
}

// the same with grad_s[nu x d] = dL/dS (required); logp and grad nullable
int gpx_fitc_lml_grad_inducing(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                               const gpx_mat* S, const double* y, double* logp, double* grad, double* grad_s) {
  GPX_ARG(ctx && f && X && S && y && grad_s, "NULL argument");
  return fitc_lml_grad_impl(ctx, f, kind, d, hyp, nhyp, X, S, y, logp, grad, grad_s);
}

// mean / var (host N, each nullable) = the leave-one-out predictions under the model's own covariance Q + G, *logp (nullable) the
// sum of their log predictive probabilities (header comment: the formulas).  One nu x nu x N solve (Y), its column sums of
// squares, alpha; no other product.
int gpx_fitc_loo(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* mean, double* var, double* logp) {
  GPX_ARG(ctx && f && y, "NULL argument");
  FITC_KIND(f, false, "fitc_loo", "it has no leave-one-out call; its objective is gpx_vfe_bound / gpx_vfe_grad");
  const int64_t n = f->n, np = f->np;
  Scratch tmp(ctx);
  FitcWork w;
  double *pm, *pv, *lp;
  GPX_TRY(tmp.get(np * 8, &pm));
  GPX_TRY(tmp.get(np * 8, &pv));
  GPX_TRY(tmp.get(np * 8, &lp));
  GPX_TRY(fitc_work_begin(ctx, f, y, false, 0, 0, false, tmp, &w));
  double* none = nullptr;
  hipLaunchKernelGGL(fitc_loo_terms_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)w.al,
                     (const double*)f->ginv, (const double*)w.ssq, (const double*)w.dy, n, np, none, none, none, none,
                     mean ? pm : none, var ? pv : none, lp);
  GPX_HIP(hipGetLastError());
  GPX_TRY(launch_sum(ctx, lp, n, ctx->d_scal));
  if (mean) GPX_HIP(hipMemcpyAsync(mean, pm, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (var) GPX_HIP(hipMemcpyAsync(var, pv, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (logp) GPX_HIP(hipMemcpyAsync(logp, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// *logp (nullable) = L_LOO, the same bits as gpx_fitc_loo's; grad[nlen + 2] = its TRUE derivatives [lengths..., signalSize, noise
// variance] (header comment: the formulas, the products and the buffers)
int gpx_fitc_loo_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                      const gpx_mat* S, const double* y, double* logp, double* grad) {
  GPX_ARG(ctx && f && X && S && y && grad, "NULL argument");
  return fitc_loo_grad_impl(ctx, f, kind, d, hyp, nhyp, X, S, y, logp, grad);
}

// mean[j] = k(z_j, X) . coeff (coeff nullable),  var[j] = k(z,z) - k_z^T P k_z (signed; nullable)
int gpx_fitc_posterior(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* X, const double* coeff, const gpx_mat* Z,
                       double* mean, double* var) {
  GPX_ARG(ctx && f && X && Z, "NULL argument");
  FITC_KIND(f, false, "fitc_posterior", "call gpx_vfe_posterior");
  GPX_ARG(X->rows == f->n && X->cols == f->kp.d && Z->cols == f->kp.d && Z->pcols == f->kp.d, "point sets do not match");
  GPX_ARG(mean == nullptr || coeff != nullptr, "coeff is required for the mean");
  const int64_t M = Z->rows, d = f->kp.d, np = f->np, nup = f->nup;
  if (M == 0) return 0;
  KParams kpz = f->kp;  // the evaluation points may reach beyond the training domain
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, X, Z));
  const ChunkRange cr(M, gpx_eval_chunk(np));
  const int64_t mc_alloc = cr.mc_alloc;
  Scratch tmp(ctx);
  const int64_t ldb = gpx_skew_ld(np), ldu = gpx_skew_ld(nup);
  double *B, *U, *dc = nullptr, *o1, *o2, *kd;
  GPX_TRY(tmp.get(mc_alloc * ldb * 8, &B));
  GPX_TRY(tmp.get(mc_alloc * ldu * 8, &U));
  GPX_TRY(tmp.get(mc_alloc * 8, &o1));
  GPX_TRY(tmp.get(mc_alloc * 8, &o2));
  GPX_TRY(tmp.get(mc_alloc * 8, &kd));
  if (mean) GPX_TRY(gpx_upload_padded(ctx, tmp, coeff, f->n, np, &dc));
  std::vector<double> h1((size_t)mc_alloc), h2((size_t)mc_alloc), hk((size_t)mc_alloc);
  for (const ChunkRange::Step c : cr) {
    const int64_t mc = c.mc, mcp = c.mcp, j0 = c.j0;
    const double* Zc = Z->p + j0 * d;
    GPX_TRY(launch_kfill(ctx, kpz, Zc, mc, X->p, f->n, 0, nullptr, 0, 0.0, B, mcp, np, ldb));
    if (mean) {
      GPX_TRY(launch_rowreduce(ctx, B, ldb, mc, np, dc, o1));
      GPX_HIP(hipMemcpyAsync(mean + j0, o1, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (var) {
      GPX_TRY(launch_rowreduce(ctx, B, ldb, mc, np, f->ginv, o1, 1));                                  // sum Gi k^2
      GPX_TRY(launch_gemm(ctx, B, ldb, f->Ks->p, f->Ks->ld, U, ldu, mcp, nup, np, true, false, false));  // -(Kuf Gi k)^T
      GPX_TRY(chol_trsm_right(ctx, f->La->p, f->La->ld, f->La->aux, U, ldu, mcp, nup));
      GPX_TRY(launch_rowreduce(ctx, U, ldu, mc, nup, nullptr, o2));
      GPX_TRY(launch_kdiag(ctx, f->kp, Zc, mc, kd));
      GPX_HIP(hipMemcpyAsync(h1.data(), o1, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipMemcpyAsync(h2.data(), o2, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipMemcpyAsync(hk.data(), kd, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
      GPX_HIP(hipStreamSynchronize(ctx->stream));
      for (int64_t j = 0; j < mc; ++j) var[j0 + j] = hk[(size_t)j] - h1[(size_t)j] + h2[(size_t)j];
    }
  }
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// *bound = F: alpha (gpx_fitc_solve's reductions and solve), the two log-determinants and trres; B is not formed
int gpx_vfe_bound(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* bound) {
  GPX_ARG(ctx && f && y && bound, "NULL argument");
  FITC_KIND(f, true, "vfe_bound", "call gpx_fitc_solve + gpx_fitc_logdet");
  std::vector<double> hal((size_t)f->n);
  GPX_TRY(gpx_fitc_solve(ctx, f, y, hal.data(), nullptr));
  return vfe_value(ctx, f, y, hal.data(), bound);
}

// *bound = F (gpx_vfe_bound's bits), grad[nlen + 2] = its TRUE derivatives [lengths..., signalSize, noise variance], grad_s[nu x d]
// = dF/dS: each nullable, at least one given (header comment: the formulas)
int gpx_vfe_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                 const gpx_mat* S, const double* y, double* bound, double* grad, double* grad_s) {
  GPX_ARG(ctx && f && X && S && y, "NULL argument");
  GPX_ARG(bound || grad || grad_s, "NULL argument: at least one of bound, grad and grad_s is required");
  return vfe_grad_impl(ctx, f, kind, d, hyp, nhyp, X, S, y, bound, grad, grad_s);
}

// the point sets of the VFE predictor's callers: S the model's inducing points, Z unpadded points of its dimension
static int vfe_point_sets(const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z) {
  GPX_ARG(S->rows == f->nu && S->cols == f->kp.d && S->pcols == f->kp.d && Z->cols == f->kp.d && Z->pcols == f->kp.d,
          "point sets do not match");
  return 0;
}

// mean[j] = k_u(z_j)^T beta_u (coeff = alpha required),  var[j] = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2 (signed); each nullable
int gpx_vfe_posterior(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double* mean,
                      double* var) {
  GPX_ARG(ctx && f && S && Z, "NULL argument");
  FITC_KIND(f, true, "vfe_posterior", "call gpx_fitc_posterior");
  GPX_TRY(vfe_point_sets(f, S, Z));
  GPX_ARG(mean == nullptr || coeff != nullptr, "coeff is required for the mean");
  const int64_t M = Z->rows, d = f->kp.d, nup = f->nup;
  if (M == 0 || (!mean && !var)) return 0;
  KParams kpz = f->kp;  // the evaluation points may reach beyond the training domain
  GPX_TRY(gpx_kparams_sets(ctx, &kpz, S, Z));
  const ChunkRange cr(M, gpx_eval_chunk(nup));
  Scratch tmp(ctx);   // its scope exit is the synchronisation the host results wait for
  VfePosteriorWork w(nup, cr.mc_alloc, var != nullptr);
  GPX_TRY(w.take(tmp, mean != nullptr));
  if (mean) GPX_TRY(w.beta(ctx, f, coeff, tmp));
  for (const ChunkRange::Step c : cr) {
    GPX_TRY(w.run(ctx, f, kpz, S, Z->p + c.j0 * d, c.mc));
    if (mean) GPX_HIP(hipMemcpyAsync(mean + c.j0, w.pm, (size_t)c.mc * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (var) GPX_HIP(hipMemcpyAsync(var + c.j0, w.pv, (size_t)c.mc * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// The argument rules of gpx_vfe_acq / gpx_vfe_acq_grad / gpx_vfe_acq_batch (their bodies: acq.hip)
static int vfe_acq_args(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq,
                        const char* what) {
  GPX_ARG(ctx && f && S && Z && coeff, "NULL argument");
  FITC_KIND(f, true, what, "the batched acquisition costs are offered on VFE models only");
  GPX_ARG(acq == GPX_ACQ_UCB || acq == GPX_ACQ_PI || acq == GPX_ACQ_EI, "acq must be GPX_ACQ_UCB, GPX_ACQ_PI or GPX_ACQ_EI");
  GPX_TRY(vfe_point_sets(f, S, Z));
  return 0;
}

int gpx_vfe_acq(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                double* cost, int64_t* best, double* best_cost) {
  GPX_TRY(vfe_acq_args(ctx, f, S, coeff, Z, acq, "vfe_acq"));
  if (Z->rows == 0) {
    if (best) *best = -1;
    if (best_cost) *best_cost = __builtin_nan("");
    return 0;
  }
  return vfe_acq_impl(ctx, f, S, coeff, Z, acq, param, cost, best, best_cost, nullptr);
}

int gpx_vfe_acq_grad(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                     double* cost, double* grad) {
  GPX_ARG(grad != nullptr, "grad is NULL");
  GPX_TRY(vfe_acq_args(ctx, f, S, coeff, Z, acq, "vfe_acq_grad"));
  FITC_ARG(f->kp.kind == GPX_K_SE || f->kp.kind == GPX_K_MATERN32 || f->kp.kind == GPX_K_MATERN52, "vfe_acq_grad",
           "acquisition gradients exist for the stationary kernels (SE, Matern 3/2, Matern 5/2) only: the Mehler kernel's "
           "prior variance depends on the point");
  if (Z->rows == 0) return 0;
  return vfe_acq_impl(ctx, f, S, coeff, Z, acq, param, cost, nullptr, nullptr, grad);
}

int gpx_vfe_acq_batch(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* C, int acq, double param,
                      int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx, double* out_cost, double* out_lie,
                      double* all_costs) {
  GPX_ARG(out_idx != nullptr, "out_idx is NULL");
  GPX_ARG(lie == GPX_LIE_BELIEVER || lie == GPX_LIE_CONSTANT, "lie must be GPX_LIE_BELIEVER or GPX_LIE_CONSTANT");
  GPX_TRY(vfe_acq_args(ctx, f, S, coeff, C, acq, "vfe_acq_batch"));
  GPX_ARG(q >= 1, "need at least one pick");
  GPX_ARG(q <= C->rows, "more picks than candidates");
  return vfe_acq_batch_impl(ctx, f, S, coeff, C, acq, param, track_best != 0, lie, lie_value, q, out_idx, out_cost, out_lie,
                            all_costs);
}

// The same three with the MES cost on the caller's sampled optima (gpx_vfe_acq_mes*): vfe_acq_args' rules but for the cost kind,
// then mes_args'
static int vfe_acq_mes_args(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z,
                            const MesSpec* mes, const char* what) {
  GPX_ARG(ctx && f && S && Z && coeff, "NULL argument");
  FITC_KIND(f, true, what, "the batched acquisition costs are offered on VFE models only");
  GPX_TRY(mes_args(mes));
  GPX_TRY(vfe_point_sets(f, S, Z));
  return 0;
}

int gpx_vfe_acq_mes(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, const double* ystar,
                    int64_t K, int sign, double* cost, int64_t* best, double* best_cost) {
  const MesSpec mes{ystar, K, sign};
  GPX_TRY(vfe_acq_mes_args(ctx, f, S, coeff, Z, &mes, "vfe_acq_mes"));
  if (Z->rows == 0) {
    if (best) *best = -1;
    if (best_cost) *best_cost = __builtin_nan("");
    return 0;
  }
  return vfe_acq_impl(ctx, f, S, coeff, Z, GPX_ACQ_MES, 0.0, cost, best, best_cost, nullptr, &mes);
}

int gpx_vfe_acq_mes_grad(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, const double* ystar,
                         int64_t K, int sign, double* cost, double* grad) {
  GPX_ARG(grad != nullptr, "grad is NULL");
  const MesSpec mes{ystar, K, sign};
  GPX_TRY(vfe_acq_mes_args(ctx, f, S, coeff, Z, &mes, "vfe_acq_mes_grad"));
  FITC_ARG(f->kp.kind == GPX_K_SE || f->kp.kind == GPX_K_MATERN32 || f->kp.kind == GPX_K_MATERN52, "vfe_acq_mes_grad",
           "acquisition gradients exist for the stationary kernels (SE, Matern 3/2, Matern 5/2) only: the Mehler kernel's "
           "prior variance depends on the point");
  if (Z->rows == 0) return 0;
  return vfe_acq_impl(ctx, f, S, coeff, Z, GPX_ACQ_MES, 0.0, cost, nullptr, nullptr, grad, &mes);
}

int gpx_vfe_acq_mes_batch(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* C,
                          const double* ystar, int64_t K, int sign, int lie, double lie_value, int64_t q, int64_t* out_idx,
                          double* out_cost, double* out_lie, double* all_costs) {
  GPX_ARG(out_idx != nullptr, "out_idx is NULL");
  GPX_ARG(lie == GPX_LIE_BELIEVER || lie == GPX_LIE_CONSTANT, "lie must be GPX_LIE_BELIEVER or GPX_LIE_CONSTANT");
  const MesSpec mes{ystar, K, sign};
  GPX_TRY(vfe_acq_mes_args(ctx, f, S, coeff, C, &mes, "vfe_acq_mes_batch"));
  GPX_ARG(q >= 1, "need at least one pick");
  GPX_ARG(q <= C->rows, "more picks than candidates");
  return vfe_acq_batch_impl(ctx, f, S, coeff, C, GPX_ACQ_MES, 0.0, 0, lie, lie_value, q, out_idx, out_cost, out_lie, all_costs, &mes);
}

// Posterior sampling on a VFE model (bodies: paths.hip and sample.hip, beside the code they share with the dense samplers; the
// argument checks are here, where the struct is)
int gpx_vfe_paths_create(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const double* omega,
                         const double* phase, int64_t nfeat, const double* w, const double* eps_u, const double* xi_q,
                         int64_t nPaths, gpx_paths** out) {
  GPX_ARG(ctx && f && S && coeff && omega && phase && w && out, "NULL argument");
  FITC_KIND(f, true, "vfe_paths_create", "pathwise sampling is offered on dense models (gpx_paths_create) and VFE models only");
  FITC_ARG(f->kp.kind == GPX_K_SE || f->kp.kind == GPX_K_MATERN32 || f->kp.kind == GPX_K_MATERN52, "vfe_paths_create",
           "paths: stationary kernels only (squared exponential, Matern 3/2, Matern 5/2)");
  GPX_TRY(vfe_point_sets(f, S, S));
  GPX_ARG(nfeat >= 1, "paths: needs at least one feature");
  GPX_ARG(nPaths >= 1, "paths: needs at least one path");
  return vfe_paths_create_impl(ctx, f, S, coeff, omega, phase, nfeat, w, eps_u, xi_q, nPaths, out);
}

int gpx_vfe_posterior_cov(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* cov) {
  GPX_ARG(ctx && f && S && Z && cov, "NULL argument");
  FITC_KIND(f, true, "vfe_posterior_cov", "a FITC model's covariance comes from gpx_fitc_dense's precision");
  GPX_TRY(vfe_point_sets(f, S, Z));
  if (Z->rows == 0) return 0;
  return vfe_posterior_cov_impl(ctx, f, S, Z, cov);
}

int gpx_vfe_psampler_create(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double nugget,
                            gpx_psampler** out) {
  GPX_ARG(ctx && f && S && coeff && Z && out, "NULL argument");
  FITC_KIND(f, true, "vfe_psampler_create", "joint sampling is offered on dense models (gpx_psampler_create) and VFE models only");
  GPX_TRY(vfe_point_sets(f, S, Z));
  GPX_ARG(nugget >= 0.0, "psampler: the nugget must not be negative");
  GPX_ARG(Z->rows >= 1, "psampler: needs at least one point");
  return vfe_psampler_create_impl(ctx, f, S, coeff, Z, nugget, out);
}

// The argument rules of gpx_vfe_acq_qei and its debug hook: gpx_acq_qei's, on a VFE model and its own S (body: sample.hip)
static int vfe_qei_args(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q,
                        double nugget) {
  GPX_ARG(ctx && f && S && coeff && Zb, "NULL argument");
  FITC_KIND(f, true, "vfe_acq_qei", "joint expected improvement is offered on dense models (gpx_acq_qei) and VFE models only");
  GPX_ARG(q >= 1 && q <= GPX_QEI_MAX_Q, "q-EI: the batch size q must be in 1 .. GPX_QEI_MAX_Q (32)");
  GPX_ARG(nugget >= 0.0, "q-EI: the nugget must not be negative");
  GPX_TRY(vfe_point_sets(f, S, Zb));
  GPX_ARG(Zb->rows >= q && Zb->rows % q == 0, "q-EI: the rows of Zb must be a positive multiple of q (consecutive q rows form one batch)");
  return 0;
}

int gpx_vfe_acq_qei(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q,
                    const double* xi, int64_t nS, double fBest, double nugget, double* cost, int64_t* best, double* best_cost,
                    int64_t* n_bad) {
  GPX_TRY(vfe_qei_args(ctx, f, S, coeff, Zb, q, nugget));
  GPX_ARG(nS >= 1 && nS < ((int64_t)1 << 31), "q-EI: needs at least one base sample (and fewer than 2^31)");
  GPX_ARG(xi != nullptr, "q-EI: xi is NULL");
  return vfe_qei_impl(ctx, f, S, coeff, Zb, q, xi, nS, fBest, nugget, cost, best, best_cost, n_bad, nullptr, nullptr, nullptr);
}

// debug (gpx_debug.h): the blocks qei_kernel works on -- gpx_vfe_acq_qei's launches with one zero base sample
int gpx_dbg_vfe_qei_blocks(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q,
                           double nugget, double* mean, double* Cb, double* Fb) {
  GPX_TRY(vfe_qei_args(ctx, f, S, coeff, Zb, q, nugget));
  GPX_ARG(mean && Cb && Fb, "NULL argument");
  const std::vector<double> xi0((size_t)q, 0.0);
  return vfe_qei_impl(ctx, f, S, coeff, Zb, q, xi0.data(), 1, 0.0, nugget, nullptr, nullptr, nullptr, nullptr, mean, Cb, Fb);
}

// Point-wise derivatives of the variational variance (bodies: vfe_design.hip; the argument checks are here, where the struct is)
int gpx_vfe_var_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                     const gpx_mat* S, const gpx_mat* Z, double* out) {
  GPX_ARG(ctx && f && X && S && Z && out, "NULL argument");
  FITC_KIND(f, true, "vfe_var_grad", "call gpx_fitc_var_grad");
  FITC_ARG(kind != GPX_K_MEHLER, "vfe_var_grad",
           "point derivatives exist for the squared exponential and the isotropic Materns only, not for the Mehler kernel");
  KParams kp;
  GPX_TRY(fitc_grad_args(f, "vfe_var_grad", kind, d, hyp, nhyp, X, S, &kp));
  GPX_ARG(Z->cols == d && Z->pcols == d, "point sets do not match");
  if (Z->rows == 0) return 0;
  return vfe_var_grad_impl(ctx, f, X, S, Z, out);
}

int gpx_vfe_var_grad_newpt(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* out) {
  GPX_ARG(ctx && f && S && Z && out, "NULL argument");
  FITC_KIND(f, true, "vfe_var_grad_newpt", "call gpx_fitc_var_grad_newpt");
  FITC_ARG(f->kp.kind == GPX_K_SE || f->kp.kind == GPX_K_MATERN32 || f->kp.kind == GPX_K_MATERN52, "vfe_var_grad_newpt",
           "point derivatives exist for the squared exponential and the isotropic Materns only, not for the Mehler kernel");
  GPX_TRY(vfe_point_sets(f, S, Z));
  if (Z->rows == 0) return 0;
  // gpx_vfe_acq_grad's own sequence with (a, b) = (0, 1): grad_z var = -2 sum_u dk(z, s_u)/dz gamma(z)[u]
  return vfe_acq_impl(ctx, f, S, nullptr, Z, GPX_ACQ_VARIANCE, 0.0, nullptr, nullptr, nullptr, out);
}

// Dense Q + G and P (host, n x n row-major, each nullable): the reference's covarianceMatrix / precisionMatrix attributes.
int gpx_fitc_dense(gpx_ctx* ctx, const gpx_fitc* f, double* cov, double* prec) {
  GPX_ARG(ctx && f, "NULL argument");
  const int64_t n = f->n, np = f->np, nup = f->nup;
  Scratch tmp(ctx);
  double *T, *C;
  const int64_t ldt = gpx_skew_ld(nup), ldc = gpx_skew_ld(np);
  GPX_TRY(tmp.get(np * ldt * 8, &T));
  GPX_TRY(tmp.get(np * ldc * 8, &C));
  std::vector<double> hv((size_t)np);
  for (int which = 0; which < 2; ++which) {
    double* dst = which == 0 ? cov : prec;
    if (!dst) continue;
    const double* dvec = which == 0 ? f->g : f->ginv;
    if (which == 0) {
      GPX_TRY(launch_transpose(ctx, f->W->p, nup, np, f->W->ld, T, ldt));  // W^T (np x nup)
    } else {
      double* Y;
      GPX_TRY(tmp.get(nup * f->Ks->ld * 8, &Y));
      GPX_TRY(gpx_copy2d(ctx, f->Ks->p, f->Ks->ld, Y, f->Ks->ld, nup, np));
      GPX_TRY(chol_trsm_left(ctx, f->La->p, f->La->ld, f->La->aux, Y, f->Ks->ld, nup, np));  // La^-1 Ks
      GPX_TRY(launch_transpose(ctx, Y, nup, np, f->Ks->ld, T, ldt));
    }
    GPX_TRY(launch_gemm(ctx, T, ldt, T, ldt, C, ldc, np, np, nup, true, false, false));  // T T^T
    GPX_HIP(hipMemcpy2DAsync(dst, (size_t)n * 8, C, (size_t)ldc * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost,
                             ctx->stream));
    GPX_HIP(hipMemcpyAsync(hv.data(), dvec, (size_t)np * 8, hipMemcpyDeviceToHost, ctx->stream));
    GPX_HIP(hipStreamSynchronize(ctx->stream));
    if (which == 0) {
      for (int64_t i = 0; i < n; ++i) dst[i * n + i] += hv[(size_t)i];  // Q + diag(g)
    } else {
      for (int64_t i = 0; i < n * n; ++i) dst[i] = -dst[i];
      for (int64_t i = 0; i < n; ++i) dst[i * n + i] += hv[(size_t)i];  // diag(ginv) - Y^T Y
    }
  }
  return 0;
}

}  // extern "C"
