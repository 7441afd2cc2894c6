// Per-pair and per-workgroup device helpers shared by the element-wise kernels of design.hip, hyper.hip, grad.hip, acq.hip and
// fitc.hip (gfx950).  __device__ __forceinline__ functions and templates only -- no kernels, no host code.  The tiled fills (kfill.hip)
// and the sums of reduce.hip / chol.hip have their own forms and do not come through here (reduce.hip's row arg-best does).
#pragma once
#include "gpx_internal.h"

// ---- covariance value for a pair of points given in global memory (generic kind and d) --------------------------------------
// sum_k ((a_k - b_k) scale_k)^2: the difference first, as the reference (kernels.py:121-122)
static __device__ __forceinline__ double scaled_dist2(const KParams& kp, const double* __restrict__ a, const double* __restrict__ b) {
  double acc = 0.0;
  for (int k = 0; k < kp.d; ++k) {
    const double e = (a[k] - b[k]) * kp.scale[k];
    acc = fma(e, e, acc);
  }
  return acc;
}

// CONSTRAINT (enforced by profiles/csrc_dedup_isa_compare.txt, not a matter of taste): the loop of scaled_dist2 stays written out
// in kpair.  Routed through the helper, mi_row_kernel, greedy_row_kernel, givar_u_kernel and keval_kernel no longer compile to
// the instruction streams that comparison holds them to.  Do not fold the two without redoing the comparison.
static __device__ __forceinline__ double kpair(const KParams& kp, const double* __restrict__ a, const double* __restrict__ b) {
  double acc = 0.0;
  if (kp.kind == GPX_K_MEHLER) {
    double pa = 0.0, pb = 0.0, cr = 0.0;
    for (int k = 0; k < kp.d; ++k) {
      const double x = a[k], y = b[k];
      pa = fma(kp.c1[k] * x, x, pa);
      pb = fma(kp.c1[k] * y, y, pb);
      cr = fma(kp.c2[k] * x, y, cr);
    }
    return kp.sig * exp(-(pa + pb - cr));
  }
  for (int k = 0; k < kp.d; ++k) {
    const double e = (a[k] - b[k]) * kp.scale[k];
    acc = fma(e, e, acc);
  }
  if (kp.kind == GPX_K_SE) return kp.sig * exp(-0.5 * acc);
  const double t = sqrt(acc);
  if (kp.kind == GPX_K_MATERN32) return kp.sig * (1.0 + t) * exp(-t);
  return kp.sig * (1.0 + t + acc * (1.0 / 3.0)) * exp(-t);
}

// ---- hyper-parameter derivative of one pair (the trace kernels of hyper.hip and the FITC gradient of fitc.hip) ---------------
// One pair of points under a stationary kernel with hyper-parameter derivatives: acc = the scaled squared distance (SE: sum_k
// e_k^2; Matern: t^2 with t = sqrt(nu') r / rho).  kv = k(a, b) without the nugget; dv = rho dk/d rho for the isotropic Materns
// (round 6; the reference's own Matern raises, kernels.py:93-97):
//   nu = 3/2: k = s (1 + t) e^-t,           dk/dt = -s t e^-t            rho dk/d rho = -t dk/dt = s t^2 e^-t
//   nu = 5/2: k = s (1 + t + t^2/3) e^-t,   dk/dt = -s t (1 + t) e^-t / 3                     = s t^2 (1 + t) e^-t / 3
static __device__ __forceinline__ void lml_pair(const KParams& kp, double acc, double* kv, double* dv) {
  if (kp.kind == GPX_K_SE) {
    *kv = kp.sig * exp(-0.5 * acc);
    *dv = 0.0;
    return;
  }
  const double t = sqrt(acc), e = kp.sig * exp(-t);
  if (kp.kind == GPX_K_MATERN32) {
    *kv = (1.0 + t) * e;
    *dv = acc * e;
  } else {
    *kv = (1.0 + t + acc * (1.0 / 3.0)) * e;
    *dv = acc * (1.0 + t) * e * (1.0 / 3.0);
  }
}
// number of length-type hyper-parameters in the trace sums: d correlation lengths (SE) or the one rho (Matern)
static __host__ __device__ __forceinline__ int lml_nd(int kind, int d) { return kind == GPX_K_SE ? d : 1; }

// The end of a 64 x 64 trace tile of 256 threads (lmlgrad_kernel, lmlgrad_slab_kernel, fitc_wsum_kernel), thread (tx, ty) =
// (t & 31, t >> 5) holding the rows ty + 8 a and the columns 2 tx + c: tk[2 a + c] = weight * K0 of its 16 pairs, drho = its sum of
// weight * rho dk/d rho, As / Bs = the raw coordinates of the tile's row / column points ([64][d] each).
// lml_tile_term: this thread's part of sum q -- q < nd: weight K0 e_q^2 (SE) or drho (Matern); q == nd: weight K0.
static __device__ __forceinline__ double lml_tile_term(const KParams& kp, int q, int nd, const double* As, const double* Bs,
                                                       const double (&tk)[16], double drho, int tx, int ty) {
  const int d = kp.d;
  double s = 0.0;
  if (q < nd && kp.kind != GPX_K_SE) {
    s = drho;
  } else if (q < nd) {
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int r = ty + 8 * a;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const double e = (As[r * d + q] - Bs[(2 * tx + c) * d + q]) * kp.scale[q];
        s = fma(tk[a * 2 + c], e * e, s);
      }
    }
  } else {
#pragma unroll
    for (int a = 0; a < 16; ++a) s += tk[a];
  }
  return s;
}
// lml_tile_store: *dst = the sum of s over the workgroup -- wave shuffles, then the 4 LDS words red[], in a fixed order.
static __device__ __forceinline__ void lml_tile_store(double s, double* red, double* dst) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __syncthreads();
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (t == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- radial pair: the kernels whose point derivative is a radial factor times the coordinate difference -------------------
// diff = u - p (zero from kp.d on), r2 = sum_l (diff_l scale_l)^2, t = sqrt(r2); DMAX = d rounded up (GPX_RADIAL_DISPATCH).
//     KIND      returns
//     SE        s e^(-r2/2) = k(u, p)
//     Matern32  e^-t
//     Matern52  (1 + t) e^-t
// The constant that turns (factor * diff) into the derivative differs between the callers' conventions (grad.hip: the
// reference's; acq.hip: the true one) and stays with them.
template <int KIND, int DMAX>
static __device__ __forceinline__ double radial_pair(const KParams& kp, const double* __restrict__ u, const double (&p)[DMAX],
                                                     double (&diff)[DMAX]) {
  double r2 = 0.0;
#pragma unroll
  for (int l = 0; l < DMAX; ++l) {
    diff[l] = 0.0;
    if (l < kp.d) {
      diff[l] = u[l] - p[l];
      const double e = diff[l] * kp.scale[l];
      r2 = fma(e, e, r2);
    }
  }
  if (KIND == GPX_K_SE) return kp.sig * exp(-0.5 * r2);
  const double t = sqrt(r2);
  return KIND == GPX_K_MATERN32 ? exp(-t) : (1.0 + t) * exp(-t);
}

// ---- fixed-order tree sum over a workgroup of 256 threads --------------------------------------------------------------------
// red: 256 doubles of LDS.  On return red[0] holds the sum, behind a barrier, for every thread.  Whoever reuses `red` puts a
// __syncthreads() between reading red[0] and the next call.
static __device__ __forceinline__ void block_sum_256(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
}

// ---- arg-reduction over a workgroup of nt threads (a power of two) ----------------------------------------------------------
// (value, index) pairs under one of three merge rules, all associative and commutative, so the winner depends neither on the
// reduction tree nor on how the candidates were dealt to threads and workgroups:
//   vi_max        first maximum (np.argmax: the smaller index on a tie); identity {-inf, INT64_MAX}; a NaN never wins, so
//                 all-NaN input leaves INT64_MAX, which the callers turn into index 0 as np.argmax does
//   vi_min        first minimum; identity {+inf, INT64_MAX}
//   argmin_merge  first minimum among the entries with i >= 0; i = -1 = nothing seen (the callers keep NaN costs out)
struct VI {
  double v;
  int64_t i;
};
static __device__ __forceinline__ VI vi_max(VI a, VI b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
static __device__ __forceinline__ VI vi_min(VI a, VI b) {
  if (b.v < a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}
static __device__ __forceinline__ VI argmin_merge(VI a, VI b) {
  if (a.i < 0) return b;
  if (b.i < 0) return a;
  return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// sv, si: nt entries of LDS each; returns the winner (sv[0], si[0]) to every thread.  nt is the workgroup size: a literal where
// the kernel fixes it (the tree is then unrolled), blockDim.x where the launch does
template <typename Merge>
static __device__ __forceinline__ VI block_arg_reduce(VI x, double* sv, int64_t* si, int nt, Merge merge) {
  const int t = threadIdx.x;
  sv[t] = x.v;
  si[t] = x.i;
  __syncthreads();
  for (int h = nt / 2; h > 0; h >>= 1) {
    if (t < h) {
      const VI m = merge(VI{sv[t], si[t]}, VI{sv[t + h], si[t + h]});
      sv[t] = m.v;
      si[t] = m.i;
    }
    __syncthreads();
  }
  return VI{sv[0], si[0]};
}
