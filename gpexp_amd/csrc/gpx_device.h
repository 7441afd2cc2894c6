// Per-pair and per-workgroup device helpers shared by the element-wise kernels of design.hip, hyper.hip, grad.hip and acq.hip
// (gfx950).  __device__ __forceinline__ functions and templates only -- no kernels, no host code.  The tiled fills (kfill.hip)
// and the reductions of reduce.hip / chol.hip have their own forms and do not come through here.
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
