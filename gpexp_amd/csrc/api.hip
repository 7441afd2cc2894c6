// extern "C" entry points of libgpx_hip.so (declared in include/gpx.h) and the small amount of
// host-side state behind them: one HIP stream per context, an exact-size caching allocator so that
// optimiser loops (gp.py:635 calls loglikeParams ~40x) do not hit hipMalloc, event-based per-class
// kernel timing for bench.py's roofline line.
#include "gpx_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>

static thread_local char g_err[1024] = "";

void gpx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- allocator -------------------------------------------------------------------------------------
static constexpr int64_t GUARD = 4096;

int gpx_dev_alloc(gpx_ctx* ctx, int64_t bytes, void** out) {
  if (bytes <= 0) bytes = 8;
  bytes = gpx_round_up(bytes, 256);
  const int64_t key = bytes + (ctx->guard ? 2 * GUARD : 0);
  void* base = nullptr;
  auto it = ctx->pool.find(key);
  if (it != ctx->pool.end()) {
    base = it->second;
    ctx->pool.erase(it);
    ctx->pool_bytes -= key;
    auto pf = ctx->pending.find(base);
    if (pf != ctx->pending.end()) {  // freed by gpx_mat_free while work may still have been queued on it: wait for that work
      for (hipEvent_t ev : pf->second->evs) (void)hipEventSynchronize(ev);
      if (pf->second.use_count() == 1)
        for (hipEvent_t ev : pf->second->evs) ctx->fence_free.push_back(ev);
      ctx->pending.erase(pf);
    }
  } else {
    hipError_t e = hipMalloc(&base, (size_t)key);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      gpx_trim(ctx);
      e = hipMalloc(&base, (size_t)key);
    }
    if (e != hipSuccess) {
      gpx_set_error("hipMalloc(%lld bytes) failed: %s", (long long)key, hipGetErrorString(e));
      return -2;
    }
  }
  if (ctx->guard) {
    GPX_HIP(hipDeviceSynchronize());
    GPX_HIP(hipMemset(base, 0xA5, (size_t)GUARD));
    GPX_HIP(hipMemset((char*)base + GUARD + bytes, 0xA5, (size_t)GUARD));
    if (ctx->guard >= 2) GPX_HIP(hipMemset((char*)base + GUARD, 0xFF, (size_t)bytes));  // poison: every double a NaN
    GPX_HIP(hipDeviceSynchronize());  // hipMemset on device memory may return before it has run; the context's streams are
                                      // non-blocking, i.e. not ordered against the null stream it runs on
    *out = (char*)base + GUARD;
  } else {
    *out = base;
  }
  ctx->out_bytes += key;
  return 0;
}

void gpx_dev_release(gpx_ctx* ctx, void* p, int64_t bytes) {
  if (!p) return;
  if (bytes <= 0) bytes = 8;
  bytes = gpx_round_up(bytes, 256);
  const int64_t key = bytes + (ctx->guard ? 2 * GUARD : 0);
  void* base = p;
  if (ctx->guard) {
    base = (char*)p - GUARD;
    std::vector<unsigned char> h((size_t)(2 * GUARD));
    (void)hipDeviceSynchronize();
    if (hipMemcpy(h.data(), base, (size_t)GUARD, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(h.data() + GUARD, (char*)p + bytes, (size_t)GUARD, hipMemcpyDeviceToHost) == hipSuccess) {
      int64_t below = 0, above = 0;
      for (int64_t i = 0; i < GUARD; ++i) {
        below += h[(size_t)i] != 0xA5;
        above += h[(size_t)(GUARD + i)] != 0xA5;
      }
      if (below || above) {
        ctx->guard_violations += 1;
        fprintf(stderr, "gpx: ALLOCATION GUARD VIOLATED: %lld-byte block, %lld bytes overwritten below, %lld above\n",
                (long long)bytes, (long long)below, (long long)above);
      }
    }
  }
  ctx->pool.insert({key, base});
  ctx->pool_bytes += key;
  ctx->out_bytes -= key;
}

// ---- profiling -------------------------------------------------------------------------------------
// Back-to-back scopes of one class on one stream share an event pair (the end event is simply re-recorded): the
// recursive factorisation issues ~2600 launches per step and two event records per launch cost ~15 ms of the timed
// region.  The 1-2 us launch gaps inside such a run are then counted as kernel time -- a slightly pessimistic
// `achieved`, within 0.5 % of the rocprofv3 kernel-only total.
// one workgroup that spins for `ticks` of the constant-rate wall clock (wall_clock64: hipDeviceAttributeWallClockRate kHz, 100 MHz
// on MI355X): GPX_CHAOS, gpx_dbg_spin and the paced replay.  (Rounds 2-3 counted s_memtime, which on gfx950 runs at the SHADER
// clock -- measured round 4: a "5 ms" spin took 0.22 ms -- so the chaos mode's delays were 0.005 .. 0.13 ms, not 0.1 .. 3 ms.)
__global__ void dbg_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}

// ticks of the wall clock per microsecond on this device (queried once)
static double spin_ticks_per_us(gpx_ctx* ctx) {
  static double tpu = 0.0;
  if (tpu == 0.0) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) {
      (void)hipGetLastError();
      khz = 100000;
    }
    tpu = (double)khz / 1000.0;
  }
  return tpu;
}

ProfScope::ProfScope(gpx_ctx* c, int cls, double flops, double bytes) : ctx(c), idx(-1) {
  if (c->chaos) {
    c->chaos = c->chaos * 6364136223846793005ULL + 1442695040888963407ULL;
    const unsigned r = (unsigned)(c->chaos >> 33);
    if ((r & 3u) == 0u)  // 0.1 .. 3 ms of the wall clock
      hipLaunchKernelGGL(dbg_spin_kernel, dim3(1), dim3(64), 0, c->stream,
                         (long long)((100.0 + (double)((r >> 2) % 2900)) * spin_ticks_per_us(c)));
  }
  if (!c->prof_on) return;
  c->prof_launches[cls] += 1;
  c->prof_flops[cls] += flops;
  c->prof_bytes[cls] += bytes;
  if (!c->prof_recs.empty()) {
    ProfRec& last = c->prof_recs.back();
    if (last.cls == cls && last.stream == c->stream && !last.open) {
      last.open = true;
      idx = (int)c->prof_recs.size() - 1;
      return;
    }
  }
  ProfRec r;
  r.cls = cls;
  r.stream = c->stream;
  r.open = true;
  hipEvent_t ev[2];
  for (int i = 0; i < 2; ++i) {
    if (!c->ev_free.empty()) {
      ev[i] = c->ev_free.back();
      c->ev_free.pop_back();
    } else if (hipEventCreate(&ev[i]) != hipSuccess) {
      return;
    }
  }
  r.a = ev[0];
  r.b = ev[1];
  (void)hipEventRecord(r.a, c->stream);
  c->prof_recs.push_back(r);
  idx = (int)c->prof_recs.size() - 1;
}

ProfScope::~ProfScope() {
  if (idx >= 0) {
    ProfRec& r = ctx->prof_recs[(size_t)idx];
    (void)hipEventRecord(r.b, r.stream);
    r.open = false;
  }
}

int gpx_prof_flush(gpx_ctx* ctx) {
  if (ctx->prof_recs.empty()) return 0;
  GPX_HIP(hipDeviceSynchronize());  // records may sit on any of the context's streams
  for (auto& r : ctx->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) ctx->prof_ms[r.cls] += ms;
    ctx->ev_free.push_back(r.a);
    ctx->ev_free.push_back(r.b);
  }
  ctx->prof_recs.clear();
  return 0;
}

// ---- kernel parameters -----------------------------------------------------------------------------
int gpx_make_kparams(int kind, int d, const double* hyp, int nhyp, KParams* kp) {
  GPX_ARG(d >= 1 && d <= GPX_MAXD, "dimension must be in [1, GPX_MAX_DIM]");
  GPX_ARG(hyp != nullptr, "hyp is NULL");
  memset(kp, 0, sizeof(*kp));
  kp->kind = kind;
  kp->d = d;
  switch (kind) {
    case GPX_K_SE:
      GPX_ARG(nhyp == d + 1, "SE needs d correlation lengths + signalSize");
      for (int k = 0; k < d; ++k) kp->scale[k] = 1.0 / hyp[k];
      kp->sig = hyp[d];
      break;
    case GPX_K_MATERN32:
    case GPX_K_MATERN52: {
      GPX_ARG(nhyp == 2, "Matern needs {rho, signalSize}");
      const double c = (kind == GPX_K_MATERN32 ? sqrt(3.0) : sqrt(5.0)) / hyp[0];
      for (int k = 0; k < d; ++k) kp->scale[k] = c;
      kp->sig = hyp[1];
      break;
    }
    case GPX_K_MEHLER: {
      GPX_ARG(nhyp == d, "Mehler needs d parameters t_k");
      double s = 1.0;
      for (int k = 0; k < d; ++k) {
        const double t = hyp[k], om = 1.0 - t * t;
        kp->scale[k] = 1.0;
        kp->c1[k] = t * t / (2.0 * om);
        kp->c2[k] = t / om;
        s *= pow(om, -0.5);
      }
      kp->sig = s;
      break;
    }
    default: gpx_set_error("unknown kernel kind %d", kind); return -1;
  }
  return 0;
}

// ---- point-set bounding boxes, centring and the exact-path decision (see KParams) -----------------------
// Also records the first non-finite coordinate (bad_row / bad_col, -1 = none): the comparisons below skip a NaN, and the fill
// kernels' clamps (v_max_f64 returns its non-NaN operand) would turn it into a covariance of exactly 0 -- gpx_kparams_sets
// refuses such a set instead, at no cost to the kernels.
static void bbox_from_host(gpx_mat* m, const double* src, int64_t rows, int64_t cols, int64_t ld) {
  m->bbox_ok = 0;
  m->bad_row = m->bad_col = -1;
  if (cols < 1 || cols > GPX_MAXD || rows < 1) return;
  for (int64_t k = 0; k < cols; ++k) m->lo[k] = m->hi[k] = src[k];
  for (int64_t i = 0; i < rows; ++i) {
    const double* r = src + i * ld;
    for (int64_t k = 0; k < cols; ++k) {
      const double v = r[k];
      if (v < m->lo[k]) m->lo[k] = v;
      if (v > m->hi[k]) m->hi[k] = v;
      if (!(fabs(v) <= 1.79769313486231570815e308) && m->bad_row < 0) {  // NaN or +-inf
        m->bad_row = i;
        m->bad_col = k;
      }
    }
  }
  m->bbox_ok = 1;
}

static int mat_bbox(gpx_ctx* ctx, const gpx_mat* cm) {
  gpx_mat* m = const_cast<gpx_mat*>(cm);  // a cache: the matrix itself is not modified
  if (m->bbox_ok || m->rows < 1) return 0;
  GPX_ARG(m->cols >= 1 && m->cols <= GPX_MAXD, "point set has more than GPX_MAX_DIM columns");
  std::vector<double> h((size_t)(m->rows * m->cols));
  GPX_HIP(hipMemcpy2DAsync(h.data(), (size_t)m->cols * 8, m->p, (size_t)m->ld * 8, (size_t)m->cols * 8, (size_t)m->rows,
                           hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  bbox_from_host(m, h.data(), m->rows, m->cols, m->cols);
  return 0;
}

// (gpx_dist.h) a point set that is a SLICE of a larger one takes the larger set's bounding box: the centring and the exact-path
// decision of every fill it enters (gpx_kparams_sets) then do not depend on how the set was sharded over the ranks (ADVICE r4:
// the sharded greedy-IVAR state differed from the single-rank one in the last bits, enough to flip a near-tie)
extern "C" int gpx_points_set_box(gpx_ctx* ctx, gpx_mat* P, const double* lo, const double* hi, int d) {
  GPX_ARG(ctx && P && lo && hi && d >= 1 && d <= GPX_MAXD && P->cols == d, "points_set_box: bad arguments");
  // the box is the caller's; the scan for non-finite coordinates (bad_row) is still of P's own rows.  Free for a set uploaded
  // from the host (scanned at upload: all gpexp_amd/device.py does); a set last written on the device pays one copy to the
  // host and a stream synchronisation here, as it would in the first fill it enters.
  GPX_TRY(mat_bbox(ctx, P));
  for (int k = 0; k < d; ++k) {
    GPX_ARG(lo[k] <= hi[k], "points_set_box: empty box");
    P->lo[k] = lo[k];
    P->hi[k] = hi[k];
  }
  P->bbox_ok = 1;
  return 0;
}

// S * sensitivity above which the expanded-form distance would cost more than ~2e-14 of relative kernel error
// (measured: 7.6e-15 at S*sens = 75, 5.8e-15 at 119: tests/test_gpu_kfill_accuracy.py, family d);
// sensitivity = max |dk/ds| / sig: 1/2 for SE and Matern-3/2, 1/6 for Matern-5/2
static double exact_threshold() {
  const char* e = getenv("GPX_EXACT_S");  // read per call: the tests force either path on the same data
  return e ? atof(e) : 120.0;
}

int gpx_kparams_sets(gpx_ctx* ctx, KParams* kp, const gpx_mat* A, const gpx_mat* B, const gpx_mat* C) {
  for (int k = 0; k < GPX_MAXD; ++k) kp->center[k] = 0.0;
  kp->exact = 0;
  const gpx_mat* sets[3] = {A, B, C};
  double lo[GPX_MAXD], hi[GPX_MAXD];
  bool any = false;
  for (const gpx_mat* s : sets) {
    if (!s || s->rows < 1) continue;
    GPX_TRY(mat_bbox(ctx, s));
    if (s->bad_row >= 0) {  // every kind, Mehler included (include/gpx.h, gpx_kfill)
      gpx_set_error("point set has a non-finite coordinate (NaN or infinity) at row %lld, column %lld",
                    (long long)s->bad_row, (long long)s->bad_col);
      return -1;
    }
    if (kp->kind == GPX_K_MEHLER) continue;
    for (int k = 0; k < kp->d; ++k) {
      if (!any || s->lo[k] < lo[k]) lo[k] = s->lo[k];
      if (!any || s->hi[k] > hi[k]) hi[k] = s->hi[k];
    }
    any = true;
  }
  if (!any || kp->kind == GPX_K_MEHLER) return 0;
  double S = 0.0;
  for (int k = 0; k < kp->d; ++k) {
    const double c = 0.5 * lo[k] + 0.5 * hi[k];
    kp->center[k] = fabs(c) < 1e300 ? c : 0.0;  // finite inputs whose midpoint would overflow the centred squares
    const double hw = (hi[k] - kp->center[k]) * kp->scale[k];
    S += 2.0 * hw * hw;  // both operands of a pair may sit at the edge of the box
  }
  const double sens = kp->kind == GPX_K_MATERN52 ? 1.0 / 6.0 : 0.5;
  kp->exact = !(S * sens <= exact_threshold());  // NaN -> exact
  return 0;
}

// C[i][j] -= sum_b P_b[i][j] for j <= i (P_b: n x n, row stride n, consecutive), partials added in batch order
__global__ __launch_bounds__(256) static void sub_partials_kernel(const double* __restrict__ P, int64_t nbat, int64_t n,
                                                                  double* __restrict__ C, int64_t ldc) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= n || j > i) return;
  double s = 0.0;
  for (int64_t b = 0; b < nbat; ++b) s += P[(b * n + i) * n + j];
  C[i * ldc + j] -= s;
}

int launch_sub_partials(gpx_ctx* ctx, const double* P, int64_t nbat, int64_t n, double* C, int64_t ldc) {
  hipLaunchKernelGGL(sub_partials_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, ctx->stream, P, nbat, n, C,
                     ldc);
  GPX_HIP(hipGetLastError());
  return 0;
}

// ---- matrices ----------------------------------------------------------------------------------------
int gpx_mat_new(gpx_ctx* ctx, int64_t rows, int64_t cols, int pad, gpx_mat** out) {
  GPX_ARG(rows >= 0 && cols >= 0, "negative shape");
  gpx_mat* m = new gpx_mat();
  m->rows = rows;
  m->cols = cols;
  m->prows = pad ? gpx_round_up(rows > 0 ? rows : 1, GPX_TILE) : (rows > 0 ? rows : 1);
  m->pcols = pad ? gpx_round_up(cols > 0 ? cols : 1, GPX_TILE) : (cols > 0 ? cols : 1);
  m->ld = pad ? gpx_skew_ld(m->pcols) : m->pcols;
  m->bytes = m->prows * m->ld * (int64_t)sizeof(double);
  m->aux = nullptr;
  m->aux_bytes = 0;
  m->factored = 0;
  m->bbox_ok = 0;
  m->bad_row = m->bad_col = -1;
  m->binv = nullptr;
  m->binv_bytes = 0;
  m->binv_ib = 0;
  void* p = nullptr;
  int r = gpx_dev_alloc(ctx, m->bytes, &p);
  if (r != 0) {
    delete m;
    return r;
  }
  m->p = (double*)p;
  ctx->live_mats.insert(m);
  *out = m;
  return 0;
}

extern "C" {

int gpx_abi_version(void) { return GPX_ABI_VERSION; }
const char* gpx_last_error(void) { return g_err; }

int gpx_create(int device, gpx_ctx** out) {
  GPX_ARG(out != nullptr, "out is NULL");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    gpx_set_error("no HIP device available (%s): libgpx_hip has no CPU fallback", hipGetErrorString(e));
    return -2;
  }
  GPX_ARG(device >= 0 && device < ndev, "device ordinal out of range");
  GPX_HIP(hipSetDevice(device));
  gpx_ctx* c = new gpx_ctx();
  { const char* g = getenv("GPX_ALLOC_GUARD"); c->guard = g ? atoi(g) : 0; }
  { const char* g = getenv("GPX_CHAOS"); c->chaos = g ? (uint64_t)strtoull(g, nullptr, 10) : 0; }
  c->guard_violations = 0;
  c->device = device;
  c->pool_bytes = 0;
  c->out_bytes = 0;
  c->comm = nullptr;
  c->rank = 0;
  c->world = 1;
  for (int i = 0; i < 3; ++i) {
    c->grp[i] = nullptr;
    c->grp_size[i] = 1;
    c->grp_rank[i] = 0;
  }
  c->Pr = c->Pc = 1;
  c->piv_min = 0.0;
  c->piv_skip = 0;
  c->pw_binv = c->pw_tmp_build = c->pw_tmp_T = nullptr;
  c->pw_ib = 0;
  c->pw_done = 0;
  c->prof_on = 0;
  for (int i = 0; i < GPX_PROF_NCLASS; ++i) {
    c->prof_launches[i] = 0;
    c->prof_ms[i] = c->prof_flops[i] = c->prof_bytes[i] = 0.0;
  }
  {
    int lo = 0, hi = 0;
    GPX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));  // hi is the numerically lowest = highest priority
    // main stream: NORMAL priority (between the chain / communication streams and the low-priority evaluation stream) when the
    // device has three levels.  It carries the updates that gate the next panel; beside a low-priority stream full of
    // bulk / evaluation GEMMs its workgroups are dispatched first (measured in the distributed replay: with the bulk updates
    // on a stream of HIGHER priority than this one a factorisation took 269 instead of 211 ms -- dispatch priority does decide
    // between two chip-filling kernels, although it does nothing for a kernel that does not fit).
    const int mainp = (lo - hi >= 2) ? (lo + hi) / 2 : lo;
    GPX_HIP(hipStreamCreateWithPriority(&c->streams[0], hipStreamNonBlocking, mainp));
    GPX_HIP(hipStreamCreateWithPriority(&c->streams[1], hipStreamNonBlocking, hi));
    GPX_HIP(hipStreamCreateWithPriority(&c->streams[2], hipStreamNonBlocking, hi));
    GPX_HIP(hipStreamCreateWithPriority(&c->streams[4], hipStreamNonBlocking, lo));
    c->stream = c->streams[0];
  }
  hipDeviceProp_t prop;
  GPX_HIP(hipGetDeviceProperties(&prop, device));
  c->cus = prop.multiProcessorCount;
  {
    // Background stream for work that should fill idle time without standing in the way of a latency-critical chain
    // (the streamed IVAR of the multi-GPU path).  A chip-filling kernel keeps refilling every slot it frees, so a small
    // kernel on another stream -- whatever its priority -- waits for the big kernel to END (scripts/cumask_check.hip:
    // 4 ms vs 14 us).  Mask bit i = CU i/8 of XCD i%8 (scripts/cumask_map.hip): the lowest 32 bits = 4 CUs on every XCD
    // stay free for the other streams.
    const int words = (c->cus + 31) / 32;
    std::vector<uint32_t> mask((size_t)words, 0xffffffffu);
    if (c->cus % 32) mask[(size_t)words - 1] = (1u << (c->cus % 32)) - 1u;
    for (int cu = 0; cu < 4; ++cu)      // CUs 0-3 of every XCD stay free
      for (int x = 0; x < 8; ++x) {
        const int bit = 8 * cu + x;
        if (bit < c->cus) mask[(size_t)bit / 32] &= ~(1u << (bit % 32));
      }
    // two streams with that mask: 3 = background (copies into the replicated factor, streamed evaluation), 5 = bulk (the
    // aggregated trailing updates of the 2-D distributed factorisation: long chip-filling launches beside the diagonal chain)
    for (int si : {3, 5}) {
      if (words < 2 || hipExtStreamCreateWithCUMask(&c->streams[si], (uint32_t)words, mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        int lo = 0, hi = 0;
        GPX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        GPX_HIP(hipStreamCreateWithPriority(&c->streams[si], hipStreamNonBlocking, lo));
      }
    }
  }
  GPX_HIP(hipMalloc((void**)&c->d_info, 256));
  GPX_HIP(hipMalloc((void**)&c->d_scal, 64 * sizeof(double)));
  GPX_HIP(hipMemset(c->d_info, 0, 256));
  c->trsv_scratch = nullptr;
  c->trsv_scratch_bytes = 0;
  c->d2_scratch = nullptr;
  c->dbg_stamps = nullptr;
  c->d2_scratch_bytes = 0;
  c->d2_inv_src = nullptr;
  c->d2_inv_nb = 0;
  c->ev_scratch = nullptr;
  c->ev_scratch_bytes = 0;
  *out = c;
  return 0;
}

// test hook: one workgroup that spins for about `ms` milliseconds (s_memtime ticks at 100 MHz; capped at 500 ms) on the
// selected stream -- delays whatever is queued behind it, so that an ordering hole between streams shows deterministically
int gpx_dbg_spin(gpx_ctx* ctx, int ms) {
  GPX_ARG(ctx && ms >= 0 && ms <= 500, "spin: 0..500 ms");
  if (ms == 0) return 0;
  hipLaunchKernelGGL(dbg_spin_kernel, dim3(1), dim3(64), 0, ctx->stream, (long long)((double)ms * 1000.0 * spin_ticks_per_us(ctx)));
  GPX_HIP(hipGetLastError());
  return 0;
}

// the same in microseconds (<= 500 000): paces the receives of a single-rank replay (scripts/replay_comm.py)
int gpx_dbg_spin_us(gpx_ctx* ctx, int64_t us) {
  GPX_ARG(ctx && us >= 0 && us <= 500000, "spin: 0..500000 us");
  if (us == 0) return 0;
  hipLaunchKernelGGL(dbg_spin_kernel, dim3(1), dim3(64), 0, ctx->stream, (long long)((double)us * spin_ticks_per_us(ctx)));
  GPX_HIP(hipGetLastError());
  return 0;
}

// Paced replay, second form: a STAMP of the wall clock taken on the selected stream (slot < 1024), and a spin that ends `us`
// microseconds after a stamp (at once when that moment has passed; never longer than 0.5 s).  A foreign delivery of the
// single-rank replay is released at "arrival of the previous panel + what its producer took", whatever this rank's
// communication stream did in between (scripts/replay_comm.py).
constexpr int GPX_DBG_STAMPS = 1024;
__global__ void dbg_stamp_kernel(long long* slot) { *slot = wall_clock64(); }
__global__ void dbg_spin_until_kernel(const long long* slot, long long ticks, long long cap) {
  const long long t0 = wall_clock64(), target = *slot + ticks;
  while (wall_clock64() < target && wall_clock64() - t0 < cap) {}
}
static int dbg_stamps_ensure(gpx_ctx* ctx) {
  if (!ctx->dbg_stamps) {
    GPX_HIP(hipMalloc((void**)&ctx->dbg_stamps, GPX_DBG_STAMPS * sizeof(long long)));
    GPX_HIP(hipMemset(ctx->dbg_stamps, 0, GPX_DBG_STAMPS * sizeof(long long)));
  }
  return 0;
}
int gpx_dbg_stamp(gpx_ctx* ctx, int slot) {
  GPX_ARG(ctx && slot >= 0 && slot < GPX_DBG_STAMPS, "stamp: slot 0..1023");
  GPX_TRY(dbg_stamps_ensure(ctx));
  hipLaunchKernelGGL(dbg_stamp_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dbg_stamps + slot);
  GPX_HIP(hipGetLastError());
  return 0;
}
int gpx_dbg_spin_until(gpx_ctx* ctx, int slot, int64_t us) {
  GPX_ARG(ctx && slot >= 0 && slot < GPX_DBG_STAMPS && us <= 500000, "spin_until: slot 0..1023, at most 500000 us");
  if (us <= 0) return 0;
  GPX_TRY(dbg_stamps_ensure(ctx));
  hipLaunchKernelGGL(dbg_spin_until_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->dbg_stamps + slot,
                     (long long)((double)us * spin_ticks_per_us(ctx)), (long long)(500000.0 * spin_ticks_per_us(ctx)));
  GPX_HIP(hipGetLastError());
  return 0;
}

int64_t gpx_dbg_guard_violations(gpx_ctx* ctx) { return ctx ? (ctx->guard ? ctx->guard_violations : -1) : -1; }

// bytes cached in the pool / handed out and not yet returned, both counted in pool keys (the rounded size a block is filed under):
// a call that returns every block under the size it took it with leaves outstanding_bytes where it found it
int gpx_dbg_pool_stats(gpx_ctx* ctx, int64_t* pooled_bytes, int64_t* outstanding_bytes) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  if (pooled_bytes) *pooled_bytes = ctx->pool_bytes;
  if (outstanding_bytes) *outstanding_bytes = ctx->out_bytes;
  return 0;
}

// writes 16 bytes past a scratch block on purpose and returns 1 if the guard check caught it (the count is restored)
int gpx_dbg_guard_selftest(gpx_ctx* ctx) {
  GPX_ARG(ctx && ctx->guard, "guard mode is off");
  void* p;
  GPX_TRY(gpx_dev_alloc(ctx, 1024, &p));
  GPX_HIP(hipMemset((char*)p + 1024, 0, 16));
  const int64_t before = ctx->guard_violations;
  gpx_dev_release(ctx, p, 1024);
  const int caught = ctx->guard_violations == before + 1;
  ctx->guard_violations = before;
  return caught;
}

int gpx_trim(gpx_ctx* ctx) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  (void)hipDeviceSynchronize();  // fenced blocks (gpx_mat_free) may still be in use on any of the context's streams
  for (auto& kv : ctx->pending)
    if (kv.second.use_count() == 1)
      for (hipEvent_t ev : kv.second->evs) ctx->fence_free.push_back(ev);
  ctx->pending.clear();
  for (auto& kv : ctx->pool) (void)hipFree(kv.second);
  ctx->pool.clear();
  ctx->pool_bytes = 0;
  return 0;
}

int gpx_destroy(gpx_ctx* ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  gpx_comm_destroy(ctx);
  gpx_prof_flush(ctx);
  gpx_trim(ctx);
  for (auto ev : ctx->ev_free) (void)hipEventDestroy(ev);
  for (auto ev : ctx->fence_free) (void)hipEventDestroy(ev);
  (void)hipFree(ctx->d_info);
  (void)hipFree(ctx->d_scal);
  if (ctx->trsv_scratch) (void)hipFree(ctx->trsv_scratch);
  if (ctx->d2_scratch) (void)hipFree(ctx->d2_scratch);
  if (ctx->dbg_stamps) (void)hipFree(ctx->dbg_stamps);
  if (ctx->ev_scratch) (void)hipFree(ctx->ev_scratch);
  for (auto ev : ctx->sync_events) (void)hipEventDestroy(ev);
  for (auto ev : ctx->la_events) (void)hipEventDestroy(ev);
  if (ctx->ev_side) (void)hipEventDestroy(ctx->ev_side);
  for (int i = 0; i < GPX_NSTREAMS; ++i) {
    bool seen = false;   // (GPX_STREAM_ALIAS: an index may share its stream with an earlier one)
    for (int j = 0; j < i; ++j) seen = seen || ctx->streams[j] == ctx->streams[i];
    if (!seen) (void)hipStreamDestroy(ctx->streams[i]);
  }
  delete ctx;
  return 0;
}

int gpx_sync(gpx_ctx* ctx) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  GPX_HIP(hipSetDevice(ctx->device));
  GPX_HIP(hipDeviceSynchronize());  // every stream of this process on this device
  return 0;
}

int gpx_stream_select(gpx_ctx* ctx, int which) {
  GPX_ARG(ctx && which >= 0 && which < GPX_NSTREAMS,
          "stream index must be 0 (main), 1 (panel), 2 (communication), 3 (background, CU-masked), 4 (evaluation) or 5 (bulk, "
          "CU-masked)");
  ctx->stream = ctx->streams[which];
  return 0;
}

static int sync_event(gpx_ctx* ctx, int id, hipEvent_t* out) {
  GPX_ARG(ctx && id >= 0 && id < 65536, "event id out of range");
  while ((int)ctx->sync_events.size() <= id) {
    hipEvent_t ev;
    static int timing = -1;   // GPX_EVENT_TIMING=1 (debug): the pipeline's events carry time stamps (gpx_dbg_event_elapsed)
    if (timing < 0) timing = getenv("GPX_EVENT_TIMING") ? atoi(getenv("GPX_EVENT_TIMING")) : 0;
    GPX_HIP(hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming));
    ctx->sync_events.push_back(ev);
  }
  *out = ctx->sync_events[(size_t)id];
  return 0;
}

// debug (gpx_debug.h): ms between the last records of two pipeline events (GPX_EVENT_TIMING=1; both must have completed);
// returns 1 when an event of the pair was never recorded
int gpx_dbg_event_elapsed(gpx_ctx* ctx, int id0, int id1, double* ms) {
  GPX_ARG(ctx && ms && id0 >= 0 && id1 >= 0, "bad arguments");
  if (id0 >= (int)ctx->sync_events.size() || id1 >= (int)ctx->sync_events.size()) return 1;
  float f = 0.0f;
  if (hipEventElapsedTime(&f, ctx->sync_events[(size_t)id0], ctx->sync_events[(size_t)id1]) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  *ms = (double)f;
  return 0;
}

int gpx_event_record(gpx_ctx* ctx, int id) {
  hipEvent_t ev;
  GPX_TRY(sync_event(ctx, id, &ev));
  GPX_HIP(hipEventRecord(ev, ctx->stream));
  return 0;
}

int gpx_event_wait(gpx_ctx* ctx, int id) {
  hipEvent_t ev;
  GPX_TRY(sync_event(ctx, id, &ev));
  GPX_HIP(hipStreamWaitEvent(ctx->stream, ev, 0));
  return 0;
}

int gpx_device_info(gpx_ctx* ctx, char* name, int name_len, int* cus, int64_t* hbm_bytes, int* clock_mhz) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  hipDeviceProp_t prop;
  GPX_HIP(hipGetDeviceProperties(&prop, ctx->device));
  if (name && name_len > 0) {
    snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (cus) *cus = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
  return 0;
}

int gpx_mat_alloc(gpx_ctx* ctx, int64_t rows, int64_t cols, int pad, gpx_mat** out) {
  GPX_ARG(ctx && out, "NULL argument");
  GPX_TRY(gpx_mat_new(ctx, rows, cols, pad, out));
  GPX_HIP(hipMemsetAsync((*out)->p, 0, (size_t)(*out)->bytes, ctx->stream));
  // the caller may use the matrix on ANY of the context's streams next (the multi-GPU pipeline fills cross matrices on
  // the background stream): the zero fill must not still be in flight on this one
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_mat_from_host(gpx_ctx* ctx, const double* src, int64_t rows, int64_t cols, int pad, gpx_mat** out) {
  GPX_ARG(ctx && out && (src || rows * cols == 0), "NULL argument");
  GPX_TRY(gpx_mat_alloc(ctx, rows, cols, pad, out));
  gpx_mat* m = *out;
  if (rows > 0 && cols > 0)
    GPX_HIP(hipMemcpy2DAsync(m->p, (size_t)m->ld * 8, src, (size_t)cols * 8, (size_t)cols * 8, (size_t)rows,
                             hipMemcpyHostToDevice, ctx->stream));
  if (!pad) bbox_from_host(m, src, rows, cols, cols);  // point sets are uploaded unpadded
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_mat_clone(gpx_ctx* ctx, const gpx_mat* src, gpx_mat** out) {
  GPX_ARG(ctx && src && out, "NULL argument");
  const int padded = src->prows != (src->rows > 0 ? src->rows : 1) || src->pcols != (src->cols > 0 ? src->cols : 1) ||
                     src->ld != src->pcols;
  GPX_TRY(gpx_mat_new(ctx, src->rows, src->cols, padded, out));
  gpx_mat* m = *out;
  if (m->bytes != src->bytes || m->ld != src->ld) {
    gpx_mat_free(ctx, m);
    *out = nullptr;
    GPX_ARG(false, "clone: storage layout of the copy differs from the source");
  }
  // (every failure from here on frees the copy and leaves *out NULL -- a half-initialised handle used to leak)
  auto fail = [&](const char* what) {
    gpx_set_error("clone: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
    gpx_mat_free(ctx, m);
    *out = nullptr;
    return -2;
  };
  if (hipMemcpyAsync(m->p, src->p, (size_t)src->bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return fail("copy");
  if (src->aux) {
    void* p = nullptr;
    int r = gpx_dev_alloc(ctx, src->aux_bytes, &p);
    if (r != 0) {
      gpx_mat_free(ctx, m);
      *out = nullptr;
      return r;
    }
    m->aux = (double*)p;
    m->aux_bytes = src->aux_bytes;
    if (hipMemcpyAsync(m->aux, src->aux, (size_t)src->aux_bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
      return fail("copy of the leaf inverses");
  }
  m->factored = src->factored;
  m->bbox_ok = src->bbox_ok;
  m->bad_row = src->bad_row;
  m->bad_col = src->bad_col;
  for (int k = 0; k < GPX_MAXD; ++k) {
    m->lo[k] = src->lo[k];
    m->hi[k] = src->hi[k];
  }
  // binv / dinv are caches rebuilt on demand (binv_ib = 0 from gpx_mat_new)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("synchronisation");
  return 0;
}

int gpx_mat_free(gpx_ctx* ctx, gpx_mat* m) {
  if (!m) return 0;
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  // Work queued on ANY of the context's streams may still reference the buffers (side-stream solves, the background
  // evaluation) and the pool may hand them out again right away.  Round 2 synchronised the whole device here -- several times
  // per cost evaluation of an optimiser loop.  Now the buffers carry a FENCE (one event per stream, recorded here) and
  // whoever reuses them waits for it (gpx_dev_alloc); the free itself never blocks.  (Guard mode checks the bands at release
  // and needs the writes to have landed: it keeps the synchronisation.)
  if (ctx->guard) {
    (void)hipDeviceSynchronize();
  } else {
    auto f = std::make_shared<gpx_ctx::Fence>();
    bool ok = true;
    for (int i = 0; i < GPX_NSTREAMS && ok; ++i) {
      hipEvent_t ev = nullptr;
      if (!ctx->fence_free.empty()) {
        ev = ctx->fence_free.back();
        ctx->fence_free.pop_back();
      } else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        ok = false;
        break;
      }
      f->evs.push_back(ev);
      if (hipEventRecord(ev, ctx->streams[i]) != hipSuccess) ok = false;
    }
    if (!ok) {
      (void)hipGetLastError();
      (void)hipDeviceSynchronize();
      for (hipEvent_t ev : f->evs) ctx->fence_free.push_back(ev);
    } else {
      // a block that comes back while an older fence is still attached keeps the NEWER one (it covers everything queued since)
      ctx->pending[m->p] = f;
      if (m->aux) ctx->pending[m->aux] = f;
      if (m->binv) ctx->pending[m->binv] = f;
      if (m->dinv) ctx->pending[m->dinv] = f;
    }
  }
  ctx->live_mats.erase(m);
  gpx_dev_release(ctx, m->p, m->bytes);
  if (m->aux) gpx_dev_release(ctx, m->aux, m->aux_bytes);
  if (m->binv) gpx_dev_release(ctx, m->binv, m->binv_bytes);
  if (m->dinv) gpx_dev_release(ctx, m->dinv, m->dinv_bytes);
  delete m;
  return 0;
}

int gpx_mat_shape(const gpx_mat* m, int64_t* rows, int64_t* cols, int64_t* ld) {
  GPX_ARG(m != nullptr, "matrix is NULL");
  if (rows) *rows = m->rows;
  if (cols) *cols = m->cols;
  if (ld) *ld = m->ld;
  return 0;
}

int gpx_mat_to_host(gpx_ctx* ctx, const gpx_mat* m, double* dst, int tri) {
  GPX_ARG(ctx && m && dst, "NULL argument");
  GPX_ARG(tri >= 0 && tri <= 2, "tri must be 0, 1 or 2");
  GPX_ARG(tri == 0 || m->rows == m->cols, "triangular extraction needs a square matrix");
  if (m->rows == 0 || m->cols == 0) return 0;
  GPX_HIP(hipMemcpy2DAsync(dst, (size_t)m->cols * 8, m->p, (size_t)m->ld * 8, (size_t)m->cols * 8,
                           (size_t)m->rows, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t n = m->rows;
  if (tri == 1) {
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = i + 1; j < n; ++j) dst[i * n + j] = 0.0;
  } else if (tri == 2) {
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = i + 1; j < n; ++j) dst[i * n + j] = dst[j * n + i];
  }
  return 0;
}

int gpx_mat_read(gpx_ctx* ctx, const gpx_mat* m, int64_t offset, int64_t count, double* dst) {
  GPX_ARG(ctx && m && dst && offset >= 0 && count >= 0 && (offset + count) * 8 <= m->bytes, "bad raw read");
  if (count == 0) return 0;
  GPX_HIP(hipMemcpyAsync(dst, m->p + offset, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_mat_write(gpx_ctx* ctx, gpx_mat* m, int64_t offset, int64_t count, const double* src) {
  GPX_ARG(ctx && m && src && offset >= 0 && count >= 0 && (offset + count) * 8 <= m->bytes, "bad raw write");
  if (count == 0) return 0;
  m->bbox_ok = 0;
  GPX_HIP(hipMemcpyAsync(m->p + offset, src, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// dst[doff : doff+n] = src[soff : soff+n] (mode 0), += src (mode 1), = 0 (mode 2; src ignored); asynchronous.
// The vector glue of the distributed substitution sweeps (gpexp_amd/dist.py).
__global__ __launch_bounds__(256) static void vec_op_kernel(double* __restrict__ dst, const double* __restrict__ src,
                                                            int64_t n, int mode) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dst[i] = mode == 0 ? src[i] : (mode == 1 ? dst[i] + src[i] : 0.0);
}

int gpx_vec_op(gpx_ctx* ctx, gpx_mat* dst, int64_t doff, const gpx_mat* src, int64_t soff, int64_t n, int mode) {
  GPX_ARG(ctx && dst && mode >= 0 && mode <= 2 && (mode == 2 || src), "bad vector operation");
  GPX_ARG(doff >= 0 && n >= 0 && (doff + n) * 8 <= dst->bytes, "destination range out of bounds");
  GPX_ARG(mode == 2 || (soff >= 0 && (soff + n) * 8 <= src->bytes), "source range out of bounds");
  if (n == 0) return 0;
  dst->bbox_ok = 0;  // a cached bounding box (point sets) does not survive a device-side write
  hipLaunchKernelGGL(vec_op_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dst->p + doff,
                     mode == 2 ? nullptr : src->p + soff, n, mode);
  GPX_HIP(hipGetLastError());
  return 0;
}

// ---- covariance assembly -----------------------------------------------------------------------------
int gpx_kfill_into(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* Z,
                   const double* nugget, int64_t nugget_len, gpx_mat* K) {
  GPX_ARG(ctx && X && K, "NULL argument");
  KParams kp;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  GPX_ARG(X->cols == d && X->pcols == d, "X must be an unpadded (N x d) point set");
  const int symmetric = (Z == nullptr);
  const gpx_mat* Bp = symmetric ? X : Z;
  GPX_ARG(Bp->cols == d && Bp->pcols == d, "Z must be an unpadded (M x d) point set");
  GPX_ARG(K->rows == X->rows && K->cols == Bp->rows, "output matrix has the wrong shape");
  GPX_ARG(K->prows % GPX_TILE == 0 && K->pcols % GPX_TILE == 0, "output matrix must be padded");
  GPX_ARG(nugget_len == 0 || nugget_len == 1 || nugget_len == X->rows, "nugget_len must be 0, 1 or N");
  GPX_ARG(symmetric || nugget_len == 0, "nugget only applies to the symmetric form");
  GPX_ARG(nugget_len == 0 || nugget != nullptr, "nugget is NULL");
  GPX_TRY(gpx_kparams_sets(ctx, &kp, X, Bp));
  Scratch sc(ctx);
  double* d_nug = nullptr;
  double nscal = 0.0;
  if (nugget_len == 1) nscal = nugget[0];
  if (nugget_len > 1) {
    GPX_TRY(sc.get(nugget_len * 8, &d_nug));
    GPX_HIP(hipMemcpyAsync(d_nug, nugget, (size_t)nugget_len * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  int r = launch_kfill(ctx, kp, X->p, X->rows, Bp->p, Bp->rows, symmetric, d_nug, nugget_len, nscal, K->p,
                       K->prows, K->pcols, K->ld);
  K->binv_ib = 0;  // block inverses (chol_potrs) belong to the previous contents
  K->factored = 0;
  return r;
}

int gpx_kfill(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* Z,
              const double* nugget, int64_t nugget_len, gpx_mat** outK) {
  GPX_ARG(ctx && X && outK, "NULL argument");
  MatHold K(ctx);
  GPX_TRY(gpx_mat_new(ctx, X->rows, Z ? Z->rows : X->rows, 1, K.put()));
  GPX_TRY(gpx_kfill_into(ctx, kind, d, hyp, nhyp, X, Z, nugget, nugget_len, K.get()));
  *outK = K.release();
  return 0;
}

int gpx_kdiag(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* Z, double* out) {
  GPX_ARG(ctx && Z && out, "NULL argument");
  KParams kp;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  GPX_ARG(Z->cols == d && Z->pcols == d, "Z must be an unpadded (M x d) point set");
  if (Z->rows == 0) return 0;
  Scratch sc(ctx);   // (its scope exit completes the copy)
  double* p;
  GPX_TRY(sc.get(Z->rows * 8, &p));
  GPX_TRY(launch_kdiag(ctx, kp, Z->p, Z->rows, p));
  GPX_HIP(hipMemcpyAsync(out, p, (size_t)Z->rows * 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// ---- factorisation and solves ----------------------------------------------------------------------
// The factorisation in two halves: potrf_begin enqueues everything (nothing blocks), potrf_end waits, reads the pivot flag,
// returns the scratch and completes the block inverses.
struct PotrfJob {
  bool blocked, built;
  void *ptb, *ptt;
  int64_t ib, tb_bytes, tt_bytes;
  int rc;
};

static int potrf_begin(gpx_ctx* ctx, gpx_mat* K, PotrfJob* J) {
  GPX_ARG(ctx && K, "NULL argument");
  GPX_ARG(K->rows == K->cols && K->prows == K->pcols && K->prows % GPX_TILE == 0, "potrf needs a padded square matrix");
  if (!K->aux) {
    K->aux_bytes = K->prows * GPX_TILE * 8;
    void* p;
    GPX_TRY(gpx_dev_alloc(ctx, K->aux_bytes, &p));
    K->aux = (double*)p;
  }
  K->binv_ib = 0;  // block inverses of an earlier factorisation are stale (the buffer itself is reused)
  K->factored = 0;
  // Large matrices take the blocked look-ahead path, which builds the explicit inverses of the 1024-order diagonal blocks
  // as it goes (its panel solves use them; potrs and the posterior solves reuse them): give it the storage.
  const int64_t np = K->prows;
  J->blocked = np >= 8192;
  J->built = false;
  J->ptb = J->ptt = nullptr;
  J->ib = chol_binv_order(np);
  const int64_t bbytes = chol_binv_elems(np) * 8;
  J->tb_bytes = ((np + J->ib - 1) / J->ib) * J->ib * J->ib * 8;
  J->tt_bytes = np * J->ib * 8;
  if (J->blocked) {
    if (K->binv && K->binv_bytes != bbytes) {
      gpx_dev_release(ctx, K->binv, K->binv_bytes);
      K->binv = nullptr;
    }
    if (!K->binv) {
      void* p;
      GPX_TRY(gpx_dev_alloc(ctx, bbytes, &p));
      K->binv = (double*)p;
      K->binv_bytes = bbytes;
    }
    GPX_TRY(gpx_dev_alloc(ctx, J->tb_bytes, &J->ptb));
    int ra = gpx_dev_alloc(ctx, J->tt_bytes, &J->ptt);
    if (ra != 0) {
      gpx_dev_release(ctx, J->ptb, J->tb_bytes);
      return ra;
    }
    ctx->pw_binv = K->binv;
    ctx->pw_ib = J->ib;
    ctx->pw_tmp_build = (double*)J->ptb;
    ctx->pw_tmp_T = (double*)J->ptt;
  }
  ctx->pw_done = 0;
  J->rc = chol_potrf(ctx, K->p, K->ld, np, K->aux, K->rows);
  J->built = ctx->pw_done != 0;
  ctx->pw_binv = ctx->pw_tmp_build = ctx->pw_tmp_T = nullptr;
  ctx->pw_ib = 0;
  ctx->pw_done = 0;
  return 0;
}

static int potrf_end(gpx_ctx* ctx, gpx_mat* K, PotrfJob* J) {
  int rc = J->rc, info = 0;
  if (rc == 0 && hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = -2;
  if (hipDeviceSynchronize() != hipSuccess && rc == 0) rc = -2;  // the look-ahead path uses three streams
  if (J->blocked) {
    gpx_dev_release(ctx, J->ptb, J->tb_bytes);
    gpx_dev_release(ctx, J->ptt, J->tt_bytes);
  }
  if (rc != 0) {
    if (rc == -2) gpx_set_error("potrf: HIP call failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
  }
  K->factored = (info == 0);
  if (info != 0) gpx_set_error("potrf: matrix is not positive definite (pivot %d <= 0)", info);
  // explicit inverses of the diagonal blocks for the solves that follow (potrs, posterior / IVAR): completed here, on the
  // factorisation's stream, so that consumers on different streams (the bench runs potrs beside IVAR) find them ready
  if (info == 0 && chol_cross_oop(K->prows)) {
    if (J->built)
      GPX_TRY(chol_binv_finish(ctx, K, J->ib));
    else
      GPX_TRY(chol_binv_ensure(ctx, K));
    GPX_HIP(hipStreamSynchronize(ctx->stream));
  }
  return info;
}

int gpx_potrf(gpx_ctx* ctx, gpx_mat* K) {
  PotrfJob J;
  GPX_TRY(potrf_begin(ctx, K, &J));
  return potrf_end(ctx, K, &J);
}

static int need_factor(const gpx_mat* L) {
  GPX_ARG(L != nullptr, "factor is NULL");
  GPX_ARG(L->factored && L->aux, "matrix has not been factored by gpx_potrf");
  return 0;
}

}  // extern "C"

int gpx_entry_args(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                   const gpx_mat* Z, const gpx_mat* C, const char* points_msg, KParams* kp) {
  GPX_TRY(need_factor(L));
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, kp));
  for (const gpx_mat* P : {X, Z, C})
    if (P) GPX_ARG(P->cols == d && P->pcols == d, points_msg);
  GPX_ARG(X->rows == L->rows, "X does not match the factor");
  return Z ? gpx_kparams_sets(ctx, kp, X, Z, C) : 0;
}

// (gpx_internal.h) the one budget rule
int64_t gpx_chunk_len(int64_t default_budget, int64_t bytes_per_col) {
  int64_t budget = default_budget;
  const char* e = getenv("GPX_CROSS_BYTES");
  if (e && atoll(e) > 0) budget = atoll(e);
  const int64_t mc = budget / bytes_per_col / GPX_TILE * GPX_TILE;
  return mc < GPX_TILE ? GPX_TILE : mc;
}

// (gpx_internal.h) the uploads of host vectors
int gpx_fill_padded(gpx_ctx* ctx, double* dev, const double* host, int64_t n, int64_t np) {
  GPX_HIP(hipMemsetAsync(dev, 0, (size_t)np * 8, ctx->stream));
  GPX_HIP(hipMemcpyAsync(dev, host, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}
int gpx_upload_padded(gpx_ctx* ctx, Scratch& sc, const double* host, int64_t n, int64_t np, double** dev) {
  GPX_TRY(sc.get(np * 8, dev));
  return gpx_fill_padded(ctx, *dev, host, n, np);
}
int gpx_upload(gpx_ctx* ctx, Scratch& sc, const double* host, int64_t count, double** dev) {
  *dev = nullptr;
  if (!host) return 0;
  GPX_TRY(sc.get(count * 8, dev));
  GPX_HIP(hipMemcpyAsync(*dev, host, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

int gpx_model_or_prior(const gpx_mat* L, const gpx_mat* X, const double* alpha, const char* msg, bool* prior) {
  *prior = !L && !X && !alpha;
  GPX_ARG(*prior || (L && X && alpha), msg);
  return 0;
}

int gpx_posterior_chunk(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* Zc, int64_t mc,
                        double* B, double* Wout, const double* alpha_dev, double* mean_dev, double* mean_host, double* ssq,
                        double* kd, double* part) {
  const int64_t n = L->rows, np = L->prows, mcp = gpx_round_up(mc, GPX_TILE), ldb = gpx_skew_ld(mcp);
  GPX_TRY(launch_kfill(ctx, kp, X->p, n, Zc, mc, 0, nullptr, 0, 0.0, B, np, mcp, ldb));
  if (alpha_dev) {
    GPX_TRY(launch_colreduce(ctx, B, ldb, n, mcp, alpha_dev, mean_dev, part));
    if (mean_host) GPX_HIP(hipMemcpyAsync(mean_host, mean_dev, (size_t)mc * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (!ssq) return 0;
  GPX_TRY(chol_cross_solve(ctx, L, B, ldb, Wout, ldb, mcp));
  GPX_TRY(launch_colreduce(ctx, Wout ? Wout : B, ldb, n, mcp, nullptr, ssq, part));
  return launch_kdiag(ctx, kp, Zc, mc, kd);
}

extern "C" {

int gpx_potrf_policy(gpx_ctx* ctx, double piv_min, int skip) {
  GPX_ARG(ctx != nullptr && piv_min >= 0.0, "bad pivot policy");
  ctx->piv_min = piv_min;
  ctx->piv_skip = skip ? 1 : 0;
  return 0;
}

int gpx_potrf_dropped(gpx_ctx* ctx, int* count) {
  GPX_ARG(ctx && count, "NULL argument");
  GPX_HIP(hipMemcpyAsync(count, ctx->d_info + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// the assembly and factorisation behind gpx_refit_rows, into the fresh matrix K; every stream it used is drained by the caller
static int refit_rows_into(gpx_ctx* ctx, const KParams& kp, const gpx_mat* X, const double* nugget, int64_t nugget_len,
                           const gpx_mat* Lold, int64_t keep, gpx_mat* K) {
  const int64_t n = X->rows, np = K->prows;
  Scratch sc(ctx);
  double* d_nug = nullptr;
  K->aux_bytes = np * GPX_TILE * 8;
  void* pa;
  GPX_TRY(gpx_dev_alloc(ctx, K->aux_bytes, &pa));
  K->aux = (double*)pa;
  // the kept rows are COPIED (device state is immutable once built: shallow copies of a GP share handles), but nothing below
  // reads the copy -- the strip solve works against the old factor, the new rows are factored on their own -- so it runs on the
  // low-priority side stream underneath (HBM-bound beside MFMA-bound work: 0.59 ms off the 4.7 at N = 16384) and is joined
  // before the result is handed out
  hipStream_t Mst = ctx->stream, Cst = ctx->streams[4];
  bool side = keep > 0 && Mst == ctx->streams[0] && Cst != Mst;
  if (side && !ctx->ev_side && hipEventCreateWithFlags(&ctx->ev_side, hipEventDisableTiming) != hipSuccess) side = false;
  if (keep > 0) {
    // (the lower triangle only, to the 512-column boundary above the diagonal -- every diagonal tile whole: nothing reads a
    // factor's blocks above those; a full factorisation leaves the assembled K there, this one whatever the pool handed out)
    if (side) {
      GPX_HIP(hipEventRecord(ctx->ev_side, Mst));
      GPX_HIP(hipStreamWaitEvent(Cst, ctx->ev_side, 0));
    }
    StreamScope copy_stream(ctx, side ? Cst : Mst);
    GPX_TRY(gpx_copy2d_lower(ctx, Lold->p, Lold->ld, K->p, K->ld, keep));
    if (hipMemcpyAsync(K->aux, Lold->aux, (size_t)keep * GPX_TILE * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
      gpx_set_error("refit_rows: copy of the leaf inverses failed");
      return -2;
    }
    if (side) GPX_HIP(hipEventRecord(ctx->ev_side, Cst));
  }
  double nscal = 0.0;
  if (nugget_len == 1) nscal = nugget[0];
  if (nugget_len > 1) {
    GPX_TRY(sc.get(nugget_len * 8, &d_nug));
    if (hipMemcpyAsync(d_nug, nugget, (size_t)nugget_len * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      gpx_set_error("refit_rows: nugget upload failed");
      return -2;
    }
  }
  GPX_HIP(hipMemsetAsync(ctx->d_info, 0, 2 * sizeof(int), ctx->stream));
  const int64_t n2 = np - keep;
  if (n2 > 0) {
    double* A21 = K->p + keep * K->ld;
    GPX_TRY(launch_kfill_rows(ctx, kp, X->p, n, keep, d_nug, nugget_len, nscal, A21, n2, np, K->ld));
    if (keep > 0) {
      // The strip solve A21 <- A21 L11^-T has few rows (one batch of design points): through the leaf recursion its products
      // have K = 128..512 on a handful of tiles (20 TF/s at N = 16384, 512 changed rows).  Large factors: through the old
      // factor's explicit 1024-order block inverses (every product K >= 1024, 64-tiles), and the small trailing SYRK -- K = keep
      // on n2^2 / 64^2 tiles, a serial k loop in a few dozen workgroups -- split over K into 1024-wide batches whose partial
      // products are then subtracted in a fixed order.
      const int64_t kc = 1024;
      const bool wide = keep >= 4096 && n2 <= 2048 && Lold->prows >= 2048;
      if (wide) {
        const int64_t ib = chol_binv_order(Lold->prows), nbat = keep / kc, rem = keep - nbat * kc;
        double *pT = nullptr, *pP = nullptr;
        const int64_t tcap = std::max<int64_t>(4 * n2 * ib, 2 * n2 * keep);   // (the solve runs its few-row products as slices)
        Scratch wide_sc(ctx);   // back to the pool before the factorisation of the new rows asks it for its own scratch
        GPX_TRY(wide_sc.get(tcap * 8, &pT));
        GPX_TRY(wide_sc.get(nbat * n2 * n2 * 8, &pP));
        GPX_TRY(chol_trsm_right_leading(ctx, const_cast<gpx_mat*>(Lold), keep, A21, K->ld, n2, pT, tcap));
        GPX_TRY(launch_gemm_batched(ctx, A21, K->ld, kc, A21, K->ld, kc, pP, n2, n2 * n2, n2, n2, kc, true, false, nbat));
        GPX_TRY(launch_sub_partials(ctx, (const double*)pP, nbat, n2, A21 + keep, K->ld));
        if (rem > 0)
          GPX_TRY(launch_gemm(ctx, A21 + nbat * kc, K->ld, A21 + nbat * kc, K->ld, A21 + keep, K->ld, n2, n2, rem, true, true, true));
      } else {
        // (against the OLD factor: the copy may still be in flight)
        GPX_TRY(chol_trsm_right(ctx, Lold->p, Lold->ld, Lold->aux, A21, K->ld, n2, keep));
        GPX_TRY(launch_gemm(ctx, A21, K->ld, A21, K->ld, A21 + keep, K->ld, n2, n2, keep, true, true, true));
      }
    }
    GPX_TRY(chol_potrf_nozero(ctx, A21 + keep, K->ld, n2, K->aux + (keep / GPX_TILE) * GPX_TILE * GPX_TILE, keep, n));
  }
  int info = 0;
  if (side) GPX_HIP(hipStreamWaitEvent(Mst, ctx->ev_side, 0));
  GPX_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  K->factored = (info == 0);
  if (info != 0) gpx_set_error("refit_rows: matrix is not positive definite (pivot %d <= 0)", info);
  return info;
}

// f2: refit when only the trailing points of the design changed.  The leading `keep` rows/columns of
// K(X)+nugget equal the matrix `Lold` factors, so its leading keep x keep factor block and leaf inverses are copied, the
// rows >= keep are assembled, and the factorisation is completed: A21 <- A21 L11^-T, A22 <- A22 - A21 A21^T, potrf(A22).
// O(N^2 b) instead of O(N^3/3) for b new points.
int gpx_refit_rows(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const double* nugget,
                   int64_t nugget_len, const gpx_mat* Lold, int64_t keep, gpx_mat** outL) {
  GPX_ARG(ctx && X && outL, "NULL argument");
  KParams kp;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  GPX_ARG(X->cols == d && X->pcols == d, "X must be an unpadded (N x d) point set");
  const int64_t n = X->rows;
  GPX_ARG(nugget_len == 0 || nugget_len == 1 || nugget_len == n, "nugget_len must be 0, 1 or N");
  GPX_ARG(nugget_len == 0 || nugget != nullptr, "nugget is NULL");
  GPX_ARG(keep >= 0 && keep % GPX_TILE == 0, "keep must be a non-negative multiple of 128");
  if (keep > 0) {
    GPX_TRY(need_factor(Lold));
    GPX_ARG(keep <= Lold->rows && keep <= n, "keep exceeds the old factor or the new point set");
  }
  GPX_TRY(gpx_kparams_sets(ctx, &kp, X));
  MatHold K(ctx);
  GPX_TRY(gpx_mat_new(ctx, n, n, 1, K.put()));
  // a status, not an early return: both streams are drained on EVERY exit before K is freed or handed out
  const int r = refit_rows_into(ctx, kp, X, nugget, nugget_len, Lold, keep, K.get());
  (void)hipStreamSynchronize(ctx->stream);
  //  an error between the fork and the join leaves the copy of the kept rows in flight on the side stream: it writes K
  // and reads Lold -- both may be freed right after this returns
  if (ctx->ev_side && ctx->streams[4] != ctx->stream) (void)hipStreamSynchronize(ctx->streams[4]);
  if (r != 0) return r;
  *outL = K.release();
  return 0;
}

int gpx_potrs(gpx_ctx* ctx, const gpx_mat* L, const double* y, double* alpha) {
  GPX_ARG(ctx && y && alpha, "NULL argument");
  GPX_TRY(need_factor(L));
  const int64_t n = L->rows, np = L->prows;
  const int64_t sb = chol_potrs_scratch_bytes(np);
  Scratch sc(ctx);   // (its scope exit completes the copy of alpha)
  double *dv, *ps;
  GPX_TRY(gpx_upload_padded(ctx, sc, y, n, np, &dv));
  GPX_TRY(sc.get(sb, &ps));
  GPX_TRY(chol_potrs(ctx, const_cast<gpx_mat*>(L), dv, ps));  // caches the block inverses in L
  GPX_HIP(hipMemcpyAsync(alpha, dv, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// device-vector form, asynchronous on the selected stream: alpha (>= padded N doubles) <- K^-1 y
int gpx_potrs_dev(gpx_ctx* ctx, const gpx_mat* L, const gpx_mat* y, gpx_mat* alpha) {
  GPX_ARG(ctx && y && alpha, "NULL argument");
  GPX_TRY(need_factor(L));
  const int64_t np = L->prows;
  GPX_ARG(y->bytes >= np * 8 && alpha->bytes >= np * 8, "y / alpha must hold the padded length (zero padded)");
  const int64_t need = chol_potrs_scratch_bytes(np);
  if (ctx->trsv_scratch_bytes < need) {
    GPX_HIP(hipDeviceSynchronize());  // the old scratch may still be in use on another stream
    if (ctx->trsv_scratch) (void)hipFree(ctx->trsv_scratch);
    ctx->trsv_scratch = nullptr;
    ctx->trsv_scratch_bytes = 0;
    GPX_HIP(hipMalloc((void**)&ctx->trsv_scratch, (size_t)need));
    ctx->trsv_scratch_bytes = need;
  }
  if (alpha->p != y->p)
    GPX_HIP(hipMemcpyAsync(alpha->p, y->p, (size_t)np * 8, hipMemcpyDeviceToDevice, ctx->stream));
  return chol_potrs(ctx, const_cast<gpx_mat*>(L), alpha->p, ctx->trsv_scratch);
}

int gpx_logdet(gpx_ctx* ctx, const gpx_mat* L, double* out) {
  GPX_ARG(ctx && out, "NULL argument");
  GPX_TRY(need_factor(L));
  GPX_TRY(launch_logdet(ctx, L->p, L->ld, L->rows, ctx->d_scal));
  GPX_HIP(hipMemcpyAsync(out, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---- posterior / IVAR ---------------------------------------------------------------------------------
// mean of v[0 .. count) by halving: v[i] += v[i + h], h = ceil(m / 2), m <- h -- the summation ORDER of the host routine this
// replaces (pairwise_mean), so results do not depend on where the reduction runs or on the chunking.  One workgroup (the
// levels are separated by workgroup barriers; 32768 values: 15 levels, ~20 us); v is consumed.
__global__ __launch_bounds__(1024) static void pairwise_mean_kernel(double* __restrict__ v, int64_t count,
                                                                     double* __restrict__ out) {
  int64_t m = count;
  while (m > 1) {
    const int64_t h = (m + 1) / 2;
    for (int64_t i = threadIdx.x; i + h < m; i += 1024) v[i] += v[i + h];
    __syncthreads();
    m = h;
  }
  if (threadIdx.x == 0) out[0] = v[0] / (double)count;
}

// the posterior-shaped passes' use of the budget rule: the (N x Mc) cross matrix under ~16 GiB
int64_t gpx_eval_chunk(int64_t np) { return gpx_chunk_len((int64_t)16 << 30, np * 8); }

// Shared body; mean/var are host arrays of length M (nullable).  For every chunk of Z: B = K(X, Zc) (N x chunk),
// mean = B^T alpha (column dots), W = L^-1 B (recursive LEFT triangular solve: NN updates B2 -= L21 W1), var = k(z,z) -
// colsum(W^2).  Layout measured both ways at C4 after the GEMM schedule change: this N x M form (NN GEMMs, 74 TF/s on
// large launches) 494.6 ms; the transposed M x N form (right solve, NT GEMMs, 72.9 TF/s) 513.8 ms.
// var_dev (device, M doubles, nullable): receives the variances when the caller reduces them on the device (IVAR) -- then
// nothing of length M crosses PCIe.
static int posterior_impl(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
                          const gpx_mat* Z, double* mean, double* var_host, double* var_dev = nullptr,
                          gpx_mat** keepW = nullptr) {
  const int64_t n = L->rows, np = L->prows, M = Z->rows, d = kp.d;
  const bool var = var_host != nullptr || var_dev != nullptr;
  if (keepW) *keepW = nullptr;
  if (M == 0) return 0;
  const ChunkRange cr(M, gpx_eval_chunk(np));
  PosteriorWork w(np, cr.mc_alloc, var);
  // keepW: the solved W = L^-1 K(X, Z) stays, as a matrix of its own, for the cost's gradient at the same design
  // (gpx_ivar_grad_w) -- when all of Z is one chunk; it then IS the buffer the solution lands in.  The caller's on success only.
  MatHold Wm(ctx);
  Scratch sc(ctx);   // its scope exit is the synchronisation the host results wait for
  // all M variances, device (when the caller did not bring its own)
  if (var && !var_dev) GPX_TRY(sc.get(M * 8, &var_dev));
  if (keepW && var && cr.single() && gpx_mat_new(ctx, n, M, 1, Wm.put()) == 0 &&
      (Wm->prows != np || Wm->ld != gpx_skew_ld(cr.mc_alloc) || Wm->bytes < w.bytesB))
    Wm.reset();
  // (the kept matrix's buffer serves as B or W; it belongs to the gpx_mat and never goes through the scratch owner)
  if (Wm.get()) (w.oop() ? w.W : w.B) = Wm->p;
  GPX_TRY(w.take(sc, mean != nullptr, false));
  if (mean) GPX_TRY(w.upload_alpha(ctx, alpha, n));
  for (const ChunkRange::Step c : cr) {
    GPX_TRY(w.run(ctx, kp, L, X, Z->p + c.j0 * d, c.mc, mean ? mean + c.j0 : nullptr));
    if (var) GPX_TRY(launch_vec_sub(ctx, w.kd, w.ssq, c.mc, var_dev + c.j0));
  }
  if (var_host) GPX_HIP(hipMemcpyAsync(var_host, var_dev, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (keepW) *keepW = Wm.release();
  return 0;
}

int gpx_posterior(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                  const double* alpha, const gpx_mat* Z, double* mean, double* var) {
  GPX_ARG(ctx && X && Z, "NULL argument");
  GPX_ARG(mean == nullptr || alpha != nullptr, "alpha is required for the mean");
  KParams kp;
  GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Z, nullptr, "point sets must be unpadded (n x d)", &kp));
  return posterior_impl(ctx, kp, L, X, alpha, Z, mean, var);
}

// fixed-order pairwise sum / M (deterministic, independent of chunking)
static double pairwise_mean(std::vector<double>& v, int64_t count) {
  int64_t m = count;
  while (m > 1) {
    int64_t h = (m + 1) / 2;
    for (int64_t i = 0; i + h < m; ++i) v[(size_t)i] += v[(size_t)(i + h)];
    m = h;
  }
  return v[0] / (double)count;
}

static int ivar_impl(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const gpx_mat* Z, double* out, gpx_mat** W);

int gpx_ivar(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
             const gpx_mat* Z, double* out) {
  return ivar_impl(ctx, kind, d, hyp, nhyp, L, X, Z, out, nullptr);
}

int gpx_ivar_keep(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                  const gpx_mat* Z, double* out, gpx_mat** W) {
  GPX_ARG(W != nullptr, "W is NULL");
  return ivar_impl(ctx, kind, d, hyp, nhyp, L, X, Z, out, W);
}

static int ivar_impl(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const gpx_mat* Z, double* out, gpx_mat** W) {
  GPX_ARG(ctx && X && Z && out, "NULL argument");
  if (W) *W = nullptr;
  KParams kp;
  GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Z, nullptr, "point sets must be unpadded (n x d)", &kp));
  GPX_ARG(Z->rows > 0, "IVAR needs at least one integration point");
  MatHold Wm(ctx);   // the kept solve: the caller's only when the cost is on its way
  Scratch sc(ctx);   // (its scope exit completes the copy of the cost)
  double* pv;
  GPX_TRY(sc.get(Z->rows * 8, &pv));
  GPX_TRY(posterior_impl(ctx, kp, L, X, nullptr, Z, nullptr, nullptr, pv, W ? Wm.put() : nullptr));
  hipLaunchKernelGGL(pairwise_mean_kernel, dim3(1), dim3(1024), 0, ctx->stream, pv, Z->rows, ctx->d_scal);
  GPX_HIP(hipMemcpyAsync(out, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (W) *W = Wm.release();
  return 0;
}

// The cost again after a refit that KEPT the leading `keep` rows of the factor (gpx_refit_rows): W = L^-1 K(X, Z) of the previous
// design is at hand (gpx_ivar_keep), and its leading rows are those of the new W -- forward substitution never looks ahead.  Only
// the rows from `keep` on are re-assembled and re-solved, in place:  W2 <- L22^-1 (K(X2, Z) - L21 W1)  -- 2 (N - keep) keep M flops
// instead of N^2 M -- and the cost is one pass over W (design state across optimiser iterations; the batch loop
// of experimentalDesign.py:694-751 pins the earlier points and moves the last batch only).
int gpx_ivar_update(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                    const gpx_mat* Z, gpx_mat* W, int64_t keep, double* out) {
  GPX_ARG(ctx && X && Z && W && out, "NULL argument");
  GPX_TRY(need_factor(L));
  GPX_ARG(ctx->live_mats.count(W), "ivar_update: W is not a live matrix of this context");
  const int64_t n = L->rows, np = L->prows, M = Z->rows, mcp = gpx_round_up(M, GPX_TILE);
  GPX_ARG(X->rows == n && M > 0, "X does not match the factor / no integration points");   // (this entry's own wording)
  KParams kp;
  GPX_TRY(gpx_entry_args(ctx, kind, d, hyp, nhyp, L, X, Z, nullptr, "point sets must be unpadded (n x d)", &kp));
  GPX_ARG(W->rows == n && W->cols == M && W->prows == np && W->pcols == mcp, "ivar_update: W has another shape");
  GPX_ARG(keep > 0 && keep < np && keep % GPX_TILE == 0, "ivar_update: keep must be a positive multiple of 128 below the padded order");
  const int64_t n2 = n - keep, n2p = np - keep, ldw = W->ld;
  const int64_t bytes_out = mcp * 8, bytes_part = colreduce_partial_elems(np, mcp) * 8 + 8;
  Scratch sc(ctx);   // (its scope exit completes the copy of the cost)
  double *pout = nullptr, *pkd = nullptr, *ppart = nullptr, *pv = nullptr;
  GPX_TRY(sc.get(bytes_out, &pout));
  GPX_TRY(sc.get(bytes_out, &pkd));
  GPX_TRY(sc.get(bytes_part, &ppart));
  GPX_TRY(sc.get(M * 8, &pv));
  double* W2 = W->p + keep * ldw;
  GPX_TRY(launch_kfill(ctx, kp, X->p + keep * d, n2, Z->p, M, 0, nullptr, 0, 0.0, W2, n2p, mcp, ldw));
  GPX_TRY(launch_gemm(ctx, L->p + keep * L->ld, L->ld, W->p, ldw, W2, ldw, n2p, mcp, keep, false, true, false));
  GPX_TRY(chol_trsm_left(ctx, L->p + keep * (L->ld + 1), L->ld, L->aux + (keep / GPX_TILE) * GPX_TILE * GPX_TILE, W2, ldw, n2p, mcp));
  GPX_TRY(launch_colreduce(ctx, W->p, ldw, n, mcp, nullptr, pout, ppart));
  GPX_TRY(launch_kdiag(ctx, kp, Z->p, M, pkd));
  GPX_TRY(launch_vec_sub(ctx, pkd, pout, M, pv));
  hipLaunchKernelGGL(pairwise_mean_kernel, dim3(1), dim3(1024), 0, ctx->stream, pv, M, ctx->d_scal);
  GPX_HIP(hipMemcpyAsync(out, ctx->d_scal, 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// GP fit + IVAR in one call: K holds the assembled covariance and is factored in place exactly as gpx_potrf does; *out =
// (1/M) sum_j var_j exactly as gpx_ivar computes it on the finished factor.  Returns the pivot status of gpx_potrf.
// (Rounds 2-5 could run the evaluation solve STREAMED underneath the factorisation, panel by panel on a low-priority stream:
// measured 720-739 ms per C4 step against 710 for factor-then-solve -- two chip-filling GEMM streams share the CUs at a loss and
// the diagonal chain starves behind the solve's long workgroups -- and removed in round 6; the idea lives on where it pays, in
// the multi-GPU panel loop of gpexp_amd/dist.py.)
int gpx_fit_ivar(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, gpx_mat* K, const gpx_mat* X, const gpx_mat* Z,
                 double* out) {
  GPX_ARG(ctx && K && X && Z && out, "NULL argument");
  KParams kp;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  GPX_ARG(X->cols == d && X->pcols == d && Z->cols == d && Z->pcols == d, "point sets must be unpadded (n x d)");
  GPX_ARG(K->rows == X->rows && Z->rows > 0, "K does not match X / IVAR needs at least one integration point");
  GPX_ARG(ctx->stream == ctx->streams[0], "gpx_fit_ivar runs from the main stream");
  GPX_TRY(gpx_kparams_sets(ctx, &kp, X, Z));
  const int64_t M = Z->rows;
  PotrfJob J;
  GPX_TRY(potrf_begin(ctx, K, &J));
  int info = potrf_end(ctx, K, &J);
  if (info != 0) return info;
  std::vector<double> var((size_t)M);
  GPX_TRY(posterior_impl(ctx, kp, K, X, nullptr, Z, nullptr, var.data()));
  *out = pairwise_mean(var, M);
  return 0;
}

// out[j] = sum_{i < rows} B[i][j]^2 for the logical columns of B (host out[B->cols]); deterministic
int gpx_col_sumsq(gpx_ctx* ctx, const gpx_mat* B, int64_t rows, double* out) {
  GPX_ARG(ctx && B && out && rows >= 0 && rows <= B->prows, "bad arguments");
  Scratch sc(ctx);   // (its scope exit completes the copy)
  double *po, *pp;
  GPX_TRY(sc.get(B->pcols * 8, &po));
  GPX_TRY(sc.get(colreduce_partial_elems(B->prows, B->pcols) * 8 + 8, &pp));
  GPX_TRY(launch_colreduce(ctx, B->p, B->ld, rows, B->pcols, nullptr, po, pp));
  GPX_HIP(hipMemcpyAsync(out, po, (size_t)B->cols * 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// out[rows] = A v (host vectors; v has A->cols entries): a deterministic row reduction over the resident matrix
int gpx_matvec(gpx_ctx* ctx, const gpx_mat* A, const double* v, double* out) {
  GPX_ARG(ctx && A && v && out, "NULL argument");
  GPX_ARG(A->pcols % 2 == 0 && A->ld % 2 == 0, "matvec needs an even padded width");
  Scratch sc(ctx);   // (its scope exit completes the copy)
  double *pv, *po;
  GPX_TRY(gpx_upload_padded(ctx, sc, v, A->cols, A->pcols, &pv));
  GPX_TRY(sc.get((A->rows > 0 ? A->rows : 1) * 8, &po));
  GPX_TRY(launch_rowreduce(ctx, A->p, A->ld, A->rows, A->pcols, pv, po));
  GPX_HIP(hipMemcpyAsync(out, po, (size_t)A->rows * 8, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// ---- measurement ---------------------------------------------------------------------------------------
int gpx_profile_enable(gpx_ctx* ctx, int on) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  if (!on) GPX_TRY(gpx_prof_flush(ctx));
  ctx->prof_on = on ? 1 : 0;
  return 0;
}

int gpx_profile_reset(gpx_ctx* ctx) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  GPX_TRY(gpx_prof_flush(ctx));
  for (int i = 0; i < GPX_PROF_NCLASS; ++i) {
    ctx->prof_launches[i] = 0;
    ctx->prof_ms[i] = ctx->prof_flops[i] = ctx->prof_bytes[i] = 0.0;
  }
  return 0;
}

int gpx_profile_get(gpx_ctx* ctx, int cls, int64_t* launches, double* ms, double* flops, double* bytes) {
  GPX_ARG(ctx != nullptr, "ctx is NULL");
  GPX_ARG(cls >= 0 && cls < GPX_PROF_NCLASS, "unknown profile class");
  GPX_TRY(gpx_prof_flush(ctx));
  if (launches) *launches = ctx->prof_launches[cls];
  if (ms) *ms = ctx->prof_ms[cls];
  if (flops) *flops = ctx->prof_flops[cls];
  if (bytes) *bytes = ctx->prof_bytes[cls];
  return 0;
}

// ---- test hooks ------------------------------------------------------------------------------------------
// the triangular-operand modes of the GEMM (launch_gemm_tri): tri = 1 / 2 / 3, see gemm_f64.hip
int gpx_dbg_gemm_tri(gpx_ctx* ctx, const gpx_mat* A, const gpx_mat* B, gpx_mat* C, int bt, int accumulate, int tri) {
  GPX_ARG(ctx && A && B && C, "NULL argument");
  const int64_t m = C->prows, n = C->pcols, k = A->pcols;
  GPX_ARG(A->prows == m, "A rows");
  GPX_ARG(bt ? (B->prows == n && B->pcols == k) : (B->prows == k && B->pcols == n), "B shape");
  GPX_TRY(launch_gemm_tri(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, bt != 0, accumulate != 0, tri == 3, tri));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_dbg_kfill_plan(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* Z,
                       int* exact, double* center) {
  GPX_ARG(ctx && X && exact && center, "NULL argument");
  KParams kp;
  GPX_TRY(gpx_make_kparams(kind, d, hyp, nhyp, &kp));
  GPX_TRY(gpx_kparams_sets(ctx, &kp, X, Z));
  *exact = kp.exact;
  for (int k = 0; k < d; ++k) center[k] = kp.center[k];
  return 0;
}

int gpx_dbg_gemm_ksplit(gpx_ctx* ctx, const gpx_mat* A, const gpx_mat* B, gpx_mat* C, int mode, int parts) {
  GPX_ARG(ctx && A && B && C && mode >= 0 && mode <= 3 && parts > 0, "bad argument");
  const int64_t m = C->prows, n = C->pcols, k = A->pcols;
  GPX_ARG(A->prows == m && B->prows == n && B->pcols == k, "operand shapes");
  Scratch sc(ctx);
  double* P;
  GPX_TRY(sc.get((int64_t)parts * m * n * 8, &P));
  return mode <= 1 ? launch_gemm_ksplit(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, mode == 1, parts, P)
                   : launch_gemm_ksplit_small(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, mode == 3, parts, P);
}

int gpx_dbg_gemm(gpx_ctx* ctx, const gpx_mat* A, const gpx_mat* B, gpx_mat* C, int bt, int accumulate, int lower) {
  GPX_ARG(ctx && A && B && C, "NULL argument");
  const int64_t m = C->prows, n = C->pcols, k = A->pcols;
  GPX_ARG(A->prows == m, "A rows");
  GPX_ARG(bt ? (B->prows == n && B->pcols == k) : (B->prows == k && B->pcols == n), "B shape");
  GPX_TRY(launch_gemm(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, bt != 0, accumulate != 0,
                      lower != 0));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_dbg_gemm_strassen(gpx_ctx* ctx, const gpx_mat* A, const gpx_mat* B, gpx_mat* C) {
  GPX_ARG(ctx && A && B && C, "NULL argument");
  const int64_t m = C->prows, n = C->pcols, k = A->pcols;
  GPX_ARG(A->prows == m && B->prows == k && B->pcols == n, "operand shapes");
  GPX_TRY(launch_gemm_strassen(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, 1, nullptr, 0));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpx_dbg_gemm_strassen_depth(gpx_ctx* ctx, const gpx_mat* A, const gpx_mat* B, gpx_mat* C, int depth) {
  GPX_ARG(ctx && A && B && C, "NULL argument");
  GPX_ARG(depth >= 0 && depth <= GPX_STRASSEN_MAX_DEPTH, "strassen: depth out of range");
  const int64_t m = C->prows, n = C->pcols, k = A->pcols;
  GPX_ARG(A->prows == m && B->prows == k && B->pcols == n, "operand shapes");
  GPX_TRY(launch_gemm_strassen(ctx, A->p, A->ld, B->p, B->ld, C->p, C->ld, m, n, k, depth, nullptr, 0));
  GPX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
