// Internal declarations shared by the HIP translation units of libgpx_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <unordered_set>
#include "../../include/gpx.h"
#include "../../include/gpx_dist.h"
#include "../../include/gpx_debug.h"

#define GPX_TILE 128          // padding / GEMM tile / Cholesky leaf size
#define GPX_MAXD GPX_MAX_DIM
#define GPX_NSTREAMS 6
#define GPX_SEG_MAX 8         // panels one trailing update of the 2-D distributed factorisation can apply at once
#ifndef GPX_G_SKEW
#define GPX_G_SKEW 0          // doubles added to the row stride of the packed panel pieces of the 2-D distributed loop (see gpx_g_ld)
#endif
#define GPX_MAX_PR 4          // process rows of the 2-D grid the segmented update supports (grids up to 4 x Pc)

// ---- error plumbing ---------------------------------------------------------------------------
void gpx_set_error(const char* fmt, ...);
#define GPX_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      gpx_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return -2;                                                                        \
    }                                                                                   \
  } while (0)
#define GPX_ARG(cond, msg)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      gpx_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, msg); \
      return -1;                                             \
    }                                                        \
  } while (0)
#define GPX_TRY(call)        \
  do {                       \
    int r_ = (call);         \
    if (r_ != 0) return r_;  \
  } while (0)

static inline int64_t gpx_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// Leading dimension for a padded row of `cols` doubles: one extra 128-byte line per row when the row stride would
// be a large power of two (N = 32768 -> 256 KiB).  Measured NEUTRAL on MI355X (GEMM 66.98 vs 66.97 TF/s: the L2 /
// channel address hashing already spreads such strides); kept because it decouples ld from the padded width.
static inline int64_t gpx_skew_ld(int64_t cols) { return (cols >= 1024 && cols % 256 == 0) ? cols + 16 : cols; }

// Row stride of the rows region of a packed panel piece (dist.hip): nb + GPX_G_SKEW doubles.  At nb = 512 a stride of nb is
// exactly 4 KiB, the textbook channel-conflict stride; measured on MI355X it makes NO difference (66.0 TF/s with skew 0, 65.9
// with 16: scripts/probe_update_multi.py -- like gpx_skew_ld, the address hashing already spreads it), so the skew is 0 and the
// pieces travel without 3 % of padding.  The stride stays a separate quantity (gpexp_amd/dist.py Grid2D.gld mirrors it).
static inline int64_t gpx_g_ld(int64_t nb) { return nb + GPX_G_SKEW; }

// ---- covariance-function parameters, passed to kernels by value ---------------------------------
// Coordinates are pre-multiplied by `scale` when staged into LDS so that
//   SE       : k = sig * exp(-0.5 * |a-b|^2)            scale_k = 1/cl_k          (kernels.py:121-122)
//   Matern32 : t = |a-b|, k = sig*(1+t)*exp(-t)          scale   = sqrt(3)/rho     (kernels.py:87-89)
//   Matern52 : t = |a-b|, k = sig*(1+t+t^2/3)*exp(-t)    scale   = sqrt(5)/rho     (not in reference)
//   Mehler   : k = sig * exp(-sum_k c1_k (a^2+b^2) - c2_k a b), sig = prod (1-t^2)^-1/2,
//              c1_k = t^2/(2(1-t^2)), c2_k = t/(1-t^2), scale = 1               (kernels.py:282-285)
//
// Stationary kernels are translation invariant, and the tiled assembly forms |a-b|^2 from the EXPANDED product
// |a|^2 + |b|^2 - 2 a.b on the MFMA pipe, whose absolute error grows like eps * (|a|^2 + |b|^2) * scale^2 -- the reference
// subtracts coordinates first (kernels.py:121-122, 87-89).  Two measures keep the assembly at the reference's accuracy
// for any input placement (gpx_kparams_sets):
//   center  the midpoint of the point sets' bounding box is subtracted from every coordinate before scaling, so the
//           expanded form only ever sees offsets of the size of the domain, not of its distance from the origin;
//   exact   when even the centred, scaled domain is wide (half-width / length scale large: S = sum_k scale_k^2 *
//           (hwA_k^2 + hwB_k^2) above GPX_EXACT_S / sensitivity), the fill forms (a_k - b_k) * scale_k directly from the
//           raw coordinates on the VALU instead -- the reference's own operation order, exact where Sterbenz applies.
// Mehler is not stationary: center = 0, exact = 0 (the reference expands its exponent the same way, kernels.py:282-285).
struct KParams {
  int kind;
  int d;
  double sig;
  double scale[GPX_MAXD];
  double c1[GPX_MAXD];
  double c2[GPX_MAXD];
  double center[GPX_MAXD];
  int exact;
};
int gpx_make_kparams(int kind, int d, const double* hyp, int nhyp, KParams* out);

// ---- objects --------------------------------------------------------------------------------------
struct gpx_mat {
  double* p;
  int64_t rows, cols;    // logical
  int64_t prows, pcols;  // padded shape
  int64_t ld;            // leading dimension >= pcols (skewed off powers of two, see gpx_skew_ld)
  int64_t bytes;
  double* aux;        // after gpx_potrf: inverses of the 128x128 diagonal blocks, (prows/128) x 128 x 128
  int64_t aux_bytes;
  int factored;
  // bounding box of a point set (cols <= GPX_MAXD), computed on the host at upload (gpx_mat_from_host) or on first use
  int bbox_ok;
  double lo[GPX_MAXD], hi[GPX_MAXD];
  int64_t bad_row, bad_col;  // first non-finite coordinate seen by that scan, -1 = none (valid while bbox_ok)
  // explicit inverses of the IB x IB diagonal blocks of the factor (and their transposes), built on the first gpx_potrs
  // after a factorisation (chol_potrs): ceil(prows / IB) blocks of IB x IB each, twice
  double* binv;
  int64_t binv_bytes;
  int64_t binv_ib;
  // block-cyclic LOCAL matrix of the 2-D distributed factorisation: explicit inverses of the diagonal blocks this rank owns
  // (slot = local block row), kept from the panel solves for the distributed substitution (gpx_dist2_trsv_diag):
  // per slot [inverse | its transpose], dinv_nb x dinv_nb doubles each; dinv_ok[slot] = the slot holds the inverse of the
  // CURRENT factor's block
  double* dinv;
  int64_t dinv_bytes;
  int64_t dinv_nb;
  std::vector<unsigned char> dinv_ok;
};

struct ProfRec {
  hipEvent_t a, b;
  int cls;
  hipStream_t stream;
  bool open;
};

struct gpx_ctx {
  int device;
  hipStream_t stream;        // currently selected stream (all launches go here)
  hipStream_t streams[GPX_NSTREAMS];  // 0 = main, 1 = panel (high priority), 2 = communication (high priority),
                             // 4 = evaluation (low priority, unmasked): the streamed IVAR solve beside the factorisation,
                             // 3 = background, 5 = bulk: CU-masked (leave 4 CUs per XCD to the other streams) when the runtime allows
  std::vector<hipEvent_t> sync_events;  // gpx_event_record / gpx_event_wait ids
  std::unordered_set<const gpx_mat*> live_mats;  // every matrix this context handed out and has not freed (gpx_program_run checks its rows against it)
  // work buffers of a blocked factorisation in flight (set by gpx_potrf around chol_potrf, NULL otherwise): storage of the
  // explicit block inverses being built, order of those blocks, scratch for their build and for the panel solves
  double* pw_binv;
  int64_t pw_ib;
  double* pw_tmp_build;
  double* pw_tmp_T;
  int pw_done;   // set by the factorisation when it has built every block inverse into pw_binv
  std::vector<hipEvent_t> la_events;    // look-ahead factorisation (chol.hip): block row k+1 + next diagonal block ready / chain done
  hipEvent_t ev_side = nullptr;         // fork / join of gpx_refit_rows' copy of the kept rows on the low-priority stream
  int cus;
  // cached device allocations (exact-size reuse)
  std::multimap<int64_t, void*> pool;
  int64_t pool_bytes;
  int64_t out_bytes;   // handed out and not yet returned, in pool keys (gpx_dbg_pool_stats)
  // deferred release (gpx_mat_free): a freed matrix's buffers go back to the pool AT ONCE, tagged with a fence -- one event per
  // stream of the context, recorded at the time of the free; whoever takes such a block out of the pool waits for the fence
  // first (normally long complete).  Replaces a device-wide synchronisation per free.
  struct Fence {
    std::vector<hipEvent_t> evs;
  };
  std::map<void*, std::shared_ptr<Fence>> pending;
  std::vector<hipEvent_t> fence_free;
  // GPX_ALLOC_GUARD=1 (debug; there is no GPU address sanitizer on this pool): every pooled allocation gets a 4 KiB band of
  // 0xA5 on either side, checked when it goes back to the pool; violations are counted and reported on stderr
  int guard;
  int64_t guard_violations;
  // GPX_CHAOS=seed (debug): every profiled launch site holds its stream back by a random 0.1-3 ms with probability 1/4, so
  // that a missing dependency between the context's streams changes the results instead of hiding behind lucky timing
  uint64_t chaos;
  // scalars
  int* d_info;      // [0] first failing pivot (1-based), 0 = ok; [1] pivots dropped in skip mode
  double piv_min;   // pivot policy of the leaf factorisation (gpx_potrf_policy): pivots <= piv_min are bad ...
  int piv_skip;     // ... and reported (0) or dropped (1)
  double* d_scal;   // small scalar workspace (>= 64 doubles)
  double* trsv_scratch;      // grown on demand, kept until gpx_destroy (lets gpx_potrs_dev stay asynchronous)
  int64_t trsv_scratch_bytes;
  double* d2_scratch;        // 2-D distributed panel solve: explicit inverse of the current diagonal block + build scratch
  int64_t d2_scratch_bytes;  // (2 nb^2 doubles; used on the PANEL stream only, in step order)
  long long* dbg_stamps;     // gpx_dbg_stamp / gpx_dbg_spin_until: wall-clock stamps taken on a stream (GPX_DBG_STAMPS slots)
  const double* d2_inv_src;  // the packed diagonal block whose inverse d2_scratch holds (gpx_dist2_panel_inv), or NULL
  int64_t d2_inv_nb;
  double* ev_scratch;        // streamed evaluation (gpx_dist_ivar_group_at): block inverses of the group + their build scratch +
  int64_t ev_scratch_bytes;  // the solved block rows W (w x m); used on ONE stream only, in group order
  // multi-GPU (RCCL communicator, opaque here; see dist.hip)
  void* comm;
  int rank, world;
  // process grid of the 2-D block-cyclic path (gpx_comm_grid): rank = pr * Pc + pc; sub-communicators from ncclCommSplit:
  // grp[0] = world (== comm), grp[1] = my process row (Pc ranks, rank pc), grp[2] = my process column (Pr ranks, rank pr)
  void* grp[3];
  int grp_size[3], grp_rank[3];
  int Pr, Pc;
  // profiling
  int prof_on;
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_free;
  int64_t prof_launches[GPX_PROF_NCLASS];
  double prof_ms[GPX_PROF_NCLASS];
  double prof_flops[GPX_PROF_NCLASS];
  double prof_bytes[GPX_PROF_NCLASS];
};

// centre + exact-path decision for fills between the given point sets (any may be NULL); see KParams
int gpx_kparams_sets(gpx_ctx* ctx, KParams* kp, const gpx_mat* A, const gpx_mat* B = nullptr, const gpx_mat* C = nullptr);
// The prologue of the (kind, d, hyp, nhyp, L, X, Z) entry points (api.hip), after the caller's own NULL check of ctx, X, Z, C:
// the kernel parameters, a factor that gpx_potrf produced, unpadded point sets (Z, C nullable; a failure reads `points_msg`: the
// callers have two wordings), X of the factor's order, and -- for the callers that fill between point sets, i.e. pass a Z -- the
// centre / exact-path decision of gpx_kparams_sets(X, Z, C).
int gpx_entry_args(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                   const gpx_mat* Z, const gpx_mat* C, const char* points_msg, KParams* kp);
int gpx_dev_alloc(gpx_ctx* ctx, int64_t bytes, void** out);
template <typename T>
int gpx_dev_alloc(gpx_ctx* ctx, int64_t bytes, T** out) {   // typed form, for a field that keeps the block
  void* p = nullptr;
  const int r = gpx_dev_alloc(ctx, bytes, &p);
  if (r == 0) *out = (T*)p;
  return r;
}
void gpx_dev_release(gpx_ctx* ctx, void* p, int64_t bytes);
int gpx_mat_new(gpx_ctx* ctx, int64_t rows, int64_t cols, int pad, gpx_mat** out);

// The one owner of pooled scratch.  The pool is keyed by size and gpx_dev_release files a block under the byte count it is
// TOLD, so the count is recorded once, where the block is taken, and every block goes back under it on scope exit -- error
// paths included -- after the work queued on it has finished.  That wait is for the context's selected stream; Scratch::Device
// waits for the whole device (grad.hip, whose passes use several of the context's streams).  An owner that took nothing does
// not wait at all: that holds for EVERY user -- an early return before the first get() no longer synchronises the stream (what
// such a path frees goes through gpx_mat_free, which is fenced) -- and keeps gpx_kfill_into without a nugget vector asynchronous.
// Buffers that outlive the call (resident state, the fields of a gpx_mat) are never registered here.
class Scratch {
 public:
  enum Sync { Stream, Device };
  explicit Scratch(gpx_ctx* c, Sync s = Stream) : ctx(c), sync(s) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  template <typename T>
  int get(int64_t bytes, T** out) {
    void* p = nullptr;
    int r = gpx_dev_alloc(ctx, bytes, &p);
    if (r == 0) {
      adopt(p, bytes);
      *out = (T*)p;
    }
    return r;
  }
  // a block the caller took from gpx_dev_alloc itself, with the byte count it asked for (loo.hip's shrinking slab, which must
  // leave gpx_dev_alloc's own out-of-memory text in place while it retries)
  void adopt(void* p, int64_t bytes) { bufs.push_back({p, bytes}); }
  ~Scratch() {
    if (bufs.empty()) return;
    if (sync == Device) (void)hipDeviceSynchronize();
    else (void)hipStreamSynchronize(ctx->stream);
    for (auto& b : bufs) gpx_dev_release(ctx, b.first, b.second);
  }

 private:
  gpx_ctx* ctx;
  Sync sync;
  std::vector<std::pair<void*, int64_t>> bufs;
};

// Owner of an object created inside a call and handed to the caller only on success (a gpx_mat, the resident state of
// gpx_givar_begin / gpx_mi_begin / gpx_fitc_fit): unless released, FREE takes it back on scope exit.  Those free functions fence or
// synchronise themselves, so the holder does not.  Declared BEFORE the Scratch of the same function: scratch is then synchronised
// and released first.
template <class T, int (*FREE)(gpx_ctx*, T*)>
class Held {
 public:
  explicit Held(gpx_ctx* c, T* obj = nullptr) : ctx(c), p(obj) {}
  Held(const Held&) = delete;
  Held& operator=(const Held&) = delete;
  ~Held() { reset(); }
  T** put() { return &p; }   // for the out-parameter of the call that creates the object
  T* get() const { return p; }
  T* operator->() const { return p; }
  T* release() {
    T* r = p;
    p = nullptr;
    return r;
  }
  void reset() {
    if (p) (void)FREE(ctx, p);
    p = nullptr;
  }

 private:
  gpx_ctx* ctx;
  T* p;
};
using MatHold = Held<gpx_mat, gpx_mat_free>;

// ctx->stream switched to another stream of the context for a scope; the previous selection comes back on every exit
struct StreamScope {
  gpx_ctx* ctx;
  hipStream_t prev;
  StreamScope(gpx_ctx* c, hipStream_t s) : ctx(c), prev(c->stream) { c->stream = s; }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
  ~StreamScope() { ctx->stream = prev; }
};

// RAII-ish profiling bracket: records events around launches of one class when profiling is on
struct ProfScope {
  gpx_ctx* ctx;
  int idx;
  ProfScope(gpx_ctx* c, int cls, double flops, double bytes);
  ~ProfScope();
};
int gpx_prof_flush(gpx_ctx* ctx);

// d rounded up to the instantiated register-array sizes of the per-point kernels templated on the dimension (grad.hip, acq.hip):
// CALL(KIND, DMAX) for a kernel whose derivative is a radial factor times the coordinate difference (SE, Matern 3/2, Matern 5/2;
// radial_pair in gpx_device.h)
#define GPX_SE_DISPATCH(K_, d_, CALL)  \
  do {                                 \
    if ((d_) <= 1) { CALL(K_, 1); }    \
    else if ((d_) <= 2) { CALL(K_, 2); } \
    else if ((d_) <= 4) { CALL(K_, 4); } \
    else if ((d_) <= 8) { CALL(K_, 8); } \
    else if ((d_) <= 16) { CALL(K_, 16); } \
    else { CALL(K_, 32); }             \
  } while (0)
#define GPX_RADIAL_DISPATCH(kind_, d_, CALL)                                    \
  do {                                                                          \
    if ((kind_) == GPX_K_SE) GPX_SE_DISPATCH(GPX_K_SE, d_, CALL);               \
    else if ((kind_) == GPX_K_MATERN32) GPX_SE_DISPATCH(GPX_K_MATERN32, d_, CALL); \
    else GPX_SE_DISPATCH(GPX_K_MATERN52, d_, CALL);                             \
  } while (0)

// ---- chunking and scratch of the posterior-shaped passes ---------------------------------------------------------------------
// The ONE reader of GPX_CROSS_BYTES (api.hip): columns per chunk that keep `bytes_per_col` bytes a column under the budget -- the
// caller's default, or GPX_CROSS_BYTES -- rounded down to 128, 128 at least.  gpx_eval_chunk: the N x chunk cross matrix of the
// posterior-shaped passes (gpx_posterior, gpx_acq) under ~16 GiB.
int64_t gpx_chunk_len(int64_t default_budget, int64_t bytes_per_col);
extern "C" __attribute__((visibility("hidden"))) int64_t gpx_eval_chunk(int64_t np);
// M evaluation points in chunks of at most mcmax: for (const ChunkRange::Step c : cr) visits (j0, mc, mcp = mc padded to 128).
// widest / mc_alloc: the longest chunk and its padded length, which the per-call buffers are sized by.
struct ChunkRange {
  struct Step { int64_t j0, mc, mcp; };
  struct It {
    int64_t j0, M, mcmax;
    Step operator*() const { return {j0, M - j0 < mcmax ? M - j0 : mcmax, gpx_round_up(M - j0 < mcmax ? M - j0 : mcmax, GPX_TILE)}; }
    void operator++() { j0 += mcmax; }
    bool operator!=(const It&) const { return j0 < M; }
  };
  int64_t M, mcmax, widest, mc_alloc;
  ChunkRange(int64_t M_, int64_t c) : M(M_), mcmax(c), widest(M_ < c ? M_ : c), mc_alloc(gpx_round_up(widest, GPX_TILE)) {}
  It begin() const { return {0, M, mcmax}; }
  It end() const { return {M, M, mcmax}; }
  bool single() const { return M <= mcmax; }
  bool last(const Step& c) const { return c.j0 + mcmax >= M; }
};
// dev[0, n) = host[0, n), 0 up to np: the one memset-and-copy pair.  gpx_upload_padded takes the np doubles from sc first;
// gpx_upload (*dev = NULL for a NULL host) the unpadded form.
int gpx_fill_padded(gpx_ctx* ctx, double* dev, const double* host, int64_t n, int64_t np);
int gpx_upload_padded(gpx_ctx* ctx, Scratch& sc, const double* host, int64_t n, int64_t np, double** dev);
int gpx_upload(gpx_ctx* ctx, Scratch& sc, const double* host, int64_t count, double** dev);
// One chunk Zc (mc points) of those passes -- the ONE sequence behind gpx_posterior, gpx_ivar and gpx_acq, so that their values
// agree by construction (api.hip):
//   B = K(X, Zc) (np x mcp, row stride gpx_skew_ld(mcp));   mean_dev = B^T alpha_dev [-> mean_host, mc doubles];
//   W = L^-1 B in place (Wout == NULL) or through the block inverses into Wout (B is consumed);   ssq = colsum(W^2);   kd = k(z, z)
// alpha_dev == NULL: no mean.  ssq == NULL: the mean only.  mean_dev and ssq may be the same buffer (the copy is queued between
// them).  Asynchronous.
int gpx_posterior_chunk(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* Zc, int64_t mc,
                        double* B, double* Wout, const double* alpha_dev, double* mean_dev, double* mean_host, double* ssq,
                        double* kd, double* part);
// C (mp x mp, row stride ldc; mp = Z's rows padded to 128) = K(Z,Z) - W^T W with W = L^-1 K(X,Z): the posterior covariance of
// gpx_posterior_cov, through two np x mp blocks from sc (design.hip)
int posterior_cov_into(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const gpx_mat* Z, Scratch& sc, double* C,
                       int64_t ldc);
// "L, X and alpha are given together, or all three NULL": the rule of the sampler constructors; *prior = all three NULL
int gpx_model_or_prior(const gpx_mat* L, const gpx_mat* X, const double* alpha, const char* msg, bool* prior);

// ---- kernel launchers (all asynchronous on ctx->stream) ------------------------------------------
// kfill.hip
int launch_kfill(gpx_ctx* ctx, const KParams& kp, const double* A, int64_t na, const double* B, int64_t nb,
                 int symmetric, const double* d_nugget, int64_t nugget_len, double nugget_scalar,
                 double* out, int64_t prows, int64_t pcols, int64_t ld);
// symmetric sub-block K[off:, off:off+pcols] of the N x N covariance (rows/cols start at point index `off`)
int launch_kfill_offset(gpx_ctx* ctx, const KParams& kp, const double* X, int64_t n, int64_t row_off, int64_t col_off,
                        const double* d_nugget, int64_t nugget_len, double nugget_scalar, double* out, int64_t prows,
                        int64_t pcols, int64_t ld);
int launch_kdiag(gpx_ctx* ctx, const KParams& kp, const double* Z, int64_t m, double* out);
int launch_kfill_cyclic(gpx_ctx* ctx, const KParams& kp, const double* X, int64_t n, const double* d_nugget,
                        int64_t nugget_len, double nugget_scalar, double* out, int64_t prows, int64_t pcols, int64_t ld,
                        int64_t nb, int Pr, int pr, int Pc, int pc);
int gpx_copy2d(gpx_ctx* ctx, const double* src, int64_t lds_, double* dst, int64_t ldd, int64_t rows, int64_t cols);
int gpx_copy2d_lower(gpx_ctx* ctx, const double* src, int64_t lds_, double* dst, int64_t ldd, int64_t n);
int launch_kfill_rows(gpx_ctx* ctx, const KParams& kp, const double* X, int64_t n, int64_t row0, const double* d_nugget,
                      int64_t nugget_len, double nugget_scalar, double* out, int64_t prows_band, int64_t pcols,
                      int64_t ld);

// gemm_f64.hip:  C[m x n] = (accumulate ? C - A*op(B) : A*op(B)),  m,n multiples of 128, k multiple of 16
// Kernels of the latency-bound chains (the diagonal block's factorisation and inversion, the panel stream of the distributed
// loop) run BESIDE chip-filling updates and share their CUs with resident GEMM waves; launched on the context's chain stream
// (streams[1]) they raise their waves' issue priority (s_setprio 3) so that the CU's arbiter serves them first.
static inline int gpx_chain_prio(const gpx_ctx* ctx) { return ctx->stream == ctx->streams[1] ? 1 : 0; }
int launch_gemm(gpx_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                int64_t m, int64_t n, int64_t k, bool bt, bool accumulate, bool lower);

int launch_gemm_tri(gpx_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                    int64_t m, int64_t n, int64_t k, bool bt, bool accumulate, bool lower, int tri);
// C -= A B (NN) through up to `depth` levels of Strassen's scheme: 7 half-size products per level, operand sums in scratch
// (gemm_f64.hip).  depth levels need m, n multiples of 128 * 2^depth and k of 16 * 2^depth (gemm_strassen_scratch_bytes: 0 =
// refused); the driver runs the deepest level <= depth that the shape admits and scratch can be had for, down to launch_gemm.
// scratch may be NULL (pool + a stream synchronisation).
// (a product of the last level has up to 2^depth destinations: gemm_f64_multi_kernel is built for 2^GPX_STRASSEN_MAX_DEPTH.  Three
// levels in the top update at C4 were measured slower than two and than one, profiles/strassen2_ivar_ab.json.)
constexpr int GPX_STRASSEN_MAX_DEPTH = 2;
int64_t gemm_strassen_scratch_bytes(int64_t m, int64_t n, int64_t k, int depth);
int launch_gemm_strassen(gpx_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                         int64_t m, int64_t n, int64_t k, int depth, double* scratch, int64_t scratch_bytes);
int launch_gemm_ksplit(gpx_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                       int64_t m, int64_t n, int64_t k, bool lower, int64_t parts, double* P, bool assign = false);
int launch_gemm_ksplit_small(gpx_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                             int64_t m, int64_t n, int64_t k, bool assign, int64_t parts, double* P);
int launch_gemm_batched(gpx_ctx* ctx, const double* A, int64_t lda, int64_t sa, const double* B, int64_t ldb, int64_t sb,
                        double* C, int64_t ldc, int64_t sc, int64_t m, int64_t n, int64_t k, bool bt, bool accumulate,
                        int64_t batch);

int launch_dist2_update(gpx_ctx* ctx, double* C, int64_t ldc, int64_t lr0, int64_t m, int64_t lc0, int64_t n, int64_t nb, int Pr,
                        int Pc, int pr, int pc, int64_t piece_stride, int64_t dsz, int nseg, const double* const* g,
                        const int64_t* ks, int below_diag);

// chol.hip
int launch_leaf(gpx_ctx* ctx, double* A, int64_t ld, double* inv, int64_t base_index, int64_t n_valid);
int chol_potrf(gpx_ctx* ctx, double* A, int64_t ld, int64_t n, double* invd, int64_t n_valid);
// same without resetting the pivot flag; `base` = global index of A's first row (for the reported pivot)
int chol_potrf_nozero(gpx_ctx* ctx, double* A, int64_t ld, int64_t n, double* invd, int64_t base, int64_t n_valid);
// X <- X * L^-T (right, lower, transposed): X is m x n (ld ldx), L n x n lower with leaf inverses invd
int chol_trsm_right(gpx_ctx* ctx, const double* L, int64_t ldl, const double* invd, double* X, int64_t ldx,
                    int64_t m, int64_t n);
// X <- X * L^-1 (right, lower, not transposed)
int chol_trsm_right_n(gpx_ctx* ctx, const double* L, int64_t ldl, const double* invd, double* X, int64_t ldx,
                      int64_t m, int64_t n);
// B <- L^-1 B (left, lower): B is n x m
int chol_trsm_left(gpx_ctx* ctx, const double* L, int64_t ldl, const double* invd, double* B, int64_t ldb,
                   int64_t n, int64_t m);
int chol_trsv(gpx_ctx* ctx, const double* L, int64_t ld, const double* invd, double* y, int64_t n, bool transposed);
// bytes of scratch chol_trsv needs for the transposed sweep of order n
int64_t chol_trsv_scratch_bytes(int64_t n);
int chol_trsv_with_scratch(gpx_ctx* ctx, const double* L, int64_t ld, const double* invd, double* y, int64_t n,
                           bool transposed, double* scratch);
int launch_logdet(gpx_ctx* ctx, const double* L, int64_t ld, int64_t n, double* d_out);
// alpha = K^-1 y through explicit inverses of the diagonal blocks (built on first use, kept in L): v (padded n doubles) is
// overwritten by the solution; scratch >= chol_potrs_scratch_bytes(n).  Asynchronous on the selected stream.
int chol_trtri(gpx_ctx* ctx, const gpx_mat* L, double* Linv, double* tmp);  // Linv (n x n, ld n) = L^-1; tmp >= (n/2)^2
int chol_binv_ensure(gpx_ctx* ctx, gpx_mat* L);
int chol_trsm_right_trailing(gpx_ctx* ctx, gpx_mat* L, int64_t r0, double* X, int64_t ldx, int64_t m, int transposed, double* T);
int chol_trsm_right_leading(gpx_ctx* ctx, gpx_mat* L, int64_t ncols, double* X, int64_t ldx, int64_t m, double* T, int64_t tcap);
int chol_trsm_right_n_leading(gpx_ctx* ctx, gpx_mat* L, int64_t ncols, double* X, int64_t ldx, int64_t m, double* T);
int chol_block_inverse(gpx_ctx* ctx, const double* D, int64_t ldd, const double* invd, double* inv, int64_t w, double* tmp);
int64_t chol_binv_order(int64_t n);
int64_t chol_binv_elems(int64_t n);
int chol_binv_finish(gpx_ctx* ctx, gpx_mat* L, int64_t ib);  // explicit inverses of L's diagonal blocks (order <= 1024), cached in L
// W (n x m, separate buffer) = L^-1 B through the block inverses: B is consumed (its lower block rows are updated in place)
int chol_trsm_left_oop(gpx_ctx* ctx, gpx_mat* L, double* B, int64_t ldb, double* W, int64_t ldw, int64_t m);
// The cross-solve rule, in one place: a freshly filled cross matrix B (L->prows x m) is solved in place below padded order 2048
// and out of place through the block inverses from 2048 on.  chol_cross_oop is the rule (gpx_potrf builds the inverses by it, the
// callers size their second buffer by it); chol_cross_solve runs chol_trsm_left on the factor's own p / ld / aux / prows when
// W == NULL and chol_trsm_left_oop into W otherwise (B is then consumed).  The caller knows which buffer holds the solution.
bool chol_cross_oop(int64_t np);
int chol_cross_solve(gpx_ctx* ctx, const gpx_mat* L, double* B, int64_t ldb, double* W, int64_t ldw, int64_t m);
// one GROUP step of a right-looking left solve: Lg = the group's w x w diagonal triangle (row stride ld, `below` more rows
// underneath it), invd = the leaf inverses of its first row block, B = the group's w rows of the right-hand sides (m columns):
//   B[0:w] <- Lg^-1 B[0:w];  B[w : w+below] -= Lg[w:, 0:w] B[0:w]
// through explicit ib-order inverses built here (inv: ceil(w/ib) ib^2 doubles, tmp: the same, W: w x ldw doubles of scratch)
int chol_trsm_left_group(gpx_ctx* ctx, const double* Lg, int64_t ld, const double* invd, int64_t w, int64_t below, int64_t ib,
                         double* B, int64_t ldb, int64_t m, double* inv, double* tmp, double* W, int64_t ldw);
// one right-looking panel step of that solve with the rows [r0, r1) of the factor only (a finished look-ahead panel): W[r0:r1]
// from B[r0:r1] through the block inverses at `binv` (order ib, row stride ib), then B[r1:] -= L[r1:, r0:r1] W[r0:r1]
int64_t chol_potrf_panel_width(int64_t n);  // width of the look-ahead panels chol_potrf uses for order n (0: not blocked)
int64_t chol_potrs_scratch_bytes(int64_t n);
int chol_potrs(gpx_ctx* ctx, gpx_mat* L, double* v, double* scratch);
// y[r] -= sum_c A[r][c] x[c] over a rows x cols block (cols a multiple of 2, ld even)
int launch_gemv_sub(gpx_ctx* ctx, const double* A, int64_t ld, int64_t rows, int64_t cols, const double* x, double* y);
int chol_block_transpose(gpx_ctx* ctx, const double* in, double* out, int64_t n);
int chol_tri_gemv(gpx_ctx* ctx, const double* M, int64_t ld, int64_t sz, const double* y, double* x, int lower);

// fitc.hip: what grad.hip needs of a FITC model (the struct is private to fitc.hip)
struct gpx_fitc;
int64_t fitc_n(const gpx_fitc* f);
int64_t fitc_np(const gpx_fitc* f);
int64_t fitc_nup(const gpx_fitc* f);
int fitc_is_vfe(const gpx_fitc* f);   // 1: fitted by gpx_vfe_fit (the FITC-only entries refuse it)
int fitc_solve_beta_t(gpx_ctx* ctx, const gpx_fitc* f, const double* B, int64_t mcp, double* Bt, double* U);
// fitc.hip: what acq.hip needs of a VFE model
struct FitcView {
  const KParams* kp;
  int64_t n, nu, np, nup;
  double noise;
  gpx_mat *Lu, *La;
};
void fitc_view(const gpx_fitc* f, FitcView* v);
// *bu (nup doubles from `tmp`, 0 on the padding) = beta_u = Quu^-1 (Kuf coeff); coeff: host, n
int vfe_beta_u(gpx_ctx* ctx, const gpx_fitc* f, const double* coeff, Scratch& tmp, double** bu);
// One chunk Zc (mc points) of the VFE predictor -- the ONE sequence behind gpx_vfe_posterior, gpx_vfe_acq and gpx_vfe_acq_grad, so
// that their values agree by construction.  With mcp = mc rounded up to 128 and row stride gpx_skew_ld(mcp):
//   B1 = K(S, Zc) (nup x mcp);   pm = B1^T bu   (bu == NULL: no mean);   B2 == NULL: the mean only.  Else B2 = K(S, Zc) again (each
//   solve consumes its right-hand side), Lu^-1 B1 and La^-1 B2 in place (Wu == NULL) or through the block inverses into Wu and Wa
//   (which may be ONE buffer when the solutions are not wanted afterwards);   su, sa = their column sums of squares;
//   kd = k(z, z);   pv = (kd - su) + sa.
// kpz: the model's kernel re-centred on S and Z.  Asynchronous.
int vfe_posterior_chunk(gpx_ctx* ctx, const gpx_fitc* f, const KParams& kpz, const gpx_mat* S, const double* Zc, int64_t mc,
                        double* B1, double* B2, double* Wu, double* Wa, const double* bu, double* pm, double* su, double* sa,
                        double* kd, double* pv, double* part);
// fitc.hip: what vfe_design.hip shares with the models.  fitc_factor: chol_potrf in place (leaf inverses in K->aux) with the
// context's pivot policy; a bad pivot is returned (> 0) with a message that reads `what`.  fitc_wgrad_rows: the row pass of dL/dS,
//   out[u][l] (na x d, device) = sum_c Mw[u][c] dk(a_u, b_c)/da_u[l]      (the TRUE derivative; weights Mw: na x nb, row stride ld)
// in a fixed order; ppart: fitc_wgrad_partial_elems(na, nb, d) doubles of scratch.
int fitc_factor(gpx_ctx* ctx, gpx_mat* K, const char* what);
int64_t fitc_wgrad_partial_elems(int64_t na, int64_t nb, int d);
int fitc_wgrad_rows(gpx_ctx* ctx, const KParams& kp, const gpx_mat* A, const gpx_mat* B, const double* Mw, int64_t ld, double* ppart,
                    double* out);
// vfe_design.hip: the body of gpx_vfe_var_grad, behind fitc.hip's argument checks
int vfe_var_grad_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* X, const gpx_mat* S, const gpx_mat* Z, double* out);
// acq.hip: the bodies of gpx_vfe_acq / gpx_vfe_acq_grad (grad_host != NULL) and gpx_vfe_acq_batch, behind fitc.hip's argument checks.
// acq = GPX_ACQ_VARIANCE (internal, not in gpx.h): the "cost" is the signed variance itself, (a, b) = (0, 1), so the gradient is
// d var(z)/dz (gpx_vfe_var_grad_newpt); coeff may then be NULL (beta_u = 0).
#define GPX_ACQ_VARIANCE (-1)
// acq = GPX_ACQ_MES (internal; the gpx_acq_mes* / gpx_vfe_acq_mes* entries' own): max-value entropy search on the K sampled optima
// of `mes` (host memory, the caller's), which then stands beside the unused scalar `param`.  mes_args (acq.hip): 1 <= K <=
// GPX_MES_MAX_K, every y* finite, sign +1 or -1 -- else an argument error that names what is wrong.
#define GPX_ACQ_MES (-2)
struct MesSpec {
  const double* ystar;
  int64_t K;
  int sign;
};
int mes_args(const MesSpec* mes);
int vfe_acq_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                 double* cost_host, int64_t* best, double* best_cost, double* grad_host, const MesSpec* mes = nullptr);
int vfe_acq_batch_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Cm, int acq,
                       double param, int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx, double* out_cost,
                       double* out_lie, double* all_costs, const MesSpec* mes = nullptr);
// paths.hip / sample.hip: the bodies of gpx_vfe_paths_create, gpx_vfe_posterior_cov and gpx_vfe_psampler_create, behind fitc.hip's
// argument checks (a VFE model, its own S, unpadded Z of at least one row, a stationary kernel for the paths)
int vfe_paths_create_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const double* omega,
                          const double* phase, int64_t nfeat, const double* w, const double* eps_u, const double* xi_q, int64_t nPaths,
                          gpx_paths** out);
int vfe_posterior_cov_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* cov);
int vfe_psampler_create_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double nugget,
                             gpx_psampler** out);
// sample.hip: the body of gpx_vfe_acq_qei and gpx_dbg_vfe_qei_blocks (dbg_*: host B x q, B x q x q, B x q x q; all three or none),
// behind fitc.hip's argument checks (a VFE model, its own S, q in range, rows of Zb a positive multiple of q, nS >= 1, nugget >= 0)
int vfe_qei_impl(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q, const double* xi,
                 int64_t nS, double fBest, double nugget, double* cost_host, int64_t* best, double* best_cost, int64_t* n_bad,
                 double* dbg_mean, double* dbg_C, double* dbg_F);
// acq.hip: out_c[0], out_i[0] (device) = the first minimum among the nparts arg-min partials {cost, index} with index >= 0
// (argmin_merge; index -1 and a NaN cost when there is none) -- gpx_acq's final reduction, for sample.hip's q-EI partials
int launch_acq_argmin(gpx_ctx* ctx, const double* part_c, const int64_t* part_i, int64_t nparts, double* out_c, int64_t* out_i);

// reduce.hip
// out[j] = sum_i B[i][j] * v[i]   (v == nullptr: sum_i B[i][j]^2), i < rows, j < pcols; deterministic
int launch_colreduce(gpx_ctx* ctx, const double* B, int64_t ld, int64_t rows, int64_t pcols, const double* v,
                     double* out, double* d_partial, int subtract = 0);
int64_t colreduce_partial_elems(int64_t rows, int64_t pcols);
int launch_rowreduce(gpx_ctx* ctx, const double* B, int64_t ld, int64_t rows, int64_t cols, const double* v,
                     double* out, int weighted_squares = 0);
int launch_sum(gpx_ctx* ctx, const double* x, int64_t n, double* d_out);
int launch_diag(gpx_ctx* ctx, const double* A, int64_t ld, int64_t n, double* out);                 // out[i] = A[i][i], i < n
int launch_vec_sub(gpx_ctx* ctx, const double* a, const double* b, int64_t n, double* out);        // out[j] = a[j] - b[j], j < n

// One workgroup per row (`rows` of them, row stride ld, mc entries, global index m0 + j): the first minimum (sign > 0) or maximum of
// the row by vi_min / vi_max on the raw values -- the smaller index wins a tie, a NaN never wins -- merged into the running winner
// idx / val unless `first`.  gpx_row_argbest_nan (host, after the copies have landed): an all-NaN row, left at index INT64_MAX,
// becomes index 0 and a NaN value, as np.argmin.
int launch_row_argbest(gpx_ctx* ctx, const double* rowsp, int64_t rows, int64_t ld, int64_t mc, int64_t m0, int sign, int first,
                       int64_t* idx, double* val);
void gpx_row_argbest_nan(int64_t rows, int64_t* idx, double* val);

// hyper.hip: out[q] = sum over the tiles of partial[tile][q], q < nq, in a fixed order (the final pass of the tiled traces)
int launch_tile_sums(gpx_ctx* ctx, const double* partial, int64_t nblocks, int nq, double* out);

// design.hip
extern "C" __attribute__((visibility("hidden"))) int gpx_potri_impl(gpx_ctx* ctx, const gpx_mat* L, gpx_mat** outP, int full);
int launch_transpose(gpx_ctx* ctx, const double* in, int64_t rows, int64_t cols, int64_t ldi, double* out, int64_t ldo);

// The input side of those passes (AcqOut, acq.hip, is the output side): the work set of gpx_posterior_chunk for chunks of up to
// mc_alloc points against a factor of padded order np (var: with the solve and its sums of squares), from the caller's Scratch.  B
// or W set before take() (posterior_impl's kept matrix) is used as it is.  The means land in `mean` when a block of their own was
// asked for, else they pass through ssq's.
struct PosteriorWork {
  const int64_t np, mc_alloc, bytesB;
  const bool var;
  double *B = nullptr, *W = nullptr, *alpha = nullptr, *mean = nullptr, *ssq = nullptr, *kd = nullptr, *part = nullptr;

  PosteriorWork(int64_t np_, int64_t mc_alloc_, bool var_)
      : np(np_), mc_alloc(mc_alloc_), bytesB(np_ * gpx_skew_ld(mc_alloc_) * 8), var(var_) {}
  bool oop() const { return var && chol_cross_oop(np); }   // the cross-solve rule: the mean alone solves nothing
  // outs == false: the mean alone, into a block of the caller's (run's mean_to) -- B, alpha and part only
  int take(Scratch& sc, bool want_mean, bool mean_block, bool outs = true) {
    if (!B) GPX_TRY(sc.get(bytesB, &B));
    if (oop() && !W) GPX_TRY(sc.get(bytesB, &W));
    if (want_mean) GPX_TRY(sc.get(np * 8, &alpha));
    if (mean_block) GPX_TRY(sc.get(mc_alloc * 8, &mean));
    if (outs) GPX_TRY(sc.get(mc_alloc * 8, &ssq));
    if (outs) GPX_TRY(sc.get(mc_alloc * 8, &kd));
    return sc.get(colreduce_partial_elems(np, mc_alloc) * 8 + 8, &part);
  }
  int upload_alpha(gpx_ctx* ctx, const double* host, int64_t n) { return gpx_fill_padded(ctx, alpha, host, n, np); }
  int run(gpx_ctx* ctx, const KParams& kp, const gpx_mat* L, const gpx_mat* X, const double* Zc, int64_t mc,
          double* mean_host = nullptr, double* mean_to = nullptr) {
    return gpx_posterior_chunk(ctx, kp, L, X, Zc, mc, B, oop() ? W : nullptr, alpha, mean_to ? mean_to : mean ? mean : ssq,
                               mean_host, var ? ssq : nullptr, kd, part);
  }
  double* solution() const { return oop() ? W : B; }   // holds L^-1 K(X, Zc) after run()
};

// The VFE counterpart: the work set of vfe_posterior_chunk for chunks of up to mc_alloc points against nup padded inducing points.
// Out of place both solutions land in Wo; a caller that wants them both afterwards (the gradient) sets Wa to a block of its own.
struct VfePosteriorWork {
  const int64_t nup, mc_alloc, bytesB;
  const bool var;
  double *B1 = nullptr, *B2 = nullptr, *Wo = nullptr, *Wa = nullptr, *part = nullptr, *pm = nullptr, *su = nullptr, *sa = nullptr;
  double *kd = nullptr, *pv = nullptr, *bu = nullptr;

  VfePosteriorWork(int64_t nup_, int64_t mc_alloc_, bool var_)
      : nup(nup_), mc_alloc(mc_alloc_), bytesB(nup_ * gpx_skew_ld(mc_alloc_) * 8), var(var_) {}
  bool oop() const { return var && chol_cross_oop(nup); }
  int take(Scratch& sc, bool want_mean) {
    GPX_TRY(sc.get(bytesB, &B1));
    GPX_TRY(sc.get(colreduce_partial_elems(nup, mc_alloc) * 8 + 8, &part));
    if (var) {
      GPX_TRY(sc.get(bytesB, &B2));
      if (oop()) GPX_TRY(sc.get(bytesB, &Wo));
      for (double** o : {&su, &sa, &kd, &pv}) GPX_TRY(sc.get(mc_alloc * 8, o));
    }
    if (want_mean) GPX_TRY(sc.get(mc_alloc * 8, &pm));
    return 0;
  }
  // beta_u through vfe_beta_u; coeff == NULL: beta_u = 0 (a cost without a mean term)
  int beta(gpx_ctx* ctx, const gpx_fitc* f, const double* coeff, Scratch& sc) {
    if (coeff) return vfe_beta_u(ctx, f, coeff, sc, &bu);
    GPX_TRY(sc.get(nup * 8, &bu));
    GPX_HIP(hipMemsetAsync(bu, 0, (size_t)nup * 8, ctx->stream));
    return 0;
  }
  int run(gpx_ctx* ctx, const gpx_fitc* f, const KParams& kpz, const gpx_mat* S, const double* Zc, int64_t mc) {
    return vfe_posterior_chunk(ctx, f, kpz, S, Zc, mc, B1, B2, Wo, Wo && Wa ? Wa : Wo, bu, pm, su, sa, kd, pv, part);
  }
  // hold Lu^-1 K(S, Zc) and La^-1 K(S, Zc) after run() (out of place without a Wa of its own: only the latter survives)
  double* solU() const { return Wo ? Wo : B1; }
  double* solA() const { return Wo ? (Wa ? Wa : Wo) : B2; }
};
