/* gpx.h -- C ABI of libgpx_hip.so: the MI355X (gfx950) GP-inference hot path behind GPEXP's API.
 *
 * The reference (goroda/GPEXP) is pure Python and has NO existing FFI/plugin layer;
 * its boundary is the Python class API.  Each entry point below replaces the NumPy/LAPACK work
 * of the reference call site cited next to it (file:line relative to the reference root) and is
 * bound from Python by ctypes in gpexp_amd/_lib.py (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - All matrices/vectors are IEEE fp64.  Host buffers are C-contiguous row-major (NumPy default),
 *    caller-owned, and must outlive the call only.
 *  - gpx_mat is a library-owned dense device matrix (row-major, leading dimension >= cols, storage
 *    padded to a multiple of 128 in both dimensions; the padding is kept as an identity / zero
 *    extension so that factorisations and solves never see an edge tile).  Free with gpx_mat_free.
 *  - Return value: 0 = ok; >0 = 1-based index of the first non-positive Cholesky pivot
 *    (the reference never fails here because numpy.linalg.pinv silently truncates, gp.py:181);
 *    <0 = argument / HIP / RCCL error, text via gpx_last_error().
 *  - Calls are blocking unless stated; one gpx_ctx per process (= per GPU); not thread-safe by
 *    contract (the reference's callers are single-threaded).
 *  - Placement independence: the stationary kernels subtract coordinates before anything else in the reference
 *    (kernels.py:121-122, 87-89).  The assembly centres every point set on its bounding-box midpoint (computed on the
 *    host at gpx_mat_from_host) and switches to raw coordinate differences when the centred domain is still wide
 *    relative to the length scales, so results do not depend on where the inputs sit (gpx_dbg_kfill_plan reports it).
 *  - Covariance kernels are passed flat as (kind, d, hyp[nhyp]):
 *      GPX_K_SE        hyp = {cl_0..cl_{d-1}, signalSize}          kernels.py:100-123
 *      GPX_K_MATERN32  hyp = {rho, signalSize}                      kernels.py:72-91
 *      GPX_K_MATERN52  hyp = {rho, signalSize}                      (absent from the reference)
 *      GPX_K_MEHLER    hyp = {t_0..t_{d-1}}                         kernels.py:183-228, 250-293
 */
#ifndef GPX_H
#define GPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_ABI_VERSION 2
#define GPX_MAX_DIM 32

typedef struct gpx_ctx gpx_ctx;
typedef struct gpx_mat gpx_mat;

enum gpx_kernel_kind { GPX_K_SE = 0, GPX_K_MATERN32 = 1, GPX_K_MATERN52 = 2, GPX_K_MEHLER = 3 };

/* names of the timed kernel classes reported by gpx_profile_get */
enum gpx_prof_class {
  GPX_PROF_KFILL = 0,   /* symmetric covariance assembly K(X,X) (HBM-bound: 8*rows*cols bytes written) */
  GPX_PROF_GEMM = 1,    /* fp64 MFMA GEMM/SYRK/TRSM-update tiles (MFMA-bound: 2*m*n*k flops) */
  GPX_PROF_LEAF = 2,    /* 128x128 diagonal potf2 + trtri */
  GPX_PROF_TRSV = 3,    /* potrs sweeps */
  GPX_PROF_REDUCE = 4,  /* column reductions / logdet */
  GPX_PROF_GREEDY = 5,  /* greedy-design scoring kernels */
  GPX_PROF_COMM = 6,    /* RCCL collectives */
  GPX_PROF_KCROSS = 7,  /* rectangular cross-covariance assembly K(X,Z): every element computed (VALU: sqrt + exp) */
  GPX_PROF_NCLASS = 8
};

/* ---- lifecycle ------------------------------------------------------------------------------ */
int gpx_abi_version(void);
const char* gpx_last_error(void);
/* device = HIP ordinal (LOCAL_RANK in the one-process-per-GPU launch).  Fails (<0) when no GPU. */
int gpx_create(int device, gpx_ctx** out);
int gpx_destroy(gpx_ctx* ctx);
int gpx_sync(gpx_ctx* ctx);   /* device-wide: every stream of the context */
/* release cached workspace back to HIP */
int gpx_trim(gpx_ctx* ctx);
/* device facts for reports: name[<=256], CU count, HBM bytes, clock MHz */
int gpx_device_info(gpx_ctx* ctx, char* name, int name_len, int* cus, int64_t* hbm_bytes, int* clock_mhz);

/* ---- device matrices ------------------------------------------------------------------------- */
/* upload a (rows x cols) host array; pad != 0 pads storage to multiples of 128 (zero filled) */
int gpx_mat_from_host(gpx_ctx* ctx, const double* src, int64_t rows, int64_t cols, int pad, gpx_mat** out);
int gpx_mat_alloc(gpx_ctx* ctx, int64_t rows, int64_t cols, int pad, gpx_mat** out);
int gpx_mat_free(gpx_ctx* ctx, gpx_mat* m);
/* device-to-device duplicate of a matrix INCLUDING its factor state (leaf inverses): the class API under a multi-process
 * launch hands every GP object its own copy of the replicated factor the distributed runner assembled (gp.py:181's
 * precisionMatrix role); blocking on the selected stream */
int gpx_mat_clone(gpx_ctx* ctx, const gpx_mat* src, gpx_mat** out);
int gpx_mat_shape(const gpx_mat* m, int64_t* rows, int64_t* cols, int64_t* ld);
/* tri: 0 = as stored, 1 = lower triangle (strict upper written as 0), 2 = lower mirrored to upper.
 * Backs the lazy GP.covarianceMatrix / GP.precisionMatrix attributes (gp.py:178-181). */
int gpx_mat_to_host(gpx_ctx* ctx, const gpx_mat* m, double* dst, int tri);

/* ---- L0/L1: covariance assembly -------------------------------------------------------------- */
/* K[i][j] = k(X_i, X_j) + nugget_i*delta_ij  (Z == NULL; N x N)      gp_kernel_utilities.py:34-68
 * K[i][j] = k(X_i, Z_j)                      (Z != NULL; N x M)      gp.py:132-135, 246-249;
 *                                                                    experimentalDesign.py:829-831
 * X, Z: device point sets (rows = points, cols = d).  nugget: host, nugget_len in {0,1,N}.
 * Non-finite coordinates: a point set holding a NaN or an infinity is REFUSED (-1, the message names the first such row and
 * column) by this and by every other entry point that assembles covariances between point sets.  The host looks while it
 * computes the set's bounding box (at upload, or on first use after a device-side write); the fill kernels themselves do not
 * check, and their clamps would turn a NaN coordinate into a covariance of exactly 0 -- which a fit would accept in silence.
 * Matrices that are not point sets (y, K, ...) are not looked at.  gpx_kdiag and gpx_kernel_eval take no such decision:
 * gpx_kernel_eval propagates NaN as libm does, gpx_kdiag of a stationary kind does not read the coordinates at all.
 * Far pairs: a pair of finite points whose covariance is below half a denormal step comes out as exactly 0, however far apart
 * (the exponent argument is clamped at -5e6 and 2^-7.2e6 takes any finite factor to 0) -- up to the point where the squared
 * scaled distance or the Matern polynomial overflows a double (scaled distance ~1e154): beyond it the entry is inf or NaN. */
int gpx_kfill(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
              const gpx_mat* X, const gpx_mat* Z, const double* nugget, int64_t nugget_len,
              gpx_mat** outK);
/* same, into an existing matrix of the right shape (no allocation inside timed loops) */
int gpx_kfill_into(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                   const gpx_mat* X, const gpx_mat* Z, const double* nugget, int64_t nugget_len,
                   gpx_mat* K);
/* k(Z_j, Z_j) for every point -> host out[M]                          gp.py:140, 251 */
int gpx_kdiag(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* Z, double* out);

/* Kernel.evaluate semantics (kernels.py:49-65): out[i] = k(A_i, B_i) for equally sized host point sets, or
 * one point against n (na == 1 or nb == 1); out has max(na, nb) entries.  Any other shape pair is an error. */
int gpx_kernel_eval(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                    const double* A, int64_t na, const double* B, int64_t nb, double* out);

/* ---- L2: factorisation and solves (replace numpy.linalg.pinv / slogdet) ---------------------- */
/* in-place lower Cholesky K = L L^T; replaces pinv at gp.py:181, 400.
   INVARIANT of every factored matrix (gpx_potrf, gpx_refit_rows, the distributed fits): only the lower triangle is defined.
   The strict upper part holds whatever the storage held before -- finite leftovers of K after gpx_potrf, possibly NaN / Inf
   pool contents after gpx_refit_rows (which copies the old factor's lower triangle only).  No entry point reads it: solves,
   posterior, gradients, gpx_potri and further refits take the lower triangle; gpx_mat_to_host(tri = 1 / 2) masks / mirrors it.
   tests/test_gpu_refit.py runs them on a refit factor whose pool blocks were NaN-filled. */
int gpx_potrf(gpx_ctx* ctx, gpx_mat* K);
/* Pivot policy of every factorisation that follows: a pivot <= piv_min is bad; skip == 0 reports it (status > 0 from
 * gpx_potrf, the default with piv_min = 0), skip != 0 DROPS the point instead -- L_jj = 1, the rest of column j and row j of
 * the inverse are 0, so solves return 0 in that component, as if the point were not in the set: what numpy.linalg.pinv
 * (gp.py:181, experimentalDesign.py:826) makes of an exactly duplicated point.  gpx_potrf_dropped: pivots dropped by the
 * last factorisation. */
int gpx_potrf_policy(gpx_ctx* ctx, double piv_min, int skip);
int gpx_potrf_dropped(gpx_ctx* ctx, int* count);
/* factor K(X)+nugget when its leading `keep` (multiple of 128) rows/columns equal the matrix Lold factors
 * (the design loop pins earlier points by bounds, experimentalDesign.py:722-724, and only the last batch moves): the
 * leading factor block is copied, rows >= keep are assembled and the factorisation is completed in O(N^2 b).
 * keep == 0 (Lold may be NULL) is a plain assemble + factor.  Status as gpx_potrf; *outL is a new library-owned matrix. */
int gpx_refit_rows(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                   const double* nugget, int64_t nugget_len, const gpx_mat* Lold, int64_t keep, gpx_mat** outL);
/* alpha = K^{-1} y from the factor; y, alpha host (N)                 gp.py:101, 435 */
int gpx_potrs(gpx_ctx* ctx, const gpx_mat* L, const double* y, double* alpha);
/* the same on device vectors (y, alpha: at least padded-N doubles, zero padded), ASYNCHRONOUS on the selected
 * stream -- lets the latency-bound sweeps run on the side stream underneath the evaluation GEMMs */
int gpx_potrs_dev(gpx_ctx* ctx, const gpx_mat* L, const gpx_mat* y, gpx_mat* alpha);
/* log det K = 2 sum log L_ii                                          gp.py:434 (slogdet) */
int gpx_logdet(gpx_ctx* ctx, const gpx_mat* L, double* out);
/* explicit inverse (lower triangle valid) for the lazy precisionMatrix attribute and lml_grad */
int gpx_potri(gpx_ctx* ctx, const gpx_mat* L, gpx_mat** outP);

/* posterior at M points: mean_j = k_j^T alpha (gp.py:137), var_j = k(z_j,z_j) - k_j^T K^{-1} k_j
 * (signed, gp.py:253-256; the caller applies abs for GP.evaluate, gp.py:145).
 * alpha (host, N) may be NULL when mean == NULL; mean / var (host, M) may each be NULL. */
int gpx_posterior(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                  const gpx_mat* L, const gpx_mat* X, const double* alpha,
                  const gpx_mat* Z, double* mean, double* var);
/* full M x M posterior covariance (compvar=2, gp.py:146-152) -> host cov[M*M] */
int gpx_posterior_cov(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                      const gpx_mat* L, const gpx_mat* X, const gpx_mat* Z, double* cov);

/* ---- L3: design-cost evaluators ---------------------------------------------------------------- */
/* IVAR = (1/M) sum_j var_j (signed mean; caller applies abs)          experimentalDesign.py:104-117 */
int gpx_ivar(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
             const gpx_mat* L, const gpx_mat* X, const gpx_mat* Z, double* out);
/* The same cost, keeping W = L^-1 K(X, Z) (N x M, a matrix of the context: release with gpx_mat_free) for the gradient AT THE
 * SAME DESIGN: an optimiser asks for the cost and then its gradient at one point (experimentalDesign.py:471-489), and the forward
 * solve is a third of the gradient's work.  *W = NULL when Z does not fit one evaluation chunk. */
int gpx_ivar_keep(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                  const gpx_mat* L, const gpx_mat* X, const gpx_mat* Z, double* out, gpx_mat** W);
/* The cost once more after gpx_refit_rows kept the leading `keep` rows of the factor: W (from gpx_ivar_keep / an earlier update, for
 * the design whose factor the refit started from) keeps its leading rows, the rows from `keep` on are re-assembled and re-solved in
 * place -- 2 (N - keep) keep M flops instead of N^2 M (the batch loop of experimentalDesign.py:694-751 moves the last batch only). */
int gpx_ivar_update(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                    const gpx_mat* Z, gpx_mat* W, int64_t keep, double* out);
/* GP fit + IVAR in one call -- what costFunctionGP_IVAR.evaluate (experimentalDesign.py:104-117: refit, then
 * evaluateVariance over the MC points) amounts to per optimiser evaluation: K (assembled, gpx_kfill) is factored in place
 * as by gpx_potrf and *out receives what gpx_ivar would return on the finished factor.  With GPX_FIT_IVAR_STREAMED=1 the
 * evaluation solve is streamed underneath the factorisation (panel events of the blocked look-ahead Cholesky, a
 * low-priority stream of its own); on one GPU that measured slower than factor-then-solve, so it is opt-in.
 * Status as gpx_potrf.  Main stream only. */
int gpx_fit_ivar(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, gpx_mat* K, const gpx_mat* X, const gpx_mat* Z,
                 double* out);
/* greedy maximum-posterior-variance selection among M candidates, nugget 0 (experimentalDesign.py:787-845).
 * keep[nkeep] = indices already selected; selects until nsel indices in total; out_idx[nsel] receives
 * keep followed by the new picks; w (host, M) optional weights; first-max tie rule (np.argmax). */
int gpx_greedy_var(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                   const gpx_mat* C, const double* w, const int64_t* keep, int64_t nkeep,
                   int64_t nsel, int64_t* out_idx);
/* one-step-lookahead greedy IVAR among candidates C for a GP already factored on X (L):
 * cost_j = IVAR(X u {c_j}) over MC points Z with noise variance `noise` on the new point;
 * out_cost[M] (host, nullable) all costs, *out_best = first arg-min.  Composition oracle: SURVEY.md 8c. */
int gpx_greedy_ivar_step(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp,
                         const gpx_mat* L, const gpx_mat* X, const gpx_mat* C, const gpx_mat* Z,
                         double noise, double* out_cost, int64_t* out_best);
/* Multi-pick greedy IVAR with RESIDENT state (composition of experimentalDesign.py:79-117 per SURVEY 8c): nsel picks cost one
 * set-up (the work of ONE gpx_greedy_ivar_step) + per pick one pass over W_C = L^-1 K(X, C) and one over cov(Z, C | design) --
 * no refit, no N^2 solve.  Picks equal nsel rounds of gpx_greedy_ivar_step + refit on the winner (a candidate may be picked
 * again, as there).  out_idx[nsel]; out_cost[nsel] (the winner's cost at each pick, optional); all_costs (nsel x M, optional). */
int gpx_greedy_ivar(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                    const gpx_mat* C, const gpx_mat* Z, double noise, int64_t nsel, int64_t* out_idx, double* out_cost,
                    double* all_costs);

/* greedy mutual-information design among M candidates with noise variance `noise`, seeded with `start`
 * (experimentalDesign.py:223-285, 753-785): out_idx[nsel] = start followed by the picks (first-max tie rule);
 * out_ratio[nsel-1] (nullable) = winning ratio var(c|A)/var(c|all\A\c) of every step.  M <= 65535. */
int gpx_mi_greedy(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* C, double noise,
                  int64_t nsel, int64_t start, int64_t* out_idx, double* out_ratio);

/* ---- Bayesian-optimisation costs (costFuncGPUCbound / costFuncPI / costFuncEI, experimentalDesign.py:889-1003) ----------------
 * The reference scores ONE point per call (the last row of trainPoints: a single-row GP.evaluate(compvar=1) + scipy.stats); these
 * score the M candidates of Z in one call, in minimisation form.  mu = posterior mean (alpha: the trained coefficients, host N),
 * s = sqrt(|var|) (GP.evaluate's abs, gp.py:145), g = (fBest - mu) / s, Phi / phi the standard normal cdf / density:
 *     GPX_ACQ_UCB  cost = -(mu - kappa s)            param = kappa   (experimentalDesign.py:899-923)
 *     GPX_ACQ_PI   cost = -Phi(g)                    param = fBest   (experimentalDesign.py:934-960)
 *     GPX_ACQ_EI   cost = -s (g Phi(g) + phi(g))     param = fBest   (experimentalDesign.py:973-1003)
 * Dense factor only (gpx_potrf / gpx_refit_rows); the kernel's prior mean is zero (gp.py:73). */
enum gpx_acq_kind { GPX_ACQ_UCB = 0, GPX_ACQ_PI = 1, GPX_ACQ_EI = 2 };
/* cost (host M, nullable) every candidate's cost; *best (nullable) = the FIRST index of the minimum among the non-NaN costs, -1 when
 * every cost is NaN; *best_cost (nullable) its cost (NaN when best == -1).  The arg-min is deterministic and does not depend on
 * how Z is chunked (GPX_CROSS_BYTES).  Only cost (when asked for) and the winner reach the host. */
int gpx_acq(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
            const double* alpha, const gpx_mat* Z, int acq, double param, double* cost, int64_t* best, double* best_cost);
/* grad (host M x d): grad[m*d + l] = d cost_m / d z_m[l], the true derivative of gpx_acq's values (NaN rows where var == 0
 * exactly); cost (host M, nullable) as gpx_acq.  Stationary kernels only (SE, Matern 3/2, Matern 5/2): Mehler is an argument
 * error. */
int gpx_acq_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const double* alpha, const gpx_mat* Z, int acq, double param, double* cost, double* grad);

/* q-point batch selection (Kriging believer / constant liar): q candidates picked one after the other, each pick scored on the
 * model CONDITIONED on the earlier picks' hallucinated observations -- the loop "cost = costFuncEI(gp, X_t, y_t); j = bestCandidate(C);
 * append (c_j, lie)" without refitting.  Resident state W_C = L^-1 K(X, C) (N x M), mu_j = K(c_j, X) alpha,
 * v_j = k(c_j, c_j) - |W_C[:, j]|^2 (signed, as gpx_posterior); `noise` is the model's scalar noise variance.  Pick t = 0 .. q-1:
 *     cost_j = A(mu_j, |v_j|; param) as gpx_acq, NaN for the candidates already picked;  s = first arg-min among the non-NaN costs
 *     delta  = v_s + noise;   y_s = mu_s (GPX_LIE_BELIEVER) or lie_value (GPX_LIE_CONSTANT)
 *     u_j    = (k(c_s, c_j) - W_C[:, s]^T W_C[:, j] - sum_{r<t} U[r][s] U[r][j]) / sqrt(delta);   U[t] = u
 *     mu_j  += u_j (y_s - mu_s) / sqrt(delta);   v_j -= u_j^2;   param = max(param, y_s) when track_best != 0
 * i.e. pick by pick the posterior of the model refitted on X + picks, y + lies.  A pivot with delta <= 1e-13 k(c_s, c_s) is
 * recorded and masked but conditions nothing (u = 0), as in gpx_greedy_var.  Per pick one pass over W_C (8 N M bytes), no refit,
 * no N^2 solve; all reductions in a fixed order (two runs agree bit for bit).  Every kernel of gpx_acq is accepted.
 * out_idx[q]; out_cost[q] (nullable) the winner's cost at each pick; out_lie[q] (nullable) the value believed at each pick;
 * all_costs (q x M, nullable) row t = the costs pick t was chosen from.  q < 1 and q > M are argument errors; a pick at which every
 * remaining cost is NaN fails with an error that names the pick. */
enum gpx_acq_lie { GPX_LIE_BELIEVER = 0, GPX_LIE_CONSTANT = 1 };
int gpx_acq_batch(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                  const double* alpha, const gpx_mat* C, double noise, int acq, double param, int track_best,
                  int lie, double lie_value, int64_t q,
                  int64_t* out_idx, double* out_cost, double* out_lie, double* all_costs);

/* ---- max-value entropy search (MES; Wang & Jegelka 2017) ------------------------------------------------------------------------
 * The three calls above for the information-theoretic cost: ystar (HOST, K doubles, 1 <= K <= GPX_MES_MAX_K, every one finite) holds
 * K samples of the global optimum VALUE -- sampled minima with sign = +1, gamma_k = (mu - ystar_k) / s; sampled maxima with sign =
 * -1, gamma_k = (ystar_k - mu) / s -- and a candidate is scored by the expected drop in entropy of its predictive distribution
 * once truncated at ystar.  With s = sqrt(|var|), lambda = phi / Phi:
 *     h(gamma)  = gamma lambda(gamma) / 2 - log Phi(gamma)     >= 0,  h(0) = log 2,  h -> 0 (gamma -> +inf),  h ~ log(-gamma) (-> -inf)
 *     h'(gamma) = -(lambda / 2) (1 + gamma (gamma + lambda))   <= 0
 *     cost = -(1/K) sum_k h(gamma_k)                            (summed in the order k = 0 .. K-1)
 *     a = dcost/dmu = -(sign / (K s)) sum_k h'(gamma_k)         b = dcost/dvar = (sgn(var) / (2 K s^2)) sum_k h'(gamma_k) gamma_k
 * h and h' are formed without cancellation for every finite gamma (a continued fraction of erfcx below gamma = -2 sqrt 2: acq.hip),
 * gamma = +inf gives h = h' = 0, gamma = -inf gives h = +inf.  The formulas are evaluated as written where var == 0 exactly (an exact
 * duplicate of a training point under zero noise): a candidate whose mean lies on the optimum side of some ystar_k (mu < ystar_k
 * for sampled minima) then has gamma_k = -inf and takes cost -inf, so it WINS the arg-min (its a and b are NaN); with the mean on
 * the other side of every ystar its cost is -0.  Mask such candidates beforehand if they are not wanted.  ystar NULL or with a non-finite entry, K out of range and sign other
 * than +1 / -1 are argument errors that name what is wrong.
 * gpx_acq_mes: every rule of gpx_acq (cost / best / best_cost nullable; the FIRST arg-min among the non-NaN costs, -1 / NaN when
 *   there is none; bits independent of the chunking under GPX_CROSS_BYTES; every kernel kind).
 * gpx_acq_mes_grad: gpx_acq_grad's rules (stationary kernels only; NaN rows where var == 0 exactly); cost holds gpx_acq_mes's bits.
 * gpx_acq_mes_batch: gpx_acq_batch's recurrence with ystar held fixed from pick to pick (there is no track_best); row 0 of all_costs
 *   holds gpx_acq_mes's bits; two runs agree bit for bit. */
#define GPX_MES_MAX_K 1024
int gpx_acq_mes(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                const double* alpha, const gpx_mat* Z, const double* ystar, int64_t K, int sign, double* cost, int64_t* best,
                double* best_cost);
int gpx_acq_mes_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const double* alpha, const gpx_mat* Z, const double* ystar, int64_t K, int sign, double* cost, double* grad);
int gpx_acq_mes_batch(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                      const double* alpha, const gpx_mat* C, double noise, const double* ystar, int64_t K, int sign, int lie,
                      double lie_value, int64_t q, int64_t* out_idx, double* out_cost, double* out_lie, double* all_costs);

/* ---- joint posterior samples, Thompson picks and Monte-Carlo q-EI -------------------------------------------------------------
 * The reference draws functions from the PRIOR (GP.generateSamples, gp.py:343-371: an SVD and numpy.random inside); these draw
 * from the posterior at the M points of Z JOINTLY, pick per draw, and score whole q-batches.  Two rules:
 *   - no random numbers are made on the device: every call takes the standard-normal BASE SAMPLES xi from the caller (host), so a
 *     result is a deterministic function of its arguments -- two calls return the same bits -- and batches are compared on
 *     common random numbers;
 *   - the covariance is made positive definite by a NUGGET on its diagonal, F = chol(C + nugget I), factored with the pivot policy
 *     (0, report) whatever gpx_potrf_policy holds (it is put back on every exit): no pivot is dropped, a pivot <= 0 comes back as
 *     its 1-based index (status > 0, as gpx_potrf).  nugget < 0 is an argument error.  Dense factor only.
 * gpx_psampler_create: resident state mean (M) and F (M x M; only these two stay).  mean_j = k_j^T alpha, the bits gpx_posterior
 *   returns; C = K(Z,Z) - W^T W with W = L^-1 K(X,Z), formed by gpx_posterior_cov's own sequence (before the nugget, the bits that
 *   call returns); after the factorisation one step of refinement, F <- F + F Phi(F^-1 (Chat - F F^T) F^-T), brings
 *   |F F^T - Chat| down to a few (M + 1) u sqrt(Chat_ii Chat_jj) / 10.  L == X == alpha == NULL: the PRIOR, C = K(Z,Z), mean 0.  Every kernel kind.  M < 1 is an argument error.  No
 *   chunking over Z (a joint draw cannot be chunked): what does not fit fails with the allocator's error.
 * gpx_psampler_draw: out[s][j] = mean_j + sum_{k <= j} F_jk xi[s][k]; xi, out: host S x M.  The product runs on the MFMA path;
 *   S is chunked under GPX_CROSS_BYTES.  A sample's bits depend neither on S nor on the chunking nor on the other samples.
 * gpx_psampler_argbest: per sample the FIRST index of the minimum (sign = +1) or maximum (sign = -1) over the M points -- exactly
 *   the first arg-best of the row gpx_psampler_draw returns for the same xi -- and its value (out_val: S, nullable); samples
 *   (S x M, nullable) the draws themselves.  Without `samples` only S indices and values reach the host (Thompson sampling). */
typedef struct gpx_psampler gpx_psampler;
int gpx_psampler_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                        const double* alpha, const gpx_mat* Z, double nugget, gpx_psampler** out);
int gpx_psampler_draw(gpx_ctx* ctx, const gpx_psampler* ps, const double* xi, int64_t S, double* out);
int gpx_psampler_argbest(gpx_ctx* ctx, const gpx_psampler* ps, const double* xi, int64_t S, int sign, int64_t* out_idx,
                         double* out_val, double* samples);
int gpx_psampler_shape(const gpx_psampler* ps, int64_t* m);
int gpx_psampler_free(gpx_ctx* ctx, gpx_psampler* ps);
/* Joint expected improvement of B batches of q points by Monte Carlo, in gpx_acq's minimisation form.  Zb: (B q) x d, consecutive q
 * rows form one batch; xi: host S x q, the SAME base samples for every batch (a sample-average approximation):
 *     cost_b = -(1/S) sum_s max(0, fBest - min_j (mu_bj + (F_b xi_s)_j)),   F_b = chol(C_b + nugget I)
 * with mu_b the posterior means (gpx_posterior's) and C_b the q x q posterior covariance of the batch.  q = 1 tends to GPX_ACQ_EI's
 * closed form as S grows.  A batch whose factorisation meets a pivot <= 0 gets cost NaN and is counted in *n_bad (nullable); the
 * call still succeeds.  cost (host B, nullable); *best / *best_cost as gpx_acq: the FIRST arg-min among the non-NaN costs, -1 (and
 * NaN) when all are NaN, whatever the chunking (whole batches under GPX_CROSS_BYTES).  1 <= q <= GPX_QEI_MAX_Q, rows of Zb a
 * multiple of q, S >= 1: anything else is an argument error.  Fixed-order reductions, no atomics: permuting the batches permutes
 * the costs bit for bit.  Dense factor only. */
#define GPX_QEI_MAX_Q 32
int gpx_acq_qei(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X, const double* alpha,
                const gpx_mat* Zb, int64_t q, const double* xi, int64_t S, double fBest, double nugget, double* cost, int64_t* best,
                double* best_cost, int64_t* n_bad);

/* ---- pathwise posterior samples (Matheron's rule): draws that are FUNCTIONS ------------------------------------------------------
 * gpx_psampler_* draws jointly at M fixed points through an M x M factor; these draw PATHS, which can be evaluated at any number of
 * points afterwards (Z is chunked under GPX_CROSS_BYTES), and differentiated:
 *     f~_s(z) = sum_j c_sj cos(omega_j . z + b_j),   c = sqrt(2 signalSize / nfeat) w            (prior path, nfeat random features)
 *     V       = alpha - (K + noise I)^-1 (f~(X) + eps)                                           (update weights, S x N)
 *     f_s(z)  = f~_s(z) + sum_i v_si k(z, x_i)                                                   (posterior path)
 * The sampler's rules hold: no random numbers are made on the device -- omega (the frequencies, draws of the kernel's spectral
 * density), phase (uniform in [0, 2 pi)), w (standard normal) and eps (the noise draw, variance = the model's noise) come from
 * the caller, so a result is a deterministic function of its arguments and two calls return the same bits.  Stationary kernels only
 * (GPX_K_SE, GPX_K_MATERN32, GPX_K_MATERN52: GPX_K_MEHLER is an argument error); dense factor only.
 * What pathwise samples are NOT: with finitely many features the prior part has covariance Phi Phi^T, not K, so the paths'
 * covariance at Z is A (Phi_J Phi_J^T) A^T + noise G G^T with G = K(Z,X) (K + noise I)^-1, A = [I, -G] and Phi_J the features at
 * (Z; X) -- it tends to the exact posterior covariance as nfeat grows.  The mean is exact.  gpx_psampler_* stays the exact sampler.
 * gpx_paths_create: evaluates the prior paths at X with gpx_paths_eval's own kernel, solves (K + noise I)^-1 (f~(X) + eps) against L
 *   (gpx_potrs_dev's solve, one right-hand side per path) and keeps omega, phase, c, V and a copy of X's points: nothing N x N stays.
 *   L == X == alpha == NULL: PRIOR paths (V = 0, N = 0).  nfeat < 1 and S < 1 are argument errors.
 * gpx_paths_eval: out[s][m] = f_s(z_m) (host S x M, nullable) by ONE product on the fp64 MFMA path whose large operand -- the
 *   features and K(X, Z) -- is generated in registers and never stored (no N x chunk buffer; the budget covers the S x chunk
 *   output).  The value of (s, m) depends on path s and on z_m alone: not on S, on the other paths or points of the call, or on the
 *   chunking, bit for bit.  sign = +1 / -1: per path the FIRST index of its minimum / maximum over the M points (best_idx: S) and
 *   the value there (best_val: S, nullable), reduced on the device and merged across chunks (the smaller index wins a tie); with
 *   out == NULL only these reach the host.  sign = 0: no pick.
 * gpx_paths_grad: point p (row p of Zp) belongs to path path[p]: grad[p][l] = d f_path[p](z_p) / d z_l, the true derivative (0 from
 *   the kernel term at z = x_i: nothing divides by the distance); val[p] (nullable) = the value there.  Fixed-order sums.
 * gpx_paths_coeff: v = V (host S x N).  gpx_paths_shape: S, nfeat, N (each nullable). */
typedef struct gpx_paths gpx_paths;
int gpx_paths_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                     const double* alpha, const double* omega, const double* phase, int64_t nfeat, const double* w,
                     const double* eps, int64_t S, gpx_paths** out);
int gpx_paths_eval(gpx_ctx* ctx, const gpx_paths* ps, const gpx_mat* Z, double* out, int sign, int64_t* best_idx,
                   double* best_val);
int gpx_paths_grad(gpx_ctx* ctx, const gpx_paths* ps, const gpx_mat* Zp, const int64_t* path, double* val, double* grad);
int gpx_paths_coeff(gpx_ctx* ctx, const gpx_paths* ps, double* v);
int gpx_paths_shape(const gpx_paths* ps, int64_t* S, int64_t* nfeat, int64_t* n);
int gpx_paths_free(gpx_ctx* ctx, gpx_paths* ps);

/* ---- hyper-parameter gradient -------------------------------------------------------------------- */
/* grad[k] = 1/2 tr((alpha alpha^T - K^-1) dK/d theta_k), theta = {hyp[0..nhyp-1], noise}; the noise entry is
 * the raw 1/2 tr(alpha alpha^T - K^-1) (the caller applies the reference's x 2*noise, gp.py:463-464).
 * Squared-exponential kernel only (gp.py:444-466 + kernels.py:125-144; the reference raises for the others). */
int gpx_lml_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const double* alpha, double* grad);

/* the same raw sums over ALL rows at once, for ONE GPU that can hold two more N x N buffers: L^-1 (N^3/3, large products),
 * U = L^-T, lower K^-1 = U U^T with the zero part of every tile's k range skipped (N^3/3), written over L^-1 -- the 2 N^3 / 3
 * flops of the slabs at the rate of large GEMMs, and N^2 less memory than gpx_potri + gpx_lml_grad (gp.py:444-466) */
int gpx_lml_grad_linv(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                      const double* alpha, double* sums);

/* ---- leave-one-out cross-validation (Rasmussen & Williams 5.4.2) ---------------------------------------------------
 * The reference has NO counterpart: validating a fit there means N refits through GP.train.  Zero prior mean, K including the
 * nugget D = diag(noise); with P = K^-1, alpha = P y, p_i = P_ii:
 *     mu_i = y_i - alpha_i / p_i,   var_i = 1 / p_i     the predictive distribution of the OBSERVATION y_i given all the others
 *                                                       (the noise of point i is included)
 *     L_LOO = sum_i [ -1/2 log var_i - (y_i - mu_i)^2 / (2 var_i) - 1/2 log 2 pi ]
 *     dL_LOO / d theta = sum_i ( alpha_i a_i - 1/2 (1 + alpha_i^2 / p_i) q_i ) / p_i,   W = P dK/d theta,
 *                        a_i = (W alpha)_i,   q_i = sum_l W_il P_il  (= [P dK P]_ii)
 * with dK as in gpx_lml_grad (coordinate differences first, then scaled; K0 = the covariance without the nugget):
 *     SE length cl_k:  K0 e_k^2 / cl_k, e_k = (x_k - x'_k) / cl_k;     Matern rho:  (rho dk/d rho) / rho;
 *     signalSize s:  K0 / s  (no product: P K0 = I - P D);              noise, a common shift of every nugget:  I.
 * One N x N x N product per LENGTH-type parameter only (d for SE, 1 for Matern).  All reductions run in a fixed order: two calls
 * agree bit for bit. */
/* mean / var (host N, each nullable), *logp = L_LOO.  Needs the factor only, so every kernel is accepted: L^-1 by the halving
 * recursion, p_i = column sums of squares of it (N^3 / 3 flops, no K^-1 is formed). */
int gpx_loo(gpx_ctx* ctx, const gpx_mat* L, const double* y, double* mean, double* var, double* logp);
/* *logp = L_LOO and grad[nlen + 2] = its TRUE derivatives in gpx_lml_grad's order [lengths..., signalSize, noise] (the noise entry
 * is the derivative w.r.t. the noise VARIANCE; no factor 2 * noise).  nugget as gpx_kfill takes it (nugget_len in {0, 1, N}) --
 * the one that went into L.  slab_rows: rows of W = P dK formed at once, a multiple of 128; 0 = the whole matrix when it fits,
 * otherwise the largest slab that does.  Squared exponential and isotropic Matern only, as gpx_lml_grad.
 * 2 N^3 / 3 + 2 nlen N^3 flops; memory: P + dK + the slab of W. */
int gpx_loo_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const double* nugget, int64_t nugget_len, const double* y, int64_t slab_rows, double* logp, double* grad);


/* ---- point-location gradients of the posterior variance ----------------------------------------------
 * For the two kernels the reference differentiates, in ITS convention: squared exponential (kernels.py:146-181, including its
 * doubled signalSize, :177) and 1-D Mehler (GPX_K_MEHLER with d == 1; kernels.py:295-324); and for GPX_K_MATERN32 /
 * GPX_K_MATERN52, which the reference does not differentiate, with the TRUE derivative (t = sqrt(2 nu) |u - p| / rho):
 *     d k(u, p) / d u = -s (3 / rho^2) e^-t (u - p)   resp.   -s (5 / (3 rho^2)) (1 + t) e^-t (u - p),
 * smooth at u = p.  Any other kind (Mehler with d > 1) is an argument error.  All entry points of this section and the two
 * gpx_fitc_var_grad* take the same kinds, with every optional argument.
 * noise_deriv (host N x d, nullable) = d noise(x_j) / d x_jl of a heteroscedastic noise model (space.noiseFunc.deriv,
 * gp.py:314-317): it enters the derivative of the covariance at coincident training points.  Nothing N x N reaches the host. */
/* grad[a*d + l] = d IVAR / d X[a][l] = (1/M) sum_m d var(z_m) / d X[a][l]
 * (costFunctionGP_IVAR.derivative, experimentalDesign.py:168-179 -> gp.py:282-341).  grad: host, N*d. */
int gpx_ivar_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                  const gpx_mat* Z, const double* noise_deriv, double* grad);
/* ... with the forward solve kept by gpx_ivar_keep for the same L, X, Z (W == NULL: exactly gpx_ivar_grad) */
int gpx_ivar_grad_w(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                    const gpx_mat* Z, const double* noise_deriv, const gpx_mat* W, double* grad);
/* ... for the design points from r0 (a multiple of 128) on only: the batch loop pins the earlier ones by equal bounds
 * (experimentalDesign.py:719-724).  Squared exponential or Matern, homoscedastic; grad: (N - r0) x d.  2 (N - r0) N M flops instead of 2 N^2 M. */
int gpx_ivar_grad_rows(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                       const gpx_mat* Z, const gpx_mat* W, int64_t r0, double* grad);
/* out[(j*d + l) * M + m] = d var(z_m) / d X[j][l]  (GP.evaluateVarianceDerivative, gp.py:282-341; host, (N*d) x M).
 * eval_bias (host N, nullable) / dk_bias (host N x d, nullable): the terms of gp.py:318-320 -- noise(x_j) added to
 * k(x_j, z_m) and noise'(x_j) subtracted from -dk(z_m, x_j)/dz for every m -- which the reference applies when the WHOLE
 * evaluation set coincides with training point j; the caller decides (rows of zeros otherwise). */
int gpx_var_grad(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                 const gpx_mat* Z, const double* noise_deriv, const double* eval_bias, const double* dk_bias,
                 double* out);
/* out[m*d + l] = d var(z_m) / d z_m[l]  (GP.evaluateVarianceDerivWRTnewpt, gp.py:261-280; host, M*d) */
int gpx_var_grad_newpt(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* L, const gpx_mat* X,
                       const gpx_mat* Z, double* out);


/* out[rows] = A v for a resident matrix (covTimesV, gp_kernel_utilities.py:107-143: the Nystrom operator application) */
int gpx_matvec(gpx_ctx* ctx, const gpx_mat* A, const double* v, double* out);

/* ---- f4: FITC sparse approximation (gp.py:182-210, 401-426; gp_kernel_utilities.py:70-104) ---------------------
 * Inducing points S (nu x d, a subset of the nodes in the reference: np.random.permutation, gp.py:188).  The model keeps
 * chol(Quu), Kuf, G = diag(K - Q) and chol(Quu + Kuf G^-1 Kfu) on the device; no N x N matrix is formed. */
typedef struct gpx_fitc gpx_fitc;
int gpx_fitc_fit(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                 double noise, gpx_fitc** out);
int gpx_fitc_free(gpx_ctx* ctx, gpx_fitc* f);
int gpx_fitc_shape(const gpx_fitc* f, int64_t* n, int64_t* nu);
/* coeff = P y with the Woodbury precision (GP.train, gp.py:100-101); quad (nullable) = y^T P y */
int gpx_fitc_solve(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* coeff, double* quad);
/* log det(Q + G) (loglikeParams, gp.py:434) */
int gpx_fitc_logdet(gpx_ctx* ctx, const gpx_fitc* f, double* out);
/* *logp = the FITC log marginal likelihood of y (as gpx_fitc_solve + gpx_fitc_logdet give it: -1/2 y^T P y - 1/2 log det(Q + G)
 * - N/2 log 2 pi; nullable) and grad[nlen + 2] = its derivatives in gpx_lml_grad's order [lengths..., signalSize, noise]; the
 * reference has no runnable counterpart.  Kernel entries are TRUE derivatives and the noise entry is the derivative w.r.t. the
 * noise VARIANCE (no factor 2 * noise), the convention of gpx_loo_grad.  (kind, d, hyp) = the kernel the model was fitted with,
 * X and S its nodes and inducing points (anything else is an argument error); squared exponential and isotropic Matern only, as
 * gpx_lml_grad (Mehler is an argument error).  y: host, N.  The model is not modified.  The 1e-12 guard that the model adds to g
 * before inverting it is IGNORED by the derivative (Gi is taken as 1 / g; the value's sum log g has no guard either).
 * With B = Quu^-1 Kuf, alpha = P y, M = alpha alpha^T - P (never formed), m = diag M:  R = B (M - diag m),  T = R B^T,
 *     dL/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) + sum_i m_i dk(x_i,x_i) ],    dL/d noise = 1/2 [ sum m - tr T ].
 * Two nu x nu x N triangular solves and three nu x nu x N products: ~8 nu^2 N flops (the fit: ~4 nu^2 N), plus one tiled pass
 * that recomputes the kernel derivatives from the coordinates (no derivative matrix is stored).  Memory: three nu x N and two
 * nu x nu work matrices; nothing N x N.  All reductions run in a fixed order: two calls agree bit for bit. */
int gpx_fitc_lml_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                      const gpx_mat* S, const double* y, double* logp, double* grad);
/* As gpx_fitc_lml_grad, plus grad_s[u*d + l] = dL / dS[u][l] (host, nu x d; required): the gradient of the FITC log marginal
 * likelihood w.r.t. the inducing-point LOCATIONS (the pseudo-inputs of Snelson & Ghahramani; S need not be a subset of X).  logp
 * and grad are nullable; every other rule of gpx_fitc_lml_grad applies, and logp / grad hold the same bits it returns.  Moving
 * s_u changes row u of Kuf and row and column u of K(S,S) only; the diagonals k(s_u,s_u), k(x_i,x_i) and the nugget inside Quu do
 * not depend on S.  With the R (nu x N) and T = R B^T (nu x nu, symmetric) of gpx_fitc_lml_grad:
 *     dL/ds_u[l] = sum_i R[u][i] dk(s_u, x_i)/ds_u[l] - sum_v 1/2 (T[u][v] + T[v][u]) dk(s_u, s_v)/ds_u[l]
 * dk(u, p)/du is the TRUE derivative of gpx_acq_grad:  SE -(u_l - p_l) / cl_l^2 k;  Matern 3/2 -sig (3 / rho^2) e^-t (u - p);
 * Matern 5/2 -sig (5 / (3 rho^2)) (1 + t) e^-t (u - p).  It is zero and smooth at u = p: coincident points (S a subset of X) need
 * no special case, and the v = u term vanishes.  No further solve or product: one row-wise weighted pass over the nu x N and the
 * nu x nu pairs from the coordinates; scratch grows by its per-segment partial sums (segments x nu x d, the segment count a
 * function of the shape only) and the nu x d result.  Fixed-order reductions, no atomics: two calls agree bit for bit. */
int gpx_fitc_lml_grad_inducing(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                               const gpx_mat* S, const double* y, double* logp, double* grad, double* grad_s);
/* Leave-one-out cross-validation of a FITC model (none in the reference).  It is taken UNDER THE MODEL'S OWN PRIOR of the
 * observations, N(0, Kt) with Kt = Q + G -- the covariance whose likelihood gpx_fitc_solve + gpx_fitc_logdet score, with the Woodbury
 * precision P the model holds: p(y_i | y_-i) is the Gaussian conditional of N(0, Kt), i.e. FITC refitted on X \ {x_i} with the
 * same inducing points and y_i predicted through the model's own cross-covariance Q.  It is NOT gpx_fitc_posterior at x_i after a
 * fit without x_i: that call keeps the reference's convention, the TRUE k(z, X) against P.
 * With Gi = diag(ginv), Y = La^-1 Ks (nu x N), ssq_i = |Y[:, i]|^2 (P = Gi - Y^T Y), alpha = P y:
 *     p_i = P_ii = ginv_i - ssq_i,     mean_i = y_i - alpha_i / p_i,     var_i = 1 / p_i
 *     L_LOO = sum_i [ 1/2 log p_i - alpha_i^2 / (2 p_i) ] - N/2 log 2 pi
 * mean / var: host N, each nullable; *logp (nullable) = L_LOO, its terms formed and summed as gpx_loo does.  Needs the fitted model
 * only, so every kernel is accepted, Mehler included.  One nu x nu x N triangular solve (Y), its column sums of squares and alpha;
 * no other product: ~nu^2 N flops, one nu x N work matrix beside the solve's consumed copy of Ks, nothing N x N.  The model is
 * not modified.  Where some p_i <= 0 or is not finite the call does what gpx_loo does: no test, it succeeds, and that point's
 * entries and *logp come out as the arithmetic gives them (NaN from log p_i <= 0, a negative var_i). */
int gpx_fitc_loo(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* mean, double* var, double* logp);
/* *logp (nullable) = L_LOO, the same bits as gpx_fitc_loo's, and grad[nlen + 2] = its derivatives in gpx_lml_grad's order
 * [lengths..., signalSize, noise]: TRUE derivatives, the noise entry w.r.t. the noise VARIANCE (no factor 2 * noise) -- the
 * convention of gpx_loo_grad and gpx_fitc_lml_grad, whose argument rules apply unchanged: (kind, d, hyp) = the kernel the model
 * was fitted with, X and S its nodes and inducing points (anything else is an argument error), squared exponential and isotropic
 * Matern only (Mehler is an argument error), the 1e-12 guard on g IGNORED by the derivative.  dL = 1/2 tr(M dKt) with the symmetric
 * M (N x N, never formed); B = Quu^-1 Kuf:
 *     r = alpha / p,   b = P r,   c_i = (1 + alpha_i^2 / p_i) / p_i,   C = diag(c)      (c is twice gpx_loo_grad's 1/2 (1 + ..))
 *     M = alpha b^T + b alpha^T - P C P,      m = diag M = 2 alpha o b - diag(P C P)
 *     R = B (M - diag m)  (nu x N),   T = R B^T  (nu x nu)
 *     dL/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) + sum_i m_i dk(x_i,x_i) ],    dL/d noise = 1/2 [ sum m - tr T ]
 * -- the last line, and everything from R on, is gpx_fitc_lml_grad's own code.  Upstream of R only nu-sized objects:
 *     C1 = B Y^T,   H = Y C Y^T,   C2 = (B diag(ginv o c)) Y^T - C1 H                                        (nu x nu each)
 *     B P C P       = B diag(ginv^2 o c) - (C1 Y) diag(c o ginv) - C2 Y
 *     diag(P C P)_i = ginv_i^2 c_i - 2 ginv_i c_i ssq_i + sum_k Y_ki (H Y)_ki
 *     B alpha b^T + B b alpha^T: two row reductions and a rank-2 update
 * The two solves of gpx_fitc_lml_grad and seven nu x nu x N products (H, H Y, C1, the scaled B Y^T, C2 Y, C1 (Y diag(c o ginv))
 * subtracted into C2 Y's result, T) plus one nu^3 (C1 H): ~16 nu^2 N flops, about twice gpx_fitc_lml_grad.  Memory: THREE nu x N
 * and THREE nu x nu work matrices (H shares T's storage), vectors and the per-tile partial sums; nothing N x N.  The model is not
 * modified.  p_i <= 0: as gpx_fitc_loo, no test.  All reductions run in a fixed order, no atomics: two calls agree bit for bit. */
int gpx_fitc_loo_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                      const gpx_mat* S, const double* y, double* logp, double* grad);
/* GP.evaluate / evaluateVariance with the FITC precision (gp.py:132-145, 246-255): mean (nullable; needs coeff) and the
 * SIGNED variance (nullable) at the M points of Z */
int gpx_fitc_posterior(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* X, const double* coeff, const gpx_mat* Z,
                       double* mean, double* var);
/* dense Q + G and P (host n x n, each nullable): the covarianceMatrix / precisionMatrix attributes (gp.py:200-206) */
int gpx_fitc_dense(gpx_ctx* ctx, const gpx_fitc* f, double* cov, double* prec);
/* GP.evaluateVarianceDerivative / evaluateVarianceDerivWRTnewpt on a FITC model: the reference computes both from whatever
 * `precisionMatrix` holds (gp.py:275, 322), for FITC the Woodbury precision of gp.py:204-206.  Same outputs and optional
 * arguments as gpx_var_grad / gpx_var_grad_newpt; (kind, d, hyp) = the kernel the model was fitted with. */
int gpx_fitc_var_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                      const gpx_mat* Z, const double* noise_deriv, const double* eval_bias, const double* dk_bias, double* out);
int gpx_fitc_var_grad_newpt(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X,
                            const gpx_mat* Z, double* out);

/* ---- VFE: Titsias' variational free energy on the same inducing-point model (none in the reference) --------------------------
 * A lower bound on the exact log marginal likelihood that never decreases when an inducing point is added -- the objective to
 * trust with the joint search over hyper-parameters, noise and inducing-point locations, where FITC's likelihood rewards
 * piled-up inducing points and a collapsing noise.  Conventions are this library's: the inducing block keeps the nugget exactly
 * as the FITC model does, Quu = K(S,S) + noise I (Titsias' construction with inducing variables u = f(S) + eps, eps ~ N(0, noise I),
 * so the bound property holds unchanged), Kuf = K(S,X), B = Quu^-1 Kuf, Q = Kfu B.  With Kt = Q + noise I, P = Kt^-1, alpha = P y
 * and q_i = Q_ii:
 *     F = -1/2 y^T alpha - 1/2 log det Kt - N/2 log 2 pi - (1 / (2 noise)) sum_i (k(x_i,x_i) - q_i)
 * A VFE model is a gpx_fitc whose G is noise I (g = noise, ginv = 1 / noise exactly, no 1e-12 guard), flagged as such, with one
 * more scalar trres = sum_i (k_ii - q_i) reduced in a fixed order at fit time.  gpx_fitc_solve, gpx_fitc_logdet, gpx_fitc_dense,
 * gpx_fitc_shape and gpx_fitc_free work on it as they are.  The FITC-only entries (gpx_fitc_lml_grad*, gpx_fitc_loo*,
 * gpx_fitc_posterior, gpx_fitc_var_grad*) refuse a VFE model with an argument error that names the call to use, and the gpx_vfe_*
 * entries refuse a FITC model the same way.  noise <= 0 is an argument error.
 * Gradient.  M = alpha alpha^T - P (never formed), Y = La^-1 Ks, P = I / noise - Y^T Y, ssq_i = |Y[:, i]|^2:
 *     R = B (M + I / noise) = (B alpha) alpha^T + (B Y^T) Y      (nu x N; no diagonal correction, unlike FITC),      T = R B^T
 *     dF/d theta = 1/2 [ 2 sum R o dKuf - sum T o dK(S,S) + sum_i m_i dk(x_i,x_i) ]    with m_i = -1 / noise
 *     dF/d noise = 1/2 [ tr M - tr T ] + trres / (2 noise^2),     tr M = sum_i (alpha_i^2 - 1 / noise + ssq_i)
 *     dF/ds_u    = sum_i R[u][i] dk(s_u,x_i)/ds_u - sum_v 1/2 (T[u][v] + T[v][u]) dk(s_u,s_v)/ds_u
 * -- the first and third lines are gpx_fitc_lml_grad's own code from R on.  The same three nu x nu x N products and two solves as
 * gpx_fitc_lml_grad, one element-wise pass fewer.  Fixed-order reductions, no atomics: two calls agree bit for bit.
 * Predictor: the optimal variational posterior of the latent f at z, with k_u = K(S, z) -- NOT gpx_fitc_posterior's convention (the
 * reference's true k(z, X) against the Woodbury precision, O(nu N) per point); O(nu^2) per point, nothing N x M is formed:
 *     mean(z) = k_u^T beta_u,   beta_u = B alpha = Quu^-1 (Kuf alpha);      var(z) = k(z,z) - |Lu^-1 k_u|^2 + |La^-1 k_u|^2  (>= 0 in exact arithmetic) */
/* a gpx_fitc whose G is noise I, flagged as a VFE model; noise <= 0 is an argument error */
int gpx_vfe_fit(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S, double noise,
                gpx_fitc** out);
/* *bound = F (the solve, the two log-determinants and trres; B is not formed).  y: host, N. */
int gpx_vfe_bound(gpx_ctx* ctx, const gpx_fitc* f, const double* y, double* bound);
/* *bound = F (the bits gpx_vfe_bound returns), grad[nlen + 2] = its TRUE derivatives [lengths..., signalSize, noise VARIANCE] (no
 * factor 2 * noise), grad_s[u*d + l] = dF / dS[u][l] (host, nu x d): each nullable, at least one given.  The argument rules of
 * gpx_fitc_lml_grad: (kind, d, hyp) = the kernel the model was fitted with, X and S its nodes and inducing points, squared
 * exponential and isotropic Matern only (Mehler is an argument error).  The model is not modified. */
int gpx_vfe_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                 const double* y, double* bound, double* grad, double* grad_s);
/* mean (nullable; needs coeff = alpha from gpx_fitc_solve, host N) and the SIGNED variance (nullable) at the M points of Z; every
 * kernel kind.  S = the model's inducing points.  Chunked over Z under GPX_CROSS_BYTES (a nu x chunk matrix), a point's values the
 * same bits whatever the chunking; one device-to-host copy per output per chunk. */
int gpx_vfe_posterior(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double* mean,
                      double* var);

/* ---- Bayesian-optimisation costs on a VFE model ----------------------------------------------------------------------------------
 * gpx_acq / gpx_acq_grad / gpx_acq_batch for the model gpx_vfe_fit built: the kernel parameters are the model's (no (kind, d, hyp)
 * arguments), S its inducing points, coeff = alpha from gpx_fitc_solve (host N, required).  Notation: Quu = K(S,S) + noise I =
 * Lu Lu^T, A = Quu + Kuf Kfu / noise = La La^T, beta_u = Quu^-1 Kuf alpha, k_u(z) = K(S, z).  A FITC model is refused with an
 * argument error (VFE models only); every kernel kind is accepted except where stated.
 *
 * gpx_vfe_acq: per chunk of Z the mean and the signed variance exactly as gpx_vfe_posterior forms them, then gpx_acq's own cost
 * formula, epilogue and arg-min.  cost / best / best_cost: as gpx_acq (each nullable; *best the FIRST arg-min among the non-NaN
 * costs, -1 when all are NaN, whatever the chunking under GPX_CROSS_BYTES). */
int gpx_vfe_acq(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                double* cost, int64_t* best, double* best_cost);
/* grad (host M x d): grad[m*d + l] = d cost_m / d z_m[l], the true derivative of gpx_vfe_acq's values; cost (host M, nullable) holds
 * gpx_vfe_acq's bits.  With a = dA/dmu, b = dA/dvar (gpx_acq_grad's table) and k(z, z) constant:
 *     gamma(z) = Quu^-1 k_u(z) - A^-1 k_u(z)                                   (a nu-vector per candidate)
 *     grad_z A = sum_u dk(z, s_u)/dz (a beta_u[u] - 2 b gamma(z)[u])
 * NaN rows where var == 0 exactly.  Per chunk the two forward solves of the values are reused, each gets its backward sweep
 * (Lu^-T, La^-T: nu^2 chunk flops each), and ONE pass over the nu inducing points per candidate takes the difference of the two
 * and the weighted sum.  Squared exponential, Matern 3/2 and 5/2; a Mehler model is an argument error. */
int gpx_vfe_acq_grad(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, int acq, double param,
                     double* cost, double* grad);
/* q-point batch selection on a VFE model whose inducing points and hyper-parameters stay fixed: the loop "cost on the grown data;
 * bestCandidate; append the pick with its believed value", where every refit is gpx_vfe_fit on X + picks with the SAME S.  One
 * more observation at c_s changes A to A + k_u(c_s) k_u(c_s)^T / noise and nothing else, so the refit is a rank-one recurrence in
 * the inducing space.  Resident state: Wa = La^-1 K(S, C) (nu x M, the only matrix kept), mu_j = k_u(c_j)^T beta_u,
 * r_j = k(c_j, c_j) - |Lu^-1 k_u(c_j)|^2 (fixed for the whole call; the Lu solve is transient), t_j = |Wa[:, j]|^2, the rows U[t].
 * Pick t = 0 .. q-1:
 *     v_j = r_j + t_j;  cost_j = A(mu_j, v_j; param), NaN for the candidates already picked;  s = first arg-min among the non-NaN costs
 *     delta = noise + t_s          (NOT v_s + noise: the observation enters through the inducing variables only)
 *     y_s = mu_s (GPX_LIE_BELIEVER) or lie_value (GPX_LIE_CONSTANT)
 *     u_j = (Wa[:, s]^T Wa[:, j] - sum_{r<t} U[r][s] U[r][j]) / sqrt(delta);   U[t] = u
 *     mu_j += u_j (y_s - mu_s) / sqrt(delta);   t_j -= u_j^2;   param = max(param, y_s) when track_best != 0
 * delta >= noise > 0: gpx_acq_batch's tiny-pivot rule has no counterpart.  Per pick one pass over Wa (8 nu M bytes); all
 * reductions in a fixed order (two runs agree bit for bit); row 0 of all_costs holds gpx_vfe_acq's bits.  Outputs and errors as
 * gpx_acq_batch. */
int gpx_vfe_acq_batch(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* C, int acq, double param,
                      int track_best, int lie, double lie_value, int64_t q, int64_t* out_idx, double* out_cost, double* out_lie,
                      double* all_costs);
/* gpx_acq_mes / gpx_acq_mes_grad / gpx_acq_mes_batch on a VFE model: the sequences of the three calls above with the MES cost on
 * ystar (host, K doubles) and sign; rules, outputs and errors as theirs (a FITC model is refused; gradients for the stationary
 * kernels only; the costs of the gradient call and row 0 of all_costs hold gpx_vfe_acq_mes's bits). */
int gpx_vfe_acq_mes(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, const double* ystar,
                    int64_t K, int sign, double* cost, int64_t* best, double* best_cost);
int gpx_vfe_acq_mes_grad(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, const double* ystar,
                         int64_t K, int sign, double* cost, double* grad);
int gpx_vfe_acq_mes_batch(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* C,
                          const double* ystar, int64_t K, int sign, int lie, double lie_value, int64_t q, int64_t* out_idx,
                          double* out_cost, double* out_lie, double* all_costs);

/* ---- posterior sampling on a VFE model --------------------------------------------------------------------------------------------
 * The two samplers above for the model gpx_vfe_fit built; the kernel parameters are the model's, S its inducing points, coeff =
 * alpha from gpx_fitc_solve (host N, required); notation as for gpx_vfe_acq.  The samplers' two rules hold (no random numbers on
 * the device; a nugget and the pivot policy (0, report)).  A FITC model is refused with an argument error.
 *
 * gpx_vfe_paths_create: DECOUPLED paths of the variational posterior (Wilson et al. 2020): Matheron's rule on (f, u) with the
 *   inducing variables u = f(S) + eps drawn from the optimal q(u) = N(Quu beta_u, Quu A^-1 Quu),
 *       f_s(z) = sum_j c_sj cos(omega_j . z + b_j) + sum_u v_su k(s_u, z),       c = sqrt(2 signalSize / nfeat) w
 *       V      = 1 beta_u^T - (F~_S + eps_u) Quu^-1 + xi_q La^-1                 (nPaths x nu;  F~_S[s][u] = f~_s(s_u))
 *   omega, phase, nfeat, w: as gpx_paths_create.  eps_u = sqrt(noise) Xi1 (the nugget draw of the inducing variables) and xi_q =
 *   Xi2 (the draw of q(u); row s of xi_q La^-1 is (La^-T xi2_s)^T): host nPaths x nu, each nullable (NULL = zeros), Xi1, Xi2
 *   standard normal.  Zero draws give the predictor's mean; the exact prior in place of the features would give the predictor's
 *   covariance (gpx_vfe_posterior_cov); with nfeat features the covariance at Z is A_J (Phi_J Phi_J^T) A_J^T + noise G_u G_u^T +
 *   K_zu A^-1 K_uz with G_u = K_zu Quu^-1, A_J = [I, -G_u] and Phi_J the features at (Z; S).  The result is an ordinary gpx_paths
 *   whose point block holds S and V: gpx_paths_eval, _grad, _coeff (nPaths x nu), _shape (n = nu) and _free serve it unchanged, with
 *   every bit-for-bit property they have.  The build runs on the device for all paths at once: f~ at S by gpx_paths_eval's own
 *   kernel, two blocked right solves against Lu and one against La (O(nu^2) per path; nothing of size N but beta_u's reduction).
 *   Stationary kernels only (a Mehler model is an argument error); nfeat < 1 and nPaths < 1 are argument errors.
 * gpx_vfe_posterior_cov: cov (host M x M) = (K(Z,Z) - Wu^T Wu) + Wa^T Wa with Wu = Lu^-1 K(S,Z), Wa = La^-1 K(S,Z), the full
 *   covariance of the variational posterior; its diagonal is gpx_vfe_posterior's variance up to the order of summation.  Every
 *   kernel kind; nothing N x M is formed; no chunking over Z.
 * gpx_vfe_psampler_create: the exact joint sampler at the M points of Z: the mean holds the bits gpx_vfe_posterior returns, C is
 *   formed as by gpx_vfe_posterior_cov, and the nugget, the factorisation, its refinement step and the pivot report are
 *   gpx_psampler_create's own, and its tail with one addition: the residual max |Chat - F F^T|_ij / sqrt(Chat_ii Chat_jj) is
 *   measured on the device after the refinement step, and while it is above 4 (M + 1) u the step is repeated (four more times at
 *   most) -- many points on a line under a squared exponential need it; a covariance that does not is left with one step.
 *   gpx_psampler_draw, _argbest, _shape and _free serve the result.  Every kernel kind.
 * gpx_vfe_acq_qei: gpx_acq_qei on the variational posterior: Monte-Carlo joint expected improvement of B batches of q points (Zb:
 *   (B q) x d, consecutive q rows one batch; xi: host nS x q, common to all batches).  mu_b holds the bits gpx_vfe_posterior
 *   returns; C_b = (k(z_i, z_j) - su_ij) + sa_ij with su = Wu_b^T Wu_b, sa = Wa_b^T Wa_b over the nu inducing rows, in the order of
 *   gpx_vfe_posterior's variance and each sum by gpx_acq_qei's rule (row slices, one fma chain per slice in ascending row, slices
 *   added in order); from the nugget on the kernel is gpx_acq_qei's: F_b = chol(C_b + nugget I), a pivot <= 0 gives cost NaN and is
 *   counted in *n_bad, a point repeated bit for bit is certain to meet one when the nugget is 0.  cost, best, best_cost, n_bad:
 *   nullable, as gpx_acq_qei; permuting the batches permutes the costs bit for bit, whatever the chunking (whole batches under
 *   GPX_CROSS_BYTES).  A batch costs O(nu q^2).  q outside 1 .. GPX_QEI_MAX_Q, rows of Zb no positive multiple of q, nS < 1 and a
 *   negative nugget are argument errors.  Every kernel kind. */
int gpx_vfe_paths_create(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const double* omega,
                         const double* phase, int64_t nfeat, const double* w, const double* eps_u, const double* xi_q,
                         int64_t nPaths, gpx_paths** out);
int gpx_vfe_posterior_cov(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* cov);
int gpx_vfe_psampler_create(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Z, double nugget,
                            gpx_psampler** out);
int gpx_vfe_acq_qei(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const double* coeff, const gpx_mat* Zb, int64_t q,
                    const double* xi, int64_t nS, double fBest, double nugget, double* cost, int64_t* best, double* best_cost,
                    int64_t* n_bad);

/* ---- IVAR design on a VFE model, in the inducing space (none in the reference) -----------------------------------------------------
 * With k_u(.) = K(S, .), Quu = K(S,S) + noise I = Lu Lu^T and, for design points X, A = Quu + sum_i k_u(x_i) k_u(x_i)^T / noise =
 * La La^T, the variational variance is var(z) = k(z,z) - k_u(z)^T Quu^-1 k_u(z) + k_u(z)^T A^-1 k_u(z): the design enters through the
 * nu x nu matrix A only and the M Monte-Carlo points Z through one Gram matrix Gz = K(S,Z) K(Z,S) / M.  With kbar = mean_z k(z,z):
 *     IVAR(X)       = kbar - tr(Lu^-1 Gz Lu^-T) + tr(La^-1 Gz La^-T)                                   (signed, not clamped)
 *     dIVAR/dx_i[l] = -(2 / noise) sum_u H[u][i] dk(x_i, s_u)/dx_i[l],      H = A^-1 Gz A^-1 K(S,X)
 * dk is the TRUE derivative (the table of gpx_fitc_lml_grad_inducing and gpx_vfe_acq_grad; for the squared exponential too: no doubled
 * signalSize).  The inducing points are constants of the function, also where a design point coincides with one (the derivative of
 * every radial kernel is zero and smooth there).  No observations are involved: the state is built from the kernel, S, the noise and
 * Z alone.
 * gpx_vfe_design_create: Lu, Gz, A0 = Quu stay on the device (three nu x nu matrices) with kbar and c0 = tr(Lu^-1 Gz Lu^-T).  Gz is
 *   accumulated over chunks of Z under GPX_CROSS_BYTES (one nu x chunk matrix, as gpx_vfe_posterior), the chunks added in index order,
 *   then scaled and mirrored: 2 nu^2 M flops; another chunking may differ in the last bits of Gz (another summation order).  Every
 *   kernel kind.  noise <= 0, M < 1, nu < 1: argument errors.  S is copied; Z is not kept.
 * gpx_vfe_design_pin: REPLACES the pinned set (it does not accumulate): A0 = Quu + K(S,Xp) K(Xp,S) / noise, 2 nu^2 p flops.  Xp NULL or
 *   of 0 rows: nothing pinned.
 * gpx_vfe_design_eval: the cost of (pinned points + the b >= 1 free points Xf) and, when grad != NULL (host b x d, grad[i*d + l]), its
 *   gradient w.r.t. Xf.  A = A0 + P P^T / noise with P = K(S,Xf), La = chol(A) (gpx_potrf's path and pivot policy: a bad pivot is
 *   returned > 0), Y1 = La^-1 Gz La^-T, cost = kbar - c0 + tr Y1; gradient: V = La^-1 P, H = La^-T (Y1 V) -- A^-1 Gz A^-1 is not formed --
 *   and one row pass over the b x nu pairs.  nu^3 / 3 + 2 nu^3 + 2 nu^2 b flops, with the gradient 6 nu^2 b + (6 d + 25) b nu more:
 *   independent of M and of the pinned count.  Work memory: two nu x nu matrices (three from order 2048) and two nu x b ones.  The
 *   gradient exists for the squared exponential and the Materns; on a Mehler state grad != NULL is an argument error that names the
 *   kernel (the cost works).  The state is not modified.
 * Fixed-order reductions, no atomics: two calls with the same arguments return the same bits. */
typedef struct gpx_vfe_design gpx_vfe_design;
int gpx_vfe_design_create(gpx_ctx* ctx, int kind, int d, const double* hyp, int nhyp, const gpx_mat* S, double noise, const gpx_mat* Z,
                          gpx_vfe_design** out);
int gpx_vfe_design_pin(gpx_ctx* ctx, gpx_vfe_design* ds, const gpx_mat* Xp);
int gpx_vfe_design_eval(gpx_ctx* ctx, const gpx_vfe_design* ds, const gpx_mat* Xf, double* cost, double* grad);
/* each output nullable: inducing points, Monte-Carlo points, points currently pinned */
int gpx_vfe_design_shape(const gpx_vfe_design* ds, int64_t* nu, int64_t* m, int64_t* pinned);
int gpx_vfe_design_free(gpx_ctx* ctx, gpx_vfe_design* ds);
/* Point-wise derivatives of the variational variance of a fitted VFE model (a FITC model is refused with the call to use instead:
 * gpx_fitc_var_grad / gpx_fitc_var_grad_newpt); squared exponential and Materns only; TRUE derivatives, S held fixed.
 * gpx_vfe_var_grad: out (host, (N d) x M): out[(k*d + l)*M + j] = d var(z_j)/dx_k[l] = -(2 / noise) E[k][j] D_l[k][j] with C = A^-1 K(S,Z)
 *   (two sweeps with the model's La), E = K(X,S) C, D_l = (dK(X,S)/dx[l]) C.  (kind, d, hyp), X, S: the model's, as gpx_vfe_grad.  Chunked
 *   over Z under GPX_CROSS_BYTES; (d + 1) products of 2 N nu chunk flops per chunk; bound by the copy of its 8 N d M bytes to the host,
 *   as gpx_var_grad.
 * gpx_vfe_var_grad_newpt: out (host, M x d): out[j*d + l] = d var(z_j)/dz_j[l] = -2 sum_u dk(z_j,s_u)/dz_j[l] gamma(z_j)[u], gamma =
 *   Quu^-1 k_u - A^-1 k_u: gpx_vfe_acq_grad's own sequence with (a, b) = (0, 1). */
int gpx_vfe_var_grad(gpx_ctx* ctx, const gpx_fitc* f, int kind, int d, const double* hyp, int nhyp, const gpx_mat* X, const gpx_mat* S,
                     const gpx_mat* Z, double* out);
int gpx_vfe_var_grad_newpt(gpx_ctx* ctx, const gpx_fitc* f, const gpx_mat* S, const gpx_mat* Z, double* out);

/* ---- measurement ------------------------------------------------------------------------------- */
/* when enabled every kernel launch of a class is bracketed by HIP events on the launch stream */
int gpx_profile_enable(gpx_ctx* ctx, int on);
int gpx_profile_reset(gpx_ctx* ctx);
/* sums since reset: launches, elapsed ms (HIP events), algorithmic flops and bytes */
int gpx_profile_get(gpx_ctx* ctx, int prof_class, int64_t* launches, double* ms, double* flops, double* bytes);

/* Test hooks (gpx_dbg_*: kernel-level entry points, allocator guards, schedule replays) are declared in gpx_debug.h; they are
 * exported by the same library but are not part of the drop-in ABI. */

#ifdef __cplusplus
}
#endif
#endif /* GPX_H */
