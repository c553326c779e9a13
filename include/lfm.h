/*
 * lfm.h — C-ABI of the MI355X-native SIM latent-force-model hot path.
 *
 * This is the drop-in boundary for the GPJax hot path of wejpurvis/DIS_project:
 * the SIM multi-output covariance (src/model.py:152-414) and the Cholesky-based
 * log marginal likelihood (src/objectives.py:21-78 -> gpjax 0.8.2
 * GaussianDistribution.log_prob). The reference is pure Python/JAX and has no
 * FFI of its own; each entry point below names the reference interface it
 * replaces. Plain pointers and sizes only (no framework types).
 *
 * Conventions
 *   - x arrays are N x 3 row-major fp64: (time, gene index, flag), the layout of
 *     dataset_3d (src/dataset.py:358-399).
 *   - All host buffers are owned by the caller and are not retained after return.
 *     Every call is synchronous at return unless its name ends in _async.
 *   - Device workspace (the Mp x Mp factor, tables, scratch) is owned by the ctx,
 *     grown on demand and reused. A ctx is bound to one device and is NOT
 *     thread-safe: create one ctx per device per host thread.
 *   - Return value: LFM_OK (0) or an LFM_E_* code; lfm_last_error() has the text.
 *     LFM_E_NOT_PD mirrors JAX's silent NaN on a failed Cholesky: the scalar
 *     output is set to NaN and the failing pivot index is in lfm_last_error().
 *     LFM_E_TIMEOUT is NOT a property of the input: a bounded device-side wait of the
 *     factorisation's cross-stream hand-off ran out (e.g. a tool serialised the two
 *     streams' dispatches) and the in-call schedule-1 re-run (lfm_ctx_fallbacks) was
 *     disabled or ran out too. The result is invalid; callers must raise, never map it to NaN.
 *   - Diagnostics (rate / layout probes, phase stamps) are declared in lfm_diag.h.
 */
#ifndef LFM_H
#define LFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFM_ABI_VERSION 5

enum {
  LFM_OK = 0,
  LFM_E_ARG = 1,    /* bad shape / pointer / value                        */
  LFM_E_HIP = 2,    /* HIP runtime error (text in lfm_last_error)          */
  LFM_E_NOT_PD = 3, /* Cholesky pivot <= 0 or NaN; scalar result is NaN    */
  LFM_E_OOM = 4,    /* device allocation failed                            */
  LFM_E_RCCL = 5,   /* RCCL not loadable / collective failed               */
  LFM_E_STATE = 6,  /* call out of order (e.g. farm not initialised)       */
  LFM_E_TIMEOUT = 7 /* device-side wait ran out: result invalid (not NaN)  */
};

/* gram / cross-covariance output selection */
enum { LFM_UPLO_FULL = 0, LFM_UPLO_LOWER = 1 };

typedef struct lfm_ctx lfm_ctx;

/*
 * Constrained hyperparameters of ExactLFM (src/model.py:64-121).
 *   true_d / true_s / true_b : [num_genes] decay D, sensitivity S, basal B
 *   l                        : lengthscale (model.py:111-121)
 *   obs_stddev               : observation std-dev; sigma^2 = obs_stddev^2 (objectives.py:66)
 *   jitter                   : static jitter added to the gram diagonal (objectives.py:71)
 * Gene indices read from x[:,1] are truncated toward zero, negative ones wrap by
 * +num_genes and the result is clamped to [0, num_genes-1] (JAX gather semantics).
 */
typedef struct {
  int64_t num_genes;
  const double* true_d;
  const double* true_s;
  const double* true_b;
  double l;
  double obs_stddev;
  double jitter;
} lfm_hyp;

/* One independent marginal-likelihood problem of a batch (restart / ablation). */
typedef struct {
  const double* x; /* [n x 3] host */
  const double* y; /* [n]     host */
  int64_t n;
  lfm_hyp hyp;
} lfm_problem;

/* Per-kernel-class timing, filled when profiling is on (HIP events on the stream each
 * launch runs on). flops / bytes are ALGORITHMIC: the blocked Cholesky's work on the
 * unpadded (n + 1)-row augmented matrix (N^3 / 3 over a factorisation), not what the
 * padded tiles issue; issued_flops is the MFMA work the launches actually issue. */
typedef struct {
  char name[32];
  int64_t launches;
  double total_ms;     /* sum of per-launch HIP-event durations              */
  double flops;        /* algorithmic flops over all launches                */
  double bytes;        /* algorithmic HBM bytes over all launches            */
  double issued_flops; /* flops issued (padded tiles, inverse-based solves)  */
} lfm_kstat;

/* ---------------------------------------------------------------- context */
int lfm_abi_version(void);
int lfm_device_count(int* out);
int lfm_ctx_create(int device, lfm_ctx** out);
void lfm_ctx_destroy(lfm_ctx* ctx);
const char* lfm_last_error(const lfm_ctx* ctx);
int lfm_ctx_synchronize(lfm_ctx* ctx);
/* Block size of the blocked Cholesky: 128 (the only size built; 0 restores it). */
int lfm_ctx_set_block(lfm_ctx* ctx, int nb);
/* Factorisation schedule of this context's MLL / gradient:
 *   3  CU-partitioned stream pair: the factor chain on LFM_SIDE_CUS reserved CUs, the bulk on
 *      the rest. Lowest latency of ONE evaluation. Single tenant: the chain needs all of its
 *      workgroups resident, so a schedule-3 factorisation holds the device's lock exclusively
 *      (threads and processes: a per-device readers-writer lock plus flock on
 *      $TMPDIR/lfm_gpu_<PCI bus id>.lock); other GPU work of the library holds it shared.
 *      Concurrent callers wait their turn; results do not depend on it.
 *   1  look-ahead on every CU. Several schedule-1 contexts driven from separate host threads
 *      share one GPU (shared holders): the throughput mode of a restart farm
 *      (farm.ConcurrentEvaluator).
 *   0  the process default (LFM_SCHED, else 3).
 * Schedule 3 on a context without a CU partition -> LFM_E_ARG. Replaces no reference call:
 * the reference's XLA executable has no schedule (src/objectives.py:43-46 is the whole MLL). */
int lfm_ctx_set_schedule(lfm_ctx* ctx, int schedule);
/* The schedule the next factorisation will run (1 or 3). */
int lfm_ctx_get_schedule(const lfm_ctx* ctx, int* out);
/* Schedule-3 calls of this context (MLL, gradient, log_prob) whose device-side waits ran past
 * their time bound (LFM_DEVICE_WAIT_MS, default 2000: e.g. another tenant of the GPU starved
 * the factor chain's co-resident workgroups) and that were therefore re-run on schedule 1
 * inside the same call. Their results are valid (LFM_OK); lfm_last_error names the stall after
 * such a call. LFM_S3_FALLBACK=0 disables the re-run (the call then returns LFM_E_TIMEOUT).
 * Reference behaviour preserved: trainer.py:126 never fails for scheduling reasons. */
int lfm_ctx_fallbacks(const lfm_ctx* ctx, int64_t* out);

/* --------------------------------------------- ExactLFM surface (model.py) */
/* mean_function (model.py:124-149): out[i] = (B/D)[i / (n / num_genes)] * int(x[i,2]). */
int lfm_mean_function_f64(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp,
                          double* out);

/* cross_covariance(kernel, x, x2) (model.py:372-394): out[i*ldo + j] = kernel(x[i], x2[j]),
 * the flag-switched kernel of model.py:152-195 (kxx / kff / kxf / kfx). */
int lfm_cross_covariance_f64(lfm_ctx* ctx, const double* x, int64_t n, const double* x2,
                             int64_t m, const lfm_hyp* hyp, double* out, int64_t ldo);

/* h(j, k, t1, t2) of model.py:315-365 element-wise over n tuples (gene indices clamped
 * as above); exposes the convolution term on its own for known-answer tests. */
int lfm_h_f64(lfm_ctx* ctx, const lfm_hyp* hyp, const int64_t* j, const int64_t* k,
              const double* t1, const double* t2, int64_t n, double* out);

/* gram(kernel, x) (model.py:396-414) plus diag_add on the diagonal; uplo = LFM_UPLO_FULL
 * writes the dense n x n, LFM_UPLO_LOWER computes only j <= i (the upper part of a host
 * output is zero-filled, of a device output left untouched). */
int lfm_gram_f64(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp, double diag_add,
                 int uplo, double* out, int64_t ldo);
/* fp32 gram (arithmetic and output in fp32; per-gene tables built in fp64). */
int lfm_gram_f32(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp, double diag_add,
                 int uplo, float* out, int64_t ldo);

/* --------------------------------- CustomConjMLL.step (objectives.py:21-78) */
/* out = constant * log N(y; m, K + jitter I + obs_stddev^2 I), constant = -1 if negative.
 * n >= 1 and n % num_genes == 0 (mean_function's broadcast, model.py:145-149), else
 * LFM_E_ARG; the same holds for lfm_mll_batch_f64's problems and lfm_mll_grad_f64. */
int lfm_mll_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n, const lfm_hyp* hyp,
                int negative, double* out);
/* nprob independent problems; out[p] per problem (NaN where not PD); status[p] optional. */
int lfm_mll_batch_f64(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, int negative,
                      double* out, int* status);

/* A batch of small problems registered once and evaluated many times — the replicate x
 * leave-one-gene-out ablation farm of src/notebook.py:33-75, each problem the MLL of
 * src/objectives.py:64-78. x / y of every problem (probs[p].x, .y, .n; n <= 128, n % num_genes
 * == 0) go to HBM here, once; of probs[p].hyp only num_genes is read (it fixes the layout of the
 * packed hyperparameters). The caller's x / y may be freed after the call. A batch belongs to
 * the device of the ctx that created it and, like a ctx, to one host thread at a time (its
 * pinned hyperparameter / result buffer is reused by every call). */
typedef struct lfm_batch lfm_batch;
int lfm_batch_create(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, lfm_batch** out);
int lfm_batch_destroy(lfm_batch* batch);
/* Doubles in the packed hyperparameter array: sum_p (3 G_p + 3). */
int lfm_batch_hyp_size(const lfm_batch* batch, int64_t* out);
/* Every problem's MLL (constant -1 if negative) in ONE launch, one workgroup per problem.
 * hyp packed: first, for each problem in order, true_d[G_p] true_s[G_p] true_b[G_p]; then, for
 * each problem in order, l, obs_stddev, jitter. out[p] per problem (NaN where not PD, with
 * status[p] = LFM_E_NOT_PD; status may be NULL); returns LFM_E_NOT_PD if any problem was.
 * Returns once every problem's result has landed in host memory (the kernel may still be
 * retiring: later work on the ctx's stream is ordered after it, lfm_batch_destroy waits for the
 * batch's last launch before it frees, and a fault that launch hits after the return is
 * reported as LFM_E_HIP by the batch's next value / gradient call). */
int lfm_batch_mll_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                      double* out, int* status);
/* Value and gradient of every problem's CustomConjMLL(negative).step in ONE launch, one
 * workgroup per problem — jax.value_and_grad(loss) at src/trainer.py:126 (before the
 * bijectors' chain rule, trainer.py:103), batched over the ablation problems of
 * src/notebook.py:33-75 / the p53 fit of src/main.py:59. Every problem needs n <= 127 and its
 * workgroup's LDS map (Sigma, x, y, and on the dataset_3d grid the gram and derivative tables)
 * within 160 KB, else LFM_E_ARG (lfm_mll_grad_f64 takes any n). hyp as lfm_batch_mll_f64; value[p] as its out[p] (the
 * same bits); grad packed in hyp's layout: for each problem dD[G_p] dS[G_p] dB[G_p] in order,
 * then for each problem d l, d obs_stddev, 0 (jitter is static, model.py:64). Not PD: value and
 * that problem's gradient NaN, status[p] = LFM_E_NOT_PD, returns LFM_E_NOT_PD. Deterministic (no
 * atomics: the same inputs give the same bits). */
int lfm_batch_mll_grad_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                           double* value, double* grad, int* status);

/* A resident batch of problems of any size 1 <= n <= LFM_MID_MAX_N — the same set of independent
 * (model, dataset) problems (src/notebook.py:33-75, each trained on CustomConjMLL(negative=True),
 * src/trainer.py:105-132) once they outgrow lfm_batch's one workgroup per problem: pooled
 * replicates (3 x 10 genes x 7 times, n = 210) or a 5-gene x 64-time grid (n = 320). Every
 * problem's MLL, or MLL and gradient, in a number of launches that depends on the largest n alone
 * (ceil((n + 1) / 64) + 2 for the value, four more with the gradient), not on the problem count.
 *   lfm_mbatch_create   x / y of every problem (probs[p].x, .y, .n) go to HBM once; of
 *     probs[p].hyp only num_genes is read. 1 <= n_p <= LFM_MID_MAX_N and n_p % G_p == 0, else
 *     LFM_E_ARG with a message naming the limit; sizes may be mixed freely, small ones included.
 *     The handle owns its device memory (the factors, S^{-1}, the partial sums; nothing in the
 *     ctx workspace, which other calls regrow): per problem, with Mp = 64 ceil((n + 1) / 64) and
 *     nb = Mp / 64,   8 (3 Mp^2 + 64 Mp + 257 nb (nb + 1) / 2 + 4 n + 3) bytes at most
 *     (29.3 MB at n = 1024, 1.0 MB at n = 128), plus 8 (6 G + 9) + 100 bytes of call buffers.
 *   lfm_mbatch_mll_f64 / lfm_mbatch_mll_grad_f64   hyp, out, value, grad and status in exactly
 *     the packed layouts of lfm_batch_mll_f64 / lfm_batch_mll_grad_f64 (the gradient's jitter
 *     slot is 0). The value is lfm_mll_f64's and the gradient lfm_mll_grad_f64's: the same
 *     constrained parameters in the same order. Not positive definite (a pivot <= 0 or NaN in
 *     whichever block column it happens): that problem's value and gradient are NaN, status[p] =
 *     LFM_E_NOT_PD and the call returns LFM_E_NOT_PD; every other problem's outputs are valid and
 *     the same bits as without it.
 *   Determinism and independence: no atomics and no device-side waits (ordering comes only from
 *     consecutive launches on the ctx's stream). The same inputs give the same bits; a problem's
 *     bits depend on its own data and hyperparameters alone, not on which other problems share
 *     the batch, on their sizes or on its position; value from the gradient call is the MLL
 *     call's out, bit for bit.
 *   Synchronous; holds the device's lock shared. A handle belongs to the device of the ctx that
 *     created it (a ctx of another device: LFM_E_ARG) and to one host thread at a time.
 *     lfm_mbatch_destroy(NULL) is LFM_E_ARG.
 * LFM_MID_MAX_N bounds the handle's memory, not its speed. A call's time is set by the largest n
 * and hardly by the problem count, so the per-problem loop of lfm_mll_f64 / lfm_mll_grad_f64
 * catches up below the cap when few problems share the call. Measured on an MI355X (DESIGN.md
 * section 4.9, scripts/mid_batch_rate.py): with 15 problems the batch is faster at every size
 * (value and gradient 7.8x at n = 160, 4.3x at 320, 2.4x at 640, 1.7x at 1020); with 4 problems
 * the loop is the faster one from n = 320 up for the value (0.99x at 320, 0.57x at 1020) and from
 * n = 640 up with the gradient (1.3x at 320, 0.80x at 640, 0.61x at 1020). */
#define LFM_MID_MAX_N 1024
typedef struct lfm_mbatch lfm_mbatch;
int lfm_mbatch_create(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, lfm_mbatch** out);
int lfm_mbatch_destroy(lfm_mbatch* batch);
/* Doubles in the packed hyperparameter array: sum_p (3 G_p + 3). */
int lfm_mbatch_hyp_size(const lfm_mbatch* batch, int64_t* out);
int lfm_mbatch_mll_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp, int negative,
                       double* out, int* status);
int lfm_mbatch_mll_grad_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp, int negative,
                            double* value, double* grad, int* status);
/* latent_predict / multi_gene_predict (model.py:420-514) of every problem of an lfm_mbatch at its
 * own test inputs: lfm_batch_posterior_f64 for problems of any mix of sizes 1 <= n <= 1024, the
 * predict half of the workflow whose fits lfm_mbatch_mll_grad_f64 serves. Per problem p:
 *   S_p = (K(x_p,x_p) + diag(diag_vec_p)) + diag_add[p] I   (the terms are added in this order:
 *         the kernel's diagonal entry, then diag_vec's, then diag_add; a NULL diag_vec adds 0.0),
 *   mean = m(t_p) + K(t_p,x_p) S_p^{-1} (y_p - m(x_p)),  cov = K(t_p,t_p) - K(t_p,x_p) S_p^{-1} K(x_p,t_p),
 *   var = diag(cov).
 * Arguments, packed layouts and semantics are lfm_batch_posterior_f64's: hyp in the packed layout
 * of lfm_mbatch_mll_f64, of which only D, S, B and l are read (the obs_stddev / jitter slots are
 * ignored: the callers' diagonal is applied by the shim, dis_project_amd.predict.
 * MidBatchPredictor); diag_vec packed [sum n_p] or NULL; diag_add [nprob]; m [nprob]; t packed
 * [sum m_p x 3], gene indices truncating, wrapping and clamping as those of x, any mix of flags;
 * mean / var packed [sum m_p]; cov packed [sum m_p^2], each problem's dense row-major m_p x m_p;
 * status [nprob] optional. var or cov may be NULL, not both: with cov == NULL no off-diagonal
 * K(t,t) entry is evaluated and nothing of size m^2 is allocated. A NULL required pointer, a
 * handle of another device, or an m_p outside 1 <= m_p <= LFM_MID_MAX_M or with m_p % G_p != 0 is
 * LFM_E_ARG (the message names the limit).
 *
 * LFM_MID_MAX_M bounds the handle's memory, as LFM_MID_MAX_N does: the call works in a second
 * device arena that the handle owns (allocated at the first posterior call, regrown when a call
 * needs more, freed by lfm_mbatch_destroy; never the ctx workspace), per problem
 * 8 (64 ceil(m_p / 64) Mp_p + 5 m_p + n_p + 1) bytes, Mp_p = 64 ceil((n_p + 1) / 64), plus
 * 8 m_p^2 with the covariance (at the caps: 36 MB and 134 MB). A failed allocation is LFM_E_OOM
 * and the handle stays usable. For more test rows on one model use lfm_post_*.
 *
 * Launches: ceil((n_max + 1) / 64) + 2 without cov and one more with it, whatever the problem
 * count and the m's: the fill (S, and T = K(t,x) spread over the grid), the factorisation's
 * column launches, one solve launch over every 64-row block of test points of every problem
 * (V = T L^{-T} on the fp64 MFMA, the mean and the variance), and the covariance's tiles.
 *
 * A problem that is not positive definite gets NaN outputs and its status, and the call returns
 * LFM_E_NOT_PD; every other problem's outputs are valid and the same bits as without it. No
 * atomics, no device-side waits and no cooperative launch: the same inputs give the same bits, and
 * a problem's bits depend on its own data, hyperparameters and test inputs alone, not on the
 * other problems, their sizes or its position. A test point's variance and its row of
 * K(t,x) L^{-T} depend on its own row of t alone, not on m_p (the mean also on the point's index
 * and m_p, through mean_function's block position). cov is exactly symmetric; when both are given
 * var is diag(cov) bit for bit; mean and var are the same bits whether or not cov is requested.
 * Synchronous; holds the device's lock shared. A posterior call and an MLL / gradient call on the
 * same handle share S, L and the block inverses; each call refills what it reads, so interleaving
 * them changes no bits of either.
 *
 * Measured (scripts/mid_predict_rate.py, profiles/mid_predict.json, mid_predict_p4.json; m = 100):
 * with 15 problems the batch is ahead of the per-problem lfm_posterior_f64 loop at every size
 * (latent marginals 11.2x at n = 160, 6.5x at 320, 4.6x at 640, 2.9x at 1020; with the covariance
 * 8.5x, 5.7x, 3.7x, 2.9x). A call's time is set by the largest n, hardly by the problem count:
 * with 4 problems the batch still leads up to n = 640 (marginals 3.6x at 160, 2.1x at 320, 1.25x
 * at 640; with the covariance 2.4x, 1.6x, 1.08x) and the loop is the faster one at n = 1020
 * (0.90x and 0.88x). */
#define LFM_MID_MAX_M 4096
int lfm_mbatch_posterior_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp,
                             const double* diag_vec, const double* diag_add, const int64_t* m,
                             const double* t, double* mean, double* var, double* cov, int* status);
/* Joint samples from, and the log density of held-out values under, the distribution that
 * multi_gene_predict returns (model.py:467-514) for every problem of an lfm_mbatch, without the
 * covariance leaving the device: GaussianDistribution.sample / .log_prob (the gpjax call of
 * objectives.py:78) of N(mean_p, cov_p + cov_add[p] I), mean_p and cov_p as
 * lfm_mbatch_posterior_f64 defines them. hyp, diag_vec, diag_add, m, t, mean and status follow
 * that call exactly; the caller applies the jitter through cov_add (the shim,
 * dis_project_amd.predict.MidBatchPredictor.sample / .log_prob, passes each model's), which joins
 * each diagonal entry of cov_p in one addition.
 *   cov_add [nprob]
 *   ystar   packed [sum m_p] or NULL; logp [nprob], given exactly when ystar is:
 *           logp[p] = log N(ystar_p; mean_p, cov_p + cov_add[p] I)
 *   seeds   [nprob], required when nsamp > 0; sample0 >= 0, nsamp >= 0
 *   mean    packed [sum m_p], may be NULL
 *   samples given exactly when nsamp > 0: problem p's block is [nsamp x m_p] row-major at offset
 *           nsamp * sum_{q<p} m_q; row s is mean_p + L_p z, L_p L_p^T the matrix above, element j
 *           of z the generator's normal (seeds[p], sample0 + s, j) defined below at lfm_randn_f64,
 *           bit for bit what lfm_randn_f64(seeds[p], ...) returns.
 * At least one of (ystar, logp) and nsamp > 0 must be asked for. Every m_p must satisfy
 * 1 <= m_p <= LFM_MID_MAX_N (1024: the covariance goes through the mid-size factorisation; for a
 * larger m on one model use lfm_post_*) and m_p % G_p == 0; nsamp <= 65536 a call (continue a
 * draw with sample0), sample0 + nsamp must not overflow. A violation, a NULL required pointer, a
 * pointer of a pair given without the other, or a handle of another device is LFM_E_ARG with a
 * message naming the limit or the pointer, and touches no caller buffer. The plan rejects in this
 * order: cov_add NULL; nsamp < 0; nothing asked for; nsamp > 65536; sample0 < 0; sample0 + nsamp
 * overflowing; then per problem m_p < 1, m_p % G_p != 0, m_p > LFM_MID_MAX_N.
 *
 * Not positive definite means a failed pivot in S_p or in the factor of cov_p + cov_add[p] I:
 * that problem's logp, samples and mean are NaN, status[p] = LFM_E_NOT_PD and the call returns
 * LFM_E_NOT_PD; every other problem's outputs are valid and the same bits as without it. (Latent
 * test rows, flag 0, give an indefinite joint covariance: DESIGN.md section 4.10.)
 *
 * Launches, on the ctx's stream in order: those of lfm_mbatch_posterior_f64 with the covariance
 * (ceil((n_max + 1) / 64) + 3, unchanged); one scale launch (problem x lower tile) that copies
 * cov_p into a fresh augmented matrix of stride 64 ceil((m_p + 1) / 64) with cov_add on the
 * diagonal and ystar_p - mean_p (or 0) as its row m_p; the mid-size factorisation's column launch,
 * unchanged, ceil((m_max + 1) / 64) times on a second problem table; with ystar the value launch,
 * unchanged; with nsamp > 0 the normals and one product launch (one workgroup per 64 x 64 tile
 * of X_p = mean_p + Z_p L_p^T, depth 64 (tj + 1) on the fp64 MFMA over the factor's lower tiles;
 * the K order and the tile shape depend on neither nsamp nor sample0). In all
 *   ceil((n_max + 1) / 64) + ceil((m_max + 1) / 64) + 4 + (ystar ? 1 : 0) + (nsamp > 0 ? 2 : 0)
 * launches, whatever the problem count. No atomics, no device-side waits, no cooperative launch,
 * no graph capture. The same inputs give the same bits; a problem's bits depend on its own data,
 * hyperparameters, test rows, cov_add, ystar and seed alone, not on the other problems, their
 * sizes or its position. Rows [0, k) of an nsamp-sample call are the k-sample call's, and rows
 * [k, nsamp) those of the call at sample0 + k. mean is lfm_mbatch_posterior_f64's mean bit for
 * bit; logp has the same bits whether or not samples are asked for, and the samples whether or
 * not ystar is given. A later lfm_mbatch_mll_f64, lfm_mbatch_mll_grad_f64,
 * lfm_mbatch_posterior_f64 or lfm_mbatch_fit_f64 call on the handle returns the bits it returns
 * on a fresh handle, because each call refills what it reads. Synchronous; holds the device's
 * lock shared.
 *
 * The call works in the posterior call's arena (with the covariance) and in a fourth device arena
 * that the handle owns (allocated at the first predictive call, regrown when a call needs more,
 * freed by lfm_mbatch_destroy; never the ctx workspace): per problem, with
 * Mq = 64 ceil((m_p + 1) / 64), nq = Mq / 64, cb = ceil(m_p / 64) and sb = ceil(nsamp / 64),
 *   8 (2 Mq^2 + 4096 nq + 2) + 152 bytes, plus 8 m_p with ystar,
 *   plus 8 (4096 sb cb + nsamp m_p) with samples
 * (at m = 1024: 19.5 MB, and 16.8 MB more per 1024 samples). A failed allocation is LFM_E_OOM and
 * the handle stays usable.
 *
 * Measured on an MI355X (scripts/mid_sample_rate.py,
 * profiles/mid_sample.json, mid_sample_p4.json; 5-gene grids, gene rows, cov_add = jitter; medians
 * of synchronous calls) against lfm_mbatch_posterior_f64 with the covariance followed by one
 * lfm_mvn_sample_f64 (for logp: lfm_log_prob_f64) per problem. With 15 problems and m = 100 the
 * one call takes 1.17 ms for 16 samples at n = 160 against the loop's 4.70 (4.0x), 1.92 against
 * 5.55 at 320 (2.9x), 3.88 against 7.39 at 640 (1.9x), 6.99 against 10.65 at 1020 (1.5x); 1024
 * samples 3.8x, 2.8x, 2.0x, 1.5x; logp alone 2.8x, 2.1x, 1.5x, 1.3x. At m = 400: 16 samples 4.8x,
 * 3.9x, 2.8x, 2.1x; 1024 samples 4.4x, 3.8x, 2.8x, 2.2x (9.97 ms against 22.31 at n = 1020); logp
 * 3.0x, 2.5x, 1.9x, 1.5x. A call's time is set by the largest n and m, hardly by the problem
 * count, so with 4 problems the lead is smaller: m = 100, 16 samples 1.6x, 1.4x, 1.2x, 1.13x;
 * 1024 samples 1.8x, 1.5x, 1.2x, 1.14x; logp 1.3x, 1.2x, 1.10x, 1.07x; m = 400, 16 samples 2.1x,
 * 1.8x, 1.5x, 1.2x; 1024 samples 1.7x, 1.6x, 1.4x, 1.3x; logp 1.2x, 1.1x, 1.09x, 1.06x. No shape
 * measured has the loop ahead. The product launch is 0.4 to 7.4 % of the call (0.027 ms for 16
 * samples at m = 100, 0.27 ms for 1024 samples at m = 400 with 15 problems) and reaches 0.1 %
 * (16 samples, m = 100) to 12 % (1024 samples, m = 400) of the 78.6 TFLOP/s fp64 matrix spec on
 * nsamp sum m^2 flops; the call's time is in the column launches. */
int lfm_mbatch_predictive_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp,
                              const double* diag_vec, const double* diag_add, const int64_t* m,
                              const double* t, const double* cov_add, const double* ystar,
                              double* logp, const uint64_t* seeds, int64_t sample0, int64_t nsamp,
                              double* mean, double* samples, int* status);

/* optax.adam(learning_rate, b1, b2, eps, eps_root) and JaxTrainer.fit's epoch handling
 * (src/trainer.py:162-228; src/main.py:45 and notebook.py:55 use adam(0.01)). */
typedef struct {
  double learning_rate, b1, b2, eps, eps_root;
  int64_t num_steps_per_epoch; /* after_epoch every this many steps, step 0 included (>= 1) */
  int fix_params;              /* after_epoch sets true_s[3] = 1.0, true_d[3] = 0.8          */
} lfm_adam;
/* JaxTrainer.fit of every problem of the batch at once, on the device: nsteps training steps
 * (trainer.py:105-132 under vscan, :198-216) in ONE launch, one workgroup per problem, no host
 * round trip between steps. Per step and problem: constrain (softplus for true_d / true_s /
 * true_b / obs_stddev, 0.5 + 3 sigmoid for l: model.py:66-121), value and gradient (as
 * lfm_batch_mll_grad_f64), the bijectors' chain rule, one Adam update of the unconstrained
 * parameters, then after_epoch on them when (step0 + s) % num_steps_per_epoch == 0 and
 * fix_params (the reference's index-3 quirk; nothing for G <= 3, as JAX drops the update).
 *   raw    [nhyp] in/out: the UNCONSTRAINED parameters in hyp's packed layout (the jitter slots
 *          hold the static jitter itself and are never changed)
 *   mu, nu [nhyp] in/out: Adam's moments (zeros to start; resumable across calls with step0)
 *   step0  steps already taken (Adam's count is step0 + s + 1)
 *   history [nsteps x nprob], step-major: each step's loss value before its update
 *   status [nprob] optional: 0, or 1 + the first step whose Cholesky failed (its loss and the
 *          parameters are NaN from there on, as under JAX); returns LFM_E_NOT_PD if any did.
 * The final constrain and after_epoch on the constrained model (trainer.py:218-222) are the
 * caller's (dis_project_amd.trainer.BatchTrainer). Problem sizes as lfm_batch_mll_grad_f64. */
int lfm_batch_fit_f64(lfm_ctx* ctx, lfm_batch* batch, const lfm_adam* opt, int negative,
                      int64_t step0, int64_t nsteps, double* raw, double* mu, double* nu,
                      double* history, int* status);
/* lfm_batch_fit_f64 for an lfm_mbatch: JaxTrainer.fit of every problem of any mix of sizes
 * 1 <= n <= LFM_MID_MAX_N on the device, with no host round trip between steps. The arguments,
 * packed layouts (lfm_mbatch_hyp_size's) and per-step semantics are lfm_batch_fit_f64's: raw, mu,
 * nu [nhyp] in/out (the jitter slots hold the static jitter and are never changed); history
 * [nsteps x nprob], step-major, each step's loss before its update; status[p] optional, 0 or
 * 1 + the first step of this call whose factorisation failed (that step's loss, every later loss
 * and the parameters are NaN from there on, as under JAX; the call then returns LFM_E_NOT_PD);
 * Adam's count is step0 + s + 1 and its bias corrections 1 - b^count come from the host's pow,
 * one pair per step; after_epoch on the unconstrained leaves when (step0 + s) %
 * num_steps_per_epoch == 0 and fix_params (nothing for G <= 3). The final constrain and the last
 * after_epoch are the caller's (dis_project_amd.trainer.MidBatchTrainer(on_device=True)).
 *
 * One call enqueues a constrain launch and then, per step, the launches of
 * lfm_mbatch_mll_grad_f64 (ceil((n_max + 1) / 64) + 6, unchanged) and one update launch
 * (one workgroup per problem: the loss, the chain rule, Adam, after_epoch and the next step's
 * constrained hyperparameters), synchronises once and downloads raw, mu, nu, history and the
 * status words. Plain stream-ordered launches: no graph capture, no device-side waits, no atomics,
 * no cooperative launch. The same inputs give the same bits; a problem's trajectory depends on
 * its own data and parameters alone, not on the other problems, their sizes or its position; a
 * fit resumed across calls (mu, nu and step0 carried over) equals the one-call fit bit for bit.
 * A fit leaves the handle usable: a later lfm_mbatch_mll_f64, lfm_mbatch_mll_grad_f64 or
 * lfm_mbatch_posterior_f64 call on it returns the bits it returns on a fresh handle, because
 * each call refills what it reads.
 *
 * A NULL batch, opt, raw, mu, nu (or history with nsteps > 0), a handle of another device,
 * step0 < 0, nsteps < 0, num_steps_per_epoch < 1 or nsteps > 65536 (resume with step0 instead)
 * is LFM_E_ARG with a message naming what was wrong; nsteps == 0 returns LFM_OK and touches
 * nothing. The call works in a third device arena that the handle owns (allocated at the first
 * fit call, regrown when a call needs more, freed by lfm_mbatch_destroy; never the ctx
 * workspace): with e(d) = 2 ceil(d / 2),
 *   8 (3 e(nhyp) + 2 nsteps + e(nsteps nprob)) + 16 ceil(nprob / 4) bytes
 * (27 KB for 15 problems of G = 5 and 150 steps). A failed allocation is LFM_E_OOM and the
 * handle stays usable.
 *
 * Synchronous; holds the device's lock shared for the WHOLE call, which at n = 1020 and 150 steps
 * is on the order of a second: schedule-3 work of other threads on the device waits that long. A
 * caller who shares the device with such work can split the fit into shorter calls with step0, at
 * no cost in bits.
 *
 * Measured on an MI355X (scripts/mid_fit_rate.py, profiles/mid_fit.json,
 * mid_fit_p4.json; 5-gene grids, 150 steps of adam(0.01) on -MLL, per step):
 * the call's time per step is the kernel time of lfm_mbatch_mll_grad_f64 (0.70 ms at n = 160,
 * 1.52 at 320, 3.77 at 640, 7.62 at 1020 with 15 problems; 0.71, 1.39, 3.08, 5.65 with 4), where
 * the host loop of MidBatchTrainer around lfm_mbatch_mll_grad_f64 takes 1.67, 2.49, 4.73, 8.58 ms
 * (15 problems: 2.37x, 1.64x, 1.26x, 1.13x) and 1.00, 1.68, 3.38, 5.96 ms (4 problems: 1.41x,
 * 1.21x, 1.10x, 1.05x): the device fit is the faster one at every size and count measured, by
 * the 0.96 ms (15 problems) or 0.30 ms (4) of host work a step that it removes. It does not
 * replace lfm_batch_fit_f64 where that applies: on 15 problems of n = 35 the one-launch small
 * fit takes 34 us a step and this call 226 us (8 launches a step), 6.6x as long. */
int lfm_mbatch_fit_f64(lfm_ctx* ctx, lfm_mbatch* batch, const lfm_adam* opt, int negative,
                       int64_t step0, int64_t nsteps, double* raw, double* mu, double* nu,
                       double* history, int* status);

/* Value and gradient of CustomConjMLL(negative).step — what jax.value_and_grad(loss)
 * differentiates at trainer.py:126, before the bijectors' chain rule (trainer.py:103) —
 * with respect to the constrained parameters. grad[3G + 2]:
 *   [0,G) true_d   [G,2G) true_s   [2G,3G) true_b   [3G] l   [3G+1] obs_stddev.
 * jitter is a static field (model.py:64) and gets no gradient. Not PD: LFM_E_NOT_PD,
 * value and grad NaN. */
int lfm_mll_grad_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                     const lfm_hyp* hyp, int negative, double* value, double* grad);

/* gpjax 0.8.2 ConjugateLOOCV.step for ExactLFM: the leave-one-out predictive log probability
 * (Rasmussen & Williams 5.4.2) of the model CustomConjMLL.step scores. With
 * S = K(x,x) + (jitter + obs_stddev^2) I (exactly what lfm_mll_f64 factors), r = y - m(x),
 * a = S^{-1} r and k_i = [S^{-1}]_ii:
 *   loo_mean[i] = y_i - a_i / k_i,   loo_var[i] = 1 / k_i,
 *   value = constant * sum_i log N(y_i; loo_mean[i], loo_var[i]),  constant = -1 if negative
 *           else +1.
 * loo_mean and loo_var (n doubles each) may each be NULL; they do not depend on negative, and
 * leaving either out changes no bit of the others. Any n >= 1 with n % num_genes == 0.
 * Not PD: LFM_E_NOT_PD, value and the per-point arrays NaN. k_i comes off the bordered factor as
 * -Bt_ii - a_i^2; should rounding leave a k_i <= 0 on a factor that is
 * PD, it propagates as IEEE NaN into its own mean and variance and into the value, with LFM_OK —
 * gpjax's sqrt of a negative. The value is summed in a fixed order: the same inputs give the same
 * bits, from either call.
 * Cost: the bordered factorisation of lfm_mll_grad_f64 (N^3 flops) and O(n) more. Measured on an
 * MI355X on the C2 grid layout (scripts/loo_rate.py,
 * profiles/loo_rate.json): 0.70 ms at N = 1024, 2.60 ms at N = 4096, 74.3 ms at N = 16384
 * (lfm_mll_grad_f64 on the same problems: 0.75, 2.61, 74.6 ms). The route without this call,
 * lfm_gram_f64 to the host and scipy's cho_factor / cho_solve(I) there, takes 1.70 s at N = 4096.
 * NULL ctx: LFM_E_ARG. NULL x / y / value / hyp or a bad n: LFM_E_ARG with a message, no caller
 * buffer touched. */
int lfm_loocv_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n, const lfm_hyp* hyp,
                  int negative, double* value, double* loo_mean /* [n], may be NULL */,
                  double* loo_var /* [n], may be NULL */);
/* Its value and gradient with respect to the constrained parameters, grad[3G + 2] in
 * lfm_mll_grad_f64's layout (jitter gets none):
 *   d value / d theta = constant * (1/2 tr(W_loo dS/dtheta) + u^T dm/dtheta),
 *   W_loo = -2 S^{-1} diag(c) S^{-1} + u a^T + a u^T,  c_i = (1 + a_i^2 / k_i) / (2 k_i),
 *   u = S^{-1} b,  b_i = a_i / k_i.
 * value has the bits lfm_loocv_f64 returns. Not PD: LFM_E_NOT_PD, value and grad NaN.
 * Cost: the bordered factorisation plus one more N^3 product on the fp64 MFMA (S^{-1} diag(c)
 * S^{-1}, lower triangle), then lfm_mll_grad_f64's reductions; no memory beyond that call's
 * 2Mp x 2Mp matrix and O(n) doubles. Measured as above: 1.04 ms at N = 1024, 4.77 ms at
 * N = 4096, 150.5 ms at N = 16384, of which the product launch 0.18, 1.72 and 71.4 ms (0.08, 0.51
 * and 0.78 of the 78.6 TFLOP/s fp64 matrix spec on its n^3 flops). */
int lfm_loocv_grad_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                       const lfm_hyp* hyp, int negative, double* value, double* grad /* [3G+2] */);

/* ------------- posterior at test inputs (latent_predict / multi_gene_predict) */
/* mean[m] = m(t) + K(t,x) S^{-1} (y - m(x)),  cov[m x m] = K(t,t) - K(t,x) S^{-1} K(x,t),
 * S = K(x,x) + diag(diag_vec) + diag_add I (diag_vec [n] may be NULL); model.py:420-514.
 * n and m must be multiples of num_genes (mean_function, model.py:145-149). The callers'
 * jitter / diagonalisation is applied by the shim. Not PD: LFM_E_NOT_PD, outputs NaN. */
int lfm_posterior_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                      const double* diag_vec, double diag_add, const double* t, int64_t m,
                      const lfm_hyp* hyp, double* mean, double* cov);

/* latent_predict / multi_gene_predict (model.py:420-514) of every problem of a resident batch
 * (lfm_batch_create) at its own test inputs, in a fixed number of launches whatever the problem
 * count — the predict half of the fit-then-predict workflow (notebook.py:91-110 and
 * utils.py:144-172 call the two predictors once per fitted model). Per problem p:
 *   S_p = K(x_p,x_p) + diag(diag_vec_p) + diag_add[p] I,
 *   mean = m(t_p) + K(t_p,x_p) S_p^{-1} (y_p - m(x_p)),  cov = K(t_p,t_p) - K(t_p,x_p) S_p^{-1} K(x_p,t_p).
 *   hyp       the packed layout of lfm_batch_mll_f64; only D, S, B and l are read (the diagonal's
 *             noise comes from diag_vec / diag_add, as in lfm_posterior_f64: the callers' jitter
 *             and sigma^2 are applied by the shim, dis_project_amd.predict.BatchPredictor)
 *   diag_vec  packed [sum n_p] in problem order, or NULL;  diag_add [nprob]
 *   m         [nprob] test rows per problem, each >= 1 and a multiple of that problem's
 *             num_genes (mean_function, model.py:145-149)
 *   t         packed [sum m_p x 3]; gene indices truncate, wrap and clamp as those of x, and any
 *             mix of flags is allowed (kxx, kxf, kfx, kff)
 *   mean      packed [sum m_p]
 *   var       packed [sum m_p], the diagonal of cov (bit for bit); may be NULL
 *   cov       packed [sum m_p^2], each problem's dense row-major m_p x m_p, exactly symmetric;
 *             may be NULL, and then no off-diagonal K(t,t) entry is evaluated (latent_predict
 *             and the plots read the marginals only). One of var / cov must be given.
 *   status    [nprob] optional: LFM_OK or LFM_E_NOT_PD per problem
 * Every problem needs n <= 127 (as lfm_batch_mll_grad_f64) and its LDS map within 160 KB, else
 * LFM_E_ARG (lfm_posterior_f64 takes any n); a NULL required pointer or a bad m is LFM_E_ARG.
 * A problem that is not positive definite gets NaN outputs and its status, and the call returns
 * LFM_E_NOT_PD; every other problem's outputs are valid and the same bits as without it. A test
 * point's mean and variance depend on its own row of t (and, through mean_function's block
 * position, on its index and m_p), not on how the batch is split over workgroups. Synchronous;
 * holds the device's lock shared; no device-side waits or atomics: the same inputs give the
 * same bits. */
int lfm_batch_posterior_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp,
                            const double* diag_vec, const double* diag_add, const int64_t* m,
                            const double* t, double* mean, double* var, double* cov, int* status);

/* ------------- resident posterior: factor a large model once, predict many times */
/* latent_predict / multi_gene_predict (model.py:420-514) condition on the training data once;
 * the notebooks then evaluate the fitted model at several sets of test times. lfm_posterior_f64
 * pays the whole N^3 / 3 factorisation on every call; a handle pays it once.
 *
 * lfm_post_create: S = K(x,x) + diag(diag_vec) + diag_add I factored once; L and
 * z = L^{-1} (y - m(x)) stay in HBM, in memory the handle owns (not the ctx workspace). x [n x 3],
 * y [n], diag_vec [n] (may be NULL) and hyp are host pointers, copied: the caller may free them.
 * n and num_genes as lfm_posterior_f64. Not PD: LFM_E_NOT_PD, *out = NULL. The handle needs
 * about 8 (n + 128)^2 bytes of device memory.
 *
 * lfm_post_predict_f64: mean [m] and cov [m x m] as lfm_posterior_f64 defines them, var [m] the
 * diagonal of cov. var or cov may be NULL, not both; m >= 1 and m % num_genes == 0, any m (no
 * n + m limit); t [m x 3] as lfm_batch_posterior_f64's.
 *   Marginals only (cov == NULL): no off-diagonal K(t,t) entry is evaluated and nothing of size
 *     m^2 is allocated. The test rows go through in chunks of the handle's chunk size; per chunk
 *     the solve works in a chunk x round_up(n, 128) buffer of doubles. The default chunk is the
 *     largest multiple of 128 rows, at most 16384, that keeps that buffer within 1 GiB.
 *   Covariance (cov != NULL): m must fit in one chunk, else LFM_E_ARG with a message naming the
 *     limit. cov is dense row-major and exactly symmetric. When both are given, var is
 *     diag(cov) bit for bit.
 *   Independence of the split: a test point's variance and its row of K(t,x) L^{-T} depend on
 *     its own row of t alone, not on m or on the chunk size. The mean depends on the point's
 *     index and on m as well (mean_function's block position), not on the chunk size. The same
 *     inputs give the same bits: no atomics and no device-side waits. Synchronous; holds the
 *     device's lock shared.
 * lfm_post_set_chunk: test rows solved per pass (0 restores the default); a multiple of 128, else
 *   LFM_E_ARG (the message goes to the ctx that created the handle).
 * Handle rules: a handle belongs to the device of the ctx that created it, which must outlive it,
 * and to one host thread at a time. A predict with a ctx of another device is LFM_E_ARG. Other
 * calls on the ctx between predicts (an MLL of a larger n, a gradient, lfm_posterior_f64) do not
 * disturb the handle. lfm_post_destroy(NULL) is LFM_E_ARG. */
typedef struct lfm_post lfm_post;
int lfm_post_create(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                    const double* diag_vec, double diag_add, const lfm_hyp* hyp, lfm_post** out);
int lfm_post_destroy(lfm_post* post);
int lfm_post_set_chunk(lfm_post* post, int64_t rows);
int lfm_post_predict_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double* mean,
                         double* var, double* cov);

/* ------------------- GaussianDistribution(loc, scale).log_prob(y) (gpjax 0.8.2) */
/* scale is a dense SPD n x n (row-major, leading dim lds; lower triangle read). */
int lfm_log_prob_f64(lfm_ctx* ctx, const double* loc, const double* scale, int64_t n,
                     int64_t lds, const double* y, double* out);

/* ------------- joint samples: GaussianDistribution(loc, scale).sample (gpjax 0.8.2) */
/* The distribution latent_predict / multi_gene_predict return (model.py:420-514) is drawn from
 * as loc + L z_s, L L^T = scale, z_s standard normal. gpjax takes its normals from JAX's threefry
 * key; this library cannot reproduce those bits and does not try: the equivalence with the
 * reference is IN DISTRIBUTION. What it fixes instead is its own generator, so that a sample can
 * be reproduced on the host, or continued in a later call, from (seed, s, j) alone.
 *
 * The generator. Element j of sample s (s the absolute sample index, sample0 + row) depends on
 * (seed, s, j) and on nothing else: not on the launch geometry, not on nsamp, n or sample0, no
 * state. With p = j >> 1:
 *   Philox4x32-10, multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl constants 0x9E3779B9,
 *   0xBB67AE85; one round maps (c0, c1, c2, c3) to
 *       (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),
 *   hi / lo the halves of the 64-bit product, and the key (k0, k1) is bumped by the Weyl
 *   constants after each round;
 *   key = (seed lo32, seed hi32), counter = (p lo32, p hi32, s lo32, s hi32) -> words w0..w3;
 *   a = (w0 | w1 << 32) >> 11, b = (w2 | w3 << 32) >> 11; u1 = (a + 1) 2^-53, u2 = (b + 1) 2^-53,
 *   both in (0, 1] and exact; r = sqrt(-2 ln u1), theta = 2 pi u2;
 *   z[2p] = r cos theta, z[2p + 1] = r sin theta.
 * Known answers: counter 0^4, key 0^2 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; seed 42, s = 0:
 * z[0:4] = -0.66537487, 1.03602381, -1.43388918, 0.42327818. The device's ln / sqrt / sin / cos
 * differ from a host libm's by a few ulp: a host restatement agrees to about 1e-14, not bit for
 * bit (tests/philox_ref.py is one).
 *
 * lfm_randn_f64: the generator alone, out[s * n + j] for s < nsamp, j < n (host).
 *
 * lfm_mvn_sample_f64: out[s] = loc + L z_s for samples sample0 .. sample0 + nsamp - 1. loc [n],
 * scale (n x n row-major, leading dim lds >= n; ONLY the lower triangle is read) and out
 * [nsamp x n] are host pointers. Works in the ctx workspace, as lfm_log_prob_f64 does:
 *   8 (Mp^2 + 128 ceil(nsamp / 128) Np + nsamp n + n) bytes, Mp = 128 ceil((n + 1) / 128),
 *   Np = 128 ceil(n / 128).
 * scale is factored on schedule 1 (shared hold of the device's lock); the product
 * X[s, i] = loc[i] + sum_{k <= i} L[i, k] Z[s, k] runs one workgroup per 128 x 128 tile of X on
 * the fp64 MFMA, at a K order and tile shape that depend on neither nsamp nor sample0. So: the
 * same call twice gives the same bits; rows [0, k) of an nsamp-sample call are the k-sample
 * call's, and rows [k, nsamp) are those of the call at sample0 + k.
 *
 * lfm_post_sample_f64: the same from a resident posterior (lfm_post_create): nsamp joint samples
 * of N(mean(t), cov(t) + diag_add I), mean and cov as lfm_post_predict_f64 defines them. cov never
 * leaves the device: it is formed as by a predict, copied into a matrix of stride
 * Mp' = 128 ceil((m + 1) / 128) that the handle owns, diag_add joins its diagonal in one addition,
 * and it is factored, multiplied and only X [nsamp x m] (and the mean, if mean != NULL) comes
 * back. m has lfm_post_predict_f64's rules with the covariance: m >= 1, m % num_genes == 0 and m
 * within one chunk, else LFM_E_ARG (the message names the limit). On top of a predict with the
 * covariance the handle grows by
 *   8 (Mp'^2 + 128 ceil(nsamp / 128) 128 ceil(m / 128) + nsamp m) bytes.
 * The result equals lfm_mvn_sample_f64 fed this handle's lfm_post_predict_f64 mean and
 * cov + diag_add I, bit for bit. The handle's factor, z and predict results are not disturbed: a
 * predict after a sample returns the bits it returned before.
 *
 * All three: nsamp < 1, sample0 < 0, sample0 + nsamp overflowing 2^63, nsamp above 2^24 in one
 * call (continue the draw with sample0), n outside [1, 2^30], a NULL required pointer or a handle
 * of another device is LFM_E_ARG with a message naming the cause. Not positive definite: every
 * output is NaN (the mean included) and the return is LFM_E_NOT_PD, JAX's NaN Cholesky. A failed
 * allocation is LFM_E_OOM, and the ctx and the handle stay usable. Synchronous; no atomics, no
 * device-side waits and no cooperative launch.
 *
 * Validity is the caller's: gene rows (flag 1) of the reference's kernel give a covariance that is
 * positive semi-definite to rounding, and diag_add makes it definite. Latent rows (flag 0) do not:
 * the joint covariance the flag-switched kernel (model.py:152-195) gives them is indefinite (its
 * smallest eigenvalue was -3 on the p53 data at m = 100), so a joint draw of latent rows is
 * LFM_E_NOT_PD, as jnp.linalg.cholesky would return NaN; latent_predict's diagonalised
 * distribution (model.py:420-465) is the one that can be sampled.
 *
 * Measured on an MI355X (scripts/sample_rate.py, profiles/post_sample.json, DESIGN.md section
 * 4.10; a resident N = 16384 model, gene rows, diag_add = obs_stddev^2, medians of synchronous
 * calls): lfm_post_sample_f64 takes 15.3 ms at m = 384, 47 ms at m = 4096 and 231 / 237 ms at
 * m = 16384 for 16 / 1024 samples; lfm_post_predict_f64 with the covariance followed by numpy's
 * cholesky and matmul takes 12.9 / 18.4 ms, 1.50 / 1.57 s and 8.4 / 8.7 s (0.85x / 1.21x, 32x /
 * 33x, 36x / 37x), and downloads 2.1 GB at m = 16384 where this call downloads 2.2 / 134 MB. At
 * m = 16384 and 1024 samples the call is the solve 100 ms, the factorisation 75 ms, the generator
 * 0.08 ms, the product 5.8 ms (0.60 of the 78.6 TFLOP/s fp64 matrix spec on its nsamp m^2 flop)
 * and 55 ms of covariance tiles, copy and download. With 16 samples the product still issues 128
 * rows: 2.6 ms, 0.02 of the spec on the algorithmic flop. */
int lfm_randn_f64(lfm_ctx* ctx, uint64_t seed, int64_t sample0, int64_t nsamp, int64_t n,
                  double* out /* host [nsamp x n] */);
/* GaussianDistribution(loc, scale).sample (gpjax 0.8.2): out[s] = loc + L z_s, L L^T = scale */
int lfm_mvn_sample_f64(lfm_ctx* ctx, const double* loc, const double* scale, int64_t n,
                       int64_t lds, uint64_t seed, int64_t sample0, int64_t nsamp,
                       double* out /* [nsamp x n] */);
/* the same from a resident posterior: N(mean(t), cov(t) + diag_add I); cov never leaves the device */
int lfm_post_sample_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                        uint64_t seed, int64_t sample0, int64_t nsamp,
                        double* mean /* [m], may be NULL */, double* out /* [nsamp x m] */);

/* ------------- held-out log density on the resident posterior */
/* gpjax 0.8.2 GaussianDistribution.log_prob (called at objectives.py:78) of the distribution
 * multi_gene_predict returns (model.py:467-514), for k held-out vectors at once and without the
 * covariance leaving the device: the other half of lfm_post_sample_f64.
 *   logp[r] = log N(ystar_r; mean(t), cov(t) + diag_add I)
 *           = -1/2 ||w_r||^2 - sum_i log L_ii - (m / 2) log 2 pi,   r < k,
 *   L L^T = cov(t) + diag_add I,   w_r = L^{-1} (ystar_r - mean),
 * mean and cov as lfm_post_predict_f64 defines them; diag_add joins each diagonal entry of cov in
 * one addition, exactly as in lfm_post_sample_f64. t [m x 3], ystar [k x m] row-major, mean [m]
 * (may be NULL) and logp [k] are host pointers.
 *
 * The route, on the ctx's stream: the predict with the covariance; cov into the handle's matrix of
 * stride Mp' = 128 ceil((m + 1) / 128), diag_add on its diagonal, the augmented row with residual
 * 0 and the factorisation on schedule 1 (these are lfm_post_sample_f64's first steps, one piece of
 * code), whose own reduction then is base = -1/2 logdet - (m / 2) log 2 pi; the 16 x 16 inverses
 * of the factor's diagonal blocks; then, in passes of at most `pass` held-out rows, the residual
 * rows R[r, j] = ystar[r, j] - mean[j] (stride Np' = 128 ceil(m / 128), zero padded) through the
 * predict's own multi-right-hand-side sweep on the fp64 MFMA against this factor, whose per-row
 * accumulator ends as ||w_r||^2, and
 *   logp[r] = base - 0.5 * ||w_r||^2:   one multiplication, which is exact, and one subtraction.
 * pass is the handle's chunk, at most the largest multiple of 128 rows, up to 16384, whose
 * pass x Np' doubles fit 1 GiB. m has lfm_post_predict_f64's rules with the covariance. On top of
 * a predict with the covariance the handle grows by
 *   8 (Mp'^2 + 17 Np' + max(0, P Np' - V) + max(0, 2 P - A) + P) bytes,
 *   P = 128 ceil(min(k, pass) / 128),  V = 128 ceil(m / 128) 128 ceil(n / 128) and A = 2 x 128
 *   ceil(m / 128): the doubles of the predict's solve workspace and row accumulators, which are
 *   free again once the covariance is formed and serve the residual rows;
 * Mp'^2 of it is the matrix a sample on the same handle uses. Nothing is placed in the ctx
 * workspace; lfm_post_destroy frees it.
 *
 * Promises:
 *   logp[r] depends on the handle, t, diag_add and row r of ystar alone: not on k, not on the pass
 *     size, not on lfm_post_set_chunk. Rows [0, j) of a k-vector call are the j-vector call's, bit
 *     for bit, and the same call twice gives the same bits.
 *   A NaN or Inf in one row of ystar (any row whose ||w_r||^2 is not finite) makes that row's logp
 *     NaN and leaves every other row's bits alone; the return is still LFM_OK.
 *   mean is lfm_post_predict_f64's mean, bit for bit.
 *   The handle's factor, z, inverses and predict results are only read: a predict or a sample
 *     after the call returns the bits it returned before.
 *   No atomics, no device-side waits, no cooperative launch, no graph capture. Synchronous; holds
 *     the device's lock shared (the factorisation runs schedule 1).
 *   Not positive definite, a failed pivot of cov + diag_add I (latent rows: see the note on
 *     validity above): every logp and the mean are NaN, the return is LFM_E_NOT_PD, and the handle
 *     and the ctx stay usable. A failed allocation is LFM_E_OOM, and both stay usable.
 *   LFM_E_ARG with a message naming the cause, no caller buffer touched, checked in this order:
 *     a NULL ctx (no message); a NULL post; a handle of another device; a NULL t / ystar / logp;
 *     m < 1 or m % num_genes != 0; m above the chunk; k < 1; k above 2^24 (split the rows of
 *     ystar over calls).
 *
 * Measured on an MI355X (scripts/post_logp_rate.py, profiles/post_logp.json, DESIGN.md section
 * 4.10.1; a resident N = 16384 model, gene rows, diag_add = obs_stddev^2, medians of synchronous
 * calls): the call takes 15.2 ms at m = 384, 48 ms at m = 4096 and 237 / 237 / 241 ms at
 * m = 16384 for 1 / 16 / 1024 vectors: the sample call's predict (109 ms of solve, both sweeps)
 * and factorisation (76 ms), whatever k. The host route, lfm_post_predict_f64 with the covariance,
 * one addition on the diagonal and lfm_log_prob_f64 per vector, takes 11.6 / 16.1 / 315 ms at
 * m = 384 (0.76x / 1.06x / 21x), 44.5 / 110 / 4560 ms at m = 4096 (0.93x / 2.3x / 94x) and
 * 289 / 1360 / 69900 ms at m = 16384 (1.2x / 5.7x / 290x; the figures for more than 16 vectors at
 * m = 4096 and more than 2 at m = 16384 are its predict plus k times the median timed vector,
 * 4.4 ms and 68 ms), uploading 2.1 GB per vector at m = 16384 where this call uploads 0.5 to
 * 135 MB. For one held-out vector at m <= 4096 the host route is the faster one. */
int lfm_post_log_prob_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                          const double* ystar /* [k x m] row-major, host */, int64_t k,
                          double* mean /* [m], may be NULL */, double* logp /* [k] */);

/* ----------------------- device-resident variants (inputs already in HBM) */
int lfm_dev_alloc(lfm_ctx* ctx, size_t bytes, void** out);
int lfm_dev_free(lfm_ctx* ctx, void* p);
int lfm_memcpy_h2d(lfm_ctx* ctx, void* dst, const void* src, size_t bytes);
int lfm_memcpy_d2h(lfm_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Sets `bytes` bytes of device memory at dst to the byte `value` (e.g. sentinel fills). */
int lfm_memset_dev(lfm_ctx* ctx, void* dst, int value, size_t bytes);
/* As lfm_mll_f64 with x / y already on the ctx's device. */
int lfm_mll_f64_dev(lfm_ctx* ctx, const double* d_x, const double* d_y, int64_t n,
                    const lfm_hyp* hyp, int negative, double* out);
/* A device-resident dataset evaluated many times (training steps, random restarts): x (and y
 * when n is small) is read back and analysed once, here, instead of on every call. The caller
 * keeps d_x / d_y allocated and unmodified until lfm_data_destroy — the reference's Dataset is
 * an immutable JAX array pair (gpjax Dataset, objectives.py:21 / trainer.py:126) likewise. */
typedef struct lfm_data lfm_data;
int lfm_data_create(lfm_ctx* ctx, const double* d_x, const double* d_y, int64_t n,
                    lfm_data** out);
int lfm_data_destroy(lfm_data* data);
/* As lfm_mll_f64_dev on a dataset handle. */
int lfm_mll_f64_data(lfm_ctx* ctx, lfm_data* data, const lfm_hyp* hyp, int negative,
                     double* out);
/* nsets hyperparameter sets on one dataset (the random restarts of BASELINE.json configs[2]:
 * CustomConjMLL.step of each model in src/notebook.py:33-75's loop over one Dataset) ->
 * out[nsets], status[nsets] (optional: LFM_OK / LFM_E_NOT_PD per set; not PD -> NaN). The
 * values are lfm_mll_f64_data's, bit for bit. On schedule 3 the evaluations are pipelined: the
 * next set's prologue runs while the previous set's factorisation is in its chain-bound tail
 * (LFM_OVERLAP, default 1). Returns LFM_E_NOT_PD if any set failed. (ABI 5) */
int lfm_mll_multi_f64(lfm_ctx* ctx, lfm_data* data, int64_t nsets, const lfm_hyp* hyps,
                      int negative, double* out, int* status);
/* As lfm_gram_f64 / _f32 with x and out on the device. */
int lfm_gram_f64_dev(lfm_ctx* ctx, const double* d_x, int64_t n, const lfm_hyp* hyp,
                     double diag_add, int uplo, double* d_out, int64_t ldo);
int lfm_gram_f32_dev(lfm_ctx* ctx, const double* d_x, int64_t n, const lfm_hyp* hyp,
                     double diag_add, int uplo, float* d_out, int64_t ldo);

/* ------------------------------------------------------------- profiling */
int lfm_profile_enable(lfm_ctx* ctx, int on);
/* Restrict event timing to kernel classes whose bit is set (bit i = entry i of
 * lfm_profile_read's list; default all): fewer events inside a timed region. */
int lfm_profile_classes(lfm_ctx* ctx, unsigned mask);
int lfm_profile_reset(lfm_ctx* ctx);
/* Copies up to max entries; *count = number of kernel classes seen. */
int lfm_profile_read(lfm_ctx* ctx, lfm_kstat* stats, int max, int* count);

/* -------------------------------- multi-GPU farm: RCCL all-gather over xGMI */
/* Rank 0 creates the 128-byte unique id; the caller ships it to every rank. */
int lfm_farm_unique_id(lfm_ctx* ctx, unsigned char id[128]);
int lfm_farm_init(lfm_ctx* ctx, const unsigned char id[128], int nranks, int rank);
/* All-gather count fp64 per rank (host in, host out: recv holds nranks*count). */
int lfm_farm_allgather_f64(lfm_ctx* ctx, const double* send, int64_t count, double* recv);
/* One farm round of a resident batch — the replicate x ablation problems of
 * src/notebook.py:33-75, each rank holding its block of them (lfm_batch_create) — with the
 * exchange on the device: the batch's kernel writes every problem's MLL straight into this rank's
 * `slots` send slots (NaN past nprob), ncclAllGather runs on the ctx's stream behind it, and a
 * publish kernel copies the gathered nranks x slots values to pinned host memory and signals the
 * host: one launch chain, one bounded wait (LFM_RCCL_TIMEOUT_S), recv[nranks * slots] filled.
 * hyp / negative / status as lfm_batch_mll_f64 (status: this rank's problems). A failed or timed-
 * out exchange aborts the communicator (LFM_E_RCCL; recv untouched; later calls LFM_E_STATE until
 * lfm_farm_init). slots >= nprob, else LFM_E_ARG. */
int lfm_farm_batch_mll_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                           int64_t slots, double* recv, int* status);
int lfm_farm_destroy(lfm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* LFM_H */
