// lfm_internal.h — shared declarations of the HIP implementation behind include/lfm.h: the
// context, the kernel units' launch wrappers and their argument structs. Every size, offset and
// grid they are launched with comes from the plain-C++ plans of lfm_host.h / lfm_small_plan.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lfm.h"
#include "../../include/lfm_diag.h"
#include "lfm_host.h"

namespace lfm {

// Kernel classes tracked by the profiler (lfm_profile_*).
enum KClass {
  K_TABLES = 0,   // per-gene erf/exp tables of the structured gram
  K_GRAM_GRID,    // structured (shared uniform time grid) gram fill
  K_GRAM_DIRECT,  // general per-pair gram fill (any x, any flags)
  K_AUGMENT,      // residual row + padding rows of the augmented factor
  K_POTRF,        // diagonal-block factor + inverse (one workgroup)
  K_TRSM,         // panel solve  X = A * Linv^T  (fp64 MFMA)
  K_SYRK,         // trailing update C -= P P^T   (fp64 MFMA)
  K_FINALIZE,     // logdet + quadratic form -> scalar
  K_SMALL,        // one-workgroup-per-problem fused small-N MLL
  K_MEAN,         // mean_function
  K_GRAD,         // MLL gradient: W-weighted kernel-derivative reduction
  K_PANEL,        // fused pending update + diagonal factor + panel solve (one block column)
  K_SIDE_SYRK,    // schedule 3: the tail of a step's trailing update on the side CUs (helper)
  K_SMALL_GRAD,   // one-workgroup-per-problem value + gradient (and the in-kernel fit)
  K_SMALL_POST,   // batched posterior predictors of the small problems (and their covariance)
  K_POST_PANEL,   // resident posterior: multi-right-hand-side panel solve against the factor
  K_POST_UPDATE,  // resident posterior: right-looking update of the test rows (fp64 MFMA)
  K_MID_FILL,     // mid-size batch: every problem's augmented matrix from the hyperparameters
  K_MID_COLUMN,   // mid-size batch: one block column of every problem's factor (fp64 MFMA)
  K_MID_INVERSE,  // mid-size batch: X = L^{-1} and S^{-1} = X^T X (fp64 MFMA)
  K_MID_PAIRS,    // mid-size batch: W-weighted kernel derivatives per lower tile
  K_MID_FINISH,   // mid-size batch: the values / the gradients joined in a fixed order
  K_SAMPLE_RANDN, // joint samples: the counter-based normal generator
  K_SAMPLE_TRMM,  // joint samples: X = loc + Z L^T per 128 x 128 tile (fp64 MFMA)
  K_LOO_PRODUCT,  // leave-one-out gradient: M = Bs Bs^T per lower 128 x 128 tile (fp64 MFMA)
  K_NCLASS
};

extern const char* const kClassName[K_NCLASS];

struct ProfEvent {
  int cls;
  hipEvent_t a, b;
  double flops, bytes, issued;
};

// Growth of a context's workspace (lfm_ctx.hip): at least 16 bytes, ctx->stream synchronised
// before the old allocation is freed, LFM_E_OOM with the size in the message; the host form
// allocates pinned memory with `flags` and reports failure as `what`.
int ensure(lfm_ctx* ctx, void** p, size_t* cap, size_t bytes);
int ensure_host(lfm_ctx* ctx, void** p, size_t* cap, size_t bytes, unsigned flags,
                const char* what);

// A buffer its context owns: device memory (Pinned: host memory), grown on demand and freed with
// the context. Reads as the pointer it holds (ctx->A + off).
template <typename T, bool Pinned = false>
struct Buf {
  T* p = nullptr;
  size_t bytes = 0;  // capacity
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  operator T*() const { return p; }
  int reserve(lfm_ctx* ctx, size_t n, unsigned flags = hipHostMallocDefault,
              const char* what = "hipHostMalloc") {
    return Pinned ? ensure_host(ctx, (void**)&p, &bytes, n, flags, what)
                  : ensure(ctx, (void**)&p, &bytes, n);
  }
  // Forget the allocation without freeing it (the farm: work still queued may write into it)
  void abandon() {
    p = nullptr;
    bytes = 0;
  }
  void release() {
    if (p) Pinned ? hipHostFree(p) : hipFree(p);
    abandon();
  }
};

// The run-time knobs, read once when the context is created (create_streams,
// lfm_ctx.hip); a restart-pipeline workspace copies its primary's.
struct Knobs {
  int side_req = 32;             // LFM_SIDE_CUS at creation: the reservation to (re)create
  int sched = 3;                                 // look-ahead schedule 1 or 3 (LFM_SCHED)
  int s3_events = 0;  // LFM_S3_EVENTS: 1 schedule 3 ordered by events, 2 its timed launches serialised
  unsigned wait_ticks = 200000000u;              // device-side wait bound, 100 MHz ticks (2 s;
                                                 // LFM_DEVICE_WAIT_MS, LFM_DEBUG_SPIN_LIMIT)
  bool grad_direct = false;                      // gradient: per-pair path only (LFM_GRAD_DIRECT)
  bool gram_fuse = true;                         // gram in the first update (LFM_GRAM_FUSE)
  int64_t w4min = 6144;   // LFM_W4_MIN: bulk super-panels while the trailing matrix has this many rows
  int64_t w2min = -1;     // LFM_W2_MIN: w = 2 down to this many rows (-1: 5120 schedule 3, else 4096)
  int w0 = 1;             // LFM_W0: width of schedule 3's first super-panel
  int helper = 1;         // LFM_HELPER: schedule 3's side-CU helper
  double helper_tc = 700, helper_min = 1200;  // LFM_HELPER_TC / LFM_HELPER_MIN, microseconds
  bool s3_fallback = true;   // LFM_S3_FALLBACK: re-run a stalled schedule-3 call on schedule 1
  double rccl_timeout_s = 300.0;  // LFM_RCCL_TIMEOUT_S: bound on every farm collective wait
  int farm_stall_ms = 0;  // LFM_DEBUG_FARM_STALL_MS: test stand-in for a late peer rank
  bool small_kernarg = true;  // LFM_SMALL_KERNARG: small batches' table in the kernel arguments
  bool farm_graph_on = true;  // LFM_FARM_GRAPH: the device-side farm round as one captured graph
  int ovl_on = 1;                    // LFM_OVERLAP: 0 evaluates lfm_mll_multi_f64's sets one by one
  int64_t ovl_at = 6144;             // LFM_OVL_AT: the tail starts at the first step whose
                                     // trailing matrix has fewer rows than this
  int ovl_reserve = 96;              // LFM_OVL_RESERVE: main CUs the overlap stream leaves to the
                                     // previous evaluation's tail
};

// A context's streams and events. A base of lfm_ctx, so they are destroyed after its members:
// deleting a context frees its buffers (Buf) first, then the events, then the streams — the
// order lfm_ctx_destroy has always had.
struct CtxStreams {
  hipStream_t stream = nullptr;  // main stream: gram fill, bulk trailing updates, finalize
  hipStream_t side = nullptr;    // high-priority look-ahead stream: panel factor + solve
  hipStream_t m3 = nullptr;      // schedule 3: bulk stream (CUs outside the chain's)
  hipStream_t s3 = nullptr;      // schedule 3: factor-chain stream (LFM_SIDE_CUS CUs)
  std::vector<hipEvent_t> evs;   // cross-stream dependency events (timing disabled)
  // profiling: event pairs not read yet, and spare events
  std::vector<ProfEvent> pending;
  std::vector<hipEvent_t> pool;
  ~CtxStreams();  // lfm_ctx.hip
};

}  // namespace lfm

struct lfm_ctx : lfm::CtxStreams {
  int device = 0;
  lfm::Knobs knobs;
  int cus = 256;                 // compute units of the device
  std::string err;
  int nb = 128;  // Cholesky block size

  // device workspace, grown on demand
  lfm::Buf<double> A;          // augmented factor (Mp x Mp) / generic matrix
  lfm::Buf<double> tab;        // gene tables (fp64)
  lfm::Buf<float> tab32;       // gene tables (fp32 copy)
  lfm::Buf<double> par;        // packed hyperparameters + layout
  lfm::Buf<double> xin;        // staged x / y / loc inputs
  lfm::Buf<double> linvT;      // 8 x 16x16 inverses of the diagonal sub-blocks
  lfm::Buf<double> parts;      // per-block logdet partials
  lfm::Buf<int> status;        // [0] first failing pivot (INT_MAX = none)
  lfm::Buf<double> wk;         // schedule 3: diagonal block + identity border
  lfm::Buf<double> xbuf;       // schedule 3: solved panel X = A21 L11^{-T}
  lfm::Buf<double> zvec;       // schedule 3: z = L^{-1} r
  lfm::Buf<double> linv_full;  // schedule 3: 128x128 block inverse
  lfm::Buf<double> xd;         // schedule 3: the chain's rows of X_{s-1}
  lfm::Buf<unsigned> flags;    // schedule 3: per-step device flags
  lfm::S3Plan s3_plan[2];      // schedule 3: the last MLL / bordered call's launch plan, reused
                               // while its inputs hold (lfm_chol_sched.hip schedule3)
  lfm::Buf<unsigned> psync;    // fused panel: [0] factor epoch, [1] slab count
  unsigned panel_epoch = 0;                      // fused panel launches so far
  int side_cus = 0;                              // CUs reserved for the side stream (LFM_SIDE_CUS)
  bool s3_yield = false;                         // this call runs schedule 1: nested in a
                                                 // shared hold of the device's tenancy lock
  int last_sched = 0;                            // schedule the last factorisation ran (diag)
  int64_t fallbacks = 0;                         // schedule-3 calls re-run on schedule 1 after a
                                                 // device-side wait timed out (lfm_ctx_fallbacks)
  lfm::Buf<double> gtab;       // gradient tables (grid layout)
  lfm::Buf<double> result;     // [0..] scalar results
  lfm::Buf<double> gacc;       // gradient accumulators + output
  lfm::Buf<double> smp_z;      // joint samples: the normals Z (lfm_randn_f64, lfm_mvn_sample_f64)
  lfm::Buf<double> smp_x;      // joint samples: X = loc + Z L^T

  lfm::Buf<unsigned long long> dbg_stamps;      // lfm_debug_stamps: chain phases 256 x 16, then
                                                // step launches 256 x 8
  lfm::Buf<unsigned long long> dbg_trace;       // lfm_debug_trace: 4 words per step-kernel unit
  int64_t dbg_trace_cap = 0, dbg_trace_cur = 0;  // records allocated / written
  unsigned dbg_trace_launch = 0;                 // launches traced so far

  // pinned host staging
  lfm::Buf<double, true> hpin;

  // profiling
  bool prof = false;
  unsigned prof_mask = ~0u;  // kernel classes timed while prof is on
  lfm_kstat stats[lfm::K_NCLASS];

  // farm (RCCL)
  void* comm = nullptr;
  bool comm_nb = false;  // communicator created non-blocking (calls polled, bounded)
  int nranks = 0, rank = -1;
  lfm::Buf<double> farm_buf;
  lfm::Buf<double, true> farm_h;    // pinned host staging of the all-gather
                                    // (its own: a copy left queued by a timed-
                                    // out call can only ever write here)
  lfm::Buf<double, true> farm_pub;  // coherent pinned: the device-side
                                    // round's gathered slots + seq word
  unsigned farm_seq = 0;    // device-side rounds published so far
  bool farm_stale = false;  // an aborted farm call may have left work queued (drained first)
  // the device-side round captured as one graph (LFM_FARM_GRAPH, default 1; read at creation),
  // replayed while its key (batch id, slots, sign, communicator generation) holds
  hipGraphExec_t farm_exec = nullptr;
  hipGraphExec_t farm_exec_old = nullptr;  // dropped by an aborted round: destroyed once drained
  uint64_t farm_exec_batch = 0, comm_gen = 0, farm_exec_gen = 0;
  int64_t farm_exec_slots = 0;
  int farm_exec_neg = -1;

  // C3's restart pipeline (lfm_mll_multi_f64): evaluation k runs on workspace
  // twin[k % 2], whose first launches (staging, gram, chain(0), X_0, chain(1), step 0) go to the
  // primary's overlap stream (CU-masked: the main CUs less LFM_OVL_RESERVE of them) once the
  // previous evaluation's tail has started, and whose later launches follow the previous
  // evaluation's in the primary's stream pair (m3 / s3, in stream order)
  lfm_ctx* twin[2] = {nullptr, nullptr};
  hipStream_t ovl_stream = nullptr;  // primary: the overlap stream
  bool borrowed = false;             // twin: stream (= the primary's ovl_stream), m3, s3 borrowed
  bool ovl = false;                  // twin: the factorisation in flight runs overlapped
  hipEvent_t ovl_tail = nullptr;     // twin: recorded on m3 ahead of its tail's first launch
  hipEvent_t ovl_done = nullptr;     // twin: recorded on m3 after its finalize
  hipEvent_t ovl_res = nullptr;      // twin: its result copied to the host (primary's stream)
};

// ---------------------------------------------------------------- helpers
namespace lfm {

// Device status word (ctx->status[0], finalize copies it to result[3]): INT_MAX = every pivot
// positive; >= 0 = first non-positive / NaN pivot; STATUS_TIMEOUT = a bounded device-side
// wait ran out (it wins the atomicMin over any pivot index).
constexpr int STATUS_TIMEOUT = -2;
// LFM_OK, LFM_E_NOT_PD (pivot index in the message) or LFM_E_TIMEOUT for a status word.
int status_code(lfm_ctx* ctx, double st, double why = 0.0);

// The next factorisation on ctx runs schedule 3: the CU-partitioned pair exists and the call
// is not nested in a shared hold of the device's tenancy lock (lfm_ctx.hip DeviceTenancy).
inline bool s3_on(const lfm_ctx* ctx) {
  return ctx->knobs.sched == 3 && ctx->side_cus > 0 && !ctx->s3_yield;
}

int set_err(lfm_ctx* ctx, int code, const std::string& msg);
int hip_fail(lfm_ctx* ctx, hipError_t e, const char* what);

// profiling hooks around a launch on ctx->stream
void prof_begin(lfm_ctx* ctx, int cls, hipEvent_t* a, hipStream_t st = nullptr);
// flops / bytes: algorithmic work of the launch; issued (< 0: = flops): what it issues
void prof_end(lfm_ctx* ctx, int cls, hipEvent_t a, double flops, double bytes,
              hipStream_t st = nullptr, double issued = -1.0);
int ensure_events(lfm_ctx* ctx, size_t count);
int prof_flush(lfm_ctx* ctx);

int chain_coresident(lfm_ctx* ctx, hipStream_t st, int G, bool* good);
int gene_clamp_host(double g, int64_t G);

// ------------------------------------------------------ launch wrappers
// Packed parameter block on the device (doubles):
//   [0,G) D   [G,2G) S   [2G,3G) B   then layout-specific arrays.
struct HypDev {
  const double* D;
  const double* S;
  const double* B;
  int G;
  double l;
};

// One problem of the fused small-N kernel: x / y in device memory; its hyperparameters as
// dsb = [true_d(G), true_s(G), true_b(G)] and sc = [l, obs_stddev, jitter], in device memory or
// in pinned host memory the kernel reads directly (lfm_batch: a resident batch uploads nothing
// per call). The kernel stages them in LDS first.
struct SmallProb {
  const double* x;
  const double* y;
  const double* dsb;
  const double* sc;
  int n, G;
  // grid layout (dataset_3d blocks on one uniform time grid; T = 0: none): the gram from the
  // per-gene tables of lfm_gram.hip (tables_doubles(G, T) doubles of LDS)
  int T = 0;
  double dt = 0.0;
  const double* times = nullptr;  // [T]
  const int* bg = nullptr;        // [n / T] gene of each block
};

// gram kernels (lfm_gram.hip)
int launch_tables(lfm_ctx* ctx, const HypDev& h, const GridLayout& lay, const double* d_times,
                  double* tab);
// diagonal elements get (v + da1) + da2 — (K + jitter I) + sigma^2 I, objectives.py:71-72
template <typename OutT>
int launch_gram_grid(lfm_ctx* ctx, const HypDev& h, const GridLayout& lay, const double* tab,
                     const int* bg, int64_t n, double da1, double da2, int uplo, OutT* out,
                     int64_t ldo);
template <typename OutT>
int launch_gram_direct(lfm_ctx* ctx, const HypDev& h, const double* x, int64_t n,
                       const double* x2, int64_t m, double da1, double da2, int uplo, OutT* out,
                       int64_t ldo);
int launch_mean(lfm_ctx* ctx, const HypDev& h, const double* x, int64_t n, double* out);
int launch_h(lfm_ctx* ctx, const HypDev& h, const int64_t* j, const int64_t* k, const double* t1,
             const double* t2, int64_t n, double* out);
int launch_augment(lfm_ctx* ctx, const HypDev& h, const double* x, const double* y,
                   const double* loc, int64_t n, double* A, int64_t lda, int64_t Mp);

// The gram of an aligned grid layout (T % 256 == 0) fused into the factorisation's first
// trailing update (schedule 3): chol_factor_solve writes only the block columns the chains
// and the first panel solve read (launch_gram_region), and the first step's update units
// generate their Sigma tiles from the tables (gram_grid_aligned_kernel's arithmetic, bit-
// identical) instead of loading them. tab: tables_doubles layout; bg: block genes.
struct GramGen {
  const double* tab = nullptr;
  const int* bg = nullptr;
  int G = 0, Tn = 0;
  double da1 = 0.0, da2 = 0.0;
  int64_t n = 0;  // rows >= n (residual, padding) come from memory (augment_kernel)
};
int launch_gram_region(lfm_ctx* ctx, const GramGen& g, int64_t r0, int64_t r1, int64_t c0,
                       int64_t c1, double* out, int64_t ldo);

// the factorisation (lfm_chol_sched.hip; its kernels: lfm_chol.hip, lfm_chol.h)
// CHOL_RESIDENT: CHOL_MLL's matrix and plan, but always on schedule 1, which leaves L in A's
// lower triangle and z in row n (schedule 3 keeps its panels in separate buffers); the
// resident posterior's fit (lfm_post_api.hip)
enum CholMode { CHOL_MLL = 0, CHOL_INVERSE = 1, CHOL_SCHUR = 2, CHOL_RESIDENT = 3 };
// gen: the gram to fuse (lfm_api decides with chol_fuses_gram; the full gram is then NOT in A)
int chol_factor_solve(lfm_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t Mp, int negative,
                      double* d_out, int mode = CHOL_MLL, const GramGen* gen = nullptr);
bool chol_fuses_gram(const lfm_ctx* ctx, int mode, const GridLayout& lay, int64_t n);

// joint samples (lfm_sample.hip): A (stride P.Mp) holds scale's lower triangle and d_loc [n] the
// mean, both on the device. Enqueues the augmented row, the factorisation (CHOL_RESIDENT, in
// place; its status lands in ctx->result), the generator into Z and the product into X (P's
// sizes). Nothing is downloaded and nothing synchronised.
int sample_enqueue(lfm_ctx* ctx, const SamplePlan& P, double* A, const double* d_loc,
                   uint64_t seed, double* Z, double* X);
// Its two halves, for a caller that reads the factor itself (lfm_post_api.hip). scale_factor: the
// augmented row with residual 0 and the factorisation of A (stride Mp, scale n x n) in place, so
// that ctx->result[0] = -1/2 logdet - (n / 2) log 2 pi. sample_draw: everything after it.
int scale_factor(lfm_ctx* ctx, double* A, int64_t n, int64_t Mp, const double* d_loc);
int sample_draw(lfm_ctx* ctx, const SamplePlan& P, double* A, const double* d_loc, uint64_t seed,
                double* Z, double* X);
// The generator alone: rows x ld normals (ld even, pairs = rows ld / 2) of samples sample0 ...
void launch_randn(lfm_ctx* ctx, double* Z, int64_t ld, int64_t rows, int64_t pairs, int grid,
                  uint64_t seed, int64_t sample0);

// The resident posterior (lfm_post.hip: the kernels and these launches, one per step of a call;
// lfm_post_api.hip: the handle and its calls). The sweep kernels' arguments:
struct PostArgs {
  double* Vt;         // the chunk's rows x Np
  int64_t ldv;
  const double* L;
  int64_t ldl;
  const double* dinv;
  const double* z;
  int64_t K0;         // the super-panel's first column
  int w;              // its width in block columns
  int tj0;            // update: first block column to the right
  double* s2;         // per-row sum v^2 over the columns solved so far
  double* sz;         // per-row sum v z
};
// The fit's matrix in L (stride Mp): S = (K + diag_add I) + diag(d_v) (d_v may be NULL), row n
int post_sigma(lfm_ctx* ctx, const HypDev& h, const double* x, const double* d_y,
               const double* d_v, int64_t n, double diag_add, double* L, int64_t Mp);
// A factor as the sweep reads it: z = its row n, row n an identity row, dinv = the inverses of
// its 16 x 16 diagonal blocks. The grids are the caller's. Launches only.
void post_factor_ready(lfm_ctx* ctx, double* L, int64_t ldl, int64_t n, int64_t Np, double* z,
                       double* dinv, unsigned z_grid, unsigned dinv_grid);
// One chunk of a predict as the plan lists it: mean into out [m] and var into out + m
int post_chunk(lfm_ctx* ctx, const PostArgs& g, const ResidentPlan& P, const PostChunk& c,
               const HypDev& h, const double* x, const double* t, double* out);
// cov (m x m, dense) = K(t, t) - Vt Vt^T from the single chunk's solved Vt
int post_cov(lfm_ctx* ctx, const HypDev& h, const ResidentPlan& P, const double* t,
             const double* Vt, double* cov);
// diag_add on A's diagonal in one addition, then scale_factor (lfm_sample.hip) on it
int post_shift_factor(lfm_ctx* ctx, double* A, int64_t m, int64_t Mp, double diag_add,
                      const double* d_loc);
// One pass of held-out rows, already in a.Vt: lp[r] = ctx->result[0] - 0.5 s2[r] after the sweep
int post_logp_pass(lfm_ctx* ctx, const PostArgs& a, const PostLogpPlan& P, const PostChunk& c,
                   const double* mean, double* lp);

// gradient kernels (lfm_grad.hip)
int launch_border_init(lfm_ctx* ctx, double* A, int64_t lda, int64_t Mp);
int posterior_blocked(lfm_ctx* ctx, const HypDev& h, const double* d_x, const double* d_y,
                      int64_t n, const double* d_dv, double diag_add, const double* d_t, int64_t m,
                      double* d_mean, double* d_cov);
int launch_grad(lfm_ctx* ctx, const HypDev& h, const double* d_x, int64_t n, const double* A,
                int64_t lda, int64_t Mp, double obs_stddev, int negative, double* acc,
                double* d_out, const GridLayout* lay = nullptr, const double* d_times = nullptr,
                const int* d_bg = nullptr);
// The same reductions over the leave-one-out weights: W (lower-stored, stride ldw) = W_loo and
// u in the mean terms (lfm_loo.hip computes both)
int launch_grad_loo(lfm_ctx* ctx, const HypDev& h, const double* d_x, int64_t n, const double* W,
                    int64_t ldw, const double* u, double obs_stddev, int negative, double* acc,
                    double* d_out, const GridLayout* lay = nullptr,
                    const double* d_times = nullptr, const int* d_bg = nullptr);
// leave-one-out CV (lfm_loo.hip) on the bordered factor in A (P = plan_loo(n)); vec: P.vec doubles
// of scratch. launch_loo_terms: mu, var, sqrt c, b and the signed value (vec + P.val; NaN on a
// failed factor). launch_loo_weights: u, Bs and the product, W_loo into A + P.w.
int launch_loo_terms(lfm_ctx* ctx, const LooPlan& P, const double* A, const double* d_y,
                     int negative, double* vec);
int launch_loo_weights(lfm_ctx* ctx, const LooPlan& P, double* A, double* vec);
// A resident batch small enough to travel in the kernel arguments (small_mll_kernel_args)
constexpr int SMALL_ARG_PROBS = 16, SMALL_ARG_HYP = 320;
struct SmallArgs {
  SmallProb probs[SMALL_ARG_PROBS];  // dsb / sc unused: the hyperparameters are below
  double hyp[SMALL_ARG_HYP];         // lfm_batch_mll_f64's packed layout
  int dsb_off[SMALL_ARG_PROBS], sc_off[SMALL_ARG_PROBS];
  double* out;
  int* status;
  int negative, tabs;
  double* grad;  // small_grad_kernel_args: the gradient, packed as hyp
};
static_assert(sizeof(SmallArgs) <= 4096, "kernel argument block");
// value and gradient of a batch of small problems (lds: small_grad_lds, non-zero): a = the
// kernel-argument form (problem table and hyperparameters in the arguments) or NULL (d_probs,
// d_offs: the table and each problem's offsets of its vectors [0, nprob) and scalars
// [nprob, 2 nprob) in the packed layout, hyperparameters read through SmallProb::dsb / sc)
int launch_small_grad(lfm_ctx* ctx, SmallArgs* a, const SmallProb* d_probs, const int* d_offs,
                      int nprob, size_t lds, int negative, double* out, double* grad, int* status);
// The optimiser of an on-device fit (lfm_batch_fit_f64, lfm_mbatch_fit_f64), as both fit kernels
// take it (fit_update, lfm_bijectors.h): optax.adam's constants, the count of the steps taken
// before this call, and after_epoch's period (num_steps_per_epoch) and switch (fix_params).
struct AdamOpt {
  double lr, b1, b2, eps, eps_root;
  int64_t step0, spe;
  int fix;
};
// the fit kernel's arguments: every problem's Adam steps on the device (small_fit_kernel)
struct SmallFitLaunch {
  const SmallProb* probs;
  const int* offs;  // [2 nprob]: each problem's offset of its vectors / scalars (packed layout)
  int nprob;
  double *raw, *mu, *nu;  // [nhyp] each, in / out
  double* history;        // [nsteps][nprob]
  const double* bias;     // [nsteps][2]
  int* status;            // [nprob]: 1 + the first step whose factor failed, or 0
  AdamOpt opt;
  int64_t nsteps;
  int negative;
};
int launch_small_fit(lfm_ctx* ctx, const SmallFitLaunch& f, size_t lds);
// the MLL of a batch of small problems (plan: plan_small_mll of the batch's SmallDims), the
// problem table and hyperparameters in the kernel arguments or in device memory
int launch_small_args(lfm_ctx* ctx, SmallArgs& a, int nprob, const SmallMllPlan& plan);
int launch_small_batch(lfm_ctx* ctx, const SmallProb* d_probs, int nprob, const SmallMllPlan& plan,
                       int negative, double* d_out, int* d_status);
void small_batch_attrs();  // the MLL kernels' LDS limit raised (before launches / capture)
// The batched posterior's arguments (small_post_kernel, small_post_cov_kernel), filled from a
// PostPlan
struct SmallPostLaunch {
  const SmallProb* probs;  // the batch's table (x, y, the grid layout; dsb / sc unused)
  const int* offs;         // [2 nprob]: each problem's vectors / scalars in the packed hyp
  const PostProb* pp;      // [nprob]
  int nprob, nsplit, unit; // grid (nprob, nsplit); a workgroup's pass is `unit` test columns
  int ntiles;              // covariance launch: tiles of the whole batch
  const double* hyp;       // device copies of the call's inputs
  const double* dv;        // NULL: no diag_vec
  const double* dadd;
  const double* t;
  double *mean, *var, *V, *cov;  // var or cov may be NULL (V: only with cov)
  int* status;             // [nprob]: 1 + the first failing pivot, or 0
};
int launch_small_post(lfm_ctx* ctx, const SmallPostLaunch& f, size_t lds);

// The mid-size resident batch (lfm_mid.hip: the kernels and launch_mid; lfm_mbatch.hip: the handle
// and its calls). The kernels' argument structs, filled from the plans of lfm_mid_plan.h.
struct MidArgs {
  const MidProb* probs;
  double* base;  // the arena; the packed hyperparameters at its start
  int* status;   // [nprob]: 0, or 1 + the first failing pivot
  int64_t out, grad;
  int negative, k;
};
// The posterior call's second arena and table; `none` for the MLL's fill.
struct MidPostArgs {
  const MidPostProb* pp;
  double* base;
  int64_t dadd;  // diag_add [nprob], doubles from base
  int maxtiles;  // units of the fill launch before the first T unit
};
struct MidNoPost {};
// The fit call's third arena (plan_mid_fit) and optimiser; s: the step of this call, or -1 for
// the constrain before step 0.
struct MidFitArgs {
  double* base;
  int64_t raw, mu, nu, bias, hist;  // doubles from base
  int* first_bad;                   // [nprob]: 1 + the first step whose factor failed, or 0
  AdamOpt opt;
  int64_t s;
  int nprob;
};
// The predictive call's fourth arena (plan_mid_draw) and its table. The launches on it take a
// MidArgs whose table is the second one (n = m_p, offsets into this arena) and whose status words
// are the first arena's: a problem whose S failed is skipped, one whose covariance fails is
// marked there.
struct MidDrawArgs {
  const MidDrawProb* dp;
  double* base;           // the fourth arena
  const double* mean;     // the posterior call's packed mean ...
  const double* cov;      // ... and covariance, in its arena
  const uint64_t* seeds;  // [nprob]
  int64_t cadd;           // cov_add [nprob], doubles from base
  int64_t nsamp;
  uint64_t sample0;
  int maxcb;
  double flops;           // host side: the product's nsamp sum m^2, for the profile
};
// One call's arguments, filled once: `a` always, and of q / f / d those that `has` names
// (MID_HAS_*). launch_mid refuses a launch whose kernel takes a block the call has not filled.
enum : unsigned { MID_HAS_POST = 1, MID_HAS_FIT = 2, MID_HAS_DRAW = 4 };
struct MidCall {
  MidArgs a;
  MidPostArgs q;
  MidFitArgs f;
  MidDrawArgs d;
  MidNoPost none;
  unsigned has;
};
// One launch of a plan's list on ctx->stream. The launch's own fields are set in the block here:
// a.k = l.k, and f.s = l.k for MID_ADAM, -1 for MID_CONSTRAIN.
int launch_mid(lfm_ctx* ctx, const MidLaunch& l, MidCall& c);

// Path of the advisory lock file behind schedule 3's cross-process tenancy (lfm_ctx.hip;
// empty if the device has no PCI bus id)
std::string tenancy_lock_path(int dev);

// Hook of the diagnostics library (liblfm_diag.so, lfm_diag.hip): one launch of the
// trailing-update kernel over a full triangle (lfm_chol_sched.hip; launch only, no kernel of its own)
int probe_update_launch(lfm_ctx* ctx, hipStream_t st, int T, int kd, int cio, int64_t n,
                        size_t xb);

}  // namespace lfm
