// lfm_api_internal.h — what the units of the extern "C" boundary share (lfm_ctx.hip, lfm_api.hip,
// lfm_post_api.hip, lfm_batch.hip, lfm_mbatch.hip, lfm_farm.hip). The kernel units see
// lfm_internal.h only.
#pragma once

#include <algorithm>
#include <functional>

#include "lfm_internal.h"

// A batch of small problems registered once (the C5 ablation farm, notebook.py:33-75): x / y
// and the problem table live in HBM; the packed hyperparameters, the results and the status
// words live in one pinned host buffer the kernel reads and writes directly, so an evaluation is
// one memcpy into that buffer, ONE kernel launch and one stream synchronise — no copy commands.
struct lfm_batch {
  uint64_t id = 0;  // unique per process (never reused): keys the farm's captured graph
  int device = 0;
  int64_t nprob = 0, nhyp = 0;
  std::vector<lfm::SmallShape> shapes;  // what the launch plans are built from
  lfm::SmallDims dims;                  // small_dims(shapes): sizes the MLL launch
  char* dmem = nullptr;     // device: x / y (+ grid times / block genes) of every problem, then
                            // the SmallProb table
  lfm::SmallProb* dprobs = nullptr;
  double* hbuf = nullptr;   // pinned host, coherent, laid out by `lay` (hyp | out | status |
                            // grad); the kernel reads / writes it directly and the host spins on
                            // the status words, so it must not be cached on the device side
  lfm::BatchLayout lay;
  hipEvent_t done = nullptr;  // recorded after every launch on the batch: destroy waits on it
  // small enough for the kernel arguments (LFM_SMALL_KERNARG, default on; read at creation)
  bool use_args = false;
  std::vector<lfm::SmallProb> table;  // host copy of the problem table
  std::vector<int> dsb_off, sc_off;  // each problem's offsets in the packed hyperparameters
  int* doffs = nullptr;              // device: dsb_off then sc_off (the gradient / fit kernels)
  size_t lds_grad = 0, lds_fit = 0;  // the gradient / fit launches' LDS (0: not possible)
  // the fit's device buffer (grown on demand; a call's FitLayout)
  char* fitbuf = nullptr;
  size_t fit_bytes = 0;
};

namespace lfm {

// ------------------------------------------------------------ lfm_ctx.hip
struct DeviceGuard {
  DeviceGuard(int dev) { hipSetDevice(dev); }
};

// The device's tenancy lock, held for the object's lifetime (the rationale: lfm_ctx.hip)
class DeviceTenancy {
 public:
  // s3: the call would run schedule 3 (exclusive); else shared
  DeviceTenancy(lfm_ctx* ctx, bool s3);
  ~DeviceTenancy();
  DeviceTenancy(const DeviceTenancy&) = delete;
  DeviceTenancy& operator=(const DeviceTenancy&) = delete;

 private:
  lfm_ctx* ctx_;
  int dev_ = -1;
  bool excl_ = false, nested_ = false;
};

// the end of a call: ctx->stream synchronised
int finish(lfm_ctx* ctx);
// attempt(), re-run once on schedule 1 if it was a schedule-3 call that stalled
int with_s3_fallback(lfm_ctx* ctx, const std::function<int()>& attempt);
// linvT, status, result and psync (zeroed) of a new context or restart-pipeline workspace
hipError_t alloc_fixed(lfm_ctx* ctx);

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// A call's copies on ctx->stream, in the order given; after the first that fails the rest do
// nothing. e may start as an earlier step's error: the copies then do nothing at all. The strided
// forms move `rows` rows of `width` bytes between pitches dp and sp (bytes).
struct Copies {
  lfm_ctx* ctx;
  hipError_t e = hipSuccess;
  void up(void* dst, const void* src, size_t n) { copy(dst, src, n, hipMemcpyHostToDevice); }
  void down(void* dst, const void* src, size_t n) { copy(dst, src, n, hipMemcpyDeviceToHost); }
  void up2d(void* dst, size_t dp, const void* src, size_t sp, size_t width, size_t rows) {
    copy2d(dst, dp, src, sp, width, rows, hipMemcpyHostToDevice);
  }
  void down2d(void* dst, size_t dp, const void* src, size_t sp, size_t width, size_t rows) {
    copy2d(dst, dp, src, sp, width, rows, hipMemcpyDeviceToHost);
  }
  void dev2d(void* dst, size_t dp, const void* src, size_t sp, size_t width, size_t rows) {
    copy2d(dst, dp, src, sp, width, rows, hipMemcpyDeviceToDevice);
  }
  void zero(void* dst, size_t n) {
    if (e == hipSuccess) e = hipMemsetAsync(dst, 0, n, ctx->stream);
  }
  // the first failure as `what`, or LFM_OK
  int done(const char* what) { return hip_fail(ctx, e, what); }
  // the end of a call's downloads: done(what), then the stream synchronised
  int landed(const char* what) {
    if (int r = done(what)) return r;
    return finish(ctx);
  }

 private:
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  }
  void copy2d(void* dst, size_t dp, const void* src, size_t sp, size_t width, size_t rows,
              hipMemcpyKind kind) {
    if (e == hipSuccess) e = hipMemcpy2DAsync(dst, dp, src, sp, width, rows, kind, ctx->stream);
  }
};

// Where a factorising call's five result words land: the last 8 doubles of ctx->hpin. stage_hyp
// stages from hpin's start and leaves 1 KiB beyond what it uploads, and a call's other pinned
// download (the gradient's ng doubles) starts at hpin[0] in a reservation of ng + 16, so neither
// reaches them.
inline double* result_words(lfm_ctx* ctx) { return ctx->hpin + (ctx->hpin.bytes / 8 - 8); }
// The end of a factorising call: ctx->result's five words to result_words(ctx) after the downloads
// already queued on c, c.landed(what), then the status word's code (LFM_OK, LFM_E_NOT_PD,
// LFM_E_TIMEOUT). *value (optional) is word 0 whenever the copies landed. LFM_E_STATE if the
// caller has not reserved 64 doubles of hpin. What to NaN-fill on which code is the caller's.
int result_tail(Copies& c, const char* what, double* value = nullptr);
// r is one of the status word's failures: the copies landed, the results are not valid
inline bool status_failed(int r) { return r == LFM_E_NOT_PD || r == LFM_E_TIMEOUT; }

// ------------------------------------------- the on-device fits' host half (both batches)
// The kernels' optimiser from the caller's and the count of the steps already taken
inline AdamOpt adam_opt(const lfm_adam* opt, int64_t step0) {
  return {opt->learning_rate, opt->b1, opt->b2, opt->eps, opt->eps_root, step0,
          opt->num_steps_per_epoch, opt->fix_params != 0};
}
// A fit call's staging, raw | mu | nu | bias as its arena lays them out (offsets in doubles from
// the arena's start, the bias table last; gaps are 0): one upload of all of it before the
// launches, one download of [0, bias) after them.
struct FitStaging {
  std::vector<double> par;
  size_t nh, raw, mu, nu, bias;
  FitStaging(const lfm_adam* opt, int64_t step0, int64_t nsteps, int64_t nhyp, size_t raw_at,
             size_t mu_at, size_t nu_at, size_t bias_at, const double* r, const double* m1,
             const double* m2)
      : par(bias_at + 2 * (size_t)nsteps, 0.0), nh((size_t)nhyp), raw(raw_at), mu(mu_at),
        nu(nu_at), bias(bias_at) {
    std::copy(r, r + nh, par.begin() + raw);
    std::copy(m1, m1 + nh, par.begin() + mu);
    std::copy(m2, m2 + nh, par.begin() + nu);
    adam_bias(opt, step0, nsteps, par.data() + bias);
  }
  // the downloaded parameters and moments to the caller; the packed layout's jitter slots pass
  // through unchanged (a static field, model.py:64)
  void back(double* r, double* m1, double* m2) const {
    std::copy(par.begin() + raw, par.begin() + raw + nh, r);
    std::copy(par.begin() + mu, par.begin() + mu + nh, m1);
    std::copy(par.begin() + nu, par.begin() + nu + nh, m2);
  }
};

inline int validate_x(lfm_ctx* ctx, const void* x, int64_t n) {
  if (!ctx) return LFM_E_ARG;
  if (!x) return set_err(ctx, LFM_E_ARG, "x is NULL");
  if (n < 1) return set_err(ctx, LFM_E_ARG, "n must be >= 1");
  if (n > (int64_t)1 << 30) return set_err(ctx, LFM_E_ARG, "n too large");
  return LFM_OK;
}

inline int check_hyp(lfm_ctx* ctx, const lfm_hyp* hyp) {
  if (!hyp) return set_err(ctx, LFM_E_ARG, "hyp is NULL");
  if (hyp->num_genes < 1 || hyp->num_genes > (1 << 20))
    return set_err(ctx, LFM_E_ARG, "num_genes must be in [1, 2^20]");
  if (!hyp->true_d || !hyp->true_s || !hyp->true_b)
    return set_err(ctx, LFM_E_ARG, "hyp true_d / true_s / true_b must not be NULL");
  return LFM_OK;
}

inline int check_mean_shape(lfm_ctx* ctx, int64_t n, const lfm_hyp* hyp) {
  // mean_function (model.py:145-149) repeats B/D in blocks of n // num_genes; the
  // reference's broadcast only succeeds when those blocks tile n exactly.
  if (n % hyp->num_genes != 0)
    return set_err(ctx, LFM_E_ARG,
                   "mean_function needs n divisible by num_genes (model.py:145-149)");
  return LFM_OK;
}

// ------------------------------------------------------------ lfm_api.hip
// Drain and free the restart pipeline's workspaces and its overlap stream
void twins_drop(lfm_ctx* ctx);
// The end of a sampling call: X (P.x_bytes) and the factorisation's status to the host,
// synchronised. Not positive definite: out (and mean, if given) NaN and LFM_E_NOT_PD.
int sample_finish(lfm_ctx* ctx, const SamplePlan& P, const double* X, double* out, double* mean);

// ---------------------------------------------------------- lfm_batch.hip
// small-N batch through one launch; probs already validated
int small_batch(lfm_ctx* ctx, int64_t np, const lfm_problem* probs, const int64_t* idx,
                int negative, double* out, int* status);

// One launch of the batch's MLL kernel: results to `out` (the pinned buffer, or a device buffer
// such as the farm's send slots), the status words (reset to -1 here, each written last by its
// workgroup after a system-scope fence) to the pinned buffer.
int batch_launch(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative, double* out);

// per-problem status words -> status[] (optional; raw: the words themselves, else LFM_OK /
// LFM_E_NOT_PD); LFM_E_NOT_PD, with msg as the context's error, if any problem failed
int batch_status(lfm_ctx* ctx, const int* words, int64_t np, int* status,
                 const char* msg = "Cholesky failed: non-positive pivot in a batch problem",
                 bool raw = false);
// msg of both on-device fits (their words are raw: 1 + the first step whose factor failed)
constexpr const char* FIT_FAILED =
    "Cholesky failed during the fit of a batch problem (its loss and parameters are NaN from "
    "that step on, as JAX's)";

// the status words of the batch's pinned buffer
inline int* batch_words(const lfm_batch* batch) {
  return reinterpret_cast<int*>(batch->hbuf + batch->lay.status);
}
// before a launch: a problem's status word is written last
inline void batch_reset(const lfm_batch* batch) {
  int* hst = batch_words(batch);
  for (int64_t q = 0; q < batch->nprob; ++q) hst[q] = -1;
}

// Result words the host is still waiting for: a signalling-NaN payload that no kernel writes
// (its arithmetic yields values or the canonical quiet NaN; the padding slots are all-ones).
constexpr uint64_t RESULT_PENDING = 0x7FF41F0DCAFE0001ull;
inline void mark_pending(double* p, int64_t count) {
  uint64_t* w = reinterpret_cast<uint64_t*>(p);
  for (int64_t q = 0; q < count; ++q) w[q] = RESULT_PENDING;
}
inline bool all_landed(const double* p, int64_t count) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
  for (int64_t q = 0; q < count; ++q)
    if (__atomic_load_n(&w[q], __ATOMIC_ACQUIRE) == RESULT_PENDING) return false;
  return true;
}

}  // namespace lfm
