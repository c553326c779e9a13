// lfm_mbatch.hip — the C boundary of the resident batch of mid-size problems (include/lfm.h
// lfm_mbatch_*, 1 <= n <= 1024): the handle, its four calls and the entry points. Every size,
// offset and launch comes from the plans of lfm_mid_plan.h; the kernels and launch_mid, which
// issues one launch of a plan's list, are lfm_mid.hip's. This unit defines no kernel.
#include <cstring>
#include <memory>

#include "lfm_api_internal.h"

using namespace lfm;

namespace lfm {

// A device arena its handle owns, grown on demand. Every call on the handle is synchronous:
// nothing of the old allocation is in flight when it is freed.
struct MidArena {
  char* p = nullptr;
  size_t bytes = 0;  // capacity
  double* doubles() const { return reinterpret_cast<double*>(p); }
  // `who` names the entry point in the message
  int grow(lfm_ctx* ctx, size_t need, const std::string& who) {
    if (bytes >= need) return LFM_OK;
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
    const hipError_t e = hipMalloc((void**)&p, need);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return set_err(ctx, LFM_E_OOM, who + ": " + std::to_string(need) +
                                         " bytes of device memory: " + hipGetErrorString(e));
    }
    bytes = need;
    return LFM_OK;
  }
};

}  // namespace lfm

// The handle: the plan, the device arena it lays out, the later calls' arenas, and a pinned buffer
// for a call's packed hyperparameters and results (hyp | out | grad | status words).
struct lfm_mbatch {
  int device = 0;
  MidPlan plan;
  std::vector<lfm::MidShape> shapes;
  char* dmem = nullptr;
  // the posterior, fit and predictive calls' arenas (plan_mid_post, plan_mid_fit, plan_mid_draw)
  enum { POST = 0, FIT, DRAW, ARENAS };
  MidArena arena[ARENAS];
  double* hbuf = nullptr;
  size_t h_out = 0, h_grad = 0, h_status = 0;  // doubles into hbuf

  double* base() const { return reinterpret_cast<double*>(dmem); }
  // a call's status words: in the first arena, and where the host reads them
  int* dev_words() const { return reinterpret_cast<int*>(dmem + plan.status); }
  int* host_words() const { return reinterpret_cast<int*>(hbuf + h_status); }
};

namespace lfm {

namespace {

// The launches on the first arena: its table, base and status words, and where a call's values
// and gradient go.
MidArgs mid_args(const lfm_mbatch* b, int negative) {
  const MidPlan& P = b->plan;
  MidArgs a{};
  a.probs = reinterpret_cast<const MidProb*>(b->dmem + P.table);
  a.base = b->base();
  a.status = b->dev_words();
  a.out = P.out;
  a.grad = P.grad;
  a.negative = negative;
  return a;
}

int mid_launches(lfm_ctx* ctx, const std::vector<MidLaunch>& list, MidCall& c) {
  for (const MidLaunch& l : list)
    if (int r = launch_mid(ctx, l, c)) return r;
  return LFM_OK;
}

// One call: the hyperparameters up, the plan's launches, the results and status words down.
int mid_call(lfm_ctx* ctx, lfm_mbatch* b, const double* hyp, int negative, bool want_grad,
             double* value, double* grad, int* status) {
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared
  const MidPlan& P = b->plan;
  const int64_t np = P.nprob, nh = P.nhyp;
  Copies cp{ctx};
  std::memcpy(b->hbuf, hyp, (size_t)nh * 8);
  cp.up(b->base() + P.hyp, b->hbuf, (size_t)nh * 8);
  if (int r = cp.done("lfm_mbatch: upload")) return r;
  MidCall c{};
  c.a = mid_args(b, negative);
  if (int r = mid_launches(ctx, want_grad ? P.value_grad : P.value, c)) return r;
  cp.down(b->hbuf + b->h_out, b->base() + P.out, (size_t)np * 8);
  if (want_grad) cp.down(b->hbuf + b->h_grad, b->base() + P.grad, (size_t)nh * 8);
  cp.down(b->host_words(), b->dev_words(), (size_t)np * sizeof(int));
  if (int r = cp.landed("lfm_mbatch: download")) return r;
  std::memcpy(value, b->hbuf + b->h_out, (size_t)np * 8);
  if (want_grad) std::memcpy(grad, b->hbuf + b->h_grad, (size_t)nh * 8);
  return batch_status(ctx, b->host_words(), np, status);
}

// One posterior call: the hyperparameters into the first arena, the diagonal and the test inputs
// into the second (grown here when this call needs more), the plan's launches, the outputs down.
// mid_post_enqueue is the first half, which the predictive call shares: the uploads and the
// launches. `who` names the entry point in a message.
int mid_post_enqueue(lfm_ctx* ctx, lfm_mbatch* b, const MidPostPlan& Q, const double* hyp,
                     const double* diag_vec, const double* diag_add, const double* t,
                     const std::string& who) {
  const MidPlan& P = b->plan;
  const int64_t np = P.nprob, nh = P.nhyp;
  MidArena& A = b->arena[lfm_mbatch::POST];
  if (int r = A.grow(ctx, Q.bytes, who)) return r;
  double* pbase = A.doubles();
  Copies cp{ctx};
  std::memcpy(b->hbuf, hyp, (size_t)nh * 8);
  cp.up(b->base() + P.hyp, b->hbuf, (size_t)nh * 8);
  cp.up(pbase + Q.dadd, diag_add, (size_t)np * 8);
  if (diag_vec) cp.up(pbase + Q.dv, diag_vec, (size_t)Q.sn * 8);
  cp.up(pbase + Q.t, t, (size_t)Q.sm * 24);
  cp.up(A.p + Q.table, Q.pp.data(), (size_t)np * sizeof(MidPostProb));
  if (int r = cp.done((who + ": upload").c_str())) return r;
  MidCall c{};
  c.a = mid_args(b, 0);  // out / grad: no launch of this list reads them
  c.q.pp = reinterpret_cast<const MidPostProb*>(A.p + Q.table);
  c.q.base = pbase;
  c.q.dadd = Q.dadd;
  c.q.maxtiles = Q.maxtiles;
  c.has = MID_HAS_POST;
  return mid_launches(ctx, Q.launches, c);
}

int mid_post_call(lfm_ctx* ctx, lfm_mbatch* b, const MidPostPlan& Q, const double* hyp,
                  const double* diag_vec, const double* diag_add, const double* t, double* mean,
                  double* var, double* cov, int* status) {
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared
  if (int r = mid_post_enqueue(ctx, b, Q, hyp, diag_vec, diag_add, t, "lfm_mbatch_posterior_f64"))
    return r;
  const int64_t np = Q.nprob;
  const double* pbase = b->arena[lfm_mbatch::POST].doubles();
  Copies cp{ctx};
  cp.down(mean, pbase + Q.mean, (size_t)Q.sm * 8);
  if (var) cp.down(var, pbase + Q.var, (size_t)Q.sm * 8);
  if (cov) cp.down(cov, pbase + Q.cov, (size_t)Q.sc * 8);
  cp.down(b->host_words(), b->dev_words(), (size_t)np * sizeof(int));
  if (int r = cp.landed("lfm_mbatch_posterior_f64: download")) return r;
  return batch_status(ctx, b->host_words(), np, status);
}

// One predictive call: the posterior call's uploads and launches with the covariance, cov_add,
// ystar, the seeds and the two tables into the fourth arena (grown here when this call needs
// more, before the posterior's arena), the plan's launches on the second table, and logp, the
// samples, the mean and the status words down. A problem whose covariance failed to factor has a
// valid mean on the device: the host replaces it with NaN.
int mid_draw_call(lfm_ctx* ctx, lfm_mbatch* b, const MidPostPlan& Q, const MidDrawPlan& D,
                  const double* hyp, const double* diag_vec, const double* diag_add,
                  const double* t, const double* cov_add, const double* ystar, double* logp,
                  const uint64_t* seeds, double* mean, double* samples, int* status) {
  const std::string who = "lfm_mbatch_predictive_f64";
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared
  const int64_t np = b->plan.nprob;
  MidArena& A = b->arena[lfm_mbatch::DRAW];
  if (int r = A.grow(ctx, D.bytes, who)) return r;
  if (int r = mid_post_enqueue(ctx, b, Q, hyp, diag_vec, diag_add, t, who)) return r;
  const double* pbase = b->arena[lfm_mbatch::POST].doubles();
  double* qbase = A.doubles();
  Copies cp{ctx};
  cp.up(qbase + D.cadd, cov_add, (size_t)np * 8);
  if (ystar) cp.up(qbase + D.ystar, ystar, (size_t)D.sm * 8);
  if (D.nsamp > 0) cp.up(A.p + D.seeds, seeds, (size_t)np * sizeof(uint64_t));
  cp.up(A.p + D.table, D.probs.data(), (size_t)np * sizeof(MidProb));
  cp.up(A.p + D.dtable, D.dp.data(), (size_t)np * sizeof(MidDrawProb));
  if (int r = cp.done("lfm_mbatch_predictive_f64: upload")) return r;
  MidCall c{};
  c.a.probs = reinterpret_cast<const MidProb*>(A.p + D.table);
  c.a.base = qbase;
  c.a.status = b->dev_words();
  c.a.out = D.out;
  c.a.negative = 0;
  c.d.dp = reinterpret_cast<const MidDrawProb*>(A.p + D.dtable);
  c.d.base = qbase;
  c.d.mean = pbase + Q.mean;
  c.d.cov = pbase + Q.cov;
  c.d.seeds = reinterpret_cast<const uint64_t*>(A.p + D.seeds);
  c.d.cadd = D.cadd;
  c.d.nsamp = D.nsamp;
  c.d.sample0 = (uint64_t)D.sample0;
  c.d.maxcb = D.maxcb;
  c.d.flops = (double)D.nsamp * (double)Q.sc;
  c.has = MID_HAS_DRAW;
  if (int r = mid_launches(ctx, D.launches, c)) return r;
  const int* hst = b->host_words();
  cp.down(b->host_words(), b->dev_words(), (size_t)np * sizeof(int));
  if (mean) cp.down(mean, pbase + Q.mean, (size_t)Q.sm * 8);
  if (logp) cp.down(logp, qbase + D.out, (size_t)np * 8);
  if (D.nsamp > 0) cp.down(samples, qbase + D.X, (size_t)(D.nsamp * D.sm) * 8);
  if (int r = cp.landed("lfm_mbatch_predictive_f64: download")) return r;
  if (mean)
    for (int64_t q = 0; q < np; ++q)
      if (hst[q] != 0)
        std::fill(mean + D.dp[q].mean, mean + D.dp[q].mean + D.dp[q].m, std::nan(""));
  return batch_status(ctx, hst, np, status,
                      "Cholesky failed: non-positive pivot in a batch problem's S or in its "
                      "predictive covariance");
}

// One fit call: raw, mu, nu and the bias corrections into the third arena (grown here when this
// call needs more), the plan's launches — the constrain, then per step the value-and-gradient
// launches and the update — enqueued without a host wait between them, one synchronise, and the
// parameters, the history and the first-bad-step words down.
int mid_fit_call(lfm_ctx* ctx, lfm_mbatch* b, const MidFitPlan& F, const lfm_adam* opt,
                 int negative, int64_t step0, double* raw, double* mu, double* nu,
                 double* history, int* status) {
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared, for the whole call
  const int64_t np = b->plan.nprob, nh = b->plan.nhyp, ns = F.nsteps;
  MidArena& A = b->arena[lfm_mbatch::FIT];
  if (int r = A.grow(ctx, F.bytes, "lfm_mbatch_fit_f64")) return r;
  double* fbase = A.doubles();
  // raw | mu | nu | bias are adjacent in the arena (raw at its start): one upload
  FitStaging stage(opt, step0, ns, nh, (size_t)F.raw, (size_t)F.mu, (size_t)F.nu, (size_t)F.bias,
                   raw, mu, nu);
  Copies cp{ctx};
  cp.up(fbase, stage.par.data(), stage.par.size() * 8);
  if (int r = cp.done("lfm_mbatch_fit_f64: upload")) return r;
  MidCall c{};
  c.a = mid_args(b, negative);
  MidFitArgs& f = c.f;
  f.base = fbase;
  f.raw = F.raw;
  f.mu = F.mu;
  f.nu = F.nu;
  f.bias = F.bias;
  f.hist = F.hist;
  f.first_bad = reinterpret_cast<int*>(A.p + F.first_bad);
  f.opt = adam_opt(opt, step0);
  f.nprob = (int)np;
  c.has = MID_HAS_FIT;
  if (int r = mid_launches(ctx, F.launches, c)) return r;
  std::vector<int> st((size_t)np);
  cp.down(stage.par.data(), fbase, (size_t)F.bias * 8);
  cp.down(history, fbase + F.hist, (size_t)(ns * np) * 8);
  cp.down(st.data(), f.first_bad, (size_t)np * sizeof(int));
  if (int r = cp.landed("lfm_mbatch_fit_f64: download")) return r;
  stage.back(raw, mu, nu);
  return batch_status(ctx, st.data(), np, status, FIT_FAILED, true);
}

}  // namespace

}  // namespace lfm

extern "C" {

int lfm_mbatch_create(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, lfm_mbatch** out) {
  if (!ctx) return LFM_E_ARG;
  if (!out || nprob < 1 || !probs) return set_err(ctx, LFM_E_ARG, "bad batch arguments");
  *out = nullptr;
  std::vector<MidShape> shapes((size_t)nprob);
  for (int64_t q = 0; q < nprob; ++q) {
    const lfm_problem& p = probs[q];
    if (int r = validate_x(ctx, p.x, p.n)) return r;
    if (!p.y) return set_err(ctx, LFM_E_ARG, "problem y is NULL");
    shapes[q] = {p.n, p.hyp.num_genes};
  }
  std::unique_ptr<lfm_mbatch> b(new lfm_mbatch);
  b->plan = plan_mid(shapes);
  b->shapes = shapes;
  const MidPlan& P = b->plan;
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  b->device = ctx->device;
  auto even = [](int64_t d) { return (size_t)((d + 1) / 2 * 2); };
  b->h_out = even(P.nhyp);
  b->h_grad = b->h_out + even(P.nprob);
  b->h_status = b->h_grad + even(P.nhyp);
  const size_t hbytes = b->h_status * 8 + (size_t)P.nprob * sizeof(int);
  hipError_t e = hipMalloc((void**)&b->dmem, P.bytes);
  if (e != hipSuccess)
    return set_err(ctx, LFM_E_OOM, "lfm_mbatch_create: " + std::to_string(P.bytes) +
                                       " bytes of device memory: " + hipGetErrorString(e));
  e = hipHostMalloc((void**)&b->hbuf, hbytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemsetAsync(b->dmem, 0, P.bytes, ctx->stream);
  // x / y of every problem (adjacent in the arena), then the table; the staging outlives the copies
  std::vector<std::vector<double>> stagings((size_t)nprob);
  Copies cp{ctx, e};
  for (int64_t q = 0; q < nprob; ++q) {
    const MidProb& m = P.probs[q];
    std::vector<double>& s = stagings[q];
    s.assign((size_t)(m.S - m.x), 0.0);
    std::memcpy(s.data(), probs[q].x, (size_t)m.n * 3 * 8);
    std::memcpy(s.data() + (m.y - m.x), probs[q].y, (size_t)m.n * 8);
    cp.up(b->base() + m.x, s.data(), s.size() * 8);
  }
  cp.up(b->dmem + P.table, P.probs.data(), (size_t)nprob * sizeof(MidProb));
  e = cp.e;
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    hipFree(b->dmem);
    if (b->hbuf) hipHostFree(b->hbuf);
    return hip_fail(ctx, e, "lfm_mbatch_create: upload");
  }
  *out = b.release();
  return LFM_OK;
}

int lfm_mbatch_destroy(lfm_mbatch* batch) {
  if (!batch) return LFM_E_ARG;
  hipSetDevice(batch->device);
  hipFree(batch->dmem);  // every call on the handle is synchronous: nothing of it is in flight
  for (MidArena& a : batch->arena)
    if (a.p) hipFree(a.p);
  hipHostFree(batch->hbuf);
  delete batch;
  return LFM_OK;
}

int lfm_mbatch_hyp_size(const lfm_mbatch* batch, int64_t* out) {
  if (!batch || !out) return LFM_E_ARG;
  *out = batch->plan.nhyp;
  return LFM_OK;
}

int lfm_mbatch_mll_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp, int negative,
                       double* out, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !out) return set_err(ctx, LFM_E_ARG, "batch / hyp / out is NULL");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  return mid_call(ctx, batch, hyp, negative, false, out, nullptr, status);
}

int lfm_mbatch_mll_grad_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp, int negative,
                            double* value, double* grad, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !value || !grad)
    return set_err(ctx, LFM_E_ARG, "batch / hyp / value / grad is NULL");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  return mid_call(ctx, batch, hyp, negative, true, value, grad, status);
}

int lfm_mbatch_posterior_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp,
                             const double* diag_vec, const double* diag_add, const int64_t* m,
                             const double* t, double* mean, double* var, double* cov,
                             int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !diag_add || !m || !t || !mean)
    return set_err(ctx, LFM_E_ARG, "batch / hyp / diag_add / m / t / mean is NULL");
  if (!var && !cov) return set_err(ctx, LFM_E_ARG, "one of var / cov must be given");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  const MidPostPlan Q = plan_mid_post(batch->shapes, m, diag_vec != nullptr, cov != nullptr);
  if (Q.reject) return set_err(ctx, LFM_E_ARG, Q.why);
  return mid_post_call(ctx, batch, Q, hyp, diag_vec, diag_add, t, mean, var, cov, status);
}

int lfm_mbatch_fit_f64(lfm_ctx* ctx, lfm_mbatch* batch, const lfm_adam* opt, int negative,
                       int64_t step0, int64_t nsteps, double* raw, double* mu, double* nu,
                       double* history, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch) return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: batch is NULL");
  if (!opt) return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: opt is NULL");
  if (!raw || !mu || !nu) return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: raw / mu / nu is NULL");
  if (nsteps > 0 && !history) return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: history is NULL");
  if (step0 < 0 || nsteps < 0)
    return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: step0 and nsteps must be >= 0");
  if (opt->num_steps_per_epoch < 1)
    return set_err(ctx, LFM_E_ARG, "lfm_mbatch_fit_f64: num_steps_per_epoch must be >= 1");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  if (nsteps == 0) return LFM_OK;
  const MidFitPlan F = plan_mid_fit(batch->shapes, nsteps);
  if (F.reject) return set_err(ctx, LFM_E_ARG, F.why);
  return mid_fit_call(ctx, batch, F, opt, negative, step0, raw, mu, nu, history, status);
}

int lfm_mbatch_predictive_f64(lfm_ctx* ctx, lfm_mbatch* batch, const double* hyp,
                              const double* diag_vec, const double* diag_add, const int64_t* m,
                              const double* t, const double* cov_add, const double* ystar,
                              double* logp, const uint64_t* seeds, int64_t sample0, int64_t nsamp,
                              double* mean, double* samples, int* status) {
  if (!ctx) return LFM_E_ARG;
  const std::string who = "lfm_mbatch_predictive_f64: ";
  if (!batch || !hyp || !diag_add || !m || !t)
    return set_err(ctx, LFM_E_ARG, who + "batch / hyp / diag_add / m / t is NULL");
  if ((ystar != nullptr) != (logp != nullptr))
    return set_err(ctx, LFM_E_ARG, who + "ystar and logp must be given together");
  if (nsamp > 0 && !seeds) return set_err(ctx, LFM_E_ARG, who + "seeds is NULL with nsamp > 0");
  if ((nsamp > 0) != (samples != nullptr))
    return set_err(ctx, LFM_E_ARG, who + "samples must be given exactly when nsamp > 0");
  if (batch->device != ctx->device)
    return set_err(ctx, LFM_E_ARG, who + "batch of another device");
  const MidDrawPlan D =
      plan_mid_draw(batch->shapes, m, cov_add != nullptr, ystar != nullptr, nsamp, sample0);
  if (D.reject) return set_err(ctx, LFM_E_ARG, D.why);
  const MidPostPlan Q = plan_mid_post(batch->shapes, m, diag_vec != nullptr, true);
  if (Q.reject) return set_err(ctx, LFM_E_ARG, Q.why);
  return mid_draw_call(ctx, batch, Q, D, hyp, diag_vec, diag_add, t, cov_add, ystar, logp, seeds,
                       mean, samples, status);
}

}  // extern "C"
