// lfm_api.hip — the large-N entry points of include/lfm.h: input staging, x-layout detection,
// mean / h / cross-covariance / gram / MLL / gradient / leave-one-out CV / posterior / log_prob /
// joint samples,
// resident data, the C3 restart pipeline and the dispatch of lfm_mll_batch_f64.
//
// Every entry point binds the ctx's device, enqueues on the ctx's stream and is
// synchronous at return (one hipStreamSynchronize per call).
#include <cstring>
#include <memory>

#include "lfm_api_internal.h"

using namespace lfm;

// A device-resident dataset evaluated many times: x (and, for small n, y) read back once,
// the grid layout analysed once per gene count.
struct lfm_data {
  const double* d_x;
  const double* d_y;
  int64_t n;
  int device;
  std::vector<double> xh, yh;
  int64_t lay_G = -1;
  GridLayout lay;
};

namespace lfm {

// -------------------------------------------------------- layout detect
int gene_clamp_host(double g, int64_t G) { return gene_index(g, (int)G); }

namespace {

// ------------------------------------------------------------- staging
struct Staged {
  HypDev h{};
  GridLayout lay;
  const double* d_times = nullptr;
  const int* d_bg = nullptr;
};

// The common preamble of the entry points, in the order their argument errors are reported: x
// and n, the call's other pointers (ptrs: all of them non-NULL, else `what`), hyp, and n against
// num_genes.
int check_problem(lfm_ctx* ctx, const double* x, int64_t n, bool ptrs, const char* what,
                  const lfm_hyp* hyp) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  if (!ptrs) return set_err(ctx, LFM_E_ARG, what);
  r = check_hyp(ctx, hyp);
  if (r) return r;
  return check_mean_shape(ctx, n, hyp);
}

// A device array to the host (synchronous): x for layout detection, y of a small problem.
int read_back(lfm_ctx* ctx, const double* d_ptr, size_t count, std::vector<double>& out,
              const char* what) {
  out.resize(count);
  Copies c{ctx};
  c.down(out.data(), d_ptr, count * 8);
  if (c.e == hipSuccess) c.e = hipStreamSynchronize(ctx->stream);
  return c.done(what);
}

// A problem's x | y into ctx->xin (reserved by the caller): x at 0, y at 3 n
void up_xy(Copies& c, const double* x, const double* y, int64_t n) {
  c.up(c.ctx->xin, x, n * 3 * 8);
  c.up(c.ctx->xin + 3 * n, y, n * 8);
}

// Uploads D, S, B (and, for a grid layout, the time vector and block genes) into ctx->par.
int stage_hyp(lfm_ctx* ctx, const lfm_hyp* hyp, const double* x_host, int64_t n, bool want_grid,
              Staged* st, const GridLayout* known = nullptr) {
  int r = check_hyp(ctx, hyp);
  if (r) return r;
  const int64_t G = hyp->num_genes;
  if (known) st->lay = *known;
  else if (want_grid && x_host) st->lay = detect_grid(x_host, n, G);
  const int64_t T = st->lay.ok ? st->lay.T : 0;
  const int64_t nblk = st->lay.ok ? st->lay.nblk : 0;
  const size_t nd = (size_t)(3 * G + T);
  const size_t bytes = nd * 8 + (size_t)nblk * 4 + 16;
  r = ctx->par.reserve(ctx, bytes);
  if (r) return r;
  r = ctx->hpin.reserve(ctx, std::max<size_t>(bytes + 1024, 1 << 16));
  if (r) return r;
  // the previous call's copy out of hpin has completed (every call ends synchronised)
  double* hp = ctx->hpin;
  std::memcpy(hp, hyp->true_d, G * 8);
  std::memcpy(hp + G, hyp->true_s, G * 8);
  std::memcpy(hp + 2 * G, hyp->true_b, G * 8);
  if (T) std::memcpy(hp + 3 * G, st->lay.times.data(), T * 8);
  if (nblk) std::memcpy(reinterpret_cast<char*>(hp) + nd * 8, st->lay.block_gene.data(), nblk * 4);
  Copies c{ctx};
  c.up(ctx->par, hp, bytes);
  r = c.done("upload hyperparameters");
  if (r) return r;
  st->h = HypDev{ctx->par, ctx->par + G, ctx->par + 2 * G, (int)G, hyp->l};
  st->d_times = ctx->par + 3 * G;
  st->d_bg = reinterpret_cast<const int*>(reinterpret_cast<const char*>(ctx->par.p) + nd * 8);
  return LFM_OK;
}

// The per-gene tables of a grid layout into ctx->tab (the gram fill's and the factorisation's).
int build_tables(lfm_ctx* ctx, const Staged& st) {
  int r = ctx->tab.reserve(ctx, tables_doubles(st.h.G, st.lay.T) * sizeof(double));
  if (r) return r;
  return launch_tables(ctx, st.h, st.lay, st.d_times, ctx->tab);
}

// Build Sigma and factor it: the lower triangle of ctx->A (leading dimension lda) with Sigma =
// (K + jitter I) + sigma^2 I for x on the device (or generated inside the first update), the
// residual row n and identity padding; then the factorisation of `mode` and the reduction into
// ctx->result.
int factor_sigma(lfm_ctx* ctx, const Staged& st, const double* d_x, const double* d_y,
                 const double* d_loc, int64_t n, const lfm_hyp* hyp, int negative, int64_t lda,
                 int mode) {
  const int64_t Mp = round_up(n + 1, 128);
  const double noise = hyp->obs_stddev * hyp->obs_stddev;  // objectives.py:66
  GramGen gen;
  const bool fuse = chol_fuses_gram(ctx, mode, st.lay, n);
  int r = LFM_OK;
  if (st.lay.ok) {
    r = build_tables(ctx, st);
    if (r) return r;
    // fused: the factorisation writes / generates Sigma itself (GramGen, lfm_chol.hip)
    if (fuse) gen = GramGen{ctx->tab, st.d_bg, st.h.G, st.lay.T, hyp->jitter, noise, n};
    else
      r = launch_gram_grid<double>(ctx, st.h, st.lay, ctx->tab, st.d_bg, n, hyp->jitter, noise,
                                   LFM_UPLO_LOWER, ctx->A, lda);
  } else {
    r = launch_gram_direct<double>(ctx, st.h, d_x, n, d_x, n, hyp->jitter, noise,
                                   LFM_UPLO_LOWER, ctx->A, lda);
  }
  if (r) return r;
  r = launch_augment(ctx, st.h, d_x, d_y, d_loc, n, ctx->A, lda, Mp);
  if (r) return r;
  return chol_factor_solve(ctx, ctx->A, lda, n, Mp, negative, ctx->result, mode,
                           fuse ? &gen : nullptr);
}

// Enqueue one MLL on ctx's streams: Sigma in ctx->A (lda = Mp), its factorisation and the
// reduction into ctx->result.
int mll_enqueue(lfm_ctx* ctx, const Staged& st, const double* d_x, const double* d_y,
                const double* d_loc, int64_t n, const lfm_hyp* hyp, int negative) {
  return factor_sigma(ctx, st, d_x, d_y, d_loc, n, hyp, negative, round_up(n + 1, 128), CHOL_MLL);
}

// The scalar result of the factorisation just enqueued, to the host (synchronous): NaN with the
// status word's error.
int read_result(lfm_ctx* ctx, double* out) {
  Copies c{ctx};
  int r = result_tail(c, "download the result", out);
  if (status_failed(r)) *out = std::nan("");
  return r;
}

// mll_enqueue, then the result to the host (synchronous).
int mll_blocked(lfm_ctx* ctx, const Staged& st, const double* d_x, const double* d_y,
                const double* d_loc, int64_t n, const lfm_hyp* hyp, int negative, double* out) {
  const int64_t Mp = round_up(n + 1, 128);
  int r = ctx->A.reserve(ctx, (size_t)Mp * Mp * sizeof(double));
  if (r) return r;
  DeviceTenancy tenancy(ctx, s3_on(ctx));  // held to the final synchronise (finish)
  return with_s3_fallback(ctx, [&]() -> int {
    int r = mll_enqueue(ctx, st, d_x, d_y, d_loc, n, hyp, negative);
    return r ? r : read_result(ctx, out);
  });
}

template <typename OutT>
int gram_impl(lfm_ctx* ctx, const double* x_host, const double* d_x, int64_t n,
              const lfm_hyp* hyp, double diag_add, int uplo, OutT* d_out, int64_t ldo) {
  Staged st;
  int r = stage_hyp(ctx, hyp, x_host, n, true, &st);
  if (r) return r;
  if (st.lay.ok) {
    r = build_tables(ctx, st);
    if (r) return r;
    return launch_gram_grid<OutT>(ctx, st.h, st.lay, ctx->tab, st.d_bg, n, diag_add, 0.0, uplo,
                                  d_out, ldo);
  }
  return launch_gram_direct<OutT>(ctx, st.h, d_x, n, d_x, n, diag_add, 0.0, uplo, d_out, ldo);
}

template <typename OutT>
int gram_host(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp, double diag_add,
              int uplo, OutT* out, int64_t ldo) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  if (!out || ldo < n) return set_err(ctx, LFM_E_ARG, "out is NULL or ldo < n");
  if (uplo != LFM_UPLO_FULL && uplo != LFM_UPLO_LOWER) return set_err(ctx, LFM_E_ARG, "bad uplo");
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);
  r = ctx->xin.reserve(ctx, (size_t)n * 3 * 8);
  if (r) return r;
  r = ctx->A.reserve(ctx, (size_t)n * n * sizeof(OutT));
  if (r) return r;
  OutT* dA = reinterpret_cast<OutT*>(ctx->A.p);
  Copies c{ctx};
  c.up(ctx->xin, x, n * 3 * 8);
  if (uplo == LFM_UPLO_LOWER) c.zero(dA, (size_t)n * n * sizeof(OutT));
  r = c.done("upload x");
  if (!r) r = gram_impl<OutT>(ctx, x, ctx->xin, n, hyp, diag_add, uplo, dA, n);
  if (r) return r;
  c.down2d(out, ldo * sizeof(OutT), dA, n * sizeof(OutT), n * sizeof(OutT), n);
  return c.landed("download gram");
}

template <typename OutT>
int gram_dev(lfm_ctx* ctx, const double* d_x, int64_t n, const lfm_hyp* hyp, double diag_add,
             int uplo, OutT* d_out, int64_t ldo) {
  int r = validate_x(ctx, d_x, n);
  if (r) return r;
  if (!d_out || ldo < n) return set_err(ctx, LFM_E_ARG, "out is NULL or ldo < n");
  if (uplo != LFM_UPLO_FULL && uplo != LFM_UPLO_LOWER) return set_err(ctx, LFM_E_ARG, "bad uplo");
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);
  std::vector<double> xh;
  r = read_back(ctx, d_x, (size_t)n * 3, xh, "read back x for layout detection");
  if (r) return r;
  r = gram_impl<OutT>(ctx, xh.data(), d_x, n, hyp, diag_add, uplo, d_out, ldo);
  if (r) return r;
  return finish(ctx);
}

// ------------------------------------------------------ C3 restart pipeline
// Workspace i of ctx's restart pipeline (lfm_mll_multi_f64): an lfm_ctx with its own buffers,
// events and flags, whose streams are ctx's — m3 / s3 (in stream order after the previous
// evaluation's launches) and the overlap stream (CU-masked: every CU outside the chain's and the
// first LFM_OVL_RESERVE main CUs, which the previous evaluation's tail keeps).
int twin_get(lfm_ctx* ctx, int i, lfm_ctx** out) {
  if (ctx->twin[i]) {
    *out = ctx->twin[i];
    return LFM_OK;
  }
  if (!ctx->ovl_stream) {
    const int lo = std::min(ctx->cus - 64, ctx->side_cus + ctx->knobs.ovl_reserve);
    std::vector<uint32_t> mk((ctx->cus + 31) / 32, 0u);
    for (int c = lo; c < ctx->cus; ++c) mk[c / 32] |= 1u << (c % 32);
    hipError_t e = hipExtStreamCreateWithCUMask(&ctx->ovl_stream, (uint32_t)mk.size(), mk.data());
    if (e != hipSuccess) {
      ctx->ovl_stream = nullptr;
      return hip_fail(ctx, e, "overlap stream");
    }
  }
  std::unique_ptr<lfm_ctx> t(new lfm_ctx());
  t->borrowed = true;
  t->device = ctx->device;
  t->stream = ctx->ovl_stream;
  t->m3 = ctx->m3;
  t->s3 = ctx->s3;
  t->side_cus = ctx->side_cus;
  t->cus = ctx->cus;
  t->knobs = ctx->knobs;
  t->knobs.sched = 3;
  t->knobs.s3_fallback = false;  // lfm_mll_multi_f64 re-runs a stalled set itself
  std::memset(t->stats, 0, sizeof(t->stats));
  hipError_t e = alloc_fixed(t.get());
  for (hipEvent_t* ev : {&t->ovl_tail, &t->ovl_done, &t->ovl_res})
    if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) {
    lfm_ctx_destroy(t.release());
    return hip_fail(ctx, e, "restart pipeline workspace");
  }
  *out = ctx->twin[i] = t.release();
  return LFM_OK;
}

}  // namespace

// Drain and free the pipeline's workspaces and its overlap stream (the pair they borrow is
// about to go, or the context is).
void twins_drop(lfm_ctx* ctx) {
  if (ctx->borrowed || (!ctx->twin[0] && !ctx->twin[1] && !ctx->ovl_stream)) return;
  for (hipStream_t st : {ctx->ovl_stream, ctx->m3, ctx->s3, ctx->stream})
    if (st) hipStreamSynchronize(st);
  for (lfm_ctx*& t : ctx->twin) {
    lfm_ctx_destroy(t);
    t = nullptr;
  }
  if (ctx->ovl_stream) hipStreamDestroy(ctx->ovl_stream);
  ctx->ovl_stream = nullptr;
}

// lfm_loocv_f64 (grad NULL) and lfm_loocv_grad_f64 (loo_mean, loo_var NULL), arguments checked:
// lfm_mll_grad_f64's route to the bordered factor, then the leave-one-out terms off its bottom
// block and, for the gradient, W_loo inside the same matrix (LooPlan) and the gradient's own
// reductions over it.
int loo_blocked(lfm_ctx* ctx, const double* x, const double* y, int64_t n, const lfm_hyp* hyp,
                int negative, double* value, double* loo_mean, double* loo_var, double* grad) {
  const LooPlan P = plan_loo(n);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  Staged st;
  int r = stage_hyp(ctx, hyp, x, n, true, &st);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 4 * 8);
  if (r) return r;
  const double* d_x = ctx->xin;
  const double* d_y = ctx->xin + 3 * n;
  Copies up{ctx};
  up_xy(up, x, y, n);
  r = up.done("upload x / y");
  if (!r) r = ctx->A.reserve(ctx, P.mat_bytes);
  // gacc: the gradient's accumulators and output (as lfm_mll_grad_f64), then the plan's vectors
  const int64_t G = hyp->num_genes;
  const size_t nacc = (size_t)(5 * G + 3), ng = grad ? (size_t)(3 * G + 2) : 0;
  if (!r) r = ctx->gacc.reserve(ctx, nacc * sizeof(double) + P.vec_bytes);
  if (r) return r;
  DeviceTenancy tenancy(ctx, s3_on(ctx));  // held to the final synchronise (finish)
  return with_s3_fallback(ctx, [&]() -> int {
    int r = factor_sigma(ctx, st, d_x, d_y, nullptr, n, hyp, negative, P.ld, CHOL_INVERSE);
    if (r) return r;
    double* vec = ctx->gacc + nacc;
    double* d_out = ctx->gacc + 2 * G + 1;
    r = launch_loo_terms(ctx, P, ctx->A, d_y, negative, vec);
    // a failed factor is known only on the device: the weights and the reductions run regardless,
    // on what may be NaN or Inf, and every output is NaN-filled below (lfm_loo.hip's header)
    if (!r && grad) r = launch_loo_weights(ctx, P, ctx->A, vec);
    if (!r && grad)
      r = launch_grad_loo(ctx, st.h, d_x, n, ctx->A + P.w, P.ld, vec + P.u, hyp->obs_stddev,
                          negative, ctx->gacc, d_out, &st.lay, st.d_times, st.d_bg);
    if (r) return r;
    r = ctx->hpin.reserve(ctx, (ng + 1 + 16) * sizeof(double));
    if (r) return r;
    Copies c{ctx};
    if (grad) c.down(ctx->hpin, d_out, ng * sizeof(double));
    c.down(ctx->hpin + ng, vec + P.val, sizeof(double));
    if (loo_mean) c.down(loo_mean, vec + P.mu, n * 8);
    if (loo_var) c.down(loo_var, vec + P.var, n * 8);
    r = result_tail(c, "download the leave-one-out results");
    if (r == LFM_OK) {
      *value = ctx->hpin[ng];
      if (grad) std::memcpy(grad, ctx->hpin, ng * sizeof(double));
    } else if (status_failed(r)) {
      const double nan = std::nan("");
      *value = nan;
      if (grad) std::fill(grad, grad + ng, nan);
      if (loo_mean) std::fill(loo_mean, loo_mean + n, nan);
      if (loo_var) std::fill(loo_var, loo_var + n, nan);
    }
    return r;
  });
}

int sample_finish(lfm_ctx* ctx, const SamplePlan& P, const double* X, double* out, double* mean) {
  Copies c{ctx};
  c.down(out, X, P.x_bytes);
  int r = result_tail(c, "download the samples");
  if (r == LFM_E_NOT_PD) {
    std::fill(out, out + P.nsamp * P.n, std::nan(""));
    if (mean) std::fill(mean, mean + P.n, std::nan(""));
  }
  return r;
}

}  // namespace lfm

// =================================================================== C ABI
extern "C" {

int lfm_mean_function_f64(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp,
                          double* out) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  if (!out) return set_err(ctx, LFM_E_ARG, "out is NULL");
  DeviceGuard g(ctx->device);
  Staged st;
  r = stage_hyp(ctx, hyp, x, n, false, &st);
  if (r) return r;
  r = check_mean_shape(ctx, n, hyp);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 4 * 8);
  if (r) return r;
  Copies c{ctx};
  c.up(ctx->xin, x, n * 3 * 8);
  r = c.done("upload x");
  if (!r) r = launch_mean(ctx, st.h, ctx->xin, n, ctx->xin + 3 * n);
  if (r) return r;
  c.down(out, ctx->xin + 3 * n, n * 8);
  return c.landed("download the mean");
}

int lfm_h_f64(lfm_ctx* ctx, const lfm_hyp* hyp, const int64_t* j, const int64_t* k,
              const double* t1, const double* t2, int64_t n, double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!j || !k || !t1 || !t2 || !out || n < 1) return set_err(ctx, LFM_E_ARG, "bad h arguments");
  DeviceGuard g(ctx->device);
  Staged st;
  int r = stage_hyp(ctx, hyp, nullptr, 0, false, &st);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 5 * 8);
  if (r) return r;
  int64_t* dj = reinterpret_cast<int64_t*>(ctx->xin.p);
  int64_t* dk = dj + n;
  double* dt1 = ctx->xin + 2 * n;
  double* dt2 = ctx->xin + 3 * n;
  double* dout = ctx->xin + 4 * n;
  Copies c{ctx};
  c.up(dj, j, n * 8);
  c.up(dk, k, n * 8);
  c.up(dt1, t1, n * 8);
  c.up(dt2, t2, n * 8);
  r = c.done("upload j / k / t1 / t2");
  if (!r) r = launch_h(ctx, st.h, dj, dk, dt1, dt2, n, dout);
  if (r) return r;
  c.down(out, dout, n * 8);
  return c.landed("download h");
}

int lfm_cross_covariance_f64(lfm_ctx* ctx, const double* x, int64_t n, const double* x2,
                             int64_t m, const lfm_hyp* hyp, double* out, int64_t ldo) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  r = validate_x(ctx, x2, m);
  if (r) return r;
  if (!out || ldo < m) return set_err(ctx, LFM_E_ARG, "out is NULL or ldo < m");
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);
  Staged st;
  r = stage_hyp(ctx, hyp, nullptr, 0, false, &st);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)(n + m) * 3 * 8);
  if (r) return r;
  r = ctx->A.reserve(ctx, (size_t)n * m * 8);
  if (r) return r;
  Copies c{ctx};
  c.up(ctx->xin, x, n * 3 * 8);
  c.up(ctx->xin + 3 * n, x2, m * 3 * 8);
  r = c.done("upload x / x2");
  if (!r) r = launch_gram_direct<double>(ctx, st.h, ctx->xin, n, ctx->xin + 3 * n, m, 0.0, 0.0,
                                 LFM_UPLO_FULL, ctx->A, m);
  if (r) return r;
  c.down2d(out, ldo * 8, ctx->A, m * 8, m * 8, n);
  return c.landed("download cross-covariance");
}

int lfm_gram_f64(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp, double diag_add,
                 int uplo, double* out, int64_t ldo) {
  return gram_host<double>(ctx, x, n, hyp, diag_add, uplo, out, ldo);
}

int lfm_gram_f32(lfm_ctx* ctx, const double* x, int64_t n, const lfm_hyp* hyp, double diag_add,
                 int uplo, float* out, int64_t ldo) {
  return gram_host<float>(ctx, x, n, hyp, diag_add, uplo, out, ldo);
}

int lfm_gram_f64_dev(lfm_ctx* ctx, const double* d_x, int64_t n, const lfm_hyp* hyp,
                     double diag_add, int uplo, double* d_out, int64_t ldo) {
  return gram_dev<double>(ctx, d_x, n, hyp, diag_add, uplo, d_out, ldo);
}

int lfm_gram_f32_dev(lfm_ctx* ctx, const double* d_x, int64_t n, const lfm_hyp* hyp,
                     double diag_add, int uplo, float* d_out, int64_t ldo) {
  return gram_dev<float>(ctx, d_x, n, hyp, diag_add, uplo, d_out, ldo);
}

int lfm_mll_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n, const lfm_hyp* hyp,
                int negative, double* out) {
  int r = check_problem(ctx, x, n, y && out, "y / out is NULL", hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  if (n <= SMALL_MAX) {
    lfm_problem p{x, y, n, *hyp};
    int64_t idx = 0;
    int st = 0;
    r = small_batch(ctx, 1, &p, &idx, negative, out, &st);
    if (r) return r;
    if (st) return set_err(ctx, LFM_E_NOT_PD, "Cholesky failed: non-positive pivot");
    return LFM_OK;
  }
  Staged st;
  r = stage_hyp(ctx, hyp, x, n, true, &st);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 4 * 8);
  if (r) return r;
  Copies c{ctx};
  up_xy(c, x, y, n);
  r = c.done("upload x / y");
  return r ? r : mll_blocked(ctx, st, ctx->xin, ctx->xin + 3 * n, nullptr, n, hyp, negative, out);
}

int lfm_mll_grad_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                     const lfm_hyp* hyp, int negative, double* value, double* grad) {
  int r = check_problem(ctx, x, n, y && value && grad, "y / value / grad is NULL", hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  Staged st;
  r = stage_hyp(ctx, hyp, x, n, true, &st);
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 4 * 8);
  if (r) return r;
  const double* d_x = ctx->xin;
  const double* d_y = ctx->xin + 3 * n;
  Copies up{ctx};
  up_xy(up, x, y, n);
  r = up.done("upload x / y");
  // bordered 2Mp x 2Mp matrix [[S_aug, .], [I, 0]] (lfm_grad.hip)
  const int64_t Mp = round_up(n + 1, 128), M2 = 2 * Mp;
  if (!r) r = ctx->A.reserve(ctx, (size_t)M2 * M2 * sizeof(double));
  const int64_t G = hyp->num_genes;
  if (!r) r = ctx->gacc.reserve(ctx, (size_t)(5 * G + 3) * sizeof(double));
  if (r) return r;
  DeviceTenancy tenancy(ctx, s3_on(ctx));  // held to the final synchronise (finish)
  return with_s3_fallback(ctx, [&]() -> int {
    int r = factor_sigma(ctx, st, d_x, d_y, nullptr, n, hyp, negative, M2, CHOL_INVERSE);
    if (r) return r;
    double* d_out = ctx->gacc + 2 * G + 1;
    r = launch_grad(ctx, st.h, d_x, n, ctx->A, M2, Mp, hyp->obs_stddev, negative, ctx->gacc, d_out,
                    &st.lay, st.d_times, st.d_bg);
    if (r) return r;
    const size_t ng = (size_t)(3 * G + 2);
    r = ctx->hpin.reserve(ctx, (ng + 16) * sizeof(double));
    if (r) return r;
    Copies c{ctx};
    c.down(ctx->hpin, d_out, ng * sizeof(double));
    r = result_tail(c, "download the gradient", value);
    if (r == LFM_OK) {
      std::memcpy(grad, ctx->hpin, ng * sizeof(double));
    } else if (status_failed(r)) {
      *value = std::nan("");
      for (size_t i = 0; i < ng; ++i) grad[i] = std::nan("");
    }
    return r;
  });
}

int lfm_loocv_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n, const lfm_hyp* hyp,
                  int negative, double* value, double* loo_mean, double* loo_var) {
  int r = check_problem(ctx, x, n, y && value, "y / value is NULL", hyp);
  if (r) return r;
  return loo_blocked(ctx, x, y, n, hyp, negative, value, loo_mean, loo_var, nullptr);
}

int lfm_loocv_grad_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                       const lfm_hyp* hyp, int negative, double* value, double* grad) {
  int r = check_problem(ctx, x, n, y && value && grad, "y / value / grad is NULL", hyp);
  if (r) return r;
  return loo_blocked(ctx, x, y, n, hyp, negative, value, nullptr, nullptr, grad);
}

int lfm_posterior_f64(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                      const double* diag_vec, double diag_add, const double* t, int64_t m,
                      const lfm_hyp* hyp, double* mean, double* cov) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  // t and m in x's place; n against num_genes follows (the same message as m's)
  r = check_problem(ctx, t, m, y && mean && cov, "y / mean / cov is NULL", hyp);
  if (r) return r;
  r = check_mean_shape(ctx, n, hyp);
  if (r) return r;
  if ((n + m) > (int64_t)1 << 17) return set_err(ctx, LFM_E_ARG, "n + m too large");
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // schedule 1 (Schur complement), shared
  Staged st;
  r = stage_hyp(ctx, hyp, nullptr, 0, false, &st);
  if (r) return r;
  // xin: x (3n) y (n) v (n) t (3m) mean (m) cov (m*m)
  const size_t nd = 5 * (size_t)n + 4 * (size_t)m + (size_t)m * m;
  r = ctx->xin.reserve(ctx, nd * 8);
  if (r) return r;
  double* d_x = ctx->xin;
  double* d_y = d_x + 3 * n;
  double* d_v = d_y + n;
  double* d_t = d_v + n;
  double* d_mean = d_t + 3 * m;
  double* d_cov = d_mean + m;
  Copies c{ctx};
  up_xy(c, x, y, n);
  if (diag_vec) c.up(d_v, diag_vec, n * 8);
  c.up(d_t, t, m * 3 * 8);
  r = c.done("upload x / y / diag_vec / t");
  if (!r) r = posterior_blocked(ctx, st.h, d_x, d_y, n, diag_vec ? d_v : nullptr, diag_add, d_t, m,
                        d_mean, d_cov);
  if (r) return r;
  c.down(mean, d_mean, m * 8);
  c.down(cov, d_cov, (size_t)m * m * 8);
  r = result_tail(c, "download mean / cov");
  if (status_failed(r)) {
    const double nan = std::nan("");
    for (int64_t i = 0; i < m; ++i) mean[i] = nan;
    for (int64_t i = 0; i < m * m; ++i) cov[i] = nan;
  }
  return r;
}

int lfm_mll_f64_dev(lfm_ctx* ctx, const double* d_x, const double* d_y, int64_t n,
                    const lfm_hyp* hyp, int negative, double* out) {
  int r = check_problem(ctx, d_x, n, d_y && out, "y / out is NULL", hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  std::vector<double> xh;
  r = read_back(ctx, d_x, (size_t)n * 3, xh, "read back x for layout detection");
  if (r) return r;
  if (n <= SMALL_MAX) {
    std::vector<double> yh;
    r = read_back(ctx, d_y, (size_t)n, yh, "read back y");
    if (r) return r;
    return lfm_mll_f64(ctx, xh.data(), yh.data(), n, hyp, negative, out);
  }
  Staged st;
  r = stage_hyp(ctx, hyp, xh.data(), n, true, &st);
  if (r) return r;
  return mll_blocked(ctx, st, d_x, d_y, nullptr, n, hyp, negative, out);
}

int lfm_data_create(lfm_ctx* ctx, const double* d_x, const double* d_y, int64_t n,
                    lfm_data** out) {
  int r = validate_x(ctx, d_x, n);
  if (r) return r;
  if (!d_y || !out) return set_err(ctx, LFM_E_ARG, "y / out is NULL");
  DeviceGuard g(ctx->device);
  std::unique_ptr<lfm_data> d(new lfm_data);
  d->d_x = d_x;
  d->d_y = d_y;
  d->n = n;
  d->device = ctx->device;
  r = read_back(ctx, d_x, (size_t)n * 3, d->xh, "read back the dataset");
  if (!r && n <= SMALL_MAX) r = read_back(ctx, d_y, (size_t)n, d->yh, "read back the dataset");
  if (r) return r;
  *out = d.release();
  return LFM_OK;
}

int lfm_data_destroy(lfm_data* data) {
  delete data;
  return LFM_OK;
}

int lfm_mll_f64_data(lfm_ctx* ctx, lfm_data* data, const lfm_hyp* hyp, int negative,
                     double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!data || !out) return set_err(ctx, LFM_E_ARG, "data / out is NULL");
  if (data->device != ctx->device) return set_err(ctx, LFM_E_ARG, "dataset of another device");
  int r = check_hyp(ctx, hyp);
  if (r) return r;
  const int64_t n = data->n;
  r = check_mean_shape(ctx, n, hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  if (n <= SMALL_MAX) return lfm_mll_f64(ctx, data->xh.data(), data->yh.data(), n, hyp, negative, out);
  if (data->lay_G != hyp->num_genes) {
    data->lay = detect_grid(data->xh.data(), n, hyp->num_genes);
    data->lay_G = hyp->num_genes;
  }
  Staged st;
  r = stage_hyp(ctx, hyp, data->xh.data(), n, true, &st, &data->lay);
  if (r) return r;
  return mll_blocked(ctx, st, data->d_x, data->d_y, nullptr, n, hyp, negative, out);
}

// C3 (BASELINE.json configs[2]): nsets hyperparameter sets on one resident dataset. On schedule
// 3 the evaluations are pipelined over two workspaces: evaluation k + 1's prologue (staging, its
// gram tables / region, chain(0), X_0, chain(1) and step 0) runs on the overlap stream while
// evaluation k is in its chain-bound tail, and the rest of it follows evaluation k's launches
// on the partitioned pair. Every evaluation runs the same kernels on the same inputs as
// lfm_mll_f64_data: the values are bit-identical. Otherwise (small n, schedule 1, profiling,
// LFM_OVERLAP=0, differing gene counts) the sets are evaluated one by one.
int lfm_mll_multi_f64(lfm_ctx* ctx, lfm_data* data, int64_t nsets, const lfm_hyp* hyps,
                      int negative, double* out, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!data || !out || nsets < 0 || (nsets > 0 && !hyps))
    return set_err(ctx, LFM_E_ARG, "data / hyps / out is NULL or nsets < 0");
  if (data->device != ctx->device) return set_err(ctx, LFM_E_ARG, "dataset of another device");
  const int64_t n = data->n;
  bool same_genes = true;
  for (int64_t k = 0; k < nsets; ++k) {
    int r = check_hyp(ctx, &hyps[k]);
    if (!r) r = check_mean_shape(ctx, n, &hyps[k]);
    if (r) return r;
    same_genes = same_genes && hyps[k].num_genes == hyps[0].num_genes;
  }
  DeviceGuard g(ctx->device);
  int worst = LFM_OK;
  // one set through lfm_mll_f64_data (its own schedule-3 fallback): NOT_PD -> NaN and status
  auto one = [&](int64_t k) -> int {
    int r = lfm_mll_f64_data(ctx, data, &hyps[k], negative, &out[k]);
    if (status) status[k] = r;
    if (r == LFM_E_NOT_PD) {
      out[k] = std::nan("");
      worst = LFM_E_NOT_PD;
      return LFM_OK;
    }
    return r;
  };
  const bool pipelined = nsets >= 2 && n > SMALL_MAX && ctx->knobs.ovl_on && s3_on(ctx) &&
                         !ctx->prof && ctx->knobs.s3_events == 0 && !ctx->dbg_stamps &&
                         !ctx->dbg_trace && same_genes;
  if (!pipelined) {
    for (int64_t k = 0; k < nsets; ++k)
      if (int r = one(k)) return r;
    if (worst) set_err(ctx, LFM_E_NOT_PD, "Cholesky failed for at least one hyperparameter set");
    return worst;
  }
  if (data->lay_G != hyps[0].num_genes) {
    data->lay = detect_grid(data->xh.data(), n, hyps[0].num_genes);
    data->lay_G = hyps[0].num_genes;
  }
  DeviceTenancy tenancy(ctx, true);  // exclusive, to the last result
  const int64_t Mp = round_up(n + 1, 128);
  lfm_ctx* tw[2];
  for (int i = 0; i < 2; ++i) {
    int r = twin_get(ctx, i, &tw[i]);
    if (!r) r = tw[i]->A.reserve(tw[i], (size_t)Mp * Mp * sizeof(double));
    if (!r) r = tw[i]->hpin.reserve(tw[i], 1 << 16);
    if (r) {
      if (r != LFM_E_ARG) ctx->err = tw[i]->err.empty() ? ctx->err : tw[i]->err;
      return r;
    }
  }
  // enqueue set k on workspace k % 2, its prologue gated on set k - 1's tail
  auto enqueue = [&](int64_t k) -> int {
    lfm_ctx* t = tw[k & 1];
    t->ovl = true;
    t->err.clear();
    if (k > 0) hipStreamWaitEvent(t->stream, tw[(k - 1) & 1]->ovl_tail, 0);
    Staged st;
    int r = stage_hyp(t, &hyps[k], data->xh.data(), n, true, &st, &data->lay);
    if (!r) r = mll_enqueue(t, st, data->d_x, data->d_y, nullptr, n, &hyps[k], negative);
    if (!r) {
      hipStreamWaitEvent(ctx->stream, t->ovl_done, 0);
      Copies c{ctx};  // the workspace's result on the primary's stream
      c.down(result_words(t), t->result, 5 * sizeof(double));
      hipEventRecord(t->ovl_res, ctx->stream);
      r = c.done("restart pipeline result copy");
      if (!r) r = hip_fail(ctx, hipGetLastError(), "restart pipeline enqueue");
    } else {
      ctx->err = t->err;
    }
    return r;
  };
  // the host side of set k: LFM_OK / LFM_E_NOT_PD (NaN), LFM_E_TIMEOUT (the caller re-runs)
  auto collect = [&](int64_t k) -> int {
    lfm_ctx* t = tw[k & 1];
    hipError_t e = hipEventSynchronize(t->ovl_res);
    if (e != hipSuccess) return hip_fail(ctx, e, "restart pipeline result");
    const double* h = result_words(t);
    out[k] = h[0];
    int r = status_code(t, h[3], h[4]);
    if (status) status[k] = r;
    if (r == LFM_E_NOT_PD) {
      out[k] = std::nan("");
      worst = LFM_E_NOT_PD;
      r = LFM_OK;
    }
    if (r) ctx->err = t->err;
    return r;
  };
  auto drain = [&] {
    for (hipStream_t st : {ctx->ovl_stream, ctx->m3, ctx->s3, ctx->stream})
      if (st) hipStreamSynchronize(st);
    tw[0]->ovl = tw[1]->ovl = false;
  };
  int64_t done = 0;  // sets collected
  int r = enqueue(0);
  for (int64_t k = 1; !r && k <= nsets; ++k) {
    if (k < nsets) r = enqueue(k);
    if (!r) {
      r = collect(k - 1);
      if (!r) done = k;
    }
  }
  drain();
  if (r == LFM_E_TIMEOUT) {
    // a device-side wait ran out (another tenant starved the chain): the rest one by one,
    // each with lfm_mll_f64_data's own schedule-1 re-run
    ctx->fallbacks += 1;
    r = LFM_OK;
    for (int64_t k = done; !r && k < nsets; ++k) r = one(k);
  }
  if (r) return r;
  if (worst) set_err(ctx, LFM_E_NOT_PD, "Cholesky failed for at least one hyperparameter set");
  return worst;
}

int lfm_mll_batch_f64(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, int negative,
                      double* out, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (nprob < 0 || (nprob > 0 && (!probs || !out)))
    return set_err(ctx, LFM_E_ARG, "bad batch arguments");
  DeviceGuard g(ctx->device);
  std::vector<int64_t> small, big;
  for (int64_t q = 0; q < nprob; ++q) {
    const lfm_problem& p = probs[q];
    int r = check_problem(ctx, p.x, p.n, p.y, "problem y is NULL", &p.hyp);
    if (r) return r;
    (p.n <= SMALL_MAX ? small : big).push_back(q);
  }
  int worst = LFM_OK;
  if (!small.empty()) {
    int r = small_batch(ctx, (int64_t)small.size(), probs, small.data(), negative, out, status);
    if (r) return r;
  }
  for (int64_t q : big) {
    int r = lfm_mll_f64(ctx, probs[q].x, probs[q].y, probs[q].n, &probs[q].hyp, negative, &out[q]);
    if (status) status[q] = r;
    if (r && r != LFM_E_NOT_PD) return r;  // LFM_E_TIMEOUT included: never a NaN slot
  }
  if (status)
    for (int64_t q = 0; q < nprob; ++q)
      if (status[q] == LFM_E_NOT_PD) worst = LFM_E_NOT_PD;
  return worst;
}

int lfm_log_prob_f64(lfm_ctx* ctx, const double* loc, const double* scale, int64_t n,
                     int64_t lds, const double* y, double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!loc || !scale || !y || !out || n < 1 || lds < n)
    return set_err(ctx, LFM_E_ARG, "bad log_prob arguments");
  DeviceGuard g(ctx->device);
  const int64_t Mp = round_up(n + 1, 128);
  int r = ctx->A.reserve(ctx, (size_t)Mp * Mp * sizeof(double));
  if (r) return r;
  r = ctx->xin.reserve(ctx, (size_t)n * 2 * 8);
  if (r) return r;
  Copies c{ctx};
  c.up(ctx->xin, loc, n * 8);
  c.up(ctx->xin + n, y, n * 8);
  r = c.done("upload loc / y");
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  DeviceTenancy tenancy(ctx, s3_on(ctx));  // held to the final synchronise (finish)
  return with_s3_fallback(ctx, [&]() -> int {
    // the factorisation overwrites A: a fallback re-run uploads scale again
    Copies c{ctx};
    c.up2d(ctx->A, Mp * 8, scale, lds * 8, n * 8, n);
    int r = c.done("upload scale");
    if (r) return r;
    HypDev h{nullptr, nullptr, nullptr, 1, 1.0};
    r = launch_augment(ctx, h, nullptr, ctx->xin + n, ctx->xin, n, ctx->A, Mp, Mp);
    if (r) return r;
    r = chol_factor_solve(ctx, ctx->A, Mp, n, Mp, 0, ctx->result);
    return r ? r : read_result(ctx, out);
  });
}

int lfm_randn_f64(lfm_ctx* ctx, uint64_t seed, int64_t sample0, int64_t nsamp, int64_t n,
                  double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!out) return set_err(ctx, LFM_E_ARG, "out is NULL");
  const SamplePlan P = plan_sample(n, nsamp, sample0);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // no factorisation: shared
  // the generator alone: nsamp rows of ld = n rounded up to a pair
  const int64_t ld = (n + 1) / 2 * 2, pairs = nsamp * (ld / 2);
  int r = ctx->smp_z.reserve(ctx, (size_t)nsamp * ld * sizeof(double));
  if (r) return r;
  launch_randn(ctx, ctx->smp_z, ld, nsamp, pairs,
               (int)std::min<int64_t>((pairs + 255) / 256, SAMPLE_RANDN_GRID), seed, sample0);
  r = hip_fail(ctx, hipGetLastError(), "sample_randn_kernel");
  if (r) return r;
  Copies c{ctx};
  c.down2d(out, n * 8, ctx->smp_z, ld * 8, n * 8, nsamp);
  return c.landed("download the normals");
}

int lfm_mvn_sample_f64(lfm_ctx* ctx, const double* loc, const double* scale, int64_t n,
                       int64_t lds, uint64_t seed, int64_t sample0, int64_t nsamp, double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!loc || !scale || !out) return set_err(ctx, LFM_E_ARG, "loc / scale / out is NULL");
  const SamplePlan P = plan_sample(n, nsamp, sample0);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  if (lds < n) return set_err(ctx, LFM_E_ARG, "lds must be >= n");
  DeviceGuard g(ctx->device);
  int r = ctx->A.reserve(ctx, P.mat_bytes);
  if (!r) r = ctx->smp_z.reserve(ctx, P.z_bytes);
  if (!r) r = ctx->smp_x.reserve(ctx, P.x_bytes);
  if (!r) r = ctx->xin.reserve(ctx, (size_t)n * sizeof(double));
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  DeviceTenancy tenancy(ctx, false);  // CHOL_RESIDENT is schedule 1: shared
  Copies c{ctx};
  c.up(ctx->xin, loc, n * 8);
  c.up2d(ctx->A, P.Mp * 8, scale, lds * 8, n * 8, n);
  r = c.done("upload loc / scale");
  if (!r) r = sample_enqueue(ctx, P, ctx->A, ctx->xin, seed, ctx->smp_z, ctx->smp_x);
  if (r) return r;
  return sample_finish(ctx, P, ctx->smp_x, out, nullptr);
}

}  // extern "C"
