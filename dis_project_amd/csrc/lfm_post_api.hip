// lfm_post_api.hip — the resident posterior's handle and entry points (include/lfm.h lfm_post_*).
// No kernel is defined here: every launch is one of lfm_post.hip's steps (lfm_internal.h), every
// copy goes through Copies and every size and grid is a plan's (lfm_host.cpp). What the calls
// compute, and in which order, is described at the head of lfm_post.hip.
#include "lfm_api_internal.h"
#include "lfm_chol.h"

using namespace lfm;

namespace lfm {

// A device buffer of the handle's, grown on demand and freed with it
struct PostBuf {
  double* p = nullptr;
  size_t cap = 0;
  PostBuf() = default;
  PostBuf(const PostBuf&) = delete;
  PostBuf& operator=(const PostBuf&) = delete;
  ~PostBuf() { hipFree(p); }  // NULL: nothing
  operator double*() const { return p; }
  int grow(lfm_ctx* ctx, size_t bytes, const char* what) {
    if (bytes <= cap) return LFM_OK;
    // every call ends synchronised: nothing in flight reads the old allocation
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc((void**)&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return set_err(ctx, LFM_E_OOM, std::string("out of device memory: ") + what + " needs " +
                                         std::to_string(bytes) + " bytes");
    }
    cap = bytes;
    return LFM_OK;
  }
};

}  // namespace lfm

struct lfm_post {
  lfm_ctx* owner = nullptr;  // the creating context: takes lfm_post_set_chunk's message
  int device = 0;
  int64_t n = 0, Np = 0, Mp = 0, G = 0;
  int64_t chunk = 0;         // 0: post_default_chunk(Np)
  double l = 0.0;
  // fixed at creation: the factor (Mp x Mp, Mp = round_up(n + 1, 128), lower triangle), the
  // Np / 128 x 8 inverses of its 16 x 16 diagonal blocks, z [Np] (zero from n), x [n x 3] and
  // D, S, B
  PostBuf L, dinv, z, x, par;
  // grown by the predicts (ResidentPlan's byte counts)
  PostBuf vt, acc, t, out, cov;
  // grown by the samples (SamplePlan's byte counts): the covariance's factor, Z and X
  PostBuf smat, sz, sx;
  // grown by the log densities (PostLogpPlan's byte counts): the inverses of the covariance
  // factor's diagonal blocks, the sweep's zero z and one pass's results
  PostBuf sdinv, szero, lp;

  HypDev hyp() const { return {par, par + G, par + 2 * G, (int)G, l}; }
};

namespace lfm {
namespace {

// The lfm_post_* calls' first three checks, in their order
int post_check(lfm_ctx* ctx, const lfm_post* post) {
  if (!ctx) return LFM_E_ARG;
  if (!post) return set_err(ctx, LFM_E_ARG, "post is NULL");
  if (ctx->device != post->device)
    return set_err(ctx, LFM_E_ARG, "the handle belongs to another device than this ctx");
  return LFM_OK;
}

// The sweep's arguments (PostArgs' order) over the handle's Vt and accumulators (rows: vt_rows)
PostArgs post_args(const lfm_post* q, int64_t ldv, const double* L, int64_t ldl,
                   const double* dinv, const double* z, int64_t rows) {
  return {q->vt, ldv, L, ldl, dinv, z, 0, 0, 0, q->acc, q->acc + rows};
}

int post_fit(lfm_ctx* ctx, lfm_post* q, const double* x, const double* y, const double* diag_vec,
             double diag_add, const lfm_hyp* hyp) {
  const int64_t n = q->n, G = q->G, Np = q->Np, Mp = q->Mp;
  int r = q->L.grow(ctx, (size_t)Mp * Mp * sizeof(double), "the resident factor");
  if (!r)
    r = q->dinv.grow(ctx, (size_t)(Np / NB) * NB * IB * sizeof(double), "the diagonal inverses");
  if (!r) r = q->z.grow(ctx, (size_t)Np * sizeof(double), "z");
  if (!r) r = q->x.grow(ctx, (size_t)n * 3 * sizeof(double), "x");
  if (!r) r = q->par.grow(ctx, (size_t)G * 3 * sizeof(double), "the hyperparameters");
  // y and the variances are only read while S is built: the ctx's staging
  if (!r) r = ctx->xin.reserve(ctx, (size_t)n * 2 * sizeof(double));
  if (!r) r = ctx->hpin.reserve(ctx, 64 * sizeof(double));
  if (r) return r;
  double* d_y = ctx->xin;
  double* d_v = d_y + n;
  Copies c{ctx};
  c.up(q->x, x, n * 3 * 8);
  c.up(d_y, y, n * 8);
  if (diag_vec) c.up(d_v, diag_vec, n * 8);
  c.up(q->par, hyp->true_d, G * 8);
  c.up(q->par + G, hyp->true_s, G * 8);
  c.up(q->par + 2 * G, hyp->true_b, G * 8);
  r = c.done("resident posterior: upload");
  if (!r) r = post_sigma(ctx, q->hyp(), q->x, d_y, diag_vec ? d_v : nullptr, n, diag_add, q->L, Mp);
  if (!r) r = chol_factor_solve(ctx, q->L, Mp, n, Mp, 0, ctx->result, CHOL_RESIDENT);
  if (r) return r;
  post_factor_ready(ctx, q->L, Mp, n, Np, q->z, q->dinv, (unsigned)((Np + 255) / 256),
                    (unsigned)(Np / NB));
  r = hip_fail(ctx, hipGetLastError(), "post_dinv_kernel");
  return r ? r : result_tail(c, "resident posterior: the fit's status");
}

// One predict with the covariance when the plan has it, left on the device: mean in q->out [m],
// var in q->out + m (marginals only), cov in q->cov (m x m, dense). Nothing is downloaded.
int post_enqueue(lfm_ctx* ctx, lfm_post* q, const ResidentPlan& P, const double* t) {
  const bool cov = P.cov_bytes != 0;
  int r = q->vt.grow(ctx, P.vt_bytes, "the solve workspace");
  if (!r) r = q->acc.grow(ctx, P.acc_bytes, "the row accumulators");
  if (!r) r = q->t.grow(ctx, P.t_bytes, "the test inputs");
  if (!r) r = q->out.grow(ctx, P.out_bytes, "mean / var");
  if (!r && cov) r = q->cov.grow(ctx, P.cov_bytes, "the covariance");
  if (r) return r;
  Copies c{ctx};
  c.up(q->t, t, P.t_bytes);
  r = c.done("resident posterior: upload t");
  if (r) return r;
  const HypDev h = q->hyp();
  const PostArgs g = post_args(q, P.Np, q->L, q->Mp, q->dinv, q->z, P.vt_rows);
  for (const PostChunk& ch : P.chunks) {
    r = post_chunk(ctx, g, P, ch, h, q->x, q->t, q->out);
    if (r) return r;
  }
  // one chunk (the plan rejected anything else): its Vt is whole
  return cov ? post_cov(ctx, h, P, q->t, q->vt, q->cov) : LFM_OK;
}

// The first steps of a sample and of a log density, in stream order: the predict with the
// covariance (mean in q->out, cov in q->cov), cov into the Mp-stride matrix q->smat, diag_add on
// its diagonal in one addition, the augmented row with residual 0 and the factorisation, which
// leaves L in q->smat's lower triangle, the status in ctx->result[3] and
// ctx->result[0] = -1/2 logdet - (m / 2) log 2 pi. q->smat holds Mp x Mp doubles.
int post_scale_factor(lfm_ctx* ctx, lfm_post* q, const ResidentPlan& P, int64_t Mp, const double* t,
                      double diag_add) {
  int r = post_enqueue(ctx, q, P, t);
  if (r) return r;
  const int64_t m = P.m;
  Copies c{ctx};
  c.dev2d(q->smat, Mp * 8, q->cov, m * 8, m * 8, m);
  r = c.done("the covariance into the factor's stride");
  return r ? r : post_shift_factor(ctx, q->smat, m, Mp, diag_add, q->out);
}

}  // namespace
}  // namespace lfm

extern "C" {

int lfm_post_create(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                    const double* diag_vec, double diag_add, const lfm_hyp* hyp, lfm_post** out) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  if (out) *out = nullptr;
  if (!y || !out) return set_err(ctx, LFM_E_ARG, "y / out is NULL");
  r = check_hyp(ctx, hyp);
  if (!r) r = check_mean_shape(ctx, n, hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // schedule 1, shared
  lfm_post* q = new lfm_post;
  q->owner = ctx;
  q->device = ctx->device;
  q->n = n;
  q->G = hyp->num_genes;
  q->Np = round_up(n, NB);
  q->Mp = round_up(n + 1, NB);
  q->l = hyp->l;
  r = post_fit(ctx, q, x, y, diag_vec, diag_add, hyp);
  if (r) {
    hipStreamSynchronize(ctx->stream);
    delete q;
    return r;
  }
  *out = q;
  return LFM_OK;
}

int lfm_post_destroy(lfm_post* post) {
  if (!post) return LFM_E_ARG;
  DeviceGuard g(post->device);
  delete post;  // its buffers with it (PostBuf)
  return LFM_OK;
}

int lfm_post_set_chunk(lfm_post* post, int64_t rows) {
  if (!post) return LFM_E_ARG;
  if (rows < 0 || rows % 128 != 0)
    return set_err(post->owner, LFM_E_ARG, "the chunk must be a multiple of 128 rows (0: default)");
  post->chunk = rows;
  return LFM_OK;
}

int lfm_post_predict_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double* mean,
                         double* var, double* cov) {
  int r = post_check(ctx, post);
  if (r) return r;
  if (!t || !mean) return set_err(ctx, LFM_E_ARG, "t / mean is NULL");
  if (!var && !cov) return set_err(ctx, LFM_E_ARG, "one of var / cov must be given");
  lfm_post* q = post;
  const ResidentPlan P = plan_post(q->n, q->G, m, q->chunk, cov != nullptr);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // no factorisation: shared
  r = post_enqueue(ctx, q, P, t);
  if (r) return r;
  Copies c{ctx};
  c.down(mean, q->out, (size_t)m * 8);
  if (cov) c.down(cov, q->cov, P.cov_bytes);
  else c.down(var, q->out + m, (size_t)m * 8);
  r = c.landed("resident posterior: download");
  if (r) return r;
  if (cov && var)
    for (int64_t i = 0; i < m; ++i) var[i] = cov[i * m + i];  // diag(cov), bit for bit
  return LFM_OK;
}

int lfm_post_sample_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                        uint64_t seed, int64_t sample0, int64_t nsamp, double* mean,
                        double* out) {
  int r = post_check(ctx, post);
  if (r) return r;
  if (!t || !out) return set_err(ctx, LFM_E_ARG, "t / out is NULL");
  lfm_post* q = post;
  const ResidentPlan P = plan_post(q->n, q->G, m, q->chunk, true);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  const SamplePlan S = plan_sample(m, nsamp, sample0);
  if (S.reject) return set_err(ctx, LFM_E_ARG, S.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // CHOL_RESIDENT is schedule 1: shared
  r = q->smat.grow(ctx, S.mat_bytes, "the covariance's factor");
  if (!r) r = q->sz.grow(ctx, S.z_bytes, "the normals");
  if (!r) r = q->sx.grow(ctx, S.x_bytes, "the samples");
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  r = post_scale_factor(ctx, q, P, S.Mp, t, diag_add);
  if (r) return r;
  r = sample_draw(ctx, S, q->smat, q->out, seed, q->sz, q->sx);
  if (r) return r;
  Copies c{ctx};
  if (mean) c.down(mean, q->out, (size_t)m * 8);
  r = c.done("resident posterior: download the mean");
  return r ? r : sample_finish(ctx, S, q->sx, out, mean);
}

int lfm_post_log_prob_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                          const double* ystar, int64_t k, double* mean, double* logp) {
  int r = post_check(ctx, post);
  if (r) return r;
  if (!t || !ystar || !logp) return set_err(ctx, LFM_E_ARG, "t / ystar / logp is NULL");
  lfm_post* q = post;
  const PostLogpPlan P = plan_post_logp(q->n, q->G, m, k, q->chunk);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // CHOL_RESIDENT is schedule 1: shared
  // the predict's Vt and accumulators serve the residual rows once the covariance is formed:
  // grown to the larger of the two uses before the predict, which then finds them large enough
  r = q->vt.grow(ctx, P.vt_bytes, "the solve workspace");
  if (!r) r = q->acc.grow(ctx, P.acc_bytes, "the row accumulators");
  if (!r) r = q->smat.grow(ctx, P.mat_bytes, "the covariance's factor");
  if (!r) r = q->sdinv.grow(ctx, P.dinv_bytes, "its diagonal inverses");
  if (!r) r = q->szero.grow(ctx, P.zero_bytes, "the zero z");
  if (!r) r = q->lp.grow(ctx, P.logp_bytes, "the log densities");
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  r = post_scale_factor(ctx, q, P.pred, P.Mp, t, diag_add);
  if (r) return r;
  // the factor as the sweep reads it: row m, which holds L^{-1} 0, becomes the identity row its
  // neighbours are and its zeros become the sweep's z; then the diagonal blocks' inverses. The
  // sweep reads the factor's 16 x 16 diagonal blocks through these inverses alone (built from
  // their lower triangles) and everything else strictly below them, so the input entries the
  // factorisation leaves above the diagonal are never read.
  post_factor_ready(ctx, q->smat, P.Mp, m, P.Np, q->szero, q->sdinv, (unsigned)P.z_grid,
                    (unsigned)P.dinv_grid);
  const PostArgs a = post_args(q, P.Np, q->smat, P.Mp, q->sdinv, q->szero, P.rows.vt_rows);
  Copies up{ctx}, down{ctx};
  for (const PostChunk& ch : P.rows.chunks) {
    r = down.done("held-out log density: download");
    if (r) return r;
    up.up2d(q->vt, P.Np * 8, ystar + ch.q0 * m, m * 8, m * 8, ch.rows);
    r = up.done("upload ystar");
    if (!r) r = post_logp_pass(ctx, a, P, ch, q->out, q->lp);
    if (r) return r;
    down.down(logp + ch.q0, q->lp, (size_t)ch.rows * 8);
  }
  if (mean) down.down(mean, q->out, (size_t)m * 8);
  r = result_tail(down, "held-out log density: download");
  if (r == LFM_E_NOT_PD) {
    std::fill(logp, logp + k, std::nan(""));
    if (mean) std::fill(mean, mean + m, std::nan(""));
  }
  return r;
}

}  // extern "C"
