// lfm_batch.hip — the small problems (n <= 128, one workgroup each) behind include/lfm.h: the
// per-call batch of lfm_mll_f64 / lfm_mll_batch_f64 and the resident lfm_batch with its MLL,
// gradient, fit and posterior calls.
#include <atomic>
#include <chrono>
#include <climits>
#include <cstring>
#include <memory>

#include "lfm_api_internal.h"

using namespace lfm;

namespace lfm {

namespace {

// host: detect the grid layout of problem p and, when its tables fit the kernel's budget, put
// its times and block genes at hd (device address dd) and fill sp's grid fields; returns the
// doubles used (at most small_grid_doubles(n))
int64_t small_grid_pack(const double* x, int64_t n, int64_t G, SmallProb& sp, double* hd,
                        const double* dd) {
  sp.T = 0;
  const GridLayout lay = detect_grid(x, n, G);
  if (!lay.ok || tables_doubles((int)G, lay.T) > (size_t)SMALL_GRID_TAB_MAX) return 0;
  const int64_t T = lay.T, nblk = lay.nblk;
  std::memcpy(hd, lay.times.data(), T * 8);
  std::memcpy(hd + T, lay.block_gene.data(), nblk * sizeof(int));
  sp.T = (int)T;
  sp.dt = lay.dt;
  sp.times = dd;
  sp.bg = reinterpret_cast<const int*>(dd + T);
  return T + (nblk + 1) / 2;
}

// One small problem into the staging area hd (device address dd) from double `off` on, and its
// table entry sp: x (3n), y (n), its hyperparameters D S B (3G) l obs_stddev jitter (3) when
// dsb is NULL (else sp points at the caller's dsb / sc), then the grid times / block genes.
// Returns the offset past it; dims follows the problems packed so far.
size_t pack_small(const lfm_problem& p, double* hd, const double* dd, size_t off,
                  const double* dsb, const double* sc, SmallProb& sp, SmallDims& dims) {
  const int64_t n = p.n, G = p.hyp.num_genes;
  std::memcpy(hd + off, p.x, 3 * n * 8);
  sp.x = dd + off;
  off += 3 * n;
  std::memcpy(hd + off, p.y, n * 8);
  sp.y = dd + off;
  off += n;
  if (!dsb) {
    dsb = dd + off;
    std::memcpy(hd + off, p.hyp.true_d, G * 8);
    std::memcpy(hd + off + G, p.hyp.true_s, G * 8);
    std::memcpy(hd + off + 2 * G, p.hyp.true_b, G * 8);
    off += 3 * G;
    sc = dd + off;
    hd[off] = p.hyp.l;
    hd[off + 1] = p.hyp.obs_stddev;
    hd[off + 2] = p.hyp.jitter;
    off += 3;
  }
  sp.dsb = dsb;
  sp.sc = sc;
  sp.n = (int)n;
  sp.G = (int)G;
  off += small_grid_pack(p.x, n, G, sp, hd + off, dd + off);
  dims.maxn = std::max<int>(dims.maxn, (int)n);
  dims.maxg = std::max<int>(dims.maxg, (int)G);
  if (sp.T)
    dims.gridtab = std::max<int>(dims.gridtab, (int)small_grid_extra((int)n, (int)G, sp.T));
  return off;
}

// the kernel-argument form of a resident batch: the problem table and the hyperparameters
void fill_small_args(const lfm_batch* batch, const double* hyp, SmallArgs& a) {
  const size_t np = (size_t)batch->nprob;
  std::memcpy(a.probs, batch->table.data(), np * sizeof(SmallProb));
  std::memcpy(a.hyp, hyp, (size_t)batch->nhyp * 8);
  std::memcpy(a.dsb_off, batch->dsb_off.data(), np * sizeof(int));
  std::memcpy(a.sc_off, batch->sc_off.data(), np * sizeof(int));
}

// The previous call on a batch returned on its status words, possibly before its kernel had
// retired: a fault past that point surfaces at the batch's next call (this query of that launch's
// completion event, long signalled in the normal case), not at some later synchronise.
int batch_prev_ok(lfm_ctx* ctx, const lfm_batch* batch) {
  if (!batch->done) return LFM_OK;
  const hipError_t e = hipEventQuery(batch->done);
  if (e != hipSuccess && e != hipErrorNotReady)
    return hip_fail(ctx, e, "the batch's previous launch");
  return LFM_OK;
}

// The host side of a call whose kernel writes results and status words into the batch's
// pinned buffer: spin until EVERY word the call reads has landed — the status words (-1 before
// the launch), the results and the gradient (RESULT_PENDING before the launch) — rather than on
// the status words alone: each word is its own completion flag, so the host never depends on the
// order in which two posted writes to host memory become visible (the kernel's system-scope fence
// orders their issue). ~µs sooner than the kernel's end-of-dispatch signal
// behind hipStreamSynchronize; past 20 ms, or while profiling (the events want the stream),
// synchronise the stream instead, which also surfaces a kernel fault.
int batch_wait(lfm_ctx* ctx, int64_t np, const int* hst, const double* vals, int64_t nv,
               const double* grads = nullptr, int64_t ng = 0) {
  bool landed = false;
  if (!ctx->prof) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      landed = true;
      for (int64_t q = 0; q < np && landed; ++q)
        landed = __atomic_load_n(&hst[q], __ATOMIC_ACQUIRE) != -1;
      landed = landed && all_landed(vals, nv) && all_landed(grads, ng);
      if (landed || std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
      __builtin_ia32_pause();
    }
  }
  return landed ? LFM_OK : finish(ctx);
}

}  // namespace

int small_batch(lfm_ctx* ctx, int64_t np, const lfm_problem* probs, const int64_t* idx,
                int negative, double* out, int* status) {
  // packed device buffer: per problem x(3n) y(n) D S B (3G) l obs_stddev jitter (3) doubles;
  // then the SmallProb array
  size_t nd = 0;
  for (int64_t q = 0; q < np; ++q) {
    const lfm_problem& p = probs[idx[q]];
    nd += 4 * (size_t)p.n + 3 * (size_t)p.hyp.num_genes + 3 + small_grid_doubles(p.n);
  }
  const size_t bytes_d = nd * 8;
  const size_t bytes_p = (size_t)np * sizeof(SmallProb);
  const size_t bytes_o = (size_t)np * (8 + 4);
  const size_t total = round_up(bytes_d, 16) + round_up(bytes_p, 16) + bytes_o + 64;
  int r = ctx->xin.reserve(ctx, total);
  if (r) return r;
  r = ctx->hpin.reserve(ctx, total + 4096);
  if (r) return r;
  char* hb = reinterpret_cast<char*>(ctx->hpin.p);
  char* db = reinterpret_cast<char*>(ctx->xin.p);
  double* hd = reinterpret_cast<double*>(hb);
  SmallProb* hp = reinterpret_cast<SmallProb*>(hb + round_up(bytes_d, 16));
  const double* dd = reinterpret_cast<const double*>(db);
  SmallDims dims;
  size_t off = 0;
  for (int64_t q = 0; q < np; ++q) {
    SmallProb sp;
    off = pack_small(probs[idx[q]], hd, dd, off, nullptr, nullptr, sp, dims);
    hp[q] = sp;
  }
  const size_t up = round_up(bytes_d, 16) + bytes_p;
  hipError_t e = hipMemcpyAsync(db, hb, up, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "upload small batch");
  double* d_out = reinterpret_cast<double*>(db + round_up(bytes_d, 16) + round_up(bytes_p, 16));
  int* d_st = reinterpret_cast<int*>(d_out + np);
  r = launch_small_batch(ctx, reinterpret_cast<const SmallProb*>(db + round_up(bytes_d, 16)),
                         (int)np, dims.maxn, dims.maxg, dims.gridtab, negative, d_out, d_st);
  if (r) return r;
  double* h_out = reinterpret_cast<double*>(hb + round_up(bytes_d, 16) + round_up(bytes_p, 16));
  e = hipMemcpyAsync(h_out, d_out, np * 12, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "download small batch");
  r = finish(ctx);
  if (r) return r;
  const int* h_st = reinterpret_cast<const int*>(h_out + np);
  for (int64_t q = 0; q < np; ++q) {
    out[idx[q]] = h_out[q];
    if (status) status[idx[q]] = h_st[q] ? LFM_E_NOT_PD : LFM_OK;
  }
  return LFM_OK;
}

int batch_launch(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative, double* out) {
  if (int r = batch_prev_ok(ctx, batch)) return r;
  const int np = (int)batch->nprob;
  const SmallDims& d = batch->dims;
  int* hst = batch_words(batch);
  batch_reset(batch);
  int r;
  if (batch->use_args) {
    // the problem table and the hyperparameters travel in the kernel arguments
    SmallArgs a;
    fill_small_args(batch, hyp, a);
    a.out = out;
    a.status = hst;
    a.negative = negative;
    r = launch_small_args(ctx, a, np, d.maxn, d.maxg, d.gridtab);
  } else {
    std::memcpy(batch->hbuf, hyp, (size_t)batch->nhyp * 8);
    r = launch_small_batch(ctx, batch->dprobs, np, d.maxn, d.maxg, d.gridtab, negative, out, hst);
  }
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  return LFM_OK;
}

int batch_status(lfm_ctx* ctx, const int* words, int64_t np, int* status, const char* msg,
                 bool raw) {
  int worst = LFM_OK;
  for (int64_t q = 0; q < np; ++q) {
    const int s = words[q] ? LFM_E_NOT_PD : LFM_OK;
    if (status) status[q] = raw ? words[q] : s;
    if (s) worst = s;
  }
  if (worst) set_err(ctx, LFM_E_NOT_PD, msg);
  return worst;
}

}  // namespace lfm

extern "C" {

int lfm_batch_create(lfm_ctx* ctx, int64_t nprob, const lfm_problem* probs, lfm_batch** out) {
  if (!ctx) return LFM_E_ARG;
  if (!out || nprob < 1 || !probs) return set_err(ctx, LFM_E_ARG, "bad batch arguments");
  *out = nullptr;
  int64_t nd = 0, nhyp = 0;
  for (int64_t q = 0; q < nprob; ++q) {
    const lfm_problem& p = probs[q];
    int r = validate_x(ctx, p.x, p.n);
    if (r) return r;
    if (!p.y) return set_err(ctx, LFM_E_ARG, "problem y is NULL");
    if (p.n > SMALL_MAX)
      return set_err(ctx, LFM_E_ARG, "lfm_batch: every problem needs n <= 128 (one workgroup each)");
    if (p.hyp.num_genes < 1 || p.hyp.num_genes > p.n)
      return set_err(ctx, LFM_E_ARG, "lfm_batch: num_genes must be in [1, n]");
    r = check_mean_shape(ctx, p.n, &p.hyp);
    if (r) return r;
    nd += 4 * p.n + small_grid_doubles(p.n);
    nhyp += 3 * p.hyp.num_genes + 3;
  }
  DeviceGuard g(ctx->device);
  std::unique_ptr<lfm_batch> b(new lfm_batch);
  static std::atomic<uint64_t> next_id{0};
  b->id = ++next_id;
  b->device = ctx->device;
  b->nprob = nprob;
  b->nhyp = nhyp;
  const size_t bytes_d = round_up(nd * 8, 16), bytes_p = round_up((size_t)nprob * sizeof(SmallProb), 16);
  const size_t bytes_o = 2 * (size_t)nprob * sizeof(int);
  hipError_t e = hipMalloc((void**)&b->dmem, bytes_d + bytes_p + bytes_o);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_create: device buffer");
  // coherent (fine-grained): the kernel reads the hyperparameters a call has just written and
  // its result / status stores must reach the host's spin without a stream synchronise,
  // whatever HIP_HOST_COHERENT says
  e = hipHostMalloc((void**)&b->hbuf, (size_t)(2 * nhyp + 2 * nprob) * 8, hipHostMallocCoherent);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    hipFree(b->dmem);
    if (b->hbuf) hipHostFree(b->hbuf);
    return hip_fail(ctx, e, "lfm_batch_create: pinned buffer");
  }
  b->dprobs = reinterpret_cast<SmallProb*>(b->dmem + bytes_d);
  b->doffs = reinterpret_cast<int*>(b->dmem + bytes_d + bytes_p);
  b->hgrad = b->hbuf + nhyp + 2 * nprob;
  std::vector<double> hd((size_t)nd);
  std::vector<SmallProb> table((size_t)nprob);
  const double* dd = reinterpret_cast<const double*>(b->dmem);
  size_t off = 0;
  int64_t hv = 0, hs = 0;
  const int64_t nvec = nhyp - 3 * nprob;  // the vectors first, then the scalars
  for (int64_t q = 0; q < nprob; ++q) {
    // the hyperparameters stay in the pinned buffer: a call writes them there
    off = pack_small(probs[q], hd.data(), dd, off, b->hbuf + hv, b->hbuf + nvec + hs, table[q],
                     b->dims);
    b->dsb_off.push_back((int)hv);
    b->sc_off.push_back((int)(nvec + hs));
    hv += 3 * probs[q].hyp.num_genes;
    hs += 3;
  }
  b->use_args = ctx->knobs.small_kernarg && nprob <= SMALL_ARG_PROBS &&
                nhyp <= SMALL_ARG_HYP;
  b->table = table;
  // the gradient / fit kernels: every problem's augmented matrix on one or two waves
  // (n + 1 <= 128) and its LDS map within a CU's 160 KB
  if (b->dims.maxn <= SMALL_GRAD_MAX) {
    b->lds_grad = small_grad_lds(table.data(), (int)nprob, 0);
    b->lds_fit = small_grad_lds(table.data(), (int)nprob, 1);
    if (b->lds_grad > 160 * 1024) b->lds_grad = 0;
    if (b->lds_fit > 160 * 1024) b->lds_fit = 0;
  }
  std::vector<int> offs(b->dsb_off);
  offs.insert(offs.end(), b->sc_off.begin(), b->sc_off.end());
  e = hipMemcpyAsync(b->dmem, hd.data(), (size_t)nd * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(b->dprobs, table.data(), (size_t)nprob * sizeof(SmallProb),
                       hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(b->doffs, offs.data(), bytes_o, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    hipFree(b->dmem);
    hipHostFree(b->hbuf);
    return hip_fail(ctx, e, "lfm_batch_create: upload");
  }
  *out = b.release();
  return LFM_OK;
}

int lfm_batch_hyp_size(const lfm_batch* batch, int64_t* out) {
  if (!batch || !out) return LFM_E_ARG;
  *out = batch->nhyp;
  return LFM_OK;
}

int lfm_batch_destroy(lfm_batch* batch) {
  if (!batch) return LFM_OK;
  hipSetDevice(batch->device);
  // an evaluation returns once its status words land, possibly before its kernel has retired:
  // wait for the batch's last launch (not the whole device: other contexts' streams may be busy
  // or stuck) before the buffers go
  if (batch->done) {
    hipEventSynchronize(batch->done);
    hipEventDestroy(batch->done);
  }
  hipFree(batch->dmem);
  if (batch->fitbuf) hipFree(batch->fitbuf);
  hipHostFree(batch->hbuf);
  delete batch;
  return LFM_OK;
}

int lfm_batch_mll_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                      double* out, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !out) return set_err(ctx, LFM_E_ARG, "batch / hyp / out is NULL");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  DeviceGuard g(ctx->device);
  const int64_t np = batch->nprob;
  double* hres = batch->hbuf + batch->nhyp;
  mark_pending(hres, np);
  int r = batch_launch(ctx, batch, hyp, negative, hres);
  if (r) return r;
  r = batch_wait(ctx, np, batch_words(batch), hres, np);
  if (r) return r;
  std::memcpy(out, hres, (size_t)np * 8);
  return batch_status(ctx, batch_words(batch), np, status);
}

int lfm_batch_mll_grad_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp, int negative,
                           double* value, double* grad, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !value || !grad)
    return set_err(ctx, LFM_E_ARG, "batch / hyp / value / grad is NULL");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  if (!batch->lds_grad)
    return set_err(ctx, LFM_E_ARG, "lfm_batch_mll_grad_f64: every problem needs n <= 127 and its "
                                   "map within 160 KB of LDS; use lfm_mll_grad_f64");
  DeviceGuard g(ctx->device);
  const int64_t np = batch->nprob;
  double* hres = batch->hbuf + batch->nhyp;
  int* hst = batch_words(batch);
  if (int e = batch_prev_ok(ctx, batch)) return e;
  batch_reset(batch);
  mark_pending(hres, np);
  mark_pending(batch->hgrad, batch->nhyp);
  int r;
  if (batch->use_args) {
    SmallArgs a;
    fill_small_args(batch, hyp, a);
    a.tabs = 1;
    r = launch_small_grad(ctx, &a, nullptr, nullptr, (int)np, batch->lds_grad, negative, hres,
                          batch->hgrad, hst);
  } else {
    std::memcpy(batch->hbuf, hyp, (size_t)batch->nhyp * 8);
    r = launch_small_grad(ctx, nullptr, batch->dprobs, batch->doffs, (int)np, batch->lds_grad,
                          negative, hres, batch->hgrad, hst);
  }
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  r = batch_wait(ctx, np, hst, hres, np, batch->hgrad, batch->nhyp);
  if (r) return r;
  std::memcpy(grad, batch->hgrad, (size_t)batch->nhyp * 8);
  std::memcpy(value, hres, (size_t)np * 8);
  return batch_status(ctx, hst, np, status);
}

int lfm_batch_fit_f64(lfm_ctx* ctx, lfm_batch* batch, const lfm_adam* opt, int negative,
                      int64_t step0, int64_t nsteps, double* raw, double* mu, double* nu,
                      double* history, int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !opt || !raw || !mu || !nu || (nsteps > 0 && !history) || step0 < 0 ||
      nsteps < 0 || opt->num_steps_per_epoch < 1)
    return set_err(ctx, LFM_E_ARG, "bad fit arguments");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  if (!batch->lds_fit)
    return set_err(ctx, LFM_E_ARG, "lfm_batch_fit_f64: every problem needs n <= 127 and its map "
                                   "within 160 KB of LDS");
  if (nsteps == 0) return LFM_OK;
  DeviceGuard g(ctx->device);
  if (int e = batch_prev_ok(ctx, batch)) return e;
  const int64_t np = batch->nprob, nh = batch->nhyp;
  const size_t b_par = 3 * (size_t)nh * 8, b_bias = 2 * (size_t)nsteps * 8;
  const size_t b_hist = (size_t)nsteps * np * 8, b_st = (size_t)np * sizeof(int);
  const size_t need = b_par + b_bias + b_hist + b_st;
  if (batch->fit_bytes < need) {
    hipStreamSynchronize(ctx->stream);
    if (batch->fitbuf) hipFree(batch->fitbuf);
    batch->fitbuf = nullptr;
    batch->fit_bytes = 0;
    hipError_t e = hipMalloc((void**)&batch->fitbuf, need);
    if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_fit_f64: device buffer");
    batch->fit_bytes = need;
  }
  double* d_par = reinterpret_cast<double*>(batch->fitbuf);
  double* d_bias = d_par + 3 * nh;
  double* d_hist = d_bias + 2 * nsteps;
  int* d_st = reinterpret_cast<int*>(d_hist + nsteps * np);
  // optax's bias corrections 1 - b^count, count = step0 + s + 1, with the host's pow (the
  // restatement's numbers: dis_project_amd/trainer.py adam)
  std::vector<double> bias((size_t)2 * nsteps), par((size_t)3 * nh);
  for (int64_t s = 0; s < nsteps; ++s) {
    const double count = (double)(step0 + s + 1);
    bias[2 * s] = 1.0 - std::pow(opt->b1, count);
    bias[2 * s + 1] = 1.0 - std::pow(opt->b2, count);
  }
  std::memcpy(par.data(), raw, nh * 8);
  std::memcpy(par.data() + nh, mu, nh * 8);
  std::memcpy(par.data() + 2 * nh, nu, nh * 8);
  hipError_t e = hipMemcpyAsync(d_par, par.data(), b_par, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_bias, bias.data(), b_bias, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_fit_f64: upload");
  SmallFitLaunch f{};
  f.probs = batch->dprobs;
  f.offs = batch->doffs;
  f.nprob = (int)np;
  f.raw = d_par;
  f.mu = d_par + nh;
  f.nu = d_par + 2 * nh;
  f.history = d_hist;
  f.bias = d_bias;
  f.status = d_st;
  f.lr = opt->learning_rate;
  f.b1 = opt->b1;
  f.b2 = opt->b2;
  f.eps = opt->eps;
  f.eps_root = opt->eps_root;
  f.step0 = step0;
  f.nsteps = nsteps;
  f.spe = opt->num_steps_per_epoch;
  f.fix = opt->fix_params != 0;
  f.negative = negative;
  int r = launch_small_fit(ctx, f, batch->lds_fit);
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  std::vector<int> st((size_t)np);
  e = hipMemcpyAsync(par.data(), d_par, b_par, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(history, d_hist, b_hist, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st.data(), d_st, b_st, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_fit_f64: download");
  r = finish(ctx);
  if (r) return r;
  // the packed layout's jitter slots pass through unchanged (a static field, model.py:64)
  std::memcpy(raw, par.data(), nh * 8);
  std::memcpy(mu, par.data() + nh, nh * 8);
  std::memcpy(nu, par.data() + 2 * nh, nh * 8);
  return batch_status(ctx, st.data(), np, status,
                      "Cholesky failed during the fit of a batch problem (its loss "
                      "and parameters are NaN from that step on, as JAX's)",
                      true);
}

int lfm_batch_posterior_f64(lfm_ctx* ctx, lfm_batch* batch, const double* hyp,
                            const double* diag_vec, const double* diag_add, const int64_t* m,
                            const double* t, double* mean, double* var, double* cov,
                            int* status) {
  if (!ctx) return LFM_E_ARG;
  if (!batch || !hyp || !diag_add || !m || !t || !mean)
    return set_err(ctx, LFM_E_ARG, "batch / hyp / diag_add / m / t / mean is NULL");
  if (!var && !cov) return set_err(ctx, LFM_E_ARG, "one of var / cov must be given");
  if (batch->device != ctx->device) return set_err(ctx, LFM_E_ARG, "batch of another device");
  const int64_t np = batch->nprob, nh = batch->nhyp;
  if (batch->dims.maxn > SMALL_GRAD_MAX || np > INT_MAX / 4)
    return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: every problem needs n <= 127; use "
                                   "lfm_posterior_f64");
  // per problem: its offsets in the packed arrays; one pass of the kernel covers `unit` test
  // columns (64, or 256 when 64 would make more than 4096 workgroups)
  std::vector<PostProb> pp((size_t)np);
  int64_t sm = 0, sn = 0, sv = 0, sc = 0, ntiles = 0, wg64 = 0;
  for (int64_t p = 0; p < np; ++p) {
    const SmallProb& sp = batch->table[p];
    if (m[p] < 1 || m[p] % sp.G != 0 || m[p] > (1 << 20))
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: m[p] must be a multiple of "
                                     "num_genes in [1, 2^20] (mean_function, model.py:145-149)");
    if (!small_post_cols(sp.n, sp.G, sp.T))
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: a problem's LDS map is past 160 KB");
    const int64_t tb = (m[p] + 15) / 16;
    pp[p] = PostProb{sm, sv, sc, (int)m[p], (int)sn, (int)ntiles, 0};
    sm += m[p];
    sn += sp.n;
    sv += cov ? sp.n * m[p] : 0;
    sc += cov ? m[p] * m[p] : 0;
    ntiles += cov ? tb * (tb + 1) / 2 : 0;
    wg64 += (m[p] + 63) / 64;
    if (sm > ((int64_t)1 << 28) || sc > ((int64_t)1 << 29) || ntiles > INT_MAX / 2)
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: test inputs too large");
  }
  const int unit = wg64 <= 4096 ? 64 : 256;
  int64_t nsplit = 1;
  for (int64_t p = 0; p < np; ++p) {
    const SmallProb& sp = batch->table[p];
    const int u = std::min(unit, small_post_cols(sp.n, sp.G, sp.T));
    nsplit = std::max(nsplit, (m[p] + u - 1) / u);
  }
  nsplit = std::min<int64_t>(nsplit, 1024);  // a workgroup takes every nsplit-th pass
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared
  if (int e = batch_prev_ok(ctx, batch)) return e;
  // inputs, staged in pinned memory and uploaded in one copy: hyp | diag_add | diag_vec | t |
  // the problem table; then the outputs: mean | var | V | cov | status
  const size_t n_in = (size_t)nh + np + (diag_vec ? sn : 0) + 3 * sm;
  const size_t b_in = n_in * 8 + (size_t)np * sizeof(PostProb);
  const size_t n_out = 2 * (size_t)sm + sv + sc;
  const size_t b_all = b_in + n_out * 8 + (size_t)np * sizeof(int);
  int r = ctx->hpin.reserve(ctx, std::max<size_t>(b_in, 64 * sizeof(double)));
  if (r) return r;
  r = ctx->xin.reserve(ctx, b_all);
  if (r) return r;
  double* hp = ctx->hpin;
  std::memcpy(hp, hyp, nh * 8);
  std::memcpy(hp + nh, diag_add, np * 8);
  if (diag_vec) std::memcpy(hp + nh + np, diag_vec, sn * 8);
  std::memcpy(hp + nh + np + (diag_vec ? sn : 0), t, 3 * sm * 8);
  std::memcpy(hp + n_in, pp.data(), (size_t)np * sizeof(PostProb));
  double* d_in = ctx->xin;
  hipError_t e = hipMemcpyAsync(d_in, hp, b_in, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_posterior_f64: upload");
  SmallPostLaunch f{};
  f.probs = batch->dprobs;
  f.offs = batch->doffs;
  f.pp = reinterpret_cast<const PostProb*>(d_in + n_in);
  f.nprob = (int)np;
  f.nsplit = (int)nsplit;
  f.unit = unit;
  f.ntiles = (int)ntiles;
  f.hyp = d_in;
  f.dadd = d_in + nh;
  f.dv = diag_vec ? d_in + nh + np : nullptr;
  f.t = d_in + nh + np + (diag_vec ? sn : 0);
  double* d_out = reinterpret_cast<double*>(reinterpret_cast<char*>(d_in) + b_in);
  f.mean = d_out;
  f.var = d_out + sm;  // always computed (the copy back is the caller's choice)
  f.V = cov ? d_out + 2 * sm : nullptr;
  f.cov = cov ? d_out + 2 * sm + sv : nullptr;
  f.status = reinterpret_cast<int*>(d_out + n_out);
  r = launch_small_post(ctx, f, small_post_lds(batch->table.data(), (int)np));
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  std::vector<int> st((size_t)np);
  e = hipMemcpyAsync(mean, f.mean, sm * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && var)
    e = hipMemcpyAsync(var, f.var, sm * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && cov)
    e = hipMemcpyAsync(cov, f.cov, sc * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st.data(), f.status, np * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_posterior_f64: download");
  r = finish(ctx);
  if (r) return r;
  return batch_status(ctx, st.data(), np, status);
}

}  // extern "C"
