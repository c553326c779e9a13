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

// The problems' shapes (what plan_small_* take), each with its grid layout detected into lays
std::vector<SmallShape> small_shapes(int64_t np, const lfm_problem* probs, const int64_t* idx,
                                     std::vector<GridLayout>& lays) {
  std::vector<SmallShape> shapes((size_t)np);
  lays.resize((size_t)np);
  for (int64_t q = 0; q < np; ++q) {
    const lfm_problem& p = probs[idx ? idx[q] : q];
    lays[q] = detect_grid(p.x, p.n, p.hyp.num_genes);
    shapes[q] = {(int)p.n, (int)p.hyp.num_genes, small_grid_T(lays[q], p.hyp.num_genes)};
  }
  return shapes;
}

// One small problem into its slots `at` (plan_small_pack) of the staging area hd (device address
// dd), and its table entry sp: x, y, its hyperparameters D S B, l obs_stddev jitter when dsb is
// NULL (else sp points at the caller's dsb / sc), then a grid problem's times / block genes.
void pack_small(const lfm_problem& p, const SmallShape& s, const GridLayout& lay,
                const SmallPack::Slot& at, double* hd, const double* dd, const double* dsb,
                const double* sc, SmallProb& sp) {
  const int64_t n = s.n, G = s.G, T = s.T;
  std::memcpy(hd + at.x, p.x, 3 * n * 8);
  std::memcpy(hd + at.y, p.y, n * 8);
  if (!dsb) {
    dsb = dd + at.dsb;
    sc = dd + at.sc;
    std::memcpy(hd + at.dsb, p.hyp.true_d, G * 8);
    std::memcpy(hd + at.dsb + G, p.hyp.true_s, G * 8);
    std::memcpy(hd + at.dsb + 2 * G, p.hyp.true_b, G * 8);
    hd[at.sc] = p.hyp.l;
    hd[at.sc + 1] = p.hyp.obs_stddev;
    hd[at.sc + 2] = p.hyp.jitter;
  }
  sp = SmallProb{dd + at.x, dd + at.y, dsb, sc, s.n, s.G};
  if (T) {
    std::memcpy(hd + at.grid, lay.times.data(), T * 8);
    std::memcpy(hd + at.grid + T, lay.block_gene.data(), lay.nblk * sizeof(int));
    sp.T = s.T;
    sp.dt = lay.dt;
    sp.times = dd + at.grid;
    sp.bg = reinterpret_cast<const int*>(dd + at.grid + T);
  }
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
  // packed device buffer: the staging area (plan_small_pack, hyperparameters inline), then the
  // SmallProb array
  std::vector<GridLayout> lays;
  const std::vector<SmallShape> shapes = small_shapes(np, probs, idx, lays);
  const SmallPack pack = plan_small_pack(shapes, true);
  const size_t bytes_d = pack.bound * 8;
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
  for (int64_t q = 0; q < np; ++q)
    pack_small(probs[idx[q]], shapes[q], lays[q], pack.at[q], hd, dd, nullptr, nullptr, hp[q]);
  const size_t up = round_up(bytes_d, 16) + bytes_p;
  Copies cp{ctx};
  cp.up(db, hb, up);
  if ((r = cp.done("upload small batch"))) return r;
  double* d_out = reinterpret_cast<double*>(db + round_up(bytes_d, 16) + round_up(bytes_p, 16));
  int* d_st = reinterpret_cast<int*>(d_out + np);
  r = launch_small_batch(ctx, reinterpret_cast<const SmallProb*>(db + round_up(bytes_d, 16)),
                         (int)np, plan_small_mll(small_dims(shapes)), negative, d_out, d_st);
  if (r) return r;
  double* h_out = reinterpret_cast<double*>(hb + round_up(bytes_d, 16) + round_up(bytes_p, 16));
  cp.down(h_out, d_out, np * 12);
  if ((r = cp.landed("download small batch"))) return r;
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
  const SmallMllPlan plan = plan_small_mll(batch->dims);
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
    r = launch_small_args(ctx, a, np, plan);
  } else {
    std::memcpy(batch->hbuf, hyp, (size_t)batch->nhyp * 8);
    r = launch_small_batch(ctx, batch->dprobs, np, plan, negative, out, hst);
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
  int64_t nhyp = 0;
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
    nhyp += 3 * p.hyp.num_genes + 3;
  }
  // the hyperparameters stay in the pinned buffer (a call writes them there): not in the staging
  std::vector<GridLayout> lays;
  const std::vector<SmallShape> shapes = small_shapes(nprob, probs, nullptr, lays);
  const SmallPack pack = plan_small_pack(shapes, false);
  const size_t nd = pack.bound;
  DeviceGuard g(ctx->device);
  std::unique_ptr<lfm_batch> b(new lfm_batch);
  static std::atomic<uint64_t> next_id{0};
  b->id = ++next_id;
  b->device = ctx->device;
  b->nprob = nprob;
  b->nhyp = nhyp;
  b->lay = batch_layout(nhyp, nprob);
  const size_t bytes_d = round_up(nd * 8, 16), bytes_p = round_up((size_t)nprob * sizeof(SmallProb), 16);
  const size_t bytes_o = 2 * (size_t)nprob * sizeof(int);
  hipError_t e = hipMalloc((void**)&b->dmem, bytes_d + bytes_p + bytes_o);
  if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_create: device buffer");
  // coherent (fine-grained): the kernel reads the hyperparameters a call has just written and
  // its result / status stores must reach the host's spin without a stream synchronise,
  // whatever HIP_HOST_COHERENT says
  e = hipHostMalloc((void**)&b->hbuf, b->lay.bytes, hipHostMallocCoherent);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    hipFree(b->dmem);
    if (b->hbuf) hipHostFree(b->hbuf);
    return hip_fail(ctx, e, "lfm_batch_create: pinned buffer");
  }
  b->dprobs = reinterpret_cast<SmallProb*>(b->dmem + bytes_d);
  b->doffs = reinterpret_cast<int*>(b->dmem + bytes_d + bytes_p);
  std::vector<double> hd(nd);
  std::vector<SmallProb> table((size_t)nprob);
  const double* dd = reinterpret_cast<const double*>(b->dmem);
  int64_t hv = 0, hs = 0;
  const int64_t nvec = nhyp - 3 * nprob;  // the vectors first, then the scalars
  const double* hhyp = b->hbuf;
  for (int64_t q = 0; q < nprob; ++q) {
    pack_small(probs[q], shapes[q], lays[q], pack.at[q], hd.data(), dd, hhyp + hv,
               hhyp + nvec + hs, table[q]);
    b->dsb_off.push_back((int)hv);
    b->sc_off.push_back((int)(nvec + hs));
    hv += 3 * probs[q].hyp.num_genes;
    hs += 3;
  }
  b->use_args = ctx->knobs.small_kernarg && nprob <= SMALL_ARG_PROBS &&
                nhyp <= SMALL_ARG_HYP;
  b->table = table;
  b->shapes = shapes;
  b->dims = small_dims(shapes);
  b->lds_grad = small_grad_lds(shapes, 0);
  b->lds_fit = small_grad_lds(shapes, 1);
  std::vector<int> offs(b->dsb_off);
  offs.insert(offs.end(), b->sc_off.begin(), b->sc_off.end());
  Copies cp{ctx};
  cp.up(b->dmem, hd.data(), nd * 8);
  cp.up(b->dprobs, table.data(), (size_t)nprob * sizeof(SmallProb));
  cp.up(b->doffs, offs.data(), bytes_o);
  if (cp.e == hipSuccess) cp.e = hipStreamSynchronize(ctx->stream);
  if (int r = cp.done("lfm_batch_create: upload")) {
    hipFree(b->dmem);
    hipHostFree(b->hbuf);
    return r;
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
  double* hres = batch->hbuf + batch->lay.out;
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
  double* hres = batch->hbuf + batch->lay.out;
  double* hgrad = batch->hbuf + batch->lay.grad;
  int* hst = batch_words(batch);
  if (int e = batch_prev_ok(ctx, batch)) return e;
  batch_reset(batch);
  mark_pending(hres, np);
  mark_pending(hgrad, batch->nhyp);
  int r;
  if (batch->use_args) {
    SmallArgs a;
    fill_small_args(batch, hyp, a);
    a.tabs = 1;
    r = launch_small_grad(ctx, &a, nullptr, nullptr, (int)np, batch->lds_grad, negative, hres,
                          hgrad, hst);
  } else {
    std::memcpy(batch->hbuf, hyp, (size_t)batch->nhyp * 8);
    r = launch_small_grad(ctx, nullptr, batch->dprobs, batch->doffs, (int)np, batch->lds_grad,
                          negative, hres, hgrad, hst);
  }
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  r = batch_wait(ctx, np, hst, hres, np, hgrad, batch->nhyp);
  if (r) return r;
  std::memcpy(grad, hgrad, (size_t)batch->nhyp * 8);
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
  const FitLayout L = fit_layout(nh, np, nsteps);
  if (batch->fit_bytes < L.bytes) {
    hipStreamSynchronize(ctx->stream);
    if (batch->fitbuf) hipFree(batch->fitbuf);
    batch->fitbuf = nullptr;
    batch->fit_bytes = 0;
    hipError_t e = hipMalloc((void**)&batch->fitbuf, L.bytes);
    if (e != hipSuccess) return hip_fail(ctx, e, "lfm_batch_fit_f64: device buffer");
    batch->fit_bytes = L.bytes;
  }
  double* d_fit = reinterpret_cast<double*>(batch->fitbuf);  // raw first
  // raw | mu | nu | bias are adjacent in the buffer (raw at its start): one upload
  FitStaging stage(opt, step0, nsteps, nh, 0, L.mu, L.nu, L.bias, raw, mu, nu);
  Copies cp{ctx};
  cp.up(d_fit, stage.par.data(), stage.par.size() * 8);
  if (int r = cp.done("lfm_batch_fit_f64: upload")) return r;
  SmallFitLaunch f{};
  f.probs = batch->dprobs;
  f.offs = batch->doffs;
  f.nprob = (int)np;
  f.raw = d_fit;
  f.mu = d_fit + L.mu;
  f.nu = d_fit + L.nu;
  f.history = d_fit + L.hist;
  f.bias = d_fit + L.bias;
  f.status = reinterpret_cast<int*>(d_fit + L.status);
  f.opt = adam_opt(opt, step0);
  f.nsteps = nsteps;
  f.negative = negative;
  if (int r = launch_small_fit(ctx, f, batch->lds_fit)) return r;
  hipEventRecord(batch->done, ctx->stream);
  std::vector<int> st((size_t)np);
  cp.down(stage.par.data(), d_fit, L.bias * 8);
  cp.down(history, f.history, (L.status - L.hist) * 8);
  cp.down(st.data(), f.status, (size_t)np * sizeof(int));
  if (int r = cp.landed("lfm_batch_fit_f64: download")) return r;
  stage.back(raw, mu, nu);
  return batch_status(ctx, st.data(), np, status, FIT_FAILED, true);
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
  const PostPlan P = plan_small_post(batch->shapes, nh, m, diag_vec != nullptr, cov != nullptr);
  switch (P.reject) {
    case PostPlan::OK: break;
    case PostPlan::BAD_M:
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: m[p] must be a multiple of "
                                     "num_genes in [1, 2^20] (mean_function, model.py:145-149)");
    case PostPlan::NO_FIT:
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: a problem's LDS map is past 160 KB");
    case PostPlan::TOO_LARGE:
      return set_err(ctx, LFM_E_ARG, "lfm_batch_posterior_f64: test inputs too large");
  }
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // shared
  if (int e = batch_prev_ok(ctx, batch)) return e;
  int r = ctx->hpin.reserve(ctx, std::max<size_t>(P.in_bytes, 64 * sizeof(double)));
  if (r) return r;
  r = ctx->xin.reserve(ctx, P.all_bytes);
  if (r) return r;
  // the inputs, staged in pinned memory and uploaded in one copy
  double* hp = ctx->hpin;
  std::memcpy(hp, hyp, nh * 8);
  std::memcpy(hp + P.dadd, diag_add, np * 8);
  if (diag_vec) std::memcpy(hp + P.dv, diag_vec, P.sn * 8);
  std::memcpy(hp + P.t, t, 3 * P.sm * 8);
  std::memcpy(hp + P.table, P.pp.data(), (size_t)np * sizeof(PostProb));
  double* d = ctx->xin;
  Copies cp{ctx};
  cp.up(d, hp, P.in_bytes);
  if ((r = cp.done("lfm_batch_posterior_f64: upload"))) return r;
  SmallPostLaunch f{};
  f.probs = batch->dprobs;
  f.offs = batch->doffs;
  f.pp = reinterpret_cast<const PostProb*>(d + P.table);
  f.nprob = (int)np;
  f.nsplit = P.nsplit;
  f.unit = P.unit;
  f.ntiles = P.ntiles;
  f.hyp = d;
  f.dadd = d + P.dadd;
  f.dv = diag_vec ? d + P.dv : nullptr;
  f.t = d + P.t;
  f.mean = d + P.mean;
  f.var = d + P.var;  // always computed (the copy back is the caller's choice)
  f.V = cov ? d + P.V : nullptr;
  f.cov = cov ? d + P.cov : nullptr;
  f.status = reinterpret_cast<int*>(d + P.status);
  r = launch_small_post(ctx, f, P.lds_bytes);
  if (r) return r;
  hipEventRecord(batch->done, ctx->stream);
  std::vector<int> st((size_t)np);
  cp.down(mean, f.mean, P.sm * 8);
  if (var) cp.down(var, f.var, P.sm * 8);
  if (cov) cp.down(cov, f.cov, P.sc * 8);
  cp.down(st.data(), f.status, np * sizeof(int));
  if ((r = cp.landed("lfm_batch_posterior_f64: download"))) return r;
  return batch_status(ctx, st.data(), np, status);
}

}  // extern "C"
