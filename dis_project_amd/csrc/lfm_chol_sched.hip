// lfm_chol_sched.hip — the host side of the blocked factorisation: chol_factor_solve plans a
// call (plan_steps, and for schedule 3 plan_s3: lfm_host.cpp, plain C++), reserves what the
// plan says and issues the launches of lfm_chol.hip's kernels (declared in lfm_chol.h). No
// kernel is defined here.
//
// Schedule 1: super-panel s + 1 is factored on a high-priority side stream (potrf / trsm /
// band syrk, or one fused panel launch) while the main stream runs the bulk of step s's
// trailing update; streams ordered by events.
// Schedule 3: on the CU-partitioned stream pair, one chain_kernel per super-panel on the side
// stream's CUs and one step_kernel per step on the rest, ordered by device counters (or, for
// tools that serialise dispatches, by events: LFM_S3_EVENTS).
#include <algorithm>
#include <utility>

#include "lfm_chol.h"

namespace lfm {

namespace {
struct Launcher {
  lfm_ctx* ctx;
  double* A;
  int64_t lda;
  int64_t Mp;   // rows of the (augmented) matrix being factored
  int64_t win;  // 0: trailing rows run to Mp; > 0: rows [s, s + win) only (bordered inverse)
  int64_t end(int64_t s) const { return win ? s + win : Mp; }
  void potrf(hipStream_t st, int64_t k, int64_t n) {
    hipEvent_t ev;
    prof_begin(ctx, K_POTRF, &ev, st);
    hipLaunchKernelGGL(potrf_diag_kernel<15>, dim3(1), dim3(256), MB_DOUBLES * sizeof(double), st,
                       A, lda, k * NB, n, ctx->linvT, ctx->parts, (int)k, ctx->status);
    prof_end(ctx, K_POTRF, ev, (double)NB * NB * NB / 3.0, 0, st);
  }
  // Panel solve of block column k over the rows below it, with the diagonal inverses.
  void trsm(hipStream_t st, int64_t k) {
    const int64_t s = (k + 1) * NB;
    const int64_t rows = end(s) - s;
    if (rows <= 0) return;
    hipEvent_t ev;
    prof_begin(ctx, K_TRSM, &ev, st);
    hipLaunchKernelGGL(trsm_kernel_v2, dim3((unsigned)(rows / 64)), dim3(256), 0, st, A, lda, s,
                       k * NB, ctx->linvT);
    prof_end(ctx, K_TRSM, ev, (double)rows * NB * NB, 2.0 * rows * NB * 8, st);
  }
  // Trailing update of tile columns [lo, hi) of the matrix starting at s0 (T = 128-tiles, in
  // 64-row slabs) with panel columns kb .. kb + kd. prio raises the look-ahead bands' waves.
  void syrk(hipStream_t st, int64_t s0, int64_t kb, int kd, int64_t T, int lo, int hi,
            int prio = 0) {
    if (T <= 0 || hi <= lo) return;
    hi = (int)std::min<int64_t>(hi, T);
    if (hi - lo > 8) hi = (int)T;  // wider than a band: the triangle of every column >= lo
    int64_t units = 0;
    double elems = 0;
    for (int tj = lo; tj < hi; ++tj) {
      units += 2 * (T - tj);
      elems += (double)(T - tj - 1) * ST * ST + (double)ST * (ST + 1) / 2;
    }
    if (units <= 0) return;
    hipEvent_t ev;
    prof_begin(ctx, K_SYRK, &ev, st);
    hipLaunchKernelGGL((syrk_kernel<true, 64>), dim3((unsigned)units), dim3(256), 0, st, A, lda,
                       s0, Panel{A + kb, lda, 0}, kd, (int)T, lo, hi, prio, 1, 0, (int64_t)0);
    prof_end(ctx, K_SYRK, ev, elems * 2.0 * kd, elems * 16.0, st);
  }
  int64_t tiles_from(int64_t s0) const { return (end(s0) - s0) / ST; }
  // Fused pending-update + factor + solve of block column k (panel_kernel).
  void panel(hipStream_t st, int64_t k, int64_t pkb, int pkd, int64_t n) {
    const int64_t kb = k * NB, s = kb + NB;
    const int64_t rows = std::max<int64_t>(end(s) - s, 0);
    const unsigned epoch = ++ctx->panel_epoch;
    hipEvent_t ev;
    prof_begin(ctx, K_PANEL, &ev, st);
    hipLaunchKernelGGL(panel_kernel, dim3((unsigned)(2 + rows / 64)), dim3(256), PANEL_LDS, st, A,
                       lda, kb, pkb, pkd, n, ctx->linvT, ctx->parts, (int)k, ctx->status,
                       ctx->psync, epoch, ctx->knobs.wait_ticks);
    prof_end(ctx, K_PANEL, ev,
             (double)NB * NB * NB / 3.0 + (double)rows * NB * NB + 2.0 * (rows + NB) * NB * pkd,
             0, st);
  }
  // Factor the super-panel of block columns [k, k + w): per column potrf + trsm, then the
  // update of the super-panel's remaining columns with it (K = 128). w = 1: one fused launch.
  void superpanel(hipStream_t st, int64_t k, int w, int64_t n) {
    if (w == 1) {
      panel(st, k, 0, 0, n);
      return;
    }
    for (int i = 0; i < w; ++i) {
      potrf(st, k + i, n);
      trsm(st, k + i);
      if (i + 1 < w) {
        const int64_t s0 = (k + i + 1) * NB;
        syrk(st, s0, (k + i) * NB, NB, tiles_from(s0), 0, w - 1 - i, 1);
      }
    }
  }
};
}  // namespace

// Start-up check for schedule 3 (coresident_kernel): can G chain-sized workgroups be resident
// together on the stream's CUs?
int chain_coresident(lfm_ctx* ctx, hipStream_t st, int G, bool* good) {
  hipFuncSetAttribute(reinterpret_cast<const void*>(&coresident_kernel),
                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)CHAIN_LDS);
  unsigned* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, 16);
  if (e != hipSuccess) return hip_fail(ctx, e, "coresident probe");
  const unsigned init[2] = {0u, 1u};
  hipMemcpyAsync(d, init, 8, hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(coresident_kernel, dim3((unsigned)G), dim3(256), CHAIN_LDS, st, d,
                     reinterpret_cast<int*>(d + 1));
  unsigned h[2] = {0u, 0u};
  hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, st);
  e = hipStreamSynchronize(st);
  hipFree(d);
  *good = e == hipSuccess && h[0] == (unsigned)G && h[1] == 1u;
  return hip_fail(ctx, e, "coresident probe");
}

// Diagnostics hook (liblfm_diag.so's lfm_probe_syrk, include/lfm_diag.h): ONE launch of the
// trailing-update kernel over a full lower triangle of T x T 128-tiles at depth kd on the
// n x n matrix ctx->A (operands prepared by the caller; X_s / X_{s+1} / counters after it).
// cio bit 0: C tile I/O (else the MFMAs alone), bit 4: on schedule 3's CU-masked bulk stream
// instead of every CU, bit 6: the step kernel's rest role (bit 5: without C loads). With bit
// 6, the rest of a w = 1 step launch's structure: bit 7 the ahead band (tile column 0 below
// the diagonal tile, the rest triangle then over columns >= 1, coherent stores, a_done
// bumps), bit 8 the tall units (X = A21 Bd at depth 128 for the rows below tile 0, no waits),
// bit 9 the panel read from a separate 128-wide buffer (the real steps' X_s) instead of A's
// own columns. Bit 11 (instead of bit 6): syrk_kernel's 128 x 128 units. Launches only: no
// kernel of its own, no allocation.
int probe_update_launch(lfm_ctx* ctx, hipStream_t st, int T, int kd, int cio, int64_t n,
                        size_t xb) {
  const unsigned units = (unsigned)((int64_t)T * (T + 1));
  const Panel pan{ctx->A, n, 0};
  if (cio & 64) {
    // the schedule-3 step kernel's rest role alone (the production unit: 16-deep stages,
    // 4 workgroups / CU, supertile order); bit 5: no C loads (C = 0, stores kept)
    StepArgs g{};
    g.A = ctx->A;
    g.lda = n;
    g.s0 = 512;
    g.px = pan;
    g.kd = kd;
    g.T = T;
    g.nr = (int)units;
    g.n = n;
    g.pad_end = INT64_MAX;
    g.spin = ctx->knobs.wait_ticks;
    g.zero_from = (cio & 32) ? 0 : INT64_MAX;
    g.copy_from = INT64_MAX;
    double* xs = ctx->A + (size_t)n * n;  // [X_s | X_{s+1} | counters]
    unsigned* ctr = reinterpret_cast<unsigned*>(xs + 2 * (xb / 8));
    if (cio & 512) g.px = Panel{xs, 128, 512};
    if (cio & 128) {
      g.wn = 1;
      g.na = 2 * (T - 1);
      g.nr = (T - 1) * T;
      g.a_done = ctr;
    }
    if (cio & 256) {
      g.tw = 1;
      g.tr0 = 512 + ST;
      g.tk0 = 0;
      g.nt = 2 * (T - 1) * TALL_SPLIT;
      g.Bd = ctx->A;
      g.X = xs + xb / 8;
      g.zvec = xs;
      g.a_done = nullptr;
    }
    const unsigned grid = (unsigned)(pad8(g.na) + pad8(g.nr) + tall_grid(g.nt, TALL_SPLIT));
    // unit-duration stamps in step slot 0 while lfm_debug_stamps is on (scripts/unit_time.py)
    g.stamps = ctx->dbg_stamps ? ctx->dbg_stamps + 256 * 16 : nullptr;
    hipLaunchKernelGGL(step_kernel, dim3(grid), dim3(256), 0, st, g);
  } else if (cio & 2048) {
    // 128 x 128 units (2 workgroups / CU, 64 x 64 per wave), the same triangle
    hipLaunchKernelGGL((syrk_kernel<true, 128>), dim3(units / 2), dim3(256), 0, st, ctx->A, n,
                       (int64_t)512, pan, kd, T, 0, T, 0, 1, 0, (int64_t)0);
  } else if (cio & 1) {
    hipLaunchKernelGGL((syrk_kernel<true, 64>), dim3(units), dim3(256), 0, st, ctx->A, n,
                       (int64_t)512, pan, kd, T, 0, T, 0, 1, 0, (int64_t)0);
  } else {
    hipLaunchKernelGGL((syrk_kernel<false, 64>), dim3(units), dim3(256), 0, st, ctx->A, n,
                       (int64_t)512, pan, kd, T, 0, T, 0, 1, 0, (int64_t)0);
  }
  return hip_fail(ctx, hipGetLastError(), "probe_update_launch");
}

bool chol_fuses_gram(const lfm_ctx* ctx, int mode, const GridLayout& lay, int64_t n) {
  return ctx->knobs.gram_fuse && lay.ok && lay.T % 256 == 0 && n % 256 == 0 && n >= 1024 &&
         s3_on(ctx) && mode != CHOL_SCHUR && mode != CHOL_RESIDENT;
}

// Diagnostics: the next region of the unit trace (lfm_debug_trace) for a launch of `grid`
// workgroups, tagged with the launch count (bit 23: a side-CU helper launch); none while the
// trace is off or full
static void trace_launch(lfm_ctx* ctx, StepArgs& g, int64_t grid, bool helper) {
  g.trace = nullptr;
  if (!ctx->dbg_trace || ctx->dbg_trace_cur + grid > ctx->dbg_trace_cap) return;
  g.trace = ctx->dbg_trace + 4 * ctx->dbg_trace_cur;
  g.trace_tag = (unsigned long long)(ctx->dbg_trace_launch++ & 0x7fffff) | (helper ? 1ull << 23 : 0);
  ctx->dbg_trace_cur += grid;
}

// The dynamic LDS sizes of the kernels that need more than the default, once per process
static void set_kernel_attrs() {
  static bool attr = false;
  if (attr) return;
  hipFuncSetAttribute(reinterpret_cast<const void*>(&panel_kernel),
                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)PANEL_LDS);
  hipFuncSetAttribute(reinterpret_cast<const void*>(&potrf_diag_kernel<15>),
                      hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)(MB_DOUBLES * sizeof(double)));
  for (const void* f : {reinterpret_cast<const void*>(&chain_kernel<false>),
                        reinterpret_cast<const void*>(&chain_kernel<true>)})
    hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CHAIN_LDS);
  attr = true;
}

// ------------------------------------------------------------ schedule 3
namespace {
// One schedule-3 factorisation being issued: the call's matrix, its plan (every count, offset
// and flop figure below is read from it) and the stream pair the launches go to.
struct S3Run {
  lfm_ctx* ctx;
  double* A;
  int64_t lda, n;
  const GramGen* gen;  // the fused gram, generated by step 0's update (NULL: Sigma in memory)
  const S3Plan& P;
  hipStream_t main, side;
  hipEvent_t* ev;
  const S3Step& step(int s) const { return P.steps[s]; }
};

// chain(s): factor block s on the side stream's CUs (one launch, see chain_kernel). dev_wait:
// it waits on the device for its inputs (xready[s]) from the main launch in flight, s >= 2.
void launch_chain(const S3Run& r, int s, bool dev_wait = true) {
  lfm_ctx* ctx = r.ctx;
  const S3Step& q = r.step(s);
  ChainArgs c{};
  c.A = r.A;
  c.lda = r.lda;
  c.Kc = q.K0;
  c.w = q.w;
  c.Wk = ctx->wk + q.wk_off;
  if (s > 0) {
    const S3Step& prev = r.step(s - 1);
    if (dev_wait && s >= 2) {
      c.xready = ctx->flags + q.f_xready;
      c.xtarget = q.xtarget;
    }
    c.kd = prev.kd;
    c.K0p = prev.K0;
    c.Bdp = ctx->wk + prev.bd_off;
    c.xd = ctx->xd;
  }
  c.n = r.n;
  c.dinv = ctx->linvT;
  c.linv = ctx->linv_full;
  c.parts = ctx->parts;
  c.status = ctx->status;
  c.zvec = ctx->zvec;
  c.bar = ctx->flags + q.f_bar;
  c.done = ctx->flags + q.f_done;
  c.spin = ctx->knobs.wait_ticks;
  c.stamps = ctx->dbg_stamps ? ctx->dbg_stamps + 16 * (size_t)std::min(s, 255) : nullptr;
  hipEvent_t pe;
  prof_begin(ctx, K_POTRF, &pe, r.side);
  hipLaunchKernelGGL(c.w == 1 ? chain_kernel<true> : chain_kernel<false>,
                     dim3((unsigned)ctx->side_cus), dim3(256), CHAIN_LDS, r.side, c);
  prof_end(ctx, K_POTRF, pe, q.chain_alg, 0, r.side, q.chain_issued);
}

// The update part of a step launch: step s's trailing update from X_s (trailing matrix from
// K1_s), the next diagonal block excluded
void update_args(const S3Run& r, StepArgs& g, int s) {
  const S3Step& q = r.step(s);
  g.A = r.A;
  g.lda = r.lda;
  g.s0 = q.K1;
  g.px = Panel{r.ctx->xbuf + q.x_off, q.kd, q.K1};
  g.kd = q.kd;
  g.T = q.T;
  g.wn = q.wn;
  g.zero_from = q.zero_from;
  if (q.gen) g.gen = *r.gen;
  g.na = q.na;
  g.nr = q.nr;
  g.status = r.ctx->status;
}

// The tall part of a step launch: X_s = A21 Bd_s, step s's rows
void tall_args(const S3Run& r, StepArgs& g, int s) {
  const S3Step& q = r.step(s);
  g.A = r.A;
  g.lda = r.lda;
  g.nt = q.nt;
  g.tr0 = q.tr0;
  g.tk0 = q.tk0;
  g.tw = q.tw;
  g.Bd = r.ctx->wk + q.bd_off;
  g.X = r.ctx->xbuf + q.x_off;
  g.copy_from = q.copy_from;
  g.zvec = r.ctx->zvec;
  g.chain_done = r.ctx->flags + q.f_done;
  g.status = r.ctx->status;
}

// One step_kernel launch of `grid` workgroups on the main stream (none for an empty grid)
void launch_step(const S3Run& r, StepArgs& g, int64_t grid, double alg, double issued) {
  g.n = r.n;  // padding rows past n are skipped
  g.pad_end = r.P.pad_end;
  if (!g.zero_from) g.zero_from = INT64_MAX;
  if (!g.copy_from) g.copy_from = INT64_MAX;
  g.spin = r.ctx->knobs.wait_ticks;
  if (grid == 0) return;
  trace_launch(r.ctx, g, grid, false);
  hipEvent_t pe;
  prof_begin(r.ctx, K_SYRK, &pe, r.main);
  hipLaunchKernelGGL(g.trace ? step_kernel_traced : step_kernel, dim3((unsigned)grid), dim3(256),
                     0, r.main, g);
  prof_end(r.ctx, K_SYRK, pe, alg, 0, r.main, issued);
}

void launch_update(const S3Run& r, int s) {  // step s's trailing update alone
  StepArgs g{};
  update_args(r, g, s);
  launch_step(r, g, r.step(s).ugrid, r.step(s).upd_alg, r.step(s).upd_issued);
}

// Side-CU helper (LFM_HELPER): while the factor chain has slack (long launches), the side
// stream runs the tail of step s's rest units after chain(s + 1), sized so it ends with the
// main launch (whose arguments g are); launch s + 1 waits for it, chain(s + 2) follows it. Its
// units store without write-through and bump no counter, so they never include a lead tile of
// chain(s + 2).
void launch_helper(const S3Run& r, const StepArgs& g, int s) {
  const S3Step& q = r.step(s);
  StepArgs h = g;
  h.na = 0;
  h.nt = 0;
  h.rest_off = q.nr_main;
  h.nr = (int)q.hu;
  h.stamps = nullptr;
  h.xready = nullptr;  // tail units: never the lead tiles
  trace_launch(r.ctx, h, q.hgrid, true);
  hipEvent_t pe;
  prof_begin(r.ctx, K_SIDE_SYRK, &pe, r.side);
  hipLaunchKernelGGL(h.trace ? helper_update_kernel_traced : helper_update_kernel,
                     dim3((unsigned)q.hgrid), dim3(256), 0, r.side, h);
  prof_end(r.ctx, K_SIDE_SYRK, pe, q.helper_alg, 0, r.side, q.helper_issued);
}

// LFM_S3_EVENTS=1: the same work ordered by stream events only (tall units in launches of
// their own after the factor's event, chains after the tall launch's event) — for tools that
// serialise dispatches (rocprofv3 --pmc), under which device-side waits between the two
// streams could never be met.
void issue_by_events(const S3Run& r, bool bordered) {
  const int S = r.P.S;
  hipEvent_t* evc = r.ev + 1;      // [S] chain(s) done
  hipEvent_t* evt = r.ev + 1 + S;  // [S] X_s complete
  launch_chain(r, 0);
  hipEventRecord(evc[0], r.side);
  for (int s = 0; s < S; ++s) {
    if (s > 0) launch_update(r, s - 1);
    hipStreamWaitEvent(r.main, evc[s], 0);
    StepArgs g{};  // X_s
    tall_args(r, g, s);
    g.chain_done = nullptr;
    launch_step(r, g, r.step(s).tgrid, r.step(s).tall_alg, r.step(s).tall_issued);
    hipEventRecord(evt[s], r.main);
    if (s + 1 < S) {
      hipStreamWaitEvent(r.side, evt[s], 0);
      launch_chain(r, s + 1, false);
      hipEventRecord(evc[s + 1], r.side);
    }
  }
  if (bordered) launch_update(r, S - 1);  // the last super-panel's update of the border block
}

// The timed schedule: every later chain(s) follows chain(s - 1) in stream order and waits on
// the device for its inputs; launch s's tall units wait for chain(s + 1) and their rows' ahead
// units. serial (LFM_S3_EVENTS=2): these same launches, each also ordered by events after
// every launch its device-side waits name (chain(s + 1) after launch s - 1, launch s after
// chain(s + 1)), so a tool that serialises dispatches counts the timed schedule's own
// launches, one for one. ovl: the overlapped prologue (chain(0), X_0, chain(1), launch 0) is on
// ctx->stream and the pair takes over after it. Returns whether the overlap tail was marked.
bool issue_device_ordered(S3Run& r, bool bordered, bool serial, bool ovl) {
  lfm_ctx* ctx = r.ctx;
  const int S = r.P.S;
  hipEvent_t* evL = r.ev + 1;          // evL[2 s] = ev[1 + 2 s]: launch s done (main)
  hipEvent_t* evH = r.ev + 2;          // evH[2 s] = ev[2 + 2 s]: helper(s) done (side)
  hipEvent_t* evC = r.ev + 2 * S + 3;  // [S] chain(s) done (serialised only)
  launch_chain(r, 0);
  if (serial) {
    hipEventRecord(evC[0], r.side);
    hipStreamWaitEvent(r.main, evC[0], 0);
  }
  {
    // X_0 once the first block is factored (its units wait for chain_done[0])
    StepArgs g{};
    tall_args(r, g, 0);
    launch_step(r, g, r.step(0).tgrid, r.step(0).tall_alg, r.step(0).tall_issued);
  }
  bool helped = false;  // the previous step had a helper launch
  bool tail_marked = false;
  for (int s = 0; s + 1 < S; ++s) {
    const S3Step& q = r.step(s);
    if (serial && s >= 1) hipStreamWaitEvent(r.side, evL[2 * (s - 1)], 0);
    launch_chain(r, s + 1);
    if (serial) {
      hipEventRecord(evC[s + 1], r.side);
      hipStreamWaitEvent(r.main, evC[s + 1], 0);
    }
    StepArgs g{};
    update_args(r, g, s);
    tall_args(r, g, s + 1);
    if (ctx->dbg_stamps) g.stamps = ctx->dbg_stamps + 256 * 16 + 8 * (size_t)std::min(s, 255);
    g.a_done = ctx->flags + q.f_adone;
    // the block after next: its tiles (rest) and rows (ahead) feed chain(s + 2)
    if (q.lead) {
      g.xready = ctx->flags + r.step(s + 2).f_xready;
      g.lead = q.lead;
    }
    g.nr = q.nr_main;  // the helper takes the rest of the enumeration
    if (helped) hipStreamWaitEvent(r.main, evH[2 * (s - 1)], 0);
    if (ctx->ovl && q.ovl_mark) {
      hipEventRecord(ctx->ovl_tail, r.main);
      tail_marked = true;
    }
    launch_step(r, g, q.grid, q.step_alg, q.step_issued);
    hipEventRecord(evL[2 * s], r.main);
    if (ovl && s == 0) {
      // the overlapped prologue ends with launch 0: the pair takes over after it (its tall
      // units waited for chain(1), so the prologue's chains are done too)
      r.main = ctx->m3;
      r.side = ctx->s3;
      hipStreamWaitEvent(r.main, evL[0], 0);
      hipStreamWaitEvent(r.side, evL[0], 0);
    }
    helped = q.hu > 0;
    if (helped) {
      // X_s and step s's C input: launch s - 1 complete
      hipStreamWaitEvent(r.side, evL[2 * (s - 1)], 0);
      launch_helper(r, g, s);
      hipEventRecord(evH[2 * s], r.side);
    }
  }
  if (bordered) launch_update(r, S - 1);  // the border block (-S_aug^{-1})
  return tail_marked;
}

// Schedule 3 on the CU-partitioned stream pair (LFM_SIDE_CUS CUs for the side stream), ordered
// after / before ctx->stream's work. Side stream, per super-panel s (columns [K0, K1), W = K1 -
// K0): chain_kernel factors only the W x W diagonal block, copied into a workspace with an
// identity border, so it also yields Bd = L11^{-T}. Main stream: one step_kernel per step
// applies step s's trailing update from X_s (the next super-panel's columns first, then the
// rest) and finishes with X_{s+1} = A21 Bd_{s+1}, the tall panel solve as a GEMM, once the side
// stream's factor of block s + 1 has landed. Cross-stream order within a step is by device
// flags (ctx->flags), reset per call.
// Overlapped (a twin workspace of lfm_mll_multi_f64, ctx->ovl): chain(0), X_0, chain(1) and
// launch 0 run on ctx->stream (the primary's overlap stream, behind this evaluation's gram),
// the rest on the shared pair, after them and after the previous evaluation's launches.
// *last: the stream the factorisation ends on; *zsplit: finalize_kernel's.
int schedule3(lfm_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t Mp, bool bordered,
              const std::vector<std::pair<int64_t, int>>& steps, const GramGen* gen,
              hipStream_t* last, int64_t* zsplit) {
  S3Params pp;
  pp.n = n;
  pp.Mp = Mp;
  pp.bordered = bordered;
  pp.fused = gen != nullptr;
  pp.prof = ctx->prof;
  pp.nb = NB;
  pp.st = ST;
  pp.tall_split = TALL_SPLIT;
  pp.supertile = SUPERTILE;
  pp.cus = ctx->cus;
  pp.side_cus = ctx->side_cus;
  pp.helper = ctx->knobs.helper;
  pp.helper_tc = ctx->knobs.helper_tc;    // chain(s + 1) + margin, us
  pp.helper_min = ctx->knobs.helper_min;  // smallest launch helped, us
  pp.ovl_at = ctx->knobs.ovl_at;
  // the plan of the context's last call in this mode, if it was built from the same inputs
  plan_s3_keep(ctx->s3_plan[bordered], steps, pp);
  const S3Plan& P = ctx->s3_plan[bordered];
  const bool ovl = ctx->ovl && ctx->knobs.s3_events == 0 && P.S >= 2;
  hipEvent_t* ev = ctx->evs.data();  // [0]: inputs ready
  hipEventRecord(ev[0], ctx->stream);
  S3Run r{ctx, A, lda, n, gen, P, ctx->m3, ctx->s3, ev};
  if (!ovl) hipStreamWaitEvent(r.main, ev[0], 0);
  int e = ctx->wk.reserve(ctx, P.wk_bytes);
  if (!e) e = ctx->xbuf.reserve(ctx, P.xbuf_bytes);
  if (!e) e = ctx->zvec.reserve(ctx, P.zvec_bytes);
  if (!e) e = ctx->linv_full.reserve(ctx, P.linv_bytes);
  if (!e) e = ctx->xd.reserve(ctx, P.xd_bytes);
  if (!e) e = ctx->flags.reserve(ctx, P.flags_bytes);
  if (e) return e;
  hipMemsetAsync(ctx->flags, 0, P.flags_bytes, ovl ? ctx->stream : r.main);
  *zsplit = P.zsplit;
  // side: chain(0) after the gram
  if (ovl) {
    r.main = r.side = ctx->stream;
  } else {
    hipEventRecord(ev[0], r.main);
    hipStreamWaitEvent(r.side, ev[0], 0);
  }
  bool tail_marked = false;
  if (ctx->knobs.s3_events == 1) issue_by_events(r, bordered);
  else tail_marked = issue_device_ordered(r, bordered, ctx->knobs.s3_events == 2, ovl);
  if (ctx->ovl && !tail_marked) hipEventRecord(ctx->ovl_tail, r.main);
  hipEventRecord(ev[2 * P.S + 1], r.side);
  hipStreamWaitEvent(r.main, ev[2 * P.S + 1], 0);
  *last = r.main;
  return LFM_OK;
}

// Schedule 1 (the posterior's Schur complement, or no CU partition): super-panel s + 1 is
// factored on the high-priority side stream while the main stream runs the bulk of step s's
// trailing update. update_last: the trailing update after the last super-panel (it matters
// only for the rows past the pivots: bordered inverse, Schur complement).
int schedule1(lfm_ctx* ctx, Launcher L, int64_t n,
              const std::vector<std::pair<int64_t, int>>& steps, bool update_last) {
  if (!ctx->side) {
    // the high-priority side stream, created on first use (schedule 3 never needs it)
    int least = 0, greatest = 0;
    hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, greatest) != hipSuccess)
      return hip_fail(ctx, hipErrorOutOfMemory, "side stream creation");
  }
  const int S = (int)steps.size();
  hipStream_t main = ctx->stream, side = ctx->side;
  hipEvent_t* ev = ctx->evs.data();  // [0]: inputs ready; E1_s = ev[1 + 2s]; E2_s = ev[2 + 2s]
  hipEventRecord(ev[0], main);
  hipStreamWaitEvent(side, ev[0], 0);
  L.superpanel(side, steps[0].first, steps[0].second, n);
  hipEventRecord(ev[1], side);
  for (int s = 0; s < S; ++s) {
    const int64_t k = steps[s].first;
    const int w = steps[s].second;
    const int64_t s0 = (k + w) * NB;
    const int64_t T = L.tiles_from(s0);
    hipStreamWaitEvent(main, ev[1 + 2 * s], 0);
    const bool nxt = s + 1 < S;
    const int wn = nxt ? steps[s + 1].second : 0;
    // main: the bulk of step s's trailing update (tile columns >= wn), depth 128 w
    if (nxt || update_last) L.syrk(main, s0, k * NB, NB * w, T, wn, (int)T);
    hipEventRecord(ev[2 + 2 * s], main);
    if (nxt) {
      // side: the next super-panel's columns first (after main's previous bulk update,
      // which wrote the same tiles), then its factorisation
      if (s > 0) hipStreamWaitEvent(side, ev[2 + 2 * (s - 1)], 0);
      if (wn == 1) {
        L.panel(side, steps[s + 1].first, k * NB, NB * w, n);
      } else {
        L.syrk(side, s0, k * NB, NB * w, T, 0, wn, 1);
        L.superpanel(side, steps[s + 1].first, steps[s + 1].second, n);
      }
      hipEventRecord(ev[1 + 2 * (s + 1)], side);
    }
  }
  return LFM_OK;
}
}  // namespace

// CHOL_MLL: factor the Mp x Mp augmented matrix (block columns holding pivots only).
// CHOL_INVERSE: A is 2Mp x 2Mp, [[S_aug, .], [I, 0]]; all Mp/NB block columns of the top
//   are eliminated with every trailing update restricted to the Mp-row window below the
//   panel (the rows the identity border has reached), leaving -S_aug^{-1} in the bottom
//   block: a Cholesky + triangular inverse + L^-T L^-1 product in N^3 flops on the same
//   three kernels.
// CHOL_SCHUR: eliminate the block columns holding the n pivots of an Mp x Mp matrix and
//   apply every trailing update, so rows >= round_up(n, NB) end up holding the Schur
//   complement (posterior covariance / mean correction, lfm_predict.hip).
int chol_factor_solve(lfm_ctx* ctx, double* A, int64_t lda, int64_t n, int64_t Mp, int negative,
                      double* d_out, int mode, const GramGen* gen) {
  set_kernel_attrs();
  const bool bordered = mode == CHOL_INVERSE;
  const int64_t npb = (n + NB - 1) / NB;  // block columns that hold pivots
  const int64_t nblk = bordered ? Mp / NB : npb;
  int r = ctx->parts.reserve(ctx, (size_t)nblk * sizeof(double));
  if (r) return r;
  // schedule 3 for the MLL and for the bordered inverse (gradient); the Schur-complement
  // posterior keeps schedule 1, and so does the resident posterior's fit, which needs L in A
  const bool s3 = s3_on(ctx) && mode != CHOL_SCHUR && mode != CHOL_RESIDENT;
  ctx->last_sched = s3 ? 3 : 1;
  // the bordered matrix's bottom rows [I, 0]: in memory for schedule 1; schedule 3 never reads
  // them before its window reaches them (StepArgs zero_from / copy_from)
  if (bordered && !s3) {
    r = launch_border_init(ctx, A, lda, Mp);
    if (r) return r;
  }
  // Step plan: super-panels of w = wbulk (5, schedule-3 MLL; else 4) block columns while the
  // trailing matrix has at least LFM_W4_MIN rows, w = 2 down to LFM_W2_MIN, then w = 1, so the
  // bulk trailing update runs with depth 128 w (C traffic per flop / w). Schedule 3: the bulk
  // width down to 6144 rows, then one or two w = 2 steps down to 5120 — the last deep update
  // would otherwise hold up the first w = 1 chains (measured 0.13-0.24 ms faster than going
  // straight to w = 1); its first super-panel is one block wide (its factor precedes any bulk
  // work).
  // bulk width: 5 block columns (W = 640) for the MLL — its C traffic per flop is 4/5 of W = 512
  // and its chain still hides behind the update (A/B: -0.23..-0.26 ms per evaluation; W = 768
  // and 896 were slower, 1024 much slower); the bordered gradient keeps 4 (5 measured equal)
  const int wbulk = s3 ? (bordered ? WBORD : WBULK) : 4;
  const int64_t w2min = ctx->knobs.w2min >= 0 ? ctx->knobs.w2min : (s3 ? 5120 : 4096);
  const std::vector<std::pair<int64_t, int>> steps =
      plan_steps(nblk, Mp, NB, bordered, s3, wbulk, ctx->knobs.w4min, w2min, ctx->knobs.w0);
  const int S = (int)steps.size();
  r = ensure_events(ctx, chol_events(S));
  if (r) return r;
  // fused gram (GramGen): in memory only the first block column (chain(0), X_0) and the next
  // super-panel's diagonal block (chain(1)); launch 0's update units generate the rest
  const bool fused = gen && s3 && S >= 2;
  if (gen) {
    const int64_t K10 = (int64_t)steps[0].second * NB;
    const int64_t K11 = fused ? (int64_t)(steps[1].first + steps[1].second) * NB : n;
    r = launch_gram_region(ctx, *gen, 0, n, 0, fused ? K10 : n, A, lda);
    if (!r && fused) r = launch_gram_region(ctx, *gen, K10, std::min(K11, n), K10, K11, A, lda);
    if (r) return r;
  }
  hipLaunchKernelGGL(status_init_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->status);
  hipStream_t main = ctx->stream;  // the stream the factorisation ends on
  int64_t zsplit = 0;              // finalize: z columns below zsplit come from ctx->zvec
  if (s3)
    r = schedule3(ctx, A, lda, n, Mp, bordered, steps, fused ? gen : nullptr, &main, &zsplit);
  else
    r = schedule1(ctx, Launcher{ctx, A, lda, bordered ? 2 * Mp : Mp, bordered ? Mp : 0}, n, steps,
                  mode == CHOL_INVERSE || mode == CHOL_SCHUR);
  if (r) return r;
  r = hip_fail(ctx, hipGetLastError(), "cholesky launch");
  if (r) return r;
  hipEvent_t pe;
  prof_begin(ctx, K_FINALIZE, &pe, main);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1024), 0, main, A, lda, n, ctx->parts,
                     (int)npb, ctx->status, negative, d_out, ctx->zvec, zsplit);
  prof_end(ctx, K_FINALIZE, pe, 0, (double)n * 8, main);
  if (ctx->ovl) {
    // overlapped: the caller reads the result after ovl_done; ctx->stream (the overlap stream)
    // must not wait, the next evaluation's prologue is queued on it
    hipEventRecord(ctx->ovl_done, main);
  } else if (main != ctx->stream) {  // schedule 3 ran on the partitioned pair: back to ctx->stream
    hipEventRecord(ctx->evs[2 * S + 2], main);
    hipStreamWaitEvent(ctx->stream, ctx->evs[2 * S + 2], 0);
  }
  return hip_fail(ctx, hipGetLastError(), "finalize_kernel");
}

}  // namespace lfm
