// lfm_host.h — host-only logic of liblfm: x-layout detection, the factorisation's step plan,
// the host mirror of the trailing update's unit enumeration, the side-CU helper's sizing and
// schedule 3's whole launch plan (plan_s3: every unit count, grid, buffer and flag offset,
// device-counter target and profiling figure of a call, which lfm_chol_sched.hip only reads);
// with lfm_small_plan.h the small-problem path's LDS map, staging and buffer layouts and its
// launch plans (plan_small_*, which lfm_small.hip and lfm_batch.hip only read); and the resident
// posterior's predict plan and its held-out log density's (plan_post, plan_post_logp, which
// lfm_post.hip and lfm_post_api.hip only read); with lfm_mid_plan.h the
// mid-size resident batch's arenas and launch plans (plan_mid, plan_mid_post, plan_mid_fit,
// plan_mid_draw, which lfm_mbatch.hip and lfm_mid.hip only read); and
// the joint samples' generator and launch plan (plan_sample, which lfm_sample.hip only reads); and
// the leave-one-out calls' map of the bordered matrix and their grids (plan_loo, which lfm_loo.hip
// and lfm_api.hip only read).
// Plain C++ (no HIP types), so lfm_host.cpp also builds into the host sanitizer check
// (tests/native, `make -C tests/native asan`) with g++ -fsanitize=address,undefined.
#pragma once

#include <atomic>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/lfm.h"  // lfm_adam
#include "lfm_mid_plan.h"    // the mid-size resident batch's layout and plan (plan_mid)
#include "lfm_small_plan.h"  // LFM_HD; the small-problem path's layout and plans

namespace lfm {

// optax's bias corrections of the nsteps steps of an on-device fit that follow step0 earlier ones
// (lfm_batch_fit_f64, lfm_mbatch_fit_f64): out[2 s] = 1 - b1^count, out[2 s + 1] = 1 - b2^count,
// count = step0 + s + 1, with the host's pow (the restatement's numbers:
// dis_project_amd/trainer.py adam). out: 2 nsteps doubles.
void adam_bias(const lfm_adam* opt, int64_t step0, int64_t nsteps, double* out);

// JAX gather semantics for a gene index stored as a float: trunc toward zero, negative wraps
// by +G, clamp to [0, G - 1] (NaN -> 0).
LFM_HD inline int gene_index(double g, int G) {
  double tg = trunc(g);
  if (tg < 0) tg += (double)G;
  if (!(tg >= 0)) tg = 0;  // also catches NaN
  if (tg > (double)(G - 1)) tg = (double)(G - 1);
  return (int)tg;
}
// int(flag) as the reference's switches read it (trunc; NaN -> 0; saturated)
LFM_HD inline long long flag_int(double f) {
  double tf = trunc(f);
  if (!(tf == tf)) return 0;
  if (tf > 4e18) tf = 4e18;
  if (tf < -4e18) tf = -4e18;
  return (long long)tf;
}

// Structure of x detected on the host: rows come in blocks of T consecutive rows that share
// one uniform time vector t[tau] = t0 + tau*dt, one gene index per block and flag 1 — the
// layout dataset_3d (src/dataset.py:358-399) produces.
struct GridLayout {
  bool ok = false;
  int T = 0;          // timepoints per block
  int nblk = 0;       // number of blocks (= n / T)
  double t0 = 0, dt = 0;
  std::vector<double> times;   // [T]  the actual time values of block 0
  std::vector<int> block_gene; // [nblk] clamped gene index per block
};

GridLayout detect_grid(const double* x, int64_t n, int64_t G);
// SmallShape::T of a small problem with this layout: on the grid path when its tables fit
inline int small_grid_T(const GridLayout& lay, int64_t G) {
  return lay.ok && tables_doubles((int)G, lay.T) <= (size_t)SMALL_GRID_TAB_MAX ? lay.T : 0;
}

// Super-panel plan of a blocked factorisation over nblk block columns of width nb: (first
// block column, width in block columns) per step. Width wbulk (the first bulk step 4) while
// the trailing matrix has >= w4min rows, 4 if wbulk does not fit, 2 down to w2min rows, else
// 1; schedule 3 starts with a super-panel of w0 (1 or 2) columns. Bordered (the gradient's
// inverse): the trailing window is a constant Mp + nb rows.
std::vector<std::pair<int64_t, int>> plan_steps(int64_t nblk, int64_t Mp, int nb, bool bordered,
                                                bool s3, int wbulk, int64_t w4min,
                                                int64_t w2min, int w0 = 1);

// Rest regions of at most this many tile columns are enumerated as bands (column by column),
// wider ones as the supertiled triangle below (lfm_chol.hip unit_tile).
constexpr int kBandMaxCols = 8;

// Host mirror of the step kernel's rest-triangle enumeration (64-row slabs x 128-column tiles,
// Q x Q supertiles; lfm_chol.hip syrk_unit): unit b -> (64-row slab ti, 128-column tile tj)
// relative to the trailing matrix, tile columns [tj_lo, T).
void rest_unit_tile(int64_t b, int T, int tj_lo, int Q, int* ti_out, int* tj_out);

// The side-CU helper's share of a step's rest units: the main launch of U unit-equivalents
// takes D0 = U t / (S_m o) alone (t: one depth-kd unit, o: slot occupancy, S_m / S_h: the
// main / side stream's workgroup slots); giving x units to the helper, which starts after
// the next chain (tc, us), balances at x t (1 / S_h + 1 / S_m) = o (D0 - tc). No helper for
// D0 < dmin; at most half the rest units.
int64_t helper_units(int kd, int na, int nr, int nt, int wnext, int nb, int cus, int side_cus,
                     double tc, double dmin);

// Caps a helper share hu (the tail [nr - hu, nr) of the enumeration) so that it holds no lead
// tile (tile rows and columns < wn + lead: the inputs of the chain two steps ahead, which only
// the main launch writes through and counts). In the supertile order every unit of triangle
// rows < lead precedes the first unit of supertile row ceil(lead / Q). Returns 0 if the
// enumeration mirror still finds a lead tile in the tail, and for band-enumerated regions
// (T - wn <= kBandMaxCols).
int64_t helper_clamp(int64_t hu, int nr, int T, int wn, int lead, int Q);

// Workgroups of a step launch's ahead / rest segment: the units padded to a multiple of 8 (one
// queue per XCD)
LFM_HD constexpr int64_t pad8(int units) { return (int64_t)(units + 7) / 8 * 8; }
// ... and of its tall segment: a multiple of 8 split (8 XCDs, the pieces of one row block back
// to back: lfm_chol.hip tall_or_xcd_range)
LFM_HD constexpr int64_t tall_grid(int64_t nt, int split) {
  return (nt + 8 * split - 1) / (8 * split) * (8 * split);
}

// Events a factorisation of S steps orders its streams with (lfm_chol_sched.hip): [0] inputs
// ready, [1, 2 S + 1) per-step pairs, [2 S + 1] side stream done, [2 S + 2] hand-back,
// [2 S + 3, 3 S + 3) the chains of LFM_S3_EVENTS=2
constexpr size_t chol_events(int S) { return 3 * (size_t)S + 3; }

// What schedule 3's plan needs besides the step list. st / tall_split / supertile: the kernels'
// tile constants (lfm_chol.h ST, TALL_SPLIT, SUPERTILE); the knobs as lfm_internal.h Knobs has
// them. prof: also enumerate the helpers' algorithmic flops (S3Step::helper_alg; a loop over
// every helper unit's rows, so only while the profiler is on).
struct S3Params {
  int64_t n = 0, Mp = 0;
  bool bordered = false, fused = false, prof = false;
  int nb = 128, st = 128, tall_split = 2, supertile = 6;
  int cus = 256, side_cus = 32;
  int helper = 1;
  double helper_tc = 700, helper_min = 1200;
  int64_t ovl_at = 6144;
};
inline bool operator==(const S3Params& a, const S3Params& b) {
  auto t = [](const S3Params& p) {
    return std::tie(p.n, p.Mp, p.bordered, p.fused, p.prof, p.nb, p.st, p.tall_split, p.supertile,
                    p.cus, p.side_cus, p.helper, p.helper_tc, p.helper_min, p.ovl_at);
  };
  return t(a) == t(b);
}

// Step s of schedule 3: super-panel s (columns [K0, K1), w block columns), its X_s (the tall
// units), its trailing update (ahead + rest units) and the launches that carry them. The
// device-ordered step launch s is update(s) + tall(s + 1); LFM_S3_EVENTS=1 launches the two
// apart.
struct S3Step {
  int64_t K0 = 0, K1 = 0;
  int w = 0, kd = 0;    // kd = W_s = nb w: the depth of the step's update
  int T = 0, wn = 0;   // trailing 128-tiles from K1; the next super-panel's width (0: none)
  int na = 0, nr = 0;   // ahead units; the whole rest enumeration (the main launch: nr - hu)
  // tall units: X_s = A[tr0 .., tk0 ..) Bd_s, tw column blocks
  int nt = 0, tw = 0;
  int64_t tr0 = 0, tk0 = 0;
  int64_t zero_from = INT64_MAX, copy_from = INT64_MAX;  // StepArgs (bordered only)
  bool gen = false;     // the update generates Sigma (fused gram: step 0)
  // chain(s + 2) starts while launch s runs: lead = w_{s+2} (0: none waits); xtarget: the lead
  // units of launch s - 2 chain(s) waits for (s >= 2), w_s (w_s + 1) rest + 2 w_s w_{s-1} ahead
  int lead = 0;
  unsigned xtarget = 0;
  int64_t hu = 0;       // the side-CU helper's share: rest units [nr_main, nr), nr_main = nr - hu
  int nr_main = 0;
  // this step's flags (offsets into the flag array): chain_done[s], a_done[s][0], bars[s],
  // xready[s]
  size_t f_done = 0, f_adone = 0, f_bar = 0, f_xready = 0;
  int64_t grid = 0;     // step launch s: pad8(na) + pad8(nr_main) + tall_grid(nt_{s+1})
  int64_t hgrid = 0;    // helper launch
  int64_t ugrid = 0, tgrid = 0;  // update(s) alone (no helper), tall(s) alone
  bool ovl_mark = false;         // the overlap tail (LFM_OVL_AT) starts ahead of launch s
  // the (s & 1) buffers, in doubles: the chain's workspace in wk, Bd_s in wk, X_s in xbuf
  size_t wk_off = 0, bd_off = 0, x_off = 0;
  // profiling (lfm_profile_read): algorithmic / issued flops of step launch s, of update(s) and
  // tall(s) alone, of the helper and of chain(s)
  double step_alg = 0, step_issued = 0, upd_alg = 0, upd_issued = 0, tall_alg = 0,
         tall_issued = 0, helper_alg = 0, helper_issued = 0, chain_alg = 0, chain_issued = 0;
};

struct S3Plan {
  // what the plan was built from: a context keeps its last plan per mode and builds the next
  // call's only when these differ (the helper's lead-tile scan makes a plan cost 0.2 - 1 ms of
  // host time at N = 16384, which would otherwise precede the call's first launch)
  S3Params params;
  std::vector<std::pair<int64_t, int>> step_list;
  int S = 0;
  int64_t Wmax = 0, Tmax = 0;
  size_t wk_bytes = 0, xbuf_bytes = 0, zvec_bytes = 0, linv_bytes = 0, xd_bytes = 0,
         flags_bytes = 0;
  // the flag array (unsigned): chain_done [S], a_done [S][Tmax], bars [S], xready [S]
  size_t nflags = 0, chain_done = 0, a_done = 0, bars = 0, xready = 0;
  int64_t pad_end = 0, zsplit = 0;
  size_t nevents = 0;
  std::vector<S3Step> steps;
};

// The whole launch plan of one schedule-3 factorisation over plan_steps' step list, computed
// once per call (lfm_chol_sched.hip reserves what it says and issues its launches).
S3Plan plan_s3(const std::vector<std::pair<int64_t, int>>& steps, const S3Params& p);
// The same through a kept plan (a context's last one in this mode): rebuilt only if it was built
// from other inputs. Returns whether it was rebuilt.
bool plan_s3_keep(S3Plan& kept, const std::vector<std::pair<int64_t, int>>& steps,
                  const S3Params& p);

// ------------------------------------------------- resident posterior (lfm_post.hip)
// A predict against a resident factor (lfm_post_predict_f64): the m test rows go through in
// chunks of `chunk` rows; per chunk Vt (rows x Np, row-major) holds K(t, x) and is solved in
// place by a right-looking sweep over super-panels of up to POST_W block columns: one panel
// launch (64 test rows per workgroup) and, while block columns remain to the right, one update
// launch (one workgroup per 128 x 128 tile). With the covariance the single chunk is followed by
// one launch over the lower 128-tiles of the m x m output.
constexpr int POST_W = 4;                                 // super-panel width, block columns
constexpr size_t POST_VT_BUDGET = (size_t)1 << 30;        // bytes of Vt the default chunk keeps to
constexpr int64_t POST_CHUNK_MAX = 16384;                 // rows; also the default's upper bound

struct PostChunk {
  int64_t q0 = 0, rows = 0;  // test rows [q0, q0 + rows)
  int64_t pad_rows = 0;      // rows rounded up to 128: what the launches of this chunk touch in Vt
  int panel_grid = 0;        // workgroups of each panel launch: 64-row slabs
  int tiles = 0;             // 128-row tiles: the update launches' grid.x
};
struct PostPanel {
  int64_t K0 = 0, K1 = 0;    // columns [K0, K1) of the factor
  int w = 0;                 // (K1 - K0) / 128
  int tj0 = 0, ntj = 0;      // the update: block columns [tj0, tj0 + ntj) (ntj = 0: no launch)
};
struct ResidentPlan {
  enum Reject { OK = 0, BAD_M, COV_CHUNK, BAD_CHUNK };
  int reject = OK;
  std::string why;           // the message of a rejection
  int64_t n = 0, Np = 0, m = 0, chunk = 0;
  std::vector<PostChunk> chunks;
  std::vector<PostPanel> panels;
  int64_t vt_rows = 0;       // rows of Vt: the largest chunk's pad_rows
  size_t vt_bytes = 0;       // vt_rows x Np doubles
  size_t acc_bytes = 0;      // two per-row accumulators of vt_rows doubles each
  size_t t_bytes = 0;        // the staged test inputs, m x 3
  size_t out_bytes = 0;      // mean [m] then var [m]
  size_t cov_bytes = 0;      // m x m (0 without the covariance)
  int cov_tiles = 0;         // 128-tiles per side of the covariance: its grid is cov_tiles^2
};
// Default chunk for a factor of Np columns: the largest multiple of 128 rows, at most
// POST_CHUNK_MAX, whose chunk x Np doubles fit POST_VT_BUDGET (at least 128)
int64_t post_default_chunk(int64_t Np);
// n training rows, G genes, m test rows, chunk rows per pass (0: the default). Rejections in
// order: m < 1 or m % G != 0; the covariance with m above the chunk; a chunk that is no
// positive multiple of 128.
ResidentPlan plan_post(int64_t n, int64_t G, int64_t m, int64_t chunk, bool want_cov);

// ------------------------------------------------- joint samples (lfm_sample.hip)
// The generator include/lfm.h defines: Philox4x32-10 on counter c and key k, in place.
LFM_HD inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
    k0 += W0;
    k1 += W1;
  }
}
// The two uniforms in (0, 1] of pair p of sample s: u1 then u2, both exact
LFM_HD inline void sample_uniforms(uint64_t seed, uint64_t s, uint64_t p, double* u1, double* u2) {
  uint32_t c[4] = {(uint32_t)p, (uint32_t)(p >> 32), (uint32_t)s, (uint32_t)(s >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)c[0] | (uint64_t)c[1] << 32) >> 11;
  const uint64_t b = ((uint64_t)c[2] | (uint64_t)c[3] << 32) >> 11;
  *u1 = (double)(a + 1) * 0x1p-53;
  *u2 = (double)(b + 1) * 0x1p-53;
}
#if defined(__HIPCC__)
// The two standard normals of pair p of sample s (elements 2 p and 2 p + 1): Box-Muller on the
// pair's uniforms. Every generator kernel calls it and keeps its own indexing. The contraction
// setting is the function's own, whatever its caller's is: a fused multiply-add changes the bits.
__device__ __forceinline__ void sample_normals(uint64_t seed, uint64_t s, uint64_t p, double* z0,
                                               double* z1) {
  #pragma clang fp contract(off)
  double u1, u2;
  sample_uniforms(seed, s, p, &u1, &u2);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  *z0 = rad * cs;
  *z1 = rad * sn;
}
#endif

// One draw of nsamp joint samples from N(loc, scale), scale n x n (lfm_mvn_sample_f64,
// lfm_post_sample_f64): scale's lower triangle sits in an Mp x Mp matrix (Mp = round_up(n + 1,
// 128): the augmented matrix chol_factor_solve factors in place), Z (zrows x ldz, samples as
// rows, every element generated, padding included: finite) holds the normals and X (nsamp x n,
// dense) the result. One workgroup per 128 x 128 tile of X: grid (tiles_i, tiles_j), workgroup
// (bx, by) owns sample rows [128 bx, 128 bx + 128) and column tile sample_tile_col(P, by),
// deepest first; its product runs over columns [0, sample_depth(tj)) of Z and L.
constexpr int64_t SAMPLE_MAX_NSAMP = (int64_t)1 << 24;  // per call; sample0 continues a draw
constexpr int64_t SAMPLE_RANDN_GRID = 1 << 16;          // workgroups of the generator at most
struct SamplePlan {
  enum Reject { OK = 0, BAD_N, BAD_NSAMP, BAD_SAMPLE0, RANGE, TOO_MANY };
  int reject = OK;
  std::string why;           // the message of a rejection
  int64_t n = 0, nsamp = 0, sample0 = 0;
  int64_t Np = 0, Mp = 0;    // round_up(n, 128), round_up(n + 1, 128)
  int64_t ldz = 0, zrows = 0;  // Z: ldz = Np, zrows = round_up(nsamp, 128)
  size_t mat_bytes = 0;      // Mp x Mp doubles
  size_t z_bytes = 0;        // zrows x ldz
  size_t x_bytes = 0;        // nsamp x n
  int tiles_i = 0, tiles_j = 0;  // the product's grid
  int64_t pairs = 0;         // the generator's threads' work: zrows x ldz / 2 pairs
  int randn_grid = 0;        // its workgroups of 256 (grid-stride above SAMPLE_RANDN_GRID)
};
inline int sample_tile_col(const SamplePlan& P, int by) { return P.tiles_j - 1 - by; }
inline int64_t sample_depth(int tj) { return 128 * ((int64_t)tj + 1); }
// Rejections in order: n < 1 or above 2^30; nsamp < 1; sample0 < 0; sample0 + nsamp above
// 2^63 - 1; nsamp above SAMPLE_MAX_NSAMP.
SamplePlan plan_sample(int64_t n, int64_t nsamp, int64_t sample0);

// ------------------------- held-out log density on the resident posterior (lfm_post.hip)
// lfm_post_log_prob_f64: k held-out vectors scored under N(mean(t), cov(t) + diag_add I). The
// predict with the covariance is plan_post's (`pred`); the covariance is factored in the sample
// call's matrix (stride Mp = round_up(m + 1, 128), mat_bytes as plan_sample's); the residual rows
// R (stride Np = round_up(m, 128)) go through the predict's own sweep against that factor in
// passes of `pass` rows: `rows` is plan_post for a factor of m columns and k test rows in chunks
// of `pass`, whose chunks are the passes and whose panels are the sweep's launches. pass is the
// handle's chunk, capped at post_default_chunk(Np), so that R stays within POST_VT_BUDGET.
constexpr int64_t LOGP_MAX_K = (int64_t)1 << 24;  // held-out vectors per call
struct PostLogpPlan {
  enum Reject { OK = 0, BAD_M, COV_CHUNK, BAD_CHUNK, BAD_K, TOO_MANY };
  int reject = OK;
  std::string why;           // the message of a rejection
  int64_t m = 0, k = 0;
  int64_t Np = 0, Mp = 0;    // round_up(m, 128), round_up(m + 1, 128)
  int64_t pass = 0;          // held-out rows per pass, a multiple of 128
  ResidentPlan pred;         // the predict with the covariance: plan_post(n, G, m, chunk, true)
  ResidentPlan rows;         // the sweep over cov's factor: plan_post(m, 1, k, pass, false)
  size_t mat_bytes = 0;      // Mp x Mp: the covariance's factor
  size_t dinv_bytes = 0;     // Np / 128 x 8 inverses of its 16 x 16 diagonal blocks
  size_t zero_bytes = 0;     // the sweep's z: Np zeros
  size_t vt_bytes = 0;       // the larger of the predict's Vt and R (rows.vt_rows x Np)
  size_t acc_bytes = 0;      // the larger of the two sweeps' row accumulators
  size_t logp_bytes = 0;     // one pass's results: rows.vt_rows doubles
  int dinv_grid = 0;         // post_dinv_kernel: one workgroup per 128-block of the factor
  int z_grid = 0;            // post_z_kernel: workgroups of 256 over Np columns
  int resid_grid = 0;        // post_resid_kernel: grid (resid_grid, pad_rows), 256 pairs each
};
// Rejections in order: plan_post's with the covariance (m < 1 or m % G != 0; m above the chunk; a
// bad chunk); k < 1; k above LOGP_MAX_K.
PostLogpPlan plan_post_logp(int64_t n, int64_t G, int64_t m, int64_t k, int64_t chunk);

// ------------------------------ leave-one-out CV (lfm_loo.hip)
// lfm_loocv_f64 / lfm_loocv_grad_f64 work inside the gradient call's bordered matrix A (2Mp x 2Mp
// at stride ld = 2Mp, Mp = round_up(n + 1, 128)). After the bordered elimination the bottom-right
// block holds Bt (lower-stored, n x n) and the row a; the top-left block (the factor, read by
// nobody after the factorisation's reduction) takes Bs = S^{-1} diag(sqrt c), Np x Np dense and
// zero-padded (Np = round_up(n, 128) <= Mp), and the top-right block (never written by either
// schedule) takes W_loo's lower triangle, n x n. Offsets are in doubles from A. The O(n) vectors
// (mu, var, sqrt c, b, u: Np doubles each, then the value and a^T b) live in scratch the context
// owns, at `vec` doubles from its start.
struct LooPlan {
  enum Reject { OK = 0, BAD_N, TOO_LARGE };
  int reject = OK;
  std::string why;           // the message of a rejection
  int64_t n = 0, Np = 0, Mp = 0, ld = 0;
  int64_t bt = 0, a = 0;     // Bt's first element and the row a
  int64_t bs = 0, w = 0;     // Bs and W_loo
  size_t mat_bytes = 0;      // ld x ld doubles
  int64_t mu = 0, var = 0, sc = 0, b = 0, u = 0, val = 0;  // from the scratch's start
  int64_t vec = 0;           // doubles of scratch: 5 Np + 2
  size_t vec_bytes = 0;
  int64_t tiles = 0;         // Np / 128
  int64_t product_grid = 0;  // loo_product_kernel: the lower 128 x 128 tiles, tiles (tiles + 1) / 2
  int64_t scale_tiles = 0;   // loo_scale_kernel: grid (scale_tiles, scale_tiles) of 64 x 64 tiles
  int64_t u_grid = 0;        // loo_u_kernel: strips of 64 rows
};
// Lower tile b of the product's grid: row tile ti, column tile tj <= ti, row-major over the
// triangle (b = ti (ti + 1) / 2 + tj).
LFM_HD inline void loo_tile(int64_t b, int64_t* ti, int64_t* tj) {
  int64_t q = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((q + 1) * (q + 2) / 2 <= b) ++q;
  while (q * (q + 1) / 2 > b) --q;
  *ti = q;
  *tj = b - q * (q + 1) / 2;
}
// Rejections in order: n < 1 or above 2^30; a matrix or a grid beyond what size_t / a launch holds.
LooPlan plan_loo(int64_t n);

// Readers-writer lock over one GPU's library work (lfm_ctx.hip DeviceTenancy: a schedule-3
// factorisation exclusive, all other GPU work shared). In-process a std::shared_mutex; across
// processes flock on `path` (LOCK_EX / LOCK_SH; the process's shared hold is counted over its
// threads, taken by the first reader and dropped by the last) behind a turnstile file (`path`
// with ".turn" for ".lock"): a writer holds the turnstile while it waits for the readers to
// drain, and every reader passes through it first, so a stream of readers, of this process or
// another, cannot starve a writer. flock is per open file description, so two TenancyLock
// objects on one path behave like two processes. Waits block; nothing is held while waiting on
// anything but these locks.
class TenancyLock {
 public:
  // Opens (creating) the lock and turnstile files once; false: unavailable (the lock is then
  // in-process only). Thread-safe; later calls return the first result.
  bool open(const std::string& path);
  void lock_exclusive();
  void unlock_exclusive();
  void lock_shared();
  void unlock_shared();
  std::string path();
  // 0, or the errno of the first flock failure (the lock is then in-process only)
  int error() const { return err_.load(std::memory_order_acquire); }
  ~TenancyLock();

 private:
  bool files() const;                     // the cross-process part is in use
  void fail(int e, const char* what);     // records (and logs) the first flock failure
  std::atomic<int> err_{0};
  bool fd_held_ = false;  // LOCK_EX on fd_ held by this process's exclusive holder
  bool sh_held_ = false;  // LOCK_SH on fd_ held for this process's shared holders (fd_mu_)
  std::shared_mutex rw_;  // in-process readers-writer lock
  std::mutex turn_mu_;    // this process's threads at the turnstile, one at a time
  std::mutex fd_mu_;      // readers_ and the flock state of fd_
  std::mutex open_mu_;
  int readers_ = 0;       // this process's shared holders (LOCK_SH held while > 0)
  int fd_ = -1, turn_ = -1;
  bool opened_ = false, ok_ = false;
  std::string path_;
};

}  // namespace lfm
