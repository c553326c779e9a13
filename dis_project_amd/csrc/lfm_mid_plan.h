// lfm_mid_plan.h — layout and launch plan of the resident batch of mid-size problems
// (lfm_mbatch_*, 1 <= n <= MID_MAX_N): every problem's regions in the handle's device arena, the
// grids and the launch list of a value call and of a value-and-gradient call. Plain C++ (part of
// lfm_host.h): lfm_mbatch.hip (the handle and its calls) and lfm_mid.hip (the kernels and their
// launcher) only read it, and tests/native/mid_plan_check.cpp checks it by enumeration under the
// sanitizers.
//
// Per problem the arena holds x [n x 3], y [n] and, with Mp = 64 ceil((n + 1) / 64) and
// nb = Mp / 64 block rows, three Mp x Mp row-major matrices:
//   S   the augmented matrix (row n: the residual y - m(x); rows past n: identity), filled per
//       call from the packed hyperparameters; the gradient call overwrites it with X = L^{-1}
//   L   the factor (row n: z = L^{-1} (y - m(x)), unit pivot)
//   W   S^{-1} over the lower tiles (gradient call)
// then the nb inverses of the factor's 64 x 64 diagonal blocks and the pairs launch's partial
// sums, MID_PART doubles per lower tile. Ordering between launches is the stream's alone: no
// launch reads what another workgroup of the same launch writes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "lfm_small_plan.h"  // LFM_HD

namespace lfm {

constexpr int MID_TILE = 64;
constexpr int MID_MAX_N = 1024;                 // LFM_MID_MAX_N
constexpr int64_t MID_MAX_PROBS = 1 << 20;      // grid.x = problems
// one tile's partial sums of 1/2 tr(W dS / d theta): by row dD [64] dS [64], by column dD [64]
// dS [64], then d l
constexpr int MID_PART = 4 * MID_TILE + 1;

LFM_HD inline int mid_blocks(int n) { return (n + 1 + MID_TILE - 1) / MID_TILE; }
LFM_HD inline int mid_tiles(int nb) { return nb * (nb + 1) / 2; }
// lower tile t -> (block row I, block column J <= I), row by row
LFM_HD inline void mid_tile_of(int t, int* I, int* J) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  *I = i;
  *J = t - i * (i + 1) / 2;
}
LFM_HD inline int mid_tile_index(int I, int J) { return I * (I + 1) / 2 + J; }

struct MidShape {
  int64_t n, G;
};

// One problem's table entry, as the kernels read it. Offsets in doubles from the arena's base;
// hv / hs: its vectors (D S B, 3 G) and scalars (l, obs_stddev, jitter) in the packed
// hyperparameters, and of its gradient in the packed gradient.
struct MidProb {
  int n, G, nb, Mp;
  int64_t hv, hs;
  int64_t x, y;
  int64_t S, L, W;
  int64_t dinv;  // [nb][64 x 64]
  int64_t part;  // [nb (nb + 1) / 2][MID_PART]
};

// What each launch's workgroup (blockIdx.x = problem p, blockIdx.y = u) owns; a workgroup whose
// problem has no such unit exits at once:
//   MID_FILL    lower tile u of S (and the status word)
//   MID_COLUMN  block (k + u, k) of L (u = 0 also the diagonal block's inverse and the status)
//   MID_VALUE   the problem's value (u = 0)
//   MID_INVERT  block column u of X = L^{-1}: tiles (i, u), i >= u, written into S
//   MID_SINV    lower tile u of W = S^{-1} = X^T X
//   MID_PAIRS   lower tile u's partial sums
//   MID_GRAD    the problem's gradient (u = 0)
// and of a posterior call (plan_mid_post), with mb = ceil(m / 64) blocks of test rows:
//   MID_POST_FILL  u < maxtiles: lower tile u of S, with the posterior's diagonal;
//                  u - maxtiles = tb * nb + k: tile (tb, k) of T = K(t, x) in the problem's V
//   MID_SOLVE      block row u of V = T L^{-T}, and the mean and variance of its 64 test rows
//   MID_COV        lower tile u of the covariance (and its mirror image)
// and of a fit call (plan_mid_fit), u = 0 alone:
//   MID_CONSTRAIN  the problem's constrained hyperparameters from its unconstrained ones, before
//                  step 0 (and its first-bad-step word cleared)
//   MID_ADAM       step k's loss and first-bad-step word, the problem's Adam update and the next
//                  step's constrained hyperparameters
// and of a predictive call (plan_mid_draw), on the second table (n = m, nq block rows):
//   MID_DRAW_SCALE    lower tile u of the covariance's augmented matrix
//   MID_DRAW_RANDN    the pairs u, u + gy, ... of the problem's normals Z
//   MID_DRAW_PRODUCT  u = sblk * maxcb + c: the 64 x 64 tile of X = mean + Z L^T of sample block
//                     sblk and column block cb - 1 - c (deepest first)
enum MidKind {
  MID_FILL = 0, MID_COLUMN, MID_VALUE, MID_INVERT, MID_SINV, MID_PAIRS, MID_GRAD,
  MID_POST_FILL, MID_SOLVE, MID_COV, MID_CONSTRAIN, MID_ADAM,
  MID_DRAW_SCALE, MID_DRAW_RANDN, MID_DRAW_PRODUCT,
  MID_KINDS  // their number: launch_mid's table has a row for each
};
struct MidLaunch {
  int kind, k;
  unsigned gx, gy;
};

struct MidPlan {
  enum Reject { OK = 0, EMPTY, BAD_N, BAD_G, TOO_MANY };
  int reject = OK;
  std::string why;
  int64_t nprob = 0, nhyp = 0;
  int maxnb = 0, maxtiles = 0;
  std::vector<MidProb> probs;
  // the arena, in doubles: the call's packed hyperparameters, values and gradient first
  int64_t hyp = 0, out = 0, grad = 0, doubles = 0;
  // then, in bytes from the arena's base: the status words [nprob] and the problem table
  size_t status = 0, table = 0, bytes = 0;
  std::vector<MidLaunch> value, value_grad;  // the two calls' launches, in stream order
};

// doubles of one problem's regions (x, y, the three matrices, the block inverses, the partials),
// each region rounded up to 2 doubles (16-byte alignment)
int64_t mid_problem_doubles(int64_t n);
// Rejections in order: no problems; too many; an n outside [1, MID_MAX_N]; a G outside [1, n] or
// that does not divide n (the first offending problem, named in `why`)
MidPlan plan_mid(const std::vector<MidShape>& shapes);

// ---------------------------------------------------------------- the posterior call
// lfm_mbatch_posterior_f64 works in a second device arena that the handle owns (allocated at the
// first posterior call, regrown when a call needs more). In doubles from its base: diag_add
// [nprob], diag_vec [sum n] (when given), t [sum m x 3], each problem's V buffer — 64 mb rows of
// Mp doubles, row-major: T = K(t, x) after the fill, V = T L^{-T} after the solve, column n of it
// -V z — then mean [sum m], var [sum m] and, when asked, cov [sum m^2], packed as the caller
// gets them; the per-problem table follows. Bytes per problem: 8 (64 mb Mp + 5 m + n + 1), plus
// 8 m^2 with the covariance. tests/native/mid_post_plan_check.cpp checks the plan by enumeration
// under the sanitizers.
constexpr int MID_MAX_M = 4096;  // LFM_MID_MAX_M

// One problem's entry of the posterior table. Offsets in doubles from the second arena's base;
// dv / cov are -1 when the call has none.
struct MidPostProb {
  int m, mb;
  int64_t dv, t, V, mean, var, cov;
};

struct MidPostPlan {
  enum Reject { OK = 0, NO_ROWS, BAD_M, TOO_MANY_ROWS };
  int reject = OK;
  std::string why;
  int64_t nprob = 0, sn = 0, sm = 0, sc = 0;  // sums of n, m and m^2
  int maxnb = 0, maxtiles = 0, maxmb = 0, maxunits = 0, maxcov = 0;
  std::vector<MidPostProb> pp;
  int64_t dadd = 0, dv = -1, t = 0, mean = 0, var = 0, cov = -1, doubles = 0;
  size_t table = 0, bytes = 0;
  std::vector<MidLaunch> launches;  // in stream order: maxnb + 2, one more with the covariance
};

// Rejections, per problem in order and within a problem in this order: m < 1; m no multiple of
// G; m > MID_MAX_M (the first offending problem and the limit are named in `why`)
MidPostPlan plan_mid_post(const std::vector<MidShape>& shapes, const int64_t* m, bool has_dv,
                          bool want_cov);

// ---------------------------------------------------------------- the fit call
// lfm_mbatch_fit_f64 works in a third device arena that the handle owns (allocated at the first
// fit call, regrown when a call needs more). In doubles from its base, each region rounded up to
// 2 doubles (16-byte alignment): raw, mu, nu [nhyp] each in the packed hyperparameters' layout,
// the bias corrections [2 nsteps] (c1, c2 of each step), history [nsteps x nprob]; then, in bytes,
// the first-bad-step words [nprob]. With e(d) = 2 ceil(d / 2):
//   bytes = 8 (3 e(nhyp) + 2 nsteps + e(nsteps nprob)) + 16 ceil(nprob / 4).
// The launch list: MID_CONSTRAIN, then per step s the value-and-gradient launches of plan_mid
// (MidPlan::value_grad, unchanged) followed by MID_ADAM with k = s: 1 + nsteps (maxnb + 7) launches.
// tests/native/mid_fit_plan_check.cpp checks the plan by enumeration under the sanitizers.
constexpr int64_t MID_FIT_MAX_STEPS = 1 << 16;  // one call's steps (a longer fit resumes: step0)

struct MidFitPlan {
  enum Reject { OK = 0, BAD_BATCH, NO_STEPS, TOO_MANY_STEPS };
  int reject = OK;
  std::string why;
  int64_t nprob = 0, nhyp = 0, nsteps = 0;
  int64_t raw = 0, mu = 0, nu = 0, bias = 0, hist = 0, doubles = 0;
  size_t first_bad = 0, bytes = 0;
  size_t per_step = 0;              // launches of one step: the value-and-gradient call's + 1
  std::vector<MidLaunch> launches;  // in stream order
};

// Rejections in order: shapes that plan_mid rejects (its message); nsteps < 1; nsteps >
// MID_FIT_MAX_STEPS (the limit is named in `why`)
MidFitPlan plan_mid_fit(const std::vector<MidShape>& shapes, int64_t nsteps);

// ---------------------------------------------------------------- the predictive call
// lfm_mbatch_predictive_f64 draws from, and scores held-out values under, N(mean_p, cov_p +
// cov_add[p] I) of every problem: after the posterior call's launches (plan_mid_post with the
// covariance, unchanged) the m_p x m_p covariance is itself an augmented matrix that
// mid_column_kernel factors, described by a second MidProb table (n = m_p) whose offsets lie in a
// fourth device arena that the handle owns (allocated at the first predictive call, regrown when a
// call needs more). With Mq = 64 ceil((m + 1) / 64), nq = Mq / 64, cb = ceil(m / 64) and
// sb = ceil(nsamp / 64), in doubles from its base, each region rounded up to 2 doubles (16-byte
// alignment): cov_add [nprob], logp [nprob], ystar [sum m] (when given); per problem the augmented
// matrix A [Mq x Mq] (lower tiles: cov + cov_add I, row m: ystar - mean or 0, identity rows), its
// factor [Mq x Mq], the nq inverses of the factor's diagonal blocks and, with samples, the
// normals Z [64 sb x 64 cb] (sample rows, padding generated too); then the samples X
// [nsamp sum m], packed as the caller gets them. In bytes after them: the seeds [nprob], the
// MidProb table and the MidDrawProb table. Per problem that is
//   8 (2 Mq^2 + 4096 nq + 2) + 8 + sizeof(MidProb) + sizeof(MidDrawProb) bytes,
//   plus 8 m with ystar, plus 8 (4096 sb cb + nsamp m) with samples
// (mid_draw_problem_bytes; the whole arena adds the rounding of the shared regions, < 64 bytes).
// The launches after the posterior's, in stream order: MID_DRAW_SCALE, MID_COLUMN for
// k = 0 .. maxnq - 1, MID_VALUE with ystar, MID_DRAW_RANDN and MID_DRAW_PRODUCT with samples:
// 1 + maxnq + (ystar ? 1 : 0) + (nsamp ? 2 : 0), whatever the problem count.
// tests/native/mid_draw_plan_check.cpp checks the plan by enumeration under the sanitizers.
constexpr int64_t MID_DRAW_MAX_NSAMP = 1 << 16;  // one call's samples (sample0 continues a draw)
constexpr int MID_DRAW_RANDN_GY = 4096;          // the generator's grid.y at most (grid-stride)

// One problem's entry of the predictive table. cov / mean: doubles into the posterior call's
// packed covariance / mean; ystar (-1 without), Z, X (-1 without samples): doubles from the
// fourth arena's base.
struct MidDrawProb {
  int m, cb, sb, pad;
  int64_t cov, mean, ystar, Z, X;
};

struct MidDrawPlan {
  enum Reject { OK = 0, NO_COV_ADD, BAD_NSAMP, NOTHING, TOO_MANY, BAD_SAMPLE0, RANGE, NO_ROWS,
                BAD_M, TOO_MANY_ROWS };
  int reject = OK;
  std::string why;
  int64_t nprob = 0, sm = 0, nsamp = 0, sample0 = 0;
  int maxnq = 0, maxtiles = 0, maxcb = 0, maxsb = 0;
  std::vector<MidProb> probs;   // the second table: n = m_p, offsets into the fourth arena
  std::vector<MidDrawProb> dp;
  int64_t cadd = 0, out = 0, ystar = -1, X = -1, doubles = 0;
  size_t seeds = 0, table = 0, dtable = 0, bytes = 0;
  std::vector<MidLaunch> launches;  // in stream order, after the posterior's
};

// bytes of one problem in the fourth arena (the formula above)
size_t mid_draw_problem_bytes(int64_t m, bool has_ystar, int64_t nsamp);
// Rejections in order: cov_add not given; nsamp < 0; neither ystar nor samples asked for;
// nsamp > MID_DRAW_MAX_NSAMP; sample0 < 0; sample0 + nsamp above 2^63 - 1; then per problem in
// order and within a problem in this order: m < 1; m no multiple of G; m > MID_MAX_N (the first
// offending problem and the limit are named in `why`).
MidDrawPlan plan_mid_draw(const std::vector<MidShape>& shapes, const int64_t* m, bool has_cov_add,
                          bool has_ystar, int64_t nsamp, int64_t sample0);

}  // namespace lfm
