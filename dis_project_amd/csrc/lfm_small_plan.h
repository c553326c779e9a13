// lfm_small_plan.h — the small-problem path's layout and launch plans (n <= SMALL_MAX, one
// workgroup per problem): the LDS map the kernels of lfm_small.hip build and the sizes derived
// from it, the staging area of a batch's inputs, the resident batch's pinned buffer, the fit's
// device buffer and the batched posterior's whole plan. Plain C++ (part of lfm_host.h): the
// kernels and lfm_batch.hip only read it, and tests/native/host_check.cpp checks it by
// enumeration (check_small_*).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define LFM_HD __host__ __device__
#else
#define LFM_HD
#endif

namespace lfm {

constexpr size_t SMALL_LDS_BYTES = 160 * 1024;  // a CU's LDS: the limit of every small launch
constexpr int SMALL_MAX = 128;       // largest n handled by small_mll_kernel
constexpr int SMALL_GRAD_MAX = 127;  // largest n of the batched gradient / fit / posterior
// largest per-problem grid table (doubles) in LDS: with n = 128 beside it the launch stays
// within SMALL_LDS_BYTES
constexpr int SMALL_GRID_TAB_MAX = 2048;

// doubles of the structured gram's per-gene tables (their layout: lfm_gram.hip)
LFM_HD inline size_t tables_doubles(int G, int T) {
  const size_t W = 2 * (size_t)T - 1;
  return 2 * (size_t)G * W + 3 * (size_t)G * T + (size_t)G * G;
}

// LDS map of one problem (doubles from the dynamic shared memory base), shared by the MLL,
// gradient and fit kernels:
//   A      [M x ld]         Sigma's lower triangle and the residual row n (M = n + 1; ld the odd
//                           one of n + 2, n + 3: a wave's accesses down a column, lane r at row r,
//                           are then free of LDS bank conflicts)
//   red    [16]             reductions
//   hyp    [3G + 3]         D S B, l, obs_stddev, jitter (the constrained parameters)
//   ktab   [3G + n + nG]    KxxTab's per-gene / per-row factors (tabs: n + 1 <= 64 in the launch):
//                           gam [G], 2G unused since the erfc form, qr [n], pr [nG]
//   colbuf [128 / 512]      the factor's column buffer(s): one wave 128; two waves (n + 1 > 64)
//                           two of 256 (rows, a zero tail, the next pivot in slot 255)
//   xs, ys [3n], [n]
//   gt     [2GW + 3GT + G^2] the grid layout's gram tables (grid problems, W = 2T - 1)
//   tms, bgs [T], [n / T]    the grid layout's times and block genes (grid problems)
// the gradient and the fit (GRAD) add, past this problem's gram tables:
//   gg     [6GW + 8GT]      the grid layout's derivative tables (grad_table_entry)
//   al, wd [128 each]       alpha = Sigma^{-1} r, diag(W)
//   accw   [4][2G + 1]      the waves' partial sums of 1/2 tr(W dSigma / d{D, S, l})
//   wb     [(n + 1) x ldw]  one wave: W's rows as the sweep leaves them (small_sweep_w)
//   gout   [3G + 3]         the gradient in the packed layout (dD dS dB, dl, d obs_stddev, 0)
//   fcol   [128]            one wave: the column buffer of the value's factor, which wave 1 runs
//                           beside wave 0's sweep (four waves factor first, in colbuf)
// and the fit (FIT): raw, mu, nu [3G + 3 each] (the unconstrained parameters, Adam's moments).
// The regions are disjoint and inside the returned size for every shape the kernels take:
// host_check's check_small_map enumerates them.
struct SmallMap {
  double *A, *red, *hyp, *ktab, *colbuf, *xs, *ys, *gt;
  double *gg, *al, *wd, *accw, *gout, *raw, *mu, *nu, *tms, *fcol, *wb;
  int* bgs;
  int n, ld, G;
};
// the four-wave sweep's buffers (small_sweep4): per step parity a row buffer (256) and its
// copy shifted by one (258), then per parity the crossing slots (128), then two wave sums
constexpr int SWEEP4_LDS = 2 * 520 + 2 * 128 + 8;
// the sweep's register width for n + 1 rows (one wave), and the row stride of its W buffer:
// slot q of lane i's row lands at wb[i ldw + q - 1] (compile-time offsets, odd stride)
LFM_HD constexpr int small_sweep_mr(int n) { return n + 1 <= 32 ? 32 : 64; }
LFM_HD constexpr int small_wb_ld(int n) { return small_sweep_mr(n) | 1; }
// doubles of the map (sm = nullptr: the size only)
LFM_HD inline size_t small_map(double* sm, int n, int G, int T, int tabs, int grad, int fit,
                               SmallMap* m) {
  size_t o = 0;
  auto take = [&](size_t k) {
    double* p = sm ? sm + o : nullptr;
    o += k;
    return p;
  };
  const size_t W = T > 0 ? 2 * (size_t)T - 1 : 0;
  SmallMap q{};
  q.n = n;
  q.ld = (n + 2) | 1;
  q.G = G;
  q.A = take((size_t)(n + 1) * q.ld);
  q.red = take(16);
  q.hyp = take(3 * (size_t)G + 3);
  q.ktab = take(tabs ? 3 * (size_t)G + n + (size_t)n * G : 0);
  o = (o + 1) & ~(size_t)1;  // 16-B aligned: the sweep reads its row buffers 16 B at a time
  // one wave: the factor's 128 or the sweep's two row buffers (2 x 64 and its copy shifted by
  // one, 2 x 64 + 2); two waves: two 256-slot column buffers
  q.colbuf = take(n + 1 > 64 ? (grad ? SWEEP4_LDS : 512) : 264);
  q.xs = take(3 * (size_t)n);
  q.ys = take((size_t)n);
  q.gt = take(T > 0 ? 2 * (size_t)G * W + 3 * (size_t)G * T + (size_t)G * G : 0);
  // the grid layout's times and block genes, staged with x and y (read every element / step)
  q.tms = take(T > 0 ? (size_t)T : 0);
  q.bgs = reinterpret_cast<int*>(take(T > 0 ? ((size_t)n / T + 1) / 2 + 1 : 0));
  if (grad) {
    q.gg = take(T > 0 ? 6 * (size_t)G * W + 8 * (size_t)G * T : 0);
    q.al = take(128);
    q.wd = take(128);
    // one wave (n + 1 <= 64): W's rows as the sweep leaves them, row stride ldw (small_wb_ld)
    q.wb = take(n + 1 <= 64 ? (size_t)(n + 1) * small_wb_ld(n) : 0);
    q.accw = take(4 * (2 * (size_t)G + 1));
    q.gout = take(3 * (size_t)G + 3);
    q.fcol = take(n + 1 <= 64 ? 128 : 0);
  }
  if (fit) {
    q.raw = take(3 * (size_t)G + 3);
    q.mu = take(3 * (size_t)G + 3);
    q.nu = take(3 * (size_t)G + 3);
  }
  if (m) *m = q;
  return o;
}

// The posterior kernel's LDS: the problem's map, then invd [n]; the K(x, t) panel follows with
// small_post_cols columns (a power of two, 16 ... 256; 0: the problem does not fit)
LFM_HD inline size_t small_post_base(int n, int G, int T) {
  return small_map(nullptr, n, G, T, n + 1 <= 64, 0, 0, nullptr) + (size_t)n;
}
LFM_HD inline int small_post_cols(int n, int G, int T) {
  const size_t base = small_post_base(n, G, T), cap = SMALL_LDS_BYTES / sizeof(double);
  for (int c = 256; c >= 16; c >>= 1)
    if (base + (size_t)n * c <= cap) return c;
  return 0;
}

// LDS doubles a grid-layout problem adds to its map: the gram tables, the times, the block genes
inline size_t small_grid_extra(int n, int G, int T) {
  return small_map(nullptr, n, G, T, 0, 0, 0, nullptr) - small_map(nullptr, n, G, 0, 0, 0, 0, nullptr);
}
// doubles a grid problem's times [T] and block genes [n / T] (ints) take in the staging area at
// most (T = n)
inline int64_t small_grid_doubles(int64_t n) { return n + (n + 1) / 2; }

// One problem as the plans see it. T: timepoints per block of its grid layout, 0 when x is not
// on one or its tables are past SMALL_GRID_TAB_MAX (lfm_host.h small_grid_T)
struct SmallShape {
  int n, G, T;
};
// what an MLL launch over small problems is sized by: the largest n and num_genes, and the
// largest small_grid_extra of the problems on the grid path (doubles; 0: none)
struct SmallDims {
  int maxn = 1, maxg = 1, gridtab = 0;
};
SmallDims small_dims(const std::vector<SmallShape>& shapes);

// The MLL launch: tables (KxxTab) when every problem has n + 1 <= 64 rows. Every other part of a
// problem's map grows with n and G, so the map of (maxn, maxg) plus the largest grid part holds
// every problem's (host_check's check_small_bound).
struct SmallMllPlan {
  size_t lds_bytes;
  int tabs;
};
SmallMllPlan plan_small_mll(const SmallDims& d);
// LDS bytes of the gradient (fit = 0) or fit (fit = 1) launch: the largest problem's map; 0 when
// a problem has n > SMALL_GRAD_MAX (two waves hold n + 1 rows) or a map past SMALL_LDS_BYTES
size_t small_grad_lds(const std::vector<SmallShape>& shapes, int fit);

// The staging area of a batch's inputs (doubles): per problem x (3n), y (n), with hyp_inline
// its hyperparameters D S B (3G) and l obs_stddev jitter (3), then a grid problem's times (T)
// and block genes (n / T ints). bound: what the callers allocate, every grid part taken at
// small_grid_doubles(n) (a problem off the grid path leaves its grid slots unused).
struct SmallPack {
  struct Slot {
    size_t x, y, dsb, sc, grid;  // dsb = sc = grid without hyp_inline
  };
  std::vector<Slot> at;
  size_t bound = 0;
};
SmallPack plan_small_pack(const std::vector<SmallShape>& shapes, bool hyp_inline);

// A resident batch's pinned buffer (doubles): hyp [nhyp] | out [nprob] | status [nprob] (ints, in
// nprob doubles) | grad [nhyp]
struct BatchLayout {
  size_t out = 0, status = 0, grad = 0, bytes = 0;
};
BatchLayout batch_layout(int64_t nhyp, int64_t nprob);
// The fit's device buffer (doubles): raw mu nu [3 nhyp] | bias [2 nsteps] | history
// [nsteps nprob] | status [nprob] (ints); each region ends where the next begins
struct FitLayout {
  size_t mu = 0, nu = 0, bias = 0, hist = 0, status = 0, bytes = 0;
};
FitLayout fit_layout(int64_t nhyp, int64_t nprob, int64_t nsteps);

// The batched posterior (lfm_batch_posterior_f64; lfm_small.hip small_post_kernel). One entry
// per problem: where its test inputs, outputs and workspace start in the call's packed arrays.
struct PostProb {
  int64_t t_off;    // rows of t / entries of mean and var before this problem's (sum of m)
  int64_t v_off;    // doubles of V = L^{-1} K(x, t) before this problem's n x m block
  int64_t cov_off;  // doubles of cov before this problem's m x m block (sum of m^2)
  int m;            // test rows
  int dv_off;       // entries of diag_vec before this problem's (sum of n)
  int tile0;        // covariance launch: 16 x 16 lower-triangle tiles before this problem's
  int pad;
};
// One call's plan. A pass of a workgroup covers min(unit, small_post_cols) test columns; unit is
// 64, or 256 when 64 would make more than 4096 workgroups; a workgroup takes every nsplit-th
// pass (grid (nprob, nsplit)). The call's one device buffer, in doubles: the inputs hyp [nhyp] |
// diag_add [nprob] | diag_vec [sn] (has_dv) | t [3 sm] | the PostProb table (in_bytes in all, staged
// in pinned memory and uploaded in one copy); then the outputs mean [sm] | var [sm] | V [sv] |
// cov [sc] | status [nprob] (ints).
struct PostPlan {
  enum Reject { OK = 0, BAD_M, NO_FIT, TOO_LARGE };
  Reject reject = OK;  // the first limit hit, problems in order (the other fields then unset)
  std::vector<PostProb> pp;
  int unit = 64, nsplit = 1, ntiles = 0;
  int64_t sm = 0, sn = 0, sv = 0, sc = 0;
  size_t dadd = 0, dv = 0, t = 0, table = 0;  // hyp at 0
  size_t mean = 0, var = 0, V = 0, cov = 0, status = 0;
  size_t in_bytes = 0, all_bytes = 0, lds_bytes = 0;
};
PostPlan plan_small_post(const std::vector<SmallShape>& shapes, int64_t nhyp, const int64_t* m,
                         bool has_dv, bool has_cov);

}  // namespace lfm
