// lfm_mid.hip — the resident batch of mid-size problems (lfm_mbatch_*, 1 <= n <= 1024): every
// problem's MLL, and its MLL and gradient, in a number of launches that depends on the largest
// problem alone. CustomConjMLL.step (src/objectives.py:21-78) and jax.value_and_grad of it
// (src/trainer.py:126) for a set of independent (model, dataset) problems, as
// src/notebook.py:33-75 trains them, above the one-workgroup limit of lfm_batch.
//
// Every problem has its own padded augmented matrix in the handle's arena (lfm_mid_plan.h: the
// layout, the grids and the launch list all come from plan_mid), in 64 x 64 tiles. A launch's
// grid is (problem, unit); a workgroup whose problem has no such unit exits at once.
//   mid_fill_kernel    S's lower tiles from the packed hyperparameters (kernel_ref per pair),
//                      the residual row n and the identity rows past it
//   mid_column_kernel  left-looking factorisation, one launch per block column k, unit = row
//                      block i >= k: the update from columns < k of block (i, k) and of the
//                      diagonal block (fp64 MFMA), the diagonal block's factor and inverse in LDS
//                      (every workgroup of the column redundantly: no workgroup waits for
//                      another), then X = A_ik L_kk^{-T}. A non-positive pivot goes to the
//                      problem's status word; later launches skip the problem.
//   mid_value_kernel   logdet and z^T z in a fixed order -> the value
//   mid_invert_kernel  X = L^{-1} by block columns (row n of it is -a, a = S^{-1} r)
//   mid_sinv_kernel    S^{-1} = X^T X over the lower tiles, depth n
//   mid_pairs_kernel   grad_pairs_kernel's work per lower tile with W = a a^T - S^{-1}: its
//                      per-row / per-column partial sums go to the tile's own scratch slots
//   mid_grad_kernel    joins the partials in a fixed order; tr(W), the mean terms, the sign
// and latent_predict / multi_gene_predict (src/model.py:420-514) of every problem at its own test
// inputs (lfm_mbatch_posterior_f64; the layout of its arena and its launches: plan_mid_post):
//   mid_fill_kernel<true>  S with the posterior's diagonal, (K + diag_vec) + diag_add, and in the
//                      same launch T = K(t, x), one unit per (test block, column block), into V
//   mid_column_kernel  as above
//   mid_solve_kernel   unit = a block of 64 test rows: V_uk = (T_uk - sum_{j<k} V_uj L_kj^T)
//                      D_k^T for k = 0 .. nb - 1 (fp64 MFMA), in place; column n of V is then
//                      -V z (the augmented row of L is z, with a unit pivot), so
//                      mean = m(t) - V[:, n], and var = k(t, t) - sum_{c<n} V_c^2 in column order
//   mid_cov_kernel     lower tile (a, b) of K(t, t) - V V^T over depth n, and its mirror image;
//                      the diagonal entries are var's
// and JaxTrainer.fit (src/trainer.py:162-228) of every problem (lfm_mbatch_fit_f64; its arena and
// launch list: plan_mid_fit): per step the value-and-gradient launches above, then
//   mid_adam_kernel    the step's loss into the history, the first-bad-step word, the bijectors'
//                      chain rule, the Adam update and after_epoch as small_fit_kernel's, and the
//                      next step's constrained hyperparameters where mid_fill_kernel reads them
//                      (before step 0: the constrain alone)
// with no host wait between the steps;
// and GaussianDistribution.sample / .log_prob (objectives.py:78) of every problem's
// multi_gene_predict distribution N(mean, cov + cov_add I) (lfm_mbatch_predictive_f64; its arena,
// second problem table and launch list: plan_mid_draw): after the posterior call's launches
//   mid_draw_scale_kernel    the covariance as an augmented matrix in mid_fill_kernel's layout:
//                      cov_add on the diagonal, row m = ystar - mean (or 0), identity rows
//   mid_column_kernel  as above, on the second table (n = m)
//   mid_value_kernel   as above: the augmented row of the factor -> the log density
//   mid_draw_randn_kernel    the problem's normals Z from its own seed (sample_randn_kernel's
//                      arithmetic: lfm_randn_f64's bits)
//   mid_draw_product_kernel  one workgroup per 64 x 64 tile of X = mean + Z L^T, depth
//                      64 (tj + 1) over the factor's lower tiles (fp64 MFMA).
// No atomics and no device-side waits: consecutive launches on one stream are the only ordering,
// so a problem's bits depend on its own data and hyperparameters alone.
//
// This unit holds the kernels and launch_mid, which issues one launch of a plan's list; their
// argument structs are in lfm_internal.h. The handle, the calls and the entry points:
// lfm_mbatch.hip.
#include <type_traits>

#include "lfm_internal.h"
#include "lfm_bijectors.h"
#include "lfm_chol_dev.h"
#include "lfm_dual.h"

namespace lfm {

namespace {

constexpr int TS = MID_TILE, LD = TS + LDP;
typedef double (*Tile)[LD];
constexpr size_t MID_LDS = (3 * (size_t)TS * LD + 2 * TS) * sizeof(double);

// A 64 x 64 tile at g (row stride ld) into LDS, as it is or transposed; rows >= rows read as 0.
__device__ __forceinline__ void stage(Tile s, const double* __restrict__ g, int64_t ld, bool tr,
                                      int rows = TS) {
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int idx = tid + 256 * e, r = idx >> 6, c = idx & 63;
    const double v = r < rows ? g[r * ld + c] : 0.0;
    if (tr) s[c][r] = v;
    else s[r][c] = v;
  }
}

// acc[jr][q] (C[16 w + (lane >> 4) + 4 q][16 jr + (lane & 15)], wave w) += sum_k sA[i][k] sB[j][k]
__device__ __forceinline__ void mma_nt(double4v (&acc)[4], Tile sA, Tile sB) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int kk = 0; kk < TS; kk += 4) {
    const double a = sA[16 * w + li][kk + lk];
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[jr] = mfma16(a, sB[16 * jr + li][kk + lk], acc[jr]);
  }
}

__device__ __forceinline__ void acc_zero(double4v (&acc)[4]) {
#pragma unroll
  for (int jr = 0; jr < 4; ++jr) acc[jr] = double4v{0, 0, 0, 0};
}

// f(row, column, value&) over the thread's 16 accumulator elements
template <typename F>
__device__ __forceinline__ void acc_each(double4v (&acc)[4], F f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int jr = 0; jr < 4; ++jr)
#pragma unroll
    for (int q = 0; q < 4; ++q) f(16 * w + lk + 4 * q, 16 * jr + li, acc[jr][q]);
}

__device__ __forceinline__ HypDev mid_hyp(const MidProb& P, const double* hyp) {
  const double* v = hyp + P.hv;
  return HypDev{v, v + P.G, v + 2 * P.G, P.G, hyp[P.hs]};
}

// ------------------------------------------------------------------ fill
// POST: the posterior's fill. The diagonal is (K + diag_vec) + diag_add instead of the MLL's
// (K + jitter) + sigma^2, and the units from q.maxtiles on fill T = K(t, x): unit tb * nb + k the
// 64 x 64 tile of test block tb and column block k of the problem's V buffer (rows past m and the
// columns from n on are 0).
template <bool POST>
__global__ __launch_bounds__(256) void mid_fill_kernel(
    MidArgs a, typename std::conditional<POST, MidPostArgs, MidNoPost>::type q) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  if constexpr (POST) {
    if ((int)blockIdx.y >= q.maxtiles) {
      const MidPostProb Q = q.pp[p];
      const int unit = (int)blockIdx.y - q.maxtiles;
      if (unit >= Q.mb * P.nb) return;
      const int tb = unit / P.nb, k = unit - tb * P.nb;
      const HypDev h = mid_hyp(P, a.base);
      const double* x = a.base + P.x;
      const double* t = q.base + Q.t;
      double* T = q.base + Q.V;
      const int c = TS * k + (tid & 63);
      double tx = 0.0, gx = 0.0, fx = 0.0;
      if (c < P.n) {
        tx = x[c * 3];
        gx = x[c * 3 + 1];
        fx = x[c * 3 + 2];
      }
      for (int e = 0; e < 16; ++e) {
        const int r = TS * tb + (tid >> 6) + 4 * e;
        double v = 0.0;
        if (r < Q.m && c < P.n) v = kernel_ref(h, t[r * 3], t[r * 3 + 1], t[r * 3 + 2], tx, gx, fx);
        T[(int64_t)r * P.Mp + c] = v;
      }
      return;
    }
  }
  if ((int)blockIdx.y >= mid_tiles(P.nb)) return;
  int I, J;
  mid_tile_of((int)blockIdx.y, &I, &J);
  if (blockIdx.y == 0 && tid == 0) a.status[p] = 0;
  const HypDev h = mid_hyp(P, a.base);
  const double sd = a.base[P.hs + 1], jit = a.base[P.hs + 2], s2 = sd * sd;
  const double* x = a.base + P.x;
  const double* y = a.base + P.y;
  double* S = a.base + P.S;
  const int n = P.n, c = TS * J + (tid & 63);
  const int64_t bs = n / P.G;
  double tb = 0.0, gb = 0.0, fb = 0.0;
  if (c < n) {
    tb = x[c * 3];
    gb = x[c * 3 + 1];
    fb = x[c * 3 + 2];
  }
  for (int e = 0; e < 16; ++e) {
    const int i = TS * I + (tid >> 6) + 4 * e;
    double v;
    if (i < n && c <= i) {
      v = kernel_ref(h, x[i * 3], x[i * 3 + 1], x[i * 3 + 2], tb, gb, fb);
      if (i == c) {
        if constexpr (POST) {
          const MidPostProb Q = q.pp[p];
          const double dv = Q.dv >= 0 ? q.base[Q.dv + i] : 0.0;
          v = (v + dv) + q.base[q.dadd + p];  // (K + diag(diag_vec)) + diag_add I
        } else {
          v = (v + jit) + s2;  // (K + jitter I) + sigma^2 I, objectives.py:71-72
        }
      }
    } else if (i == n && c < n) {
      v = y[c] - mean_at(h, x, c, bs);
    } else {
      v = (i == c) ? 1.0 : 0.0;
    }
    S[(int64_t)i * P.Mp + c] = v;
  }
}

// ------------------------------------------------------------------ column k
// The Cholesky factor of the block in sA (lower part read) and its inverse into sR, both in
// place, over the block's first nlim columns (the columns past them are identity columns of
// the augmented matrix: the residual row has a unit pivot). 256 threads: row tid >> 2, the
// row's elements dealt round-robin to its four threads; per column two barriers and, between
// them, one round of independent LDS loads (a step is LDS latency, not arithmetic). Row j of
// the inverse stays unscaled until the end (the rows below take it times 1 / L_jj). sdiag:
// 2 x 64 doubles. Returns the first column whose pivot is not positive, or -1.
__device__ int factor_invert(Tile sA, Tile sR, double* sdiag, int nlim) {
  const int tid = threadIdx.x, i = tid >> 2, q = tid & 3;
  double* sinv = sdiag + TS;
  for (int e = 0; e < 16; ++e) {
    const int idx = tid + 256 * e, r = idx >> 6, c = idx & 63;
    sR[r][c] = r == c ? 1.0 : 0.0;
  }
  if (tid < TS) {
    sdiag[tid] = 1.0;
    sinv[tid] = 1.0;
  }
  int fail = -1;
  for (int j = 0; j < nlim; ++j) {
    __syncthreads();
    const double d = sA[j][j];
    if (!(d > 0.0)) {
      fail = j;
      break;
    }
    const double inv = 1.0 / sqrt(d);
    if (i > j && q == 0) sA[i][j] *= inv;
    if (i == j && q == 0) {
      sdiag[j] = d * inv;
      sinv[j] = inv;
    }
    __syncthreads();
    if (i > j) {
      const double lij = sA[i][j], lr = lij * inv;
      double m[16], t[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int c = q + 4 * u;
        const bool inA = c > j && c <= i && c < nlim, inR = c <= j;
        m[u] = inA ? sA[c][j] : (inR ? sR[j][c] : 0.0);
        t[u] = inA ? sA[i][c] : (inR ? sR[i][c] : 0.0);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int c = q + 4 * u;
        const bool inA = c > j && c <= i && c < nlim, inR = c <= j;
        if (inA) sA[i][c] = t[u] - lij * m[u];
        else if (inR) sR[i][c] = t[u] - lr * m[u];
      }
    }
  }
  __syncthreads();
  if (fail < 0) {
    for (int e = 0; e < 16; ++e) {
      const int idx = tid + 256 * e, r = idx >> 6, c = idx & 63;
      if (c > r) sA[r][c] = 0.0;
      else if (c == r) sA[r][c] = sdiag[r];
      if (c <= r) sR[r][c] *= sinv[r];
    }
    __syncthreads();
  }
  return fail;
}

__global__ __launch_bounds__(256) void mid_column_kernel(MidArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS, sR = sB + TS;
  double* sdiag = sm + 3 * TS * LD;
  const int p = blockIdx.x, k = a.k, i = k + (int)blockIdx.y;
  const MidProb P = a.probs[p];
  if (i >= P.nb || a.status[p] != 0) return;
  const int64_t ld = P.Mp;
  const double* S = a.base + P.S;
  double* L = a.base + P.L;
  double4v accC[4], accD[4];
  acc_zero(accC);
  acc_zero(accD);
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    if (i > k) stage(sA, L + (int64_t)i * TS * ld + j * TS, ld, false);
    stage(sB, L + (int64_t)k * TS * ld + j * TS, ld, false);
    __syncthreads();
    if (i > k) mma_nt(accC, sA, sB);
    mma_nt(accD, sB, sB);
  }
  __syncthreads();
  // the updated diagonal block; the columns from the residual row's on are identity columns
  const int nloc = P.n - k * TS, nlim = nloc < TS ? (nloc > 0 ? nloc : 0) : TS;
  const double* Skk = S + (int64_t)k * TS * ld + k * TS;
  acc_each(accD, [&](int r, int c, double v) {
    sA[r][c] = c < nlim ? Skk[r * ld + c] - v : (r == c ? 1.0 : 0.0);
  });
  __syncthreads();
  const int fail = factor_invert(sA, sR, sdiag, nlim);
  if (fail >= 0) {
    if (i == k && threadIdx.x == 0) a.status[p] = 1 + k * TS + fail;
    return;
  }
  if (i == k) {
    double* Lkk = L + (int64_t)k * TS * ld + k * TS;
    double* Dk = a.base + P.dinv + (int64_t)k * TS * TS;
    for (int e = 0; e < 16; ++e) {
      const int idx = threadIdx.x + 256 * e, r = idx >> 6, c = idx & 63;
      Lkk[r * ld + c] = sA[r][c];
      Dk[r * TS + c] = sR[r][c];
    }
    return;
  }
  // X = (A_ik - update) L_kk^{-T}
  const double* Sik = S + (int64_t)i * TS * ld + k * TS;
  acc_each(accC, [&](int r, int c, double v) { sB[r][c] = Sik[r * ld + c] - v; });
  __syncthreads();
  acc_zero(accC);
  mma_nt(accC, sB, sR);
  double* Lik = L + (int64_t)i * TS * ld + k * TS;
  acc_each(accC, [&](int r, int c, double v) { Lik[r * ld + c] = v; });
}

// ------------------------------------------------------------------ value
// sum over the workgroup (256 threads) in a fixed order; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void mid_value_kernel(MidArgs a) {
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  const double* L = a.base + P.L;
  const int64_t ld = P.Mp;
  const bool failed = a.status[p] != 0;
  double q = 0.0, lg = 0.0;
  if (!failed)
    for (int c = tid; c < P.n; c += 256) {
      const double z = L[(int64_t)P.n * ld + c];
      q += z * z;
      lg += log(L[(int64_t)c * ld + c]);
    }
  const double Q = block_sum(q, red), LG = block_sum(lg, red);
  if (tid == 0) {
    const double two_pi = 6.283185307179586476925;
    double mll = -0.5 * ((double)P.n * log(two_pi) + 2.0 * LG + Q);
    mll *= a.negative ? -1.0 : 1.0;
    a.base[a.out + p] = failed ? __builtin_nan("") : mll;
  }
}

// ------------------------------------------------------------------ X = L^{-1}
// Block column c of X into S's tiles (i, c), i >= c, top down:
//   X_cc = L_cc^{-1},   X_ic = -L_ii^{-1} sum_{c <= m < i} L_im X_mc.
// The tiles this workgroup wrote above are the ones it reads back (workgroup barrier between).
__global__ __launch_bounds__(256) void mid_invert_kernel(MidArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS;
  const int p = blockIdx.x, c = blockIdx.y;
  const MidProb P = a.probs[p];
  if (c >= P.nb || a.status[p] != 0) return;
  const int64_t ld = P.Mp;
  const double* L = a.base + P.L;
  const double* Di = a.base + P.dinv;
  double* X = a.base + P.S;
  for (int e = 0; e < 16; ++e) {
    const int idx = threadIdx.x + 256 * e, r = idx >> 6, cc = idx & 63;
    X[((int64_t)c * TS + r) * ld + c * TS + cc] = Di[(int64_t)c * TS * TS + r * TS + cc];
  }
  for (int i = c + 1; i < P.nb; ++i) {
    double4v acc[4];
    acc_zero(acc);
    for (int m = c; m < i; ++m) {
      __syncthreads();  // also: the tile (m, c) written above is visible to the whole workgroup
      stage(sA, L + (int64_t)i * TS * ld + m * TS, ld, false);
      stage(sB, X + (int64_t)m * TS * ld + c * TS, ld, true);
      __syncthreads();
      mma_nt(acc, sA, sB);
    }
    __syncthreads();
    acc_each(acc, [&](int r, int cc, double v) { sB[cc][r] = v; });
    stage(sA, Di + (int64_t)i * TS * TS, TS, false);
    __syncthreads();
    acc_zero(acc);
    mma_nt(acc, sA, sB);
    double* Xic = X + (int64_t)i * TS * ld + c * TS;
    acc_each(acc, [&](int r, int cc, double v) { Xic[r * ld + cc] = -v; });
  }
}

// ------------------------------------------------------------------ S^{-1} = X^T X
// Lower tile (I, J): sum over the block rows m >= I of X_mI^T X_mJ, the rows from n on left out
// (row n of X is -a; the rows past it are identity rows).
__global__ __launch_bounds__(256) void mid_sinv_kernel(MidArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS;
  const int p = blockIdx.x;
  const MidProb P = a.probs[p];
  if ((int)blockIdx.y >= mid_tiles(P.nb) || a.status[p] != 0) return;
  int I, J;
  mid_tile_of((int)blockIdx.y, &I, &J);
  const int64_t ld = P.Mp;
  const double* X = a.base + P.S;
  double4v acc[4];
  acc_zero(acc);
  for (int m = I; m < P.nb; ++m) {
    const int rows = P.n - m * TS;
    if (rows <= 0) break;
    __syncthreads();
    stage(sA, X + (int64_t)m * TS * ld + I * TS, ld, true, rows);
    stage(sB, X + (int64_t)m * TS * ld + J * TS, ld, true, rows);
    __syncthreads();
    mma_nt(acc, sA, sB);
  }
  double* W = a.base + P.W + (int64_t)I * TS * ld + J * TS;
  acc_each(acc, [&](int r, int c, double v) { W[r * ld + c] = v; });
}

// ------------------------------------------------------------------ pairs
// Tile (I, J) of 1/2 tr(W dS / d theta), W = a a^T - S^{-1}: one thread per column, 16 rows
// each (wave w the rows w, w + 4, ...). Per pair the kernel's derivatives come from kernel_grad
// (lfm_dual.h), weighted by W (x 1/2 on the diagonal). A row's sums over the tile's columns and
// a column's over its rows go to the tile's MID_PART scratch slots, d l last.
__global__ __launch_bounds__(256) void mid_pairs_kernel(MidArgs a) {
  __shared__ double cred[2][4][TS];
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const MidProb P = a.probs[p];
  if ((int)blockIdx.y >= mid_tiles(P.nb) || a.status[p] != 0) return;
  int I, J;
  mid_tile_of((int)blockIdx.y, &I, &J);
  const HypDev h = mid_hyp(P, a.base);
  const int n = P.n;
  const int64_t ld = P.Mp;
  const double* x = a.base + P.x;
  const double* Wm = a.base + P.W;
  const double* xn = a.base + P.S + (int64_t)n * ld;  // row n of X: -a
  double* part = a.base + P.part + (int64_t)blockIdx.y * MID_PART;
  const int c = TS * J + lane;
  const bool cv = c < n;
  const int cc = cv ? c : n - 1;
  const double tb = x[cc * 3], gb = x[cc * 3 + 1], fb = x[cc * 3 + 2];
  const double ac = -xn[cc];
  double cD = 0.0, cS = 0.0, sl = 0.0;
  for (int e = 0; e < 16; ++e) {
    const int r = w + 4 * e, i = TS * I + r;  // wave-uniform
    PairGrad o{0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n && cv && c <= i) {
      double wgt = (-xn[i]) * ac - Wm[(int64_t)i * ld + c];
      if (c == i) wgt *= 0.5;
      kernel_grad(h, x[i * 3], x[i * 3 + 1], x[i * 3 + 2], tb, gb, fb, wgt, o);
    }
    const double rD = wave_sum(o.dDr), rS = wave_sum(o.dSr);
    if (lane == 0) {
      part[r] = rD;
      part[TS + r] = rS;
    }
    cD += o.dDc;
    cS += o.dSc;
    sl += o.dl;
  }
  cred[0][w][lane] = cD;
  cred[1][w][lane] = cS;
  const double s_l = block_sum(sl, red);  // its barriers also cover cred
  if (w == 0) {
    part[2 * TS + lane] = ((cred[0][0][lane] + cred[0][1][lane]) + cred[0][2][lane]) + cred[0][3][lane];
    part[3 * TS + lane] = ((cred[1][0][lane] + cred[1][1][lane]) + cred[1][2][lane]) + cred[1][3][lane];
    if (lane == 0) part[4 * TS] = s_l;
  }
}

// ------------------------------------------------------------------ gradient
// One workgroup per problem: each row's share of dD / dS (its tiles' row sums left to right,
// then its column sums top down), each gene's rows in index order, d l over the tiles in order,
// tr(W), the mean terms of m_i = (B/D)[i // (n/G)] flag_i (model.py:124-149) and the sign, as
// grad_finish_kernel. Packed as the hyperparameters; the jitter slot is 0.
__global__ __launch_bounds__(256) void mid_grad_kernel(MidArgs a) {
  __shared__ double vD[MID_MAX_N], vS[MID_MAX_N];
  __shared__ int gi[MID_MAX_N];
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  const int n = P.n, G = P.G;
  double* gv = a.base + a.grad + P.hv;
  double* gs = a.base + a.grad + P.hs;
  if (a.status[p] != 0) {
    const double nan = __builtin_nan("");
    for (int g = tid; g < 3 * G; g += 256) gv[g] = nan;
    if (tid == 0) {
      gs[0] = nan;
      gs[1] = nan;
      gs[2] = 0.0;
    }
    return;
  }
  const HypDev h = mid_hyp(P, a.base);
  const int64_t ld = P.Mp;
  const double* x = a.base + P.x;
  const double* Wm = a.base + P.W;
  const double* xn = a.base + P.S + (int64_t)n * ld;
  const double* part = a.base + P.part;
  const double sign = a.negative ? -1.0 : 1.0;
  double tr = 0.0;
  for (int i = tid; i < n; i += 256) {
    const int I = i >> 6, r = i & 63;
    double sD = 0.0, sS = 0.0;
    for (int J = 0; J <= I; ++J) {
      const double* t = part + (int64_t)mid_tile_index(I, J) * MID_PART;
      sD += t[r];
      sS += t[TS + r];
    }
    for (int I2 = I; I2 < P.nb; ++I2) {
      const double* t = part + (int64_t)mid_tile_index(I2, I) * MID_PART;
      sD += t[2 * TS + r];
      sS += t[3 * TS + r];
    }
    vD[i] = sD;
    vS[i] = sS;
    gi[i] = gene_index(x[i * 3 + 1], G);
    tr += xn[i] * xn[i] - Wm[(int64_t)i * ld + i];
  }
  const double T = block_sum(tr, red);  // its barriers also cover vD / vS / gi
  const int bs = n / G;
  for (int g = tid; g < G; g += 256) {
    double aD = 0.0, aS = 0.0, af = 0.0;
    for (int i = 0; i < n; ++i)
      if (gi[i] == g) {
        aD += vD[i];
        aS += vS[i];
      }
    for (int i = g * bs; i < (g + 1) * bs; ++i) af += (-xn[i]) * (double)flag_int(x[i * 3 + 2]);
    const double D = h.D[g], B = h.B[g];
    gv[g] = sign * (aD - B / (D * D) * af);
    gv[G + g] = sign * aS;
    gv[2 * G + g] = sign * (af / D);
  }
  if (tid == 0) {
    double dl = 0.0;
    const int nt = mid_tiles(P.nb);
    for (int t = 0; t < nt; ++t) dl += part[(int64_t)t * MID_PART + 4 * TS];
    gs[0] = sign * dl;
    gs[1] = sign * a.base[P.hs + 1] * T;
    gs[2] = 0.0;
  }
}

// ------------------------------------------------------------------ V = T L^{-T}
// Block row u of V, left to right: V_uk = (T_uk - sum_{j<k} V_uj L_kj^T) D_k^T, D_k the inverse
// of the factor's diagonal block. The tiles this workgroup wrote to its own rows of V are the
// ones it reads back (workgroup barrier between), as mid_invert_kernel. A row of V depends on its
// own row of T alone. Thread r < 64 then owns test row 64 u + r: the sum of its squares over the
// columns < n in column order, and column n, which is -(V z)_r.
__global__ __launch_bounds__(256) void mid_solve_kernel(MidArgs a, MidPostArgs q) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS;
  const int p = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  const MidPostProb Q = q.pp[p];
  if (u >= Q.mb) return;
  const int row = TS * u + tid;
  double* mean = q.base + Q.mean;
  double* var = q.base + Q.var;
  if (a.status[p] != 0) {
    if (tid < TS && row < Q.m) {
      mean[row] = __builtin_nan("");
      var[row] = __builtin_nan("");
    }
    return;
  }
  const int64_t ld = P.Mp;
  const int n = P.n;
  const double* L = a.base + P.L;
  const double* Di = a.base + P.dinv;
  double* V = q.base + Q.V + (int64_t)u * TS * ld;
  double vacc = 0.0, vn = 0.0;
  for (int k = 0; k < P.nb; ++k) {
    double4v acc[4];
    acc_zero(acc);
    for (int j = 0; j < k; ++j) {
      __syncthreads();  // also: the tile (u, j) written below is visible to the whole workgroup
      stage(sA, V + j * TS, ld, false);
      stage(sB, L + (int64_t)k * TS * ld + j * TS, ld, false);
      __syncthreads();
      mma_nt(acc, sA, sB);
    }
    __syncthreads();
    const double* Tuk = V + k * TS;
    acc_each(acc, [&](int r, int c, double v) { sA[r][c] = Tuk[r * ld + c] - v; });
    stage(sB, Di + (int64_t)k * TS * TS, TS, false);
    __syncthreads();
    acc_zero(acc);
    mma_nt(acc, sA, sB);
    __syncthreads();
    double* Vuk = V + k * TS;
    acc_each(acc, [&](int r, int c, double v) {
      Vuk[r * ld + c] = v;
      sA[r][c] = v;
    });
    __syncthreads();
    if (tid < TS) {
      const int lim = n - k * TS;  // the columns of this block below n
      for (int c = 0; c < TS && c < lim; ++c) vacc = fma(sA[tid][c], sA[tid][c], vacc);
      if (lim >= 0 && lim < TS) vn = sA[tid][lim];
    }
  }
  if (tid < TS && row < Q.m) {
    const HypDev h = mid_hyp(P, a.base);
    const double* t = q.base + Q.t;
    const double* tr = t + 3 * row;
    mean[row] = mean_at(h, t, row, Q.m / P.G) - vn;
    var[row] = kernel_ref(h, tr[0], tr[1], tr[2], tr[0], tr[1], tr[2]) - vacc;
  }
}

// A 64 x 64 tile at g into LDS with the columns >= cols read as 0
__device__ __forceinline__ void stage_cols(Tile s, const double* __restrict__ g, int64_t ld,
                                           int cols) {
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int idx = tid + 256 * e, r = idx >> 6, c = idx & 63;
    s[r][c] = c < cols ? g[r * ld + c] : 0.0;
  }
}

// ------------------------------------------------------------------ covariance
// Lower tile (A, B) of the test blocks: k(t_i, t_j) - sum_{c<n} V_ic V_jc for j <= i, written to
// (i, j) and to (j, i); the columns of V from n on are left out, as mid_sinv_kernel leaves out
// X's rows. The diagonal entries are var's (the solve's sums in column order).
__global__ __launch_bounds__(256) void mid_cov_kernel(MidArgs a, MidPostArgs q) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS;
  const int p = blockIdx.x;
  const MidProb P = a.probs[p];
  const MidPostProb Q = q.pp[p];
  if ((int)blockIdx.y >= mid_tiles(Q.mb)) return;
  int A, B;
  mid_tile_of((int)blockIdx.y, &A, &B);
  const int64_t ld = P.Mp, m = Q.m;
  double* cov = q.base + Q.cov;
  const bool failed = a.status[p] != 0;
  double4v acc[4];
  acc_zero(acc);
  if (!failed) {
    const double* V = q.base + Q.V;
    for (int k = 0; k < P.nb; ++k) {
      const int cols = P.n - k * TS;
      if (cols <= 0) break;
      __syncthreads();
      stage_cols(sA, V + (int64_t)A * TS * ld + k * TS, ld, cols);
      stage_cols(sB, V + (int64_t)B * TS * ld + k * TS, ld, cols);
      __syncthreads();
      mma_nt(acc, sA, sB);
    }
  }
  const HypDev h = mid_hyp(P, a.base);
  const double* t = q.base + Q.t;
  const double* var = q.base + Q.var;
  acc_each(acc, [&](int r, int c, double s) {
    const int64_t i = TS * A + r, j = TS * B + c;
    if (i >= m || j > i) return;
    double v = __builtin_nan("");
    if (!failed) {
      const double* ti = t + 3 * i;
      const double* tj = t + 3 * j;
      v = i == j ? var[i] : kernel_ref(h, ti[0], ti[1], ti[2], tj[0], tj[1], tj[2]) - s;
    }
    cov[i * m + j] = v;
    cov[j * m + i] = v;
  });
}

// ------------------------------------------------------------------ the predictive distribution
// The launches on the predictive call's fourth arena (MidDrawArgs) take a MidArgs whose table is
// the second one (n = m_p) and whose status words are the first arena's.

// Lower tile (I, J) of the covariance's augmented matrix, in mid_fill_kernel's layout: the lower
// triangle of cov_p with cov_add[p] joining the diagonal in one addition, row m the residual
// ystar - mean (0 without ystar), identity rows past it; above the diagonal of a diagonal tile 0.
__global__ __launch_bounds__(256) void mid_draw_scale_kernel(MidArgs a, MidDrawArgs d) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  if ((int)blockIdx.y >= mid_tiles(P.nb) || a.status[p] != 0) return;
  int I, J;
  mid_tile_of((int)blockIdx.y, &I, &J);
  const MidDrawProb D = d.dp[p];
  const int m = P.n, c = TS * J + (tid & 63);
  const double* cov = d.cov + D.cov;
  const double* mean = d.mean + D.mean;
  const double* ys = D.ystar >= 0 ? d.base + D.ystar : nullptr;
  const double ca = d.base[d.cadd + p];
  double* A = a.base + P.S;
  for (int e = 0; e < 16; ++e) {
    const int i = TS * I + (tid >> 6) + 4 * e;
    double v;
    if (i < m && c <= i) {
      v = cov[(int64_t)i * m + c];
      if (i == c) v = v + ca;
    } else if (i == m && c < m) {
      v = ys ? ys[c] - mean[c] : 0.0;
    } else {
      v = (i == c) ? 1.0 : 0.0;
    }
    A[(int64_t)i * P.Mp + c] = v;
  }
}

// The problem's normals Z [64 sb x 64 cb], row r sample sample0 + r: sample_randn_kernel's
// sample_normals (lfm_host.h) on the problem's own seed, so element (r, j) is lfm_randn_f64's
// (seeds[p], sample0 + r, j) bit for bit; the padding rows and columns are generated too.
__global__ __launch_bounds__(256) void mid_draw_randn_kernel(MidArgs a, MidDrawArgs d) {
  const int p = blockIdx.x;
  if (a.status[p] != 0) return;
  const MidDrawProb D = d.dp[p];
  const int64_t ld = (int64_t)TS * D.cb, half = ld >> 1, pairs = (int64_t)TS * D.sb * half;
  const uint64_t seed = d.seeds[p];
  double* Z = d.base + D.Z;
  for (int64_t q = (int64_t)blockIdx.y * 256 + threadIdx.x; q < pairs;
       q += (int64_t)gridDim.y * 256) {
    const int64_t r = q / half, pp = q - r * half;
    double2 v;
    sample_normals(seed, d.sample0 + (uint64_t)r, (uint64_t)pp, &v.x, &v.y);
    *reinterpret_cast<double2*>(&Z[r * ld + 2 * pp]) = v;
  }
}

constexpr size_t MID_DRAW_LDS = 2 * (size_t)TS * LD * sizeof(double);

// The 64 x 64 tile (sample block, column block tj) of X = mean + Z L^T: depth 64 (tj + 1) over
// the factor's lower tiles (tj, k), k <= tj, in that order whatever nsamp and sample0 are; a row
// of X depends on its own row of Z alone. mean joins in one addition on the masked store. A
// failed problem's samples are NaN.
__global__ __launch_bounds__(256) void mid_draw_product_kernel(MidArgs a, MidDrawArgs d) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  Tile sA = reinterpret_cast<Tile>(sm), sB = sA + TS;
  const int p = blockIdx.x;
  const MidProb P = a.probs[p];
  const MidDrawProb D = d.dp[p];
  const int sblk = (int)blockIdx.y / d.maxcb, c = (int)blockIdx.y - sblk * d.maxcb;
  if (c >= D.cb) return;
  const int tj = D.cb - 1 - c, m = P.n;
  const bool failed = a.status[p] != 0;
  double4v acc[4];
  acc_zero(acc);
  if (!failed) {
    const int64_t ldz = (int64_t)TS * D.cb, ld = P.Mp;
    const double* Z = d.base + D.Z + (int64_t)sblk * TS * ldz;
    const double* L = a.base + P.L + (int64_t)tj * TS * ld;
    for (int k = 0; k <= tj; ++k) {
      __syncthreads();
      stage(sA, Z + k * TS, ldz, false);
      stage(sB, L + k * TS, ld, false);
      __syncthreads();
      mma_nt(acc, sA, sB);
    }
  }
  const double* mean = d.mean + D.mean;
  double* X = d.base + D.X;
  acc_each(acc, [&](int r, int cc, double v) {
    const int64_t s = (int64_t)TS * sblk + r, j = (int64_t)TS * tj + cc;
    if (s < d.nsamp && j < m) X[s * m + j] = failed ? __builtin_nan("") : mean[j] + v;
  });
}

// ------------------------------------------------------------------ the fit's update
// JaxTrainer.step's tail (trainer.py:105-132) and after_epoch (trainer.py:133-160, 205-210) of
// every problem after step s's value-and-gradient launches: history[s] = the value; the
// first-bad-step word latched from the problem's status word (a failed step's value and gradient
// are NaN, and so are the parameters from there on); per trainable parameter (3 G + 2 of them,
// any number of passes of 256) small_fit_kernel's step (fit_update, lfm_bijectors.h) with the
// host's bias corrections, and the next step's constrained value into the first arena's packed
// hyperparameters, where mid_fill_kernel reads it. s < 0: the constrain alone, of all 3 G + 3
// slots (the jitter slot passes through: a static field). A thread touches its own parameter's
// slots alone; thread 0 the problem's history and first-bad words.
__global__ __launch_bounds__(256) void mid_adam_kernel(MidArgs a, MidFitArgs f) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const MidProb P = a.probs[p];
  const int G = P.G, nh = 3 * G + 3;
  double* raw = f.base + f.raw;
  double* hyp = a.base;  // MidPlan::hyp = 0
  auto slot = [&](int i) { return i < 3 * G ? P.hv + i : P.hs + (i - 3 * G); };
  if (f.s < 0) {
    for (int i = tid; i < nh; i += 256) hyp[slot(i)] = fit_constrain(i, G, raw[slot(i)]);
    if (tid == 0) f.first_bad[p] = 0;
    return;
  }
  const int64_t s = f.s;
  if (tid == 0) {
    f.base[f.hist + s * f.nprob + p] = a.base[a.out + p];
    if (a.status[p] != 0 && f.first_bad[p] == 0) f.first_bad[p] = (int)s + 1;
  }
  double* mom1 = f.base + f.mu;
  double* mom2 = f.base + f.nu;
  const double* grad = a.base + a.grad;
  const double c1 = f.base[f.bias + 2 * s], c2 = f.base[f.bias + 2 * s + 1];
  for (int i = tid; i < nh - 1; i += 256) {
    const int64_t gi = slot(i);
    const FitSlot u = fit_update(f.opt, i, G, s, raw[gi], grad[gi], mom1[gi], mom2[gi], c1, c2);
    mom1[gi] = u.mu;
    mom2[gi] = u.nu;
    raw[gi] = u.x;
    hyp[gi] = fit_constrain(i, G, u.x);
  }
}

// ------------------------------------------------------------------ the launcher
// One row per MidKind: the profile class, the dynamic LDS (the size of the launch and of the
// kernel's raised limit), the name in an error message, the blocks of MidCall the kernel takes
// besides `a`, the kernel (for its attribute) and its launch.
struct MidRow {
  int cls;
  size_t lds;
  const char* name;
  unsigned needs;
  const void* kernel;
  void (*issue)(const MidCall& c, dim3 grid, size_t lds, hipStream_t st);
};

constexpr unsigned mid_need(MidNoPost MidCall::*) { return 0; }
constexpr unsigned mid_need(MidPostArgs MidCall::*) { return MID_HAS_POST; }
constexpr unsigned mid_need(MidFitArgs MidCall::*) { return MID_HAS_FIT; }
constexpr unsigned mid_need(MidDrawArgs MidCall::*) { return MID_HAS_DRAW; }

template <auto Kernel, auto... Block>
void mid_issue(const MidCall& c, dim3 grid, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, st, c.a, c.*Block...);
}
// The row of a kernel launched as Kernel(c.a, c.*Block...): what it needs follows from Block.
template <auto Kernel, auto... Block>
MidRow mid_row(int cls, size_t lds, const char* name) {
  return {cls, lds, name, (0u | ... | mid_need(Block)), reinterpret_cast<const void*>(Kernel),
          &mid_issue<Kernel, Block...>};
}

const MidRow mid_rows[] = {
    mid_row<&mid_fill_kernel<false>, &MidCall::none>(K_MID_FILL, 0, "mid_fill_kernel"),
    mid_row<&mid_column_kernel>(K_MID_COLUMN, MID_LDS, "mid_column_kernel"),
    mid_row<&mid_value_kernel>(K_MID_FINISH, 0, "mid_value_kernel"),
    mid_row<&mid_invert_kernel>(K_MID_INVERSE, MID_LDS, "mid_invert_kernel"),
    mid_row<&mid_sinv_kernel>(K_MID_INVERSE, MID_LDS, "mid_sinv_kernel"),
    mid_row<&mid_pairs_kernel>(K_MID_PAIRS, 0, "mid_pairs_kernel"),
    mid_row<&mid_grad_kernel>(K_MID_FINISH, 0, "mid_grad_kernel"),
    mid_row<&mid_fill_kernel<true>, &MidCall::q>(K_MID_FILL, 0, "mid_fill_kernel (posterior)"),
    mid_row<&mid_solve_kernel, &MidCall::q>(K_MID_INVERSE, MID_LDS, "mid_solve_kernel"),
    mid_row<&mid_cov_kernel, &MidCall::q>(K_MID_FINISH, MID_LDS, "mid_cov_kernel"),
    mid_row<&mid_adam_kernel, &MidCall::f>(K_MID_FINISH, 0, "mid_adam_kernel"),  // MID_CONSTRAIN
    mid_row<&mid_adam_kernel, &MidCall::f>(K_MID_FINISH, 0, "mid_adam_kernel"),  // MID_ADAM
    mid_row<&mid_draw_scale_kernel, &MidCall::d>(K_MID_FILL, 0, "mid_draw_scale_kernel"),
    mid_row<&mid_draw_randn_kernel, &MidCall::d>(K_SAMPLE_RANDN, 0, "mid_draw_randn_kernel"),
    mid_row<&mid_draw_product_kernel, &MidCall::d>(K_SAMPLE_TRMM, MID_DRAW_LDS,
                                                   "mid_draw_product_kernel"),
};
static_assert(sizeof(mid_rows) / sizeof(mid_rows[0]) == MID_KINDS, "a row per MidKind, in order");

}  // namespace

int launch_mid(lfm_ctx* ctx, const MidLaunch& l, MidCall& c) {
  static const bool attrs = [] {
    for (const MidRow& r : mid_rows)
      if (r.lds > 0)
        hipFuncSetAttribute(r.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds);
    return true;
  }();
  (void)attrs;
  if (l.kind < 0 || l.kind >= MID_KINDS)
    return set_err(ctx, LFM_E_STATE, "plan_mid: unknown launch kind " + std::to_string(l.kind));
  const MidRow& r = mid_rows[l.kind];
  if ((r.needs & c.has) != r.needs)
    return set_err(ctx, LFM_E_STATE, std::string("launch_mid: ") + r.name + " (kind " +
                                         std::to_string(l.kind) +
                                         ") takes arguments this call has not filled");
  c.a.k = l.k;
  if (r.needs & MID_HAS_FIT) c.f.s = l.kind == MID_ADAM ? l.k : -1;
  hipEvent_t ev;
  prof_begin(ctx, r.cls, &ev);
  r.issue(c, dim3(l.gx, l.gy), r.lds, ctx->stream);
  prof_end(ctx, r.cls, ev, l.kind == MID_DRAW_PRODUCT ? c.d.flops : 0, 0);
  return hip_fail(ctx, hipGetLastError(), r.name);
}

}  // namespace lfm

