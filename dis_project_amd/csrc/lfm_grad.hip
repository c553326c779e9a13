// lfm_grad.hip — gradient of the log marginal likelihood on gfx950.
//
// What jax.value_and_grad(loss) computes at src/trainer.py:126 for
// CustomConjMLL.step (src/objectives.py:21-78), before the bijectors' chain rule:
//     d log N(y; m, S) / d theta = 1/2 tr(W dS/dtheta) + a^T dm/dtheta,
//     a = S^{-1} r,  W = a a^T - S^{-1},  r = y - m,
// for theta in true_d, true_s, true_b [G], l and obs_stddev (jitter is static, model.py:64).
//
// S^{-1} comes from the bordered factorisation (lfm_chol_sched.hip, chol_factor_solve with
// bordered = 1): the 2Mp x 2Mp matrix [[S_aug, .], [I, 0]] is eliminated through its first
// Mp columns, which leaves -(L_aug^{-T} L_aug^{-1}) in the bottom block. With the residual
// row n of the augmented factor (z = L^{-1} r, unit pivot) that block is
//     Bt[i][j] = -(S^{-1} + a a^T)[i][j]   (i, j < n),     Bt[n][j] = a_j,
// so W = Bt + 2 a a^T and a needs no extra solve.
//
// grad_pairs_kernel: one thread per column c of a 256-column x GR-row tile of the lower
//   triangle; per pair the kernel value and its derivatives in (D_row, D_col, l) are
//   evaluated with forward-mode duals on the cancellation-free erfc form of h
//   (model.py:315-365, the identities of lfm_gram.hip), weighted by W (x 1/2 on the
//   diagonal), and summed into per-gene accumulators (row gene: wave-uniform, flushed on
//   change; column gene: flushed at the end). Bound: VALU (erfc / exp), ~20 special
//   functions per pair; W is read once (8 B per pair).
// grad_finish_kernel: tr(W), the mean terms of m_i = (B/D)[i // (n/G)] flag_i
//   (model.py:124-149), the sign of CustomConjMLL(negative) and NaN on a failed factor.
//
// The three reductions take W and the mean terms' vector from a policy: MllWeight forms
// W = Bt + 2 a a^T inline and uses a; LooWeight reads the finished W_loo of lfm_loo.hip and uses
// u = S^{-1} b (the leave-one-out objective's gradient has the same shape).
#include "lfm_dual.h"

namespace lfm {

// ---------------------------------------------------------------- weights
// col(c): what at() needs of column c, read once per thread; at(i, c, col(c)): W[i][c], c <= i;
// diag(i): W[i][i]; mean(i): the vector v of the mean terms v^T dm.
struct MllWeight {
  const double* __restrict__ Bt;
  int64_t ldb;
  const double* __restrict__ al;
  __device__ __forceinline__ double col(int64_t c) const { return al[c]; }
  __device__ __forceinline__ double at(int64_t i, int64_t c, double ac) const {
    return Bt[i * ldb + c] + 2.0 * al[i] * ac;
  }
  __device__ __forceinline__ double diag(int64_t i) const {
    return Bt[i * ldb + i] + 2.0 * al[i] * al[i];
  }
  __device__ __forceinline__ double mean(int64_t i) const { return al[i]; }
};
struct LooWeight {
  const double* __restrict__ W;
  int64_t ldw;
  const double* __restrict__ u;
  __device__ __forceinline__ double col(int64_t) const { return 0.0; }
  __device__ __forceinline__ double at(int64_t i, int64_t c, double) const {
    return W[i * ldw + c];
  }
  __device__ __forceinline__ double diag(int64_t i) const { return W[i * ldw + i]; }
  __device__ __forceinline__ double mean(int64_t i) const { return u[i]; }
};

// ---------------------------------------------------------------- kernels
// Bottom rows of the bordered matrix: row Mp + i = e_i in the first Mp columns, 0 after.
__global__ void border_init_kernel(double* __restrict__ A, int64_t lda, int64_t Mp) {
  const int64_t i = blockIdx.y;
  double* row = A + (Mp + i) * lda;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= Mp + i;
       c += (int64_t)gridDim.x * blockDim.x)
    row[c] = (c == i) ? 1.0 : 0.0;
}

// acc layout: [0,G) dD  [G,2G) dS  [2G] dl   (kernel terms of 1/2 tr(W dK))
constexpr int GR = 32;
template <class WP>
__global__ __launch_bounds__(256) void grad_pairs_kernel(HypDev p, const double* __restrict__ x,
                                                         int64_t n, WP wp,
                                                         double* __restrict__ acc) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * GR;
  if ((int64_t)blockIdx.x * 256 > r0 + GR - 1) return;  // tile entirely above the diagonal
  const int lane = threadIdx.x & 63;
  const int G = p.G;
  const bool cv = c < n;
  const int64_t cc = cv ? c : n - 1;
  const double tb = x[cc * 3], gb = x[cc * 3 + 1], fb = x[cc * 3 + 2];
  const int k = gene_index(gb, G);
  const double ac = wp.col(cc);
  double cD = 0.0, cS = 0.0, rD = 0.0, rS = 0.0, sl = 0.0;
  int jcur = -1;
  const int64_t rend = min(r0 + GR, n);
  for (int64_t i = r0; i < rend; ++i) {
    const double ta = x[i * 3], ga = x[i * 3 + 1], fa = x[i * 3 + 2];
    const int j = gene_index(ga, G);  // wave-uniform
    if (j != jcur) {
      if (jcur >= 0) {
        const double sD = wave_sum(rD), sS = wave_sum(rS);
        if (lane == 0) {
          unsafeAtomicAdd(acc + jcur, sD);
          unsafeAtomicAdd(acc + G + jcur, sS);
        }
      }
      rD = rS = 0.0;
      jcur = j;
    }
    if (!cv || c > i) continue;
    double wgt = wp.at(i, c, ac);
    if (c == i) wgt *= 0.5;
    PairGrad o{0.0, 0.0, 0.0, 0.0, 0.0};
    kernel_grad(p, ta, ga, fa, tb, gb, fb, wgt, o);
    rD += o.dDr;
    rS += o.dSr;
    cD += o.dDc;
    cS += o.dSc;
    sl += o.dl;
  }
  if (jcur >= 0) {
    const double sD = wave_sum(rD), sS = wave_sum(rS);
    if (lane == 0) {
      unsafeAtomicAdd(acc + jcur, sD);
      unsafeAtomicAdd(acc + G + jcur, sS);
    }
  }
  const double s_l = wave_sum(sl);
  if (lane == 0) unsafeAtomicAdd(acc + 2 * G, s_l);
  // column genes: one atomic per wave when the wave's columns share a gene
  const int k0 = __shfl(k, 0);
  if (__all(k == k0)) {
    const double sD = wave_sum(cD), sS = wave_sum(cS);
    if (lane == 0) {
      unsafeAtomicAdd(acc + k0, sD);
      unsafeAtomicAdd(acc + G + k0, sS);
    }
  } else if (cv) {
    unsafeAtomicAdd(acc + k, cD);
    unsafeAtomicAdd(acc + G + k, cS);
  }
}

// One workgroup: tr(W), mean terms, sign, NaN on a failed factor.
// out: [0,G) d  [G,2G) s  [2G,3G) b  [3G] l  [3G+1] obs_stddev.
template <class WP>
__global__ __launch_bounds__(1024) void grad_finish_kernel(
    HypDev p, const double* __restrict__ x, int64_t n, WP wp, const double* __restrict__ acc,
    double obs_stddev, const double* __restrict__ result, int negative,
    double* __restrict__ out) {
  __shared__ double red[16];
  const int tid = threadIdx.x, G = p.G;
  const bool failed = (int)result[3] != INT_MAX;
  const double sign = negative ? -1.0 : 1.0;
  double tr = 0.0;
  for (int64_t i = tid; i < n; i += 1024) tr += wp.diag(i);
  tr = wave_sum(tr);
  if ((tid & 63) == 0) red[tid >> 6] = tr;
  const int64_t bs = n / G;
  for (int g = tid; g < G; g += 1024) {
    double af = 0.0;  // sum over mean block g of a_i flag_i (model.py:145-149)
    for (int64_t i = (int64_t)g * bs; i < (int64_t)(g + 1) * bs; ++i)
      af += wp.mean(i) * (double)flag_int(x[i * 3 + 2]);
    const double D = p.D[g], B = p.B[g];
    const double gd = acc[g] - B / (D * D) * af;
    const double nan = __builtin_nan("");
    out[g] = failed ? nan : sign * gd;
    out[G + g] = failed ? nan : sign * acc[G + g];
    out[2 * G + g] = failed ? nan : sign * (af / D);
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w];
    const double nan = __builtin_nan("");
    out[3 * G] = failed ? nan : sign * acc[2 * G];
    out[3 * G + 1] = failed ? nan : sign * obs_stddev * t;
  }
}

// ------------------------------------------------------- grid (table) path
// (tables: grad_table_entry, lfm_dual.h)
__global__ void grad_tables_kernel(HypDev p, int T, double dt, const double* __restrict__ times,
                                   double* __restrict__ tab) {
  const int64_t total = (int64_t)grad_tables_doubles(p.G, T);
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x)
    tab[idx] = grad_table_entry(p, T, dt, times, idx);
}

// One workgroup per 64-row x 256-column lower tile (T % 256 == 0: the tile lies in one
// (gene j, gene k) block), the tile's Toeplitz windows and row tables staged in LDS, one
// thread per column. Per element the kernel value and its three derivatives (D_j, D_k, l)
// cost 12 conflict-free LDS reads, ~35 FMAs and one coalesced read of W; the gene-pair
// constant Cm = S_j S_k l sqrt(pi)/2 / (D_j + D_k) is applied once per tile to the
// W-weighted sums, which go out as five atomics per workgroup.
// acc layout as grad_pairs_kernel: [0,G) dD  [G,2G) dS  [2G] dl.
template <class WP>
__global__ __launch_bounds__(256) void grad_grid_kernel(HypDev p, const double* __restrict__ tab,
                                                        int Tn, const int* __restrict__ bg,
                                                        int64_t n, WP wp,
                                                        double* __restrict__ acc) {
  constexpr int R = 64, C = 256, WIN = C + R - 1;
  __shared__ double sT[12][WIN];   // k-side tables at d, j-side tables at -d
  __shared__ double sR[8][R];      // row (tau) tables
  __shared__ double red[4][4];
  // 1-D grid over the lower tiles (as gram_grid_aligned_kernel)
  const int64_t b = blockIdx.x;
  int64_t q = (int64_t)((sqrt(2.0 * (double)b + 1.0) - 1.0) * 0.5);
  while (2 * (q + 1) * (q + 2) <= b) ++q;
  while (2 * q * (q + 1) > b) --q;
  const int64_t off = b - 2 * q * (q + 1);
  const int64_t r0 = (4 * q + off / (q + 1)) * R, c0 = (off % (q + 1)) * C;
  const int tid = threadIdx.x, G = p.G;
  const int64_t W = 2 * (int64_t)Tn - 1, nW = (int64_t)G * W, nT = (int64_t)G * Tn;
  const double* Tt = tab;           // Toeplitz tables, table w at Tt + w nW
  const double* Pt = tab + 6 * nW;  // time tables, table w at Pt + w nT
  const int j = bg[r0 / Tn], k = bg[c0 / Tn];
  const int tau0 = (int)(r0 % Tn), tp0 = (int)(c0 % Tn);
  const int dmin = tp0 - tau0 - (R - 1);
  for (int e = tid; e < WIN; e += 256) {
    const int64_t d = dmin + e;
#pragma unroll
    for (int w = 0; w < 6; ++w) {
      sT[w][e] = Tt[w * nW + (int64_t)k * W + (Tn - 1) + d];
      sT[6 + w][e] = Tt[w * nW + (int64_t)j * W + (Tn - 1) - d];
    }
  }
  if (tid < R) {
    const int64_t kr = (int64_t)k * Tn + tau0 + tid, jr = (int64_t)j * Tn + tau0 + tid;
    sR[0][tid] = Pt[0 * nT + kr];  // Pk(tau), dPk/dD, dPk/dl
    sR[1][tid] = Pt[1 * nT + kr];
    sR[2][tid] = Pt[2 * nT + kr];
    sR[3][tid] = Pt[3 * nT + jr];  // Ej(tau), dEj/dD
    sR[4][tid] = Pt[4 * nT + jr];
    sR[5][tid] = Pt[5 * nT + jr];  // Qj(tau), dQj/dD, dQj/dl
    sR[6][tid] = Pt[6 * nT + jr];
    sR[7][tid] = Pt[7 * nT + jr];
  }
  const int tp = tp0 + tid;
  const int64_t kc = (int64_t)k * Tn + tp, jc = (int64_t)j * Tn + tp;
  const double Pj = Pt[0 * nT + jc], PjD = Pt[1 * nT + jc], Pjl = Pt[2 * nT + jc];
  const double Ek = Pt[3 * nT + kc], EkD = Pt[4 * nT + kc];
  const double Qk = Pt[5 * nT + kc], QkD = Pt[6 * nT + kc], Qkl = Pt[7 * nT + kc];
  const int64_t c = c0 + tid;
  const double ac = wp.col(c);
  __syncthreads();
  double sV = 0.0, sVj = 0.0, sVk = 0.0, sVl = 0.0;
#pragma unroll 4
  for (int i = 0; i < R; ++i) {
    const int64_t row = r0 + i;
    if (c > row || row >= n) continue;
    const int e = tid + (R - 1) - i;
    const double Wk = sT[0][e], Xk = sT[1][e], WkD = sT[2][e], XkD = sT[3][e];
    const double Wkl = sT[4][e], Xkl = sT[5][e];
    const double Wj = sT[6][e], Xj = sT[7][e], WjD = sT[8][e], XjD = sT[9][e];
    const double Wjl = sT[10][e], Xjl = sT[11][e];
    const double Pk = sR[0][i], PkD = sR[1][i], Pkl = sR[2][i];
    const double Ej = sR[3][i], EjD = sR[4][i], Qj = sR[5][i], QjD = sR[6][i], Qjl = sR[7][i];
    const double EE = Ek * Ej, QQ = Qk + Qj;
    const double V = Wk + Wj - Xk * Pk - Xj * Pj - EE * QQ;
    const double Vk = WkD - XkD * Pk - Xk * PkD - EkD * Ej * QQ - EE * QkD;
    const double Vj = WjD - XjD * Pj - Xj * PjD - Ek * EjD * QQ - EE * QjD;
    const double Vl = Wkl - Xkl * Pk - Xk * Pkl + Wjl - Xjl * Pj - Xj * Pjl - EE * (Qkl + Qjl);
    double w = wp.at(row, c, ac);
    if (row == c) w *= 0.5;
    sV += w * V;
    sVj += w * Vj;
    sVk += w * Vk;
    sVl += w * Vl;
  }
  sV = wave_sum(sV);
  sVj = wave_sum(sVj);
  sVk = wave_sum(sVk);
  sVl = wave_sum(sVl);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = sV;
    red[tid >> 6][1] = sVj;
    red[tid >> 6][2] = sVk;
    red[tid >> 6][3] = sVl;
  }
  __syncthreads();
  if (tid == 0) {
    const double V = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const double Vj = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    const double Vk = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const double Vl = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    const double l = p.l, iDD = 1.0 / (p.D[j] + p.D[k]);
    const double Cm = p.S[j] * p.S[k] * l * kSqrtPi * 0.5 * iDD;
    unsafeAtomicAdd(acc + j, Cm * (Vj - V * iDD));
    unsafeAtomicAdd(acc + k, Cm * (Vk - V * iDD));
    unsafeAtomicAdd(acc + G + j, Cm * V / p.S[j]);
    unsafeAtomicAdd(acc + G + k, Cm * V / p.S[k]);
    unsafeAtomicAdd(acc + 2 * G, Cm * (V / l + Vl));
  }
}

int launch_border_init(lfm_ctx* ctx, double* A, int64_t lda, int64_t Mp) {
  hipEvent_t ev;
  prof_begin(ctx, K_AUGMENT, &ev);
  dim3 grid((unsigned)std::min<int64_t>((2 * Mp + 255) / 256, 64), (unsigned)Mp);
  hipLaunchKernelGGL(border_init_kernel, grid, dim3(256), 0, ctx->stream, A, lda, Mp);
  prof_end(ctx, K_AUGMENT, ev, 0, (double)Mp * Mp * 1.5 * 8);
  return hip_fail(ctx, hipGetLastError(), "border_init_kernel");
}

namespace {
// The reductions of 1/2 tr(W dS) + v^T dm over the weights wp
template <class WP>
int launch_grad_with(lfm_ctx* ctx, const HypDev& h, const double* d_x, int64_t n, const WP& wp,
                     double obs_stddev, int negative, double* acc, double* d_out,
                     const GridLayout* lay, const double* d_times, const int* d_bg) {
  hipMemsetAsync(acc, 0, (size_t)(2 * h.G + 1) * sizeof(double), ctx->stream);
  // the table path on the aligned grid layout (T % 256 == 0, the C2-C4 shape), else the
  // general per-pair dual-number path (LFM_GRAD_DIRECT=1 forces it: a test's cross-check)
  const bool grid = lay && lay->ok && lay->T % 256 == 0 && n % 256 == 0 && !ctx->knobs.grad_direct;
  hipEvent_t ev;
  prof_begin(ctx, K_GRAD, &ev);
  if (grid) {
    int r = ctx->gtab.reserve(ctx, grad_tables_doubles(h.G, lay->T) * sizeof(double));
    if (r) return r;
    const size_t nt = grad_tables_doubles(h.G, lay->T);
    hipLaunchKernelGGL(grad_tables_kernel, dim3((unsigned)std::min<size_t>((nt + 255) / 256, 4096)),
                       dim3(256), 0, ctx->stream, h, lay->T, lay->dt, d_times, ctx->gtab);
    const int64_t Q = n / 256;
    hipLaunchKernelGGL(grad_grid_kernel<WP>, dim3((unsigned)(2 * Q * (Q + 1))), dim3(256), 0,
                       ctx->stream, h, ctx->gtab, lay->T, d_bg, n, wp, acc);
  } else {
    dim3 grid2((unsigned)((n + 255) / 256), (unsigned)((n + GR - 1) / GR));
    hipLaunchKernelGGL(grad_pairs_kernel<WP>, grid2, dim3(256), 0, ctx->stream, h, d_x, n, wp,
                       acc);
  }
  prof_end(ctx, K_GRAD, ev, 0, (double)n * (n + 1) / 2 * 8);
  int r = hip_fail(ctx, hipGetLastError(), "grad kernel");
  if (r) return r;
  hipLaunchKernelGGL(grad_finish_kernel<WP>, dim3(1), dim3(1024), 0, ctx->stream, h, d_x, n, wp,
                     acc, obs_stddev, ctx->result, negative, d_out);
  return hip_fail(ctx, hipGetLastError(), "grad_finish_kernel");
}
}  // namespace

int launch_grad(lfm_ctx* ctx, const HypDev& h, const double* d_x, int64_t n, const double* A,
                int64_t lda, int64_t Mp, double obs_stddev, int negative, double* acc,
                double* d_out, const GridLayout* lay, const double* d_times, const int* d_bg) {
  const double* Bt = A + Mp * lda + Mp;
  return launch_grad_with(ctx, h, d_x, n, MllWeight{Bt, lda, Bt + n * lda}, obs_stddev, negative,
                          acc, d_out, lay, d_times, d_bg);
}

int launch_grad_loo(lfm_ctx* ctx, const HypDev& h, const double* d_x, int64_t n, const double* W,
                    int64_t ldw, const double* u, double obs_stddev, int negative, double* acc,
                    double* d_out, const GridLayout* lay, const double* d_times,
                    const int* d_bg) {
  return launch_grad_with(ctx, h, d_x, n, LooWeight{W, ldw, u}, obs_stddev, negative, acc, d_out,
                          lay, d_times, d_bg);
}

}  // namespace lfm
