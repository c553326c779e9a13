// lfm_loo.hip — the leave-one-out CV objective on gfx950 (gpjax 0.8.2 ConjugateLOOCV.step,
// Rasmussen & Williams 5.4.2).
//
// With S = K + (jitter + obs_stddev^2) I, r = y - m, a = S^{-1} r and k_i = [S^{-1}]_ii:
//     mu_i = y_i - a_i / k_i,   var_i = 1 / k_i,
//     value = sum_i (-1/2 log 2 pi + 1/2 log k_i - 1/2 a_i^2 / k_i),
//     d value / d theta = 1/2 tr(W_loo dS/dtheta) + u^T dm/dtheta,
//     W_loo = -2 M + u a^T + a u^T,   M = S^{-1} diag(c) S^{-1},
//     c_i = (1 + a_i^2 / k_i) / (2 k_i),   b_i = a_i / k_i,   u = S^{-1} b.
//
// The bordered factorisation (lfm_grad.hip's header) leaves Bt = -(S^{-1} + a a^T), lower-stored,
// and the row a in the bottom-right block of the 2Mp x 2Mp matrix, so k_i = -Bt_ii - a_i^2 and
// S^{-1}[i][j] = -Bt[i][j] - a_i a_j. Where everything lives: LooPlan (lfm_host.h).
//
// loo_terms_kernel    one workgroup: the diagonal of Bt and a -> mu, var, sqrt c, b, the value and
//                     a^T b, both summed in a fixed order (per thread, per wave, then the 16 wave
//                     sums in turn): the same inputs give the same bits.
// loo_u_kernel        u = S^{-1} b over the lower-stored block, one workgroup per strip of 64
//                     rows: the strip's own rows left of the diagonal (a wave per row), then the
//                     rows below it, read along their 64 contiguous columns of the strip (a lane
//                     per column). Every element of Bt is read once; no atomics.
// loo_scale_kernel    Bs = S^{-1} diag(sqrt c) as a dense Np x Np panel, mirrored from the lower
//                     triangle through a 64 x 64 LDS tile, zero where row or column is >= n: on a
//                     successful factor every value the product reads is finite.
// loo_product_kernel  one workgroup per lower 128 x 128 tile of M = Bs Bs^T at depth Np on the
//                     fp64 MFMA (gemm_accumulate, as post_cov_kernel); the epilogue writes
//                     W_loo[i][j] = -2 acc + u_i a_j + a_i u_j for j <= i < n.
// The reductions over W_loo are lfm_grad.hip's (launch_grad_loo).
// A failed factor (not PD, a device-side wait that ran out) is known only on the device: the
// launches after loo_terms_kernel still run, over a Bt that may hold NaN or Inf, and Bs and W_loo
// are then not finite either. Nothing faults on that and nothing reads them afterwards:
// loo_terms_kernel and grad_finish_kernel write NaN from the status word, the caller's outputs
// are NaN-filled on the host, and the next factorising call rewrites what it reads.
#include "lfm_chol_dev.h"
#include "lfm_dual.h"

namespace lfm {

namespace {

__global__ __launch_bounds__(1024) void loo_terms_kernel(
    const double* __restrict__ Bt, int64_t ldb, const double* __restrict__ al,
    const double* __restrict__ y, int64_t n, const double* __restrict__ result, int negative,
    double* __restrict__ mu, double* __restrict__ var, double* __restrict__ sc,
    double* __restrict__ b, double* __restrict__ val) {
  #pragma clang fp contract(off)
  __shared__ double red[2][16];
  const int tid = threadIdx.x;
  const double half_log_2pi = 0.91893853320467274178;
  double sv = 0.0, sab = 0.0;
  for (int64_t i = tid; i < n; i += 1024) {
    const double a = al[i];
    const double k = -Bt[i * ldb + i] - a * a;  // <= 0 from rounding: NaN from here on, as gpjax
    const double bi = a / k;
    const double z2 = a * bi;
    sv += (0.5 * log(k) - half_log_2pi) - 0.5 * z2;
    sab += a * bi;
    mu[i] = y[i] - bi;
    var[i] = 1.0 / k;
    sc[i] = sqrt((1.0 + z2) / (2.0 * k));
    b[i] = bi;
  }
  sv = wave_sum(sv);
  sab = wave_sum(sab);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sv;
    red[1][tid >> 6] = sab;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0, ab = 0.0;
    for (int w = 0; w < 16; ++w) {
      t += red[0][w];
      ab += red[1][w];
    }
    const bool failed = (int)result[3] != INT_MAX;
    val[0] = failed ? __builtin_nan("") : (negative ? -t : t);
    val[1] = ab;
  }
}

__global__ __launch_bounds__(256) void loo_u_kernel(const double* __restrict__ Bt, int64_t ldb,
                                                    const double* __restrict__ al,
                                                    const double* __restrict__ b,
                                                    const double* __restrict__ val, int64_t n,
                                                    double* __restrict__ u) {
  __shared__ double srow[64];
  __shared__ double scol[4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int64_t rend = min(r0 + 64, n);
  // rows of the strip, columns up to the diagonal: wave w takes rows r0 + w, r0 + w + 4, ...
  for (int64_t i = r0 + w; i < rend; i += 4) {
    const double* row = Bt + i * ldb;
    double s = 0.0;
    for (int64_t j = lane; j <= i; j += 64) s += row[j] * b[j];
    s = wave_sum(s);
    if (lane == 0) srow[i - r0] = s;
  }
  // rows below the diagonal element of column r0 + lane: Bt[j][col], j > col
  const int64_t col = r0 + lane;
  double s = 0.0;
  if (col < n) {
#pragma unroll 4
    for (int64_t j = r0 + 1 + w; j < n; j += 4)
      if (j > col) s += Bt[j * ldb + col] * b[j];
  }
  scol[w][lane] = s;
  __syncthreads();
  if (tid < 64 && col < n) {
    const double t = srow[tid] + (((scol[0][tid] + scol[1][tid]) + scol[2][tid]) + scol[3][tid]);
    u[col] = -t - al[col] * val[1];
  }
}

__global__ __launch_bounds__(256) void loo_scale_kernel(const double* __restrict__ Bt, int64_t ldb,
                                                        const double* __restrict__ al,
                                                        const double* __restrict__ sc, int64_t n,
                                                        double* __restrict__ Bs, int64_t lds) {
  __shared__ double s[64][65];
  const int ti = blockIdx.y, tj = blockIdx.x;  // tile of Bs
  const int hi = max(ti, tj), lo = min(ti, tj);
  const int64_t R0 = (int64_t)hi * 64, C0 = (int64_t)lo * 64;
  const int tid = threadIdx.x, lc = tid & 63, lr0 = tid >> 6;
  // the lower-stored tile (hi, lo) of Bt; what lies above the diagonal of a diagonal tile is
  // never selected below
  for (int r = lr0; r < 64; r += 4) {
    const int64_t i = R0 + r, j = C0 + lc;
    s[r][lc] = (i < n && j <= i) ? Bt[i * ldb + j] : 0.0;
  }
  __syncthreads();
  const int64_t j = (int64_t)tj * 64 + lc;
  const bool cv = j < n;
  const double aj = cv ? al[j] : 0.0, scj = cv ? sc[j] : 0.0;
  for (int r = lr0; r < 64; r += 4) {
    const int64_t i = (int64_t)ti * 64 + r;
    double v = 0.0;
    if (cv && i < n) {
      const double bt = i >= j ? s[i - R0][j - C0] : s[j - R0][i - C0];
      v = (-bt - al[i] * aj) * scj;
    }
    Bs[i * lds + j] = v;
  }
}

__global__ __launch_bounds__(256, 2) void loo_product_kernel(const double* __restrict__ Bs,
                                                             int64_t lds, int Np,
                                                             const double* __restrict__ al,
                                                             const double* __restrict__ u,
                                                             int64_t n, double* __restrict__ W,
                                                             int64_t ldw) {
  __shared__ __attribute__((aligned(16))) double sPbuf[(ST + ST) * (KB + LDP)];
  double(*sP)[KB + LDP] = reinterpret_cast<double(*)[KB + LDP]>(sPbuf);
  int64_t ti, tj;
  loo_tile(blockIdx.x, &ti, &tj);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = ti * ST, j0 = tj * ST;
  double acc[16][4];
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = 0.0;
  gemm_accumulate<ST>(Bs + i0 * lds, lds, Bs + j0 * lds, lds, Np, acc, sP);
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  double aj[4], uj[4];
#pragma unroll
  for (int jr = 0; jr < 4; ++jr) {
    const int64_t j = j0 + wc + jr * 16 + (lane & 15);
    aj[jr] = j < n ? al[j] : 0.0;
    uj[jr] = j < n ? u[j] : 0.0;
  }
#pragma unroll
  for (int ir = 0; ir < 16; ++ir) {
    const int64_t i = i0 + wr + ir * 4 + (lane >> 4);
    if (i >= n) continue;
    const double ai = al[i], ui = u[i];
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      const int64_t j = j0 + wc + jr * 16 + (lane & 15);
      if (j <= i) W[i * ldw + j] = -2.0 * acc[ir][jr] + ui * aj[jr] + ai * uj[jr];
    }
  }
}

}  // namespace

int launch_loo_terms(lfm_ctx* ctx, const LooPlan& P, const double* A, const double* d_y,
                     int negative, double* vec) {
  hipEvent_t ev;
  prof_begin(ctx, K_GRAD, &ev);
  hipLaunchKernelGGL(loo_terms_kernel, dim3(1), dim3(1024), 0, ctx->stream, A + P.bt, P.ld,
                     A + P.a, d_y, P.n, ctx->result, negative, vec + P.mu, vec + P.var,
                     vec + P.sc, vec + P.b, vec + P.val);
  prof_end(ctx, K_GRAD, ev, 0, (double)P.n * 7 * 8);
  return hip_fail(ctx, hipGetLastError(), "loo_terms_kernel");
}

int launch_loo_weights(lfm_ctx* ctx, const LooPlan& P, double* A, double* vec) {
  const double* Bt = A + P.bt;
  const double* al = A + P.a;
  const double n = (double)P.n;
  hipEvent_t ev;
  // one event pair for both small kernels: the profile does not separate them
  prof_begin(ctx, K_GRAD, &ev);
  hipLaunchKernelGGL(loo_u_kernel, dim3((unsigned)P.u_grid), dim3(256), 0, ctx->stream, Bt, P.ld,
                     al, vec + P.b, vec + P.val, P.n, vec + P.u);
  hipLaunchKernelGGL(loo_scale_kernel, dim3((unsigned)P.scale_tiles, (unsigned)P.scale_tiles),
                     dim3(256), 0, ctx->stream, Bt, P.ld, al, vec + P.sc, P.n, A + P.bs, P.ld);
  prof_end(ctx, K_GRAD, ev, 0, (n * (n + 1) + (double)P.Np * P.Np) * 8);
  int r = hip_fail(ctx, hipGetLastError(), "loo_u_kernel / loo_scale_kernel");
  if (r) return r;
  prof_begin(ctx, K_LOO_PRODUCT, &ev);
  hipLaunchKernelGGL(loo_product_kernel, dim3((unsigned)P.product_grid), dim3(256), 0, ctx->stream,
                     A + P.bs, P.ld, (int)P.Np, al, vec + P.u, P.n, A + P.w, P.ld);
  // algorithmic: n^3 (the lower triangle of an n x n x n product); issued: whole tiles
  prof_end(ctx, K_LOO_PRODUCT, ev, n * n * n,
           (double)P.product_grid * (2.0 * ST * P.Np + ST * ST) * 8, nullptr,
           (double)P.product_grid * 2.0 * ST * ST * P.Np);
  return hip_fail(ctx, hipGetLastError(), "loo_product_kernel");
}

}  // namespace lfm
