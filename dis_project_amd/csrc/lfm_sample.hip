// lfm_sample.hip — joint samples from a Gaussian: the kernels and their launches (the entry
// points lfm_randn_f64 and lfm_mvn_sample_f64 are lfm_api.hip's; lfm_post_sample_f64, in
// lfm_post_api.hip, ends here too).
//
// Reference: gpjax 0.8.2 GaussianDistribution.sample(seed, sample_shape): loc + L z per sample,
// L L^T = scale, z standard normal. Here, with samples as rows:
//     X[s, i] = loc[i] + sum_{k <= i} L[i, k] Z[s, k].
//   sample_randn_kernel  Z from the counter-based generator the header defines (Philox4x32-10,
//                        Box-Muller): one thread per pair (s, p) writes z[2p], z[2p + 1] of
//                        sample sample0 + s as one 16-byte store. Element (s, j) depends on
//                        (seed, s, j) alone; Z's padding rows and columns are generated too, so
//                        every value the product reads is finite.
//   sample_tril_kernel   the strict upper triangle of the factor's diagonal 128-blocks, which
//                        the factorisation leaves holding the input's entries: zero.
//   sample_trmm_kernel   one workgroup per 128 x 128 tile of X: gemm_accumulate at depth
//                        128 (tj + 1) with the Z rows as panel i and the L rows as panel j,
//                        deepest column tiles first; loc joins in one addition on the masked store.
// Every size and grid is plan_sample's (lfm_host.cpp). The K order and the tile shape depend on
// neither nsamp nor sample0, rows have one owner and the launches follow each other on one
// stream: no atomics, no device-side waits, the same bits however a draw is split over calls.
#include "lfm_internal.h"
#include "lfm_chol_dev.h"

using namespace lfm;

namespace lfm {
namespace {

// rows x ld (ld even) normals: row r is sample s0 + r, columns [0, ld)
__global__ __launch_bounds__(256) void sample_randn_kernel(double* __restrict__ Z, int64_t ld,
                                                           int64_t pairs, uint64_t seed,
                                                           uint64_t s0) {
  const int64_t half = ld >> 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pairs;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / half, p = q - r * half;
    double2 v;
    sample_normals(seed, s0 + (uint64_t)r, (uint64_t)p, &v.x, &v.y);
    *reinterpret_cast<double2*>(&Z[r * ld + 2 * p]) = v;
  }
}

// one workgroup per diagonal 128-block of L
__global__ __launch_bounds__(256) void sample_tril_kernel(double* __restrict__ L, int64_t ldl) {
  double* D = L + (int64_t)blockIdx.x * NB * (ldl + 1);
  for (int idx = threadIdx.x; idx < NB * NB; idx += 256) {
    const int r = idx / NB, c = idx - r * NB;
    if (c > r) D[r * ldl + c] = 0.0;
  }
}

struct SampleArgs {
  const double* Z;
  int64_t ldz;
  const double* L;
  int64_t ldl;
  const double* loc;
  double* X;          // nsamp x n, dense
  int64_t n, nsamp;
  int ntj;            // column tiles: blockIdx.y = 0 is the deepest, ntj - 1
};

__global__ __launch_bounds__(256, 2) void sample_trmm_kernel(SampleArgs g) {
  __shared__ __attribute__((aligned(16))) double sPbuf[(ST + ST) * (KB + LDP)];
  double(*sP)[KB + LDP] = reinterpret_cast<double(*)[KB + LDP]>(sPbuf);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tj = g.ntj - 1 - (int)blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * ST, j0 = (int64_t)tj * ST;
  double acc[16][4];
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = 0.0;
  gemm_accumulate<ST>(g.Z + i0 * g.ldz, g.ldz, g.L + j0 * g.ldl, g.ldl, (tj + 1) * NB, acc, sP);
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      const int64_t s = i0 + wr + ir * 4 + (lane >> 4), i = j0 + wc + jr * 16 + (lane & 15);
      if (s < g.nsamp && i < g.n) g.X[s * g.n + i] = g.loc[i] + acc[ir][jr];
    }
}

}  // namespace

void launch_randn(lfm_ctx* ctx, double* Z, int64_t ld, int64_t rows, int64_t pairs, int grid,
                  uint64_t seed, int64_t sample0) {
  hipEvent_t ev;
  prof_begin(ctx, K_SAMPLE_RANDN, &ev);
  hipLaunchKernelGGL(sample_randn_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, Z, ld,
                     pairs, seed, (uint64_t)sample0);
  prof_end(ctx, K_SAMPLE_RANDN, ev, 0, (double)rows * ld * 8);
}

int scale_factor(lfm_ctx* ctx, double* A, int64_t n, int64_t Mp, const double* d_loc) {
  // the augmented row: y = loc, residual 0, so the MLL the factorisation also produces is
  // -1/2 logdet - (n / 2) log 2 pi (a draw does not use it; lfm_post_log_prob_f64 does)
  const HypDev h{nullptr, nullptr, nullptr, 1, 1.0};
  int r = launch_augment(ctx, h, nullptr, d_loc, d_loc, n, A, Mp, Mp);
  if (r) return r;
  return chol_factor_solve(ctx, A, Mp, n, Mp, 0, ctx->result, CHOL_RESIDENT);
}

int sample_enqueue(lfm_ctx* ctx, const SamplePlan& P, double* A, const double* d_loc,
                   uint64_t seed, double* Z, double* X) {
  int r = scale_factor(ctx, A, P.n, P.Mp, d_loc);
  return r ? r : sample_draw(ctx, P, A, d_loc, seed, Z, X);
}

int sample_draw(lfm_ctx* ctx, const SamplePlan& P, double* A, const double* d_loc, uint64_t seed,
                double* Z, double* X) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(sample_tril_kernel, dim3((unsigned)P.tiles_j), dim3(256), 0, st, A, P.Mp);
  launch_randn(ctx, Z, P.ldz, P.zrows, P.pairs, P.randn_grid, seed, P.sample0);
  SampleArgs g{Z, P.ldz, A, P.Mp, d_loc, X, P.n, P.nsamp, P.tiles_j};
  hipEvent_t ev;
  prof_begin(ctx, K_SAMPLE_TRMM, &ev);
  hipLaunchKernelGGL(sample_trmm_kernel, dim3((unsigned)P.tiles_i, (unsigned)P.tiles_j), dim3(256),
                     0, st, g);
  double issued = 0.0;
  for (int tj = 0; tj < P.tiles_j; ++tj) issued += 2.0 * P.zrows * ST * (double)sample_depth(tj);
  prof_end(ctx, K_SAMPLE_TRMM, ev, (double)P.nsamp * P.n * P.n,
           ((double)P.zrows * P.ldz + 0.5 * P.Np * P.Np + (double)P.nsamp * P.n) * 8, nullptr,
           issued);
  return hip_fail(ctx, hipGetLastError(), "joint samples: launches");
}

}  // namespace lfm
