// lfm_post.hip — the resident posterior (include/lfm.h lfm_post_*): factor a large model once,
// predict many times. The kernels and the functions that launch them, one per step of a call;
// the handle and the entry points are lfm_post_api.hip's.
//
// Reference: ExactLFM.latent_predict / multi_gene_predict, src/model.py:420-514:
//     mean = m(t) + K(t,x) S^{-1} (y - m(x)),   cov = K(t,t) - K(t,x) S^{-1} K(x,t),
//     S = K(x,x) + diag(v) + c I = L L^T.
// lfm_post_create builds S and the residual row in memory the handle owns and factors it on
// schedule 1 (chol_factor_solve, CHOL_RESIDENT), which leaves L in the lower triangle and
// z = L^{-1} (y - m(x)) in row n; z is copied out, row n is made an identity row again, and the
// 16 x 16 inverses of L's diagonal blocks are rebuilt from L (post_dinv_kernel). A predict then
// needs V = K(t,x) L^{-T} only:
//     mean = m(t) + V z,   var = k(t,t) - sum_c V_c^2,   cov = K(t,t) - V V^T.
// Test points are rows. Per chunk, Vt (rows x Np, row-major) is filled with K(t,x) and solved in
// place by a right-looking sweep over super-panels of up to POST_W block columns:
//   post_panel_kernel   64 test rows per workgroup: the super-panel's block columns one by one,
//                       each after the in-panel update from the ones before it (gemm_accumulate)
//                       by the 16-column substitution of trsm_rows against L and the handle's
//                       inverses; the rows' sum v^2 and sum v z join two per-row accumulators.
//   post_update_kernel  one workgroup per 128 x 128 tile of the columns to the right:
//                       C -= Vt[ti, K0:K1] L[tj, K0:K1]^T at depth 128 w on the fp64 MFMA.
// Every launch, grid and byte count is plan_post's (lfm_host.cpp); the K order and the tile
// shape depend on neither m nor the chunk, rows have one owner per launch and the launches
// follow each other on one stream: no atomics, no device-side waits, the same bits whatever
// the split.
// lfm_post_sample_f64 draws joint samples from such a predict without the covariance leaving the
// device: the predict with the covariance, cov copied into an Mp' = round_up(m + 1, 128)-stride
// matrix of the handle's, diag_add on its diagonal, then lfm_sample.hip's factor, generator and
// product (sample_draw). The handle's L, z and dinv are only read.
// lfm_post_log_prob_f64 scores k held-out vectors under the same distribution: the sample's first
// steps (post_scale_factor, written once for both), whose factorisation at residual 0 reduces to
// base = -1/2 logdet - (m / 2) log 2 pi; the factor made readable by the sweep above (row m an
// identity row, post_dinv_kernel on its diagonal blocks); then per pass of held-out rows
//   post_resid_kernel   R = ystar - mean in place in Vt's memory, zero padded, 16-byte accesses;
//   the same panel / update launches against the covariance's factor with z = 0, after which the
//                       accumulator s2 is ||L^{-1} (ystar_r - mean)||^2;
//   post_logp_kernel    logp[r] = base - 0.5 * s2[r].
// Every size, grid and pass is plan_post_logp's (lfm_host.cpp).
#include "lfm_internal.h"
#include "lfm_chol_dev.h"

using namespace lfm;

namespace lfm {
namespace {

// ------------------------------------------------------------------ fit
__global__ void post_diag_kernel(double* __restrict__ A, int64_t lda,
                                 const double* __restrict__ dv, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i * lda + i] += dv[i];  // S = (K + c I) + diag(v), as posterior_fill_kernel
}

// z = row n of the factored matrix, zero from column n; row n itself, where it lies inside the
// pivot block columns (n < Np), becomes the identity row its neighbours are
__global__ void post_z_kernel(double* __restrict__ L, int64_t ldl, int64_t n, int64_t Np,
                              double* __restrict__ z) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Np) return;
  z[c] = c < n ? L[n * ldl + c] : 0.0;
  if (n < Np && c <= n) L[n * ldl + c] = c == n ? 1.0 : 0.0;
}

// The eight 16 x 16 inverses of one diagonal block's diagonal sub-blocks, row-major as
// trsm_rows reads them: one workgroup per 128-block, thread (cb, j) column j of inv(L_cb) by
// forward substitution.
__global__ __launch_bounds__(128) void post_dinv_kernel(const double* __restrict__ L,
                                                        int64_t ldl,
                                                        double* __restrict__ dinv) {
  const int cb = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int64_t d0 = (int64_t)blockIdx.x * NB + cb * IB;
  const double* D = L + d0 * ldl + d0;
  double* out = dinv + ((int64_t)blockIdx.x * (NB / IB) + cb) * IB * IB;
  double xv[IB];
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    double s = i == j ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; ++k) s = fma(-D[i * ldl + k], xv[k], s);
    xv[i] = i < j ? 0.0 : s / D[i * ldl + i];
    out[i * IB + j] = xv[i];
  }
}

// --------------------------------------------------------------- predict
// Columns [n, Np) of the chunk's rows and the whole of its padding rows [rows, pad_rows): zero
__global__ void post_pad_kernel(double* __restrict__ Vt, int64_t ldv, int64_t n, int64_t rows) {
  const int64_t row = blockIdx.y;
  for (int64_t c = (row < rows ? n : 0) + threadIdx.x; c < ldv; c += blockDim.x)
    Vt[row * ldv + c] = 0.0;
}

// trsm_rows (lfm_chol.hip) with the solved rows and the factor in different matrices: the 64
// rows in sA are columns [kb, kb + 128) of V (row 0 = the workgroup's first row, stride ldv);
// L_kk is read from L (stride ldl) and its 16 x 16 inverses from dinv (this block's eight).
//   X_cb = (A_cb - sum_{q < cb} X_q L_{cb,q}^T) * Dinv_cb^T,  cb = 0..7 (16 columns each).
__device__ __forceinline__ void post_trsm_rows(double (*__restrict__ sA)[NB + 1],
                                               double* __restrict__ V, int64_t ldv, int64_t kb,
                                               const double* __restrict__ L, int64_t ldl,
                                               const double* __restrict__ dinv) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int wr = w * IB;
  const double* Lrow = L + (kb + li) * ldl + kb + lk;  // L[li][lk]
  constexpr int NCB = NB / IB;
  double bf[2][NB / 4];
  double dv[2][IB / 4];
#pragma unroll
  for (int ks = 0; ks < IB / 4; ++ks) dv[0][ks] = dinv[li * IB + ks * 4 + lk];
  __syncthreads();
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int cur = cb & 1, nxt = cur ^ 1;
    if (cb + 1 < NCB) {
#pragma unroll
      for (int st = 0; st < (cb + 1) * 4; ++st)
        bf[nxt][st] = Lrow[(int64_t)(cb + 1) * IB * ldl + st * 4];
#pragma unroll
      for (int ks = 0; ks < IB / 4; ++ks)
        dv[nxt][ks] = dinv[(cb + 1) * IB * IB + li * IB + ks * 4 + lk];
    }
    double4v acc0, acc1 = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc0[r] = sA[wr + lk + 4 * r][cb * IB + li];
#pragma unroll
    for (int st = 0; st < cb * 4; ++st) {
      if (st & 1) acc1 = mfma16(-sA[wr + li][st * 4 + lk], bf[cur][st], acc1);
      else acc0 = mfma16(-sA[wr + li][st * 4 + lk], bf[cur][st], acc0);
    }
    acc0 += acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[wr + lk + 4 * r][cb * IB + li] = acc0[r];
    wave_lds_fence();
    double4v zz = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < IB / 4; ++ks)
      zz = mfma16(sA[wr + li][cb * IB + ks * 4 + lk], dv[cur][ks], zz);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[wr + lk + 4 * r][cb * IB + li] = zz[r];
    wave_lds_fence();
  }
  // the wave's 16 rows back to HBM
  for (int idx = lane; idx < IB * (NB / 2); idx += 64) {
    const int r = idx / (NB / 2), q2 = idx - r * (NB / 2);
    double2 v;
    v.x = sA[wr + r][2 * q2];
    v.y = sA[wr + r][2 * q2 + 1];
    *reinterpret_cast<double2*>(&V[(wr + r) * ldv + kb + 2 * q2]) = v;
  }
}

// One LDS buffer, first the staging of the in-panel product, then the 64 x 128 rows being solved.
// The in-panel product stages PKS = 64 columns at a time: a panel launch has few workgroups (one
// per 64 test rows), so nothing else hides its global-load latency (as the factor chain's CKS).
constexpr int PKS = 64;
constexpr int POST_PANEL_LDS = (64 + ST) * (PKS + LDP);
static_assert(POST_PANEL_LDS >= 64 * (NB + 1), "panel LDS union");

__global__ __launch_bounds__(256) void post_panel_kernel(PostArgs g) {
  __shared__ __attribute__((aligned(16))) double smem[POST_PANEL_LDS];
  __shared__ double zs[NB];  // z of the block column being solved
  double(*sA)[NB + 1] = reinterpret_cast<double(*)[NB + 1]>(smem);
  double(*sP)[PKS + LDP] = reinterpret_cast<double(*)[PKS + LDP]>(smem);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  double* V = g.Vt + r0 * g.ldv;
  // Row ar = tid / 4 is summed by its four threads, thread aq the columns 16 aq + j + 64 h
  // (j < 16, h < 2: distinct LDS banks over a wave), and their partial sums join in the order
  // ((0 + 1) + 2) + 3; thread aq = 0 keeps the row's accumulators, block columns join in order
  const int ar = tid >> 2, aq = tid & 3;
  double run2 = 0.0, runz = 0.0;
  if (aq == 0 && g.K0 > 0) {
    run2 = g.s2[r0 + ar];
    runz = g.sz[r0 + ar];
  }
  for (int b = 0; b < g.w; ++b) {
    const int64_t kb = g.K0 + (int64_t)b * NB;
    if (b == 0) {
      for (int idx = tid; idx < 64 * (NB / 2); idx += 256) {
        const int r = idx / (NB / 2), q2 = idx - r * (NB / 2);
        const double2 v = *reinterpret_cast<const double2*>(&V[r * g.ldv + kb + 2 * q2]);
        sA[r][2 * q2] = v.x;
        sA[r][2 * q2 + 1] = v.y;
      }
    } else {
      // in-panel update: the rows' solved columns [K0, kb) against L[kb .., K0 .. kb)
      double acc[8][4];
#pragma unroll
      for (int ir = 0; ir < 8; ++ir)
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = 0.0;
      gemm_accumulate<64, false, false, PKS>(V + g.K0, g.ldv, g.L + kb * g.ldl + g.K0, g.ldl,
                                             b * NB, acc, sP);
      __syncthreads();  // the staging is read out: the buffer becomes the rows
      const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
#pragma unroll
      for (int ir = 0; ir < 8; ++ir)
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) {
          const int r = wr + ir * 4 + (lane >> 4), c = wc + jr * 16 + (lane & 15);
          sA[r][c] = V[r * g.ldv + kb + c] - acc[ir][jr];
        }
    }
    if (tid < NB) zs[tid] = g.z[kb + tid];
    post_trsm_rows(sA, V, g.ldv, kb, g.L, g.ldl, g.dinv + (kb / NB) * (NB / IB) * IB * IB);
    __syncthreads();  // every wave's rows are final, in sA and in memory
    double p2 = 0.0, pz = 0.0;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int c = 16 * aq + j + 64 * hh;
        const double v = sA[ar][c];
        p2 = fma(v, v, p2);
        pz = fma(v, zs[c], pz);
      }
    const int l0 = lane & ~3;
    const double s2 = ((__shfl(p2, l0) + __shfl(p2, l0 + 1)) + __shfl(p2, l0 + 2)) +
                      __shfl(p2, l0 + 3);
    const double sz = ((__shfl(pz, l0) + __shfl(pz, l0 + 1)) + __shfl(pz, l0 + 2)) +
                      __shfl(pz, l0 + 3);
    run2 += s2;
    runz += sz;
    __syncthreads();  // the rows are read out: the buffer becomes the staging again
  }
  if (aq == 0) {
    g.s2[r0 + ar] = run2;
    g.sz[r0 + ar] = runz;
  }
}

// Tile (ti, tj0 + blockIdx.y) of Vt: C -= Vt[ti, K0:K1] L[tj, K0:K1]^T, depth 128 w. The bulk
// update's staging (KB-deep stages, stride KB + LDP). Whole tiles only: Vt has pad_rows rows.
__global__ __launch_bounds__(256, 2) void post_update_kernel(PostArgs g) {
  __shared__ __attribute__((aligned(16))) double sPbuf[(ST + ST) * (KB + LDP)];
  double(*sP)[KB + LDP] = reinterpret_cast<double(*)[KB + LDP]>(sPbuf);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * ST, j0 = (int64_t)(g.tj0 + blockIdx.y) * ST;
  double acc[16][4];
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = 0.0;
  gemm_accumulate<ST>(g.Vt + i0 * g.ldv + g.K0, g.ldv, g.L + j0 * g.ldl + g.K0, g.ldl, g.w * NB,
                      acc, sP);
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  double* C = g.Vt + i0 * g.ldv + j0;
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      double* c = C + (wr + ir * 4 + (lane >> 4)) * g.ldv + wc + jr * 16 + (lane & 15);
      *c -= acc[ir][jr];
    }
}

// mean and variance of the chunk's rows [q0, q0 + rows) from the accumulators; the mean's block
// position from the global index and the global m
__global__ void post_finish_kernel(HypDev p, const double* __restrict__ t, int64_t q0,
                                   int64_t rows, int64_t m, const double* __restrict__ s2,
                                   const double* __restrict__ sz, double* __restrict__ mean,
                                   double* __restrict__ var) {
  #pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= rows) return;
  const int64_t gq = q0 + q;
  const double* tq = t + gq * 3;
  mean[gq] = mean_at(p, t, gq, m / p.G) + sz[q];
  var[gq] = kernel_ref(p, tq[0], tq[1], tq[2], tq[0], tq[1], tq[2]) - s2[q];
}

// Lower 128-tile (ti >= tj) of the m x m covariance: C -= Vt[ti] Vt[tj]^T at depth Np, mirrored
// on the way out (ragged last tiles masked on load and store)
__global__ __launch_bounds__(256, 2) void post_cov_kernel(const double* __restrict__ Vt,
                                                          int64_t ldv, double* __restrict__ C,
                                                          int64_t m) {
  __shared__ __attribute__((aligned(16))) double sPbuf[(ST + ST) * (KB + LDP)];
  if (blockIdx.y > blockIdx.x) return;
  double(*sP)[KB + LDP] = reinterpret_cast<double(*)[KB + LDP]>(sPbuf);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * ST, j0 = (int64_t)blockIdx.y * ST;
  double acc[16][4];
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = 0.0;
  gemm_accumulate<ST>(Vt + i0 * ldv, ldv, Vt + j0 * ldv, ldv, (int)ldv, acc, sP);
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
#pragma unroll
  for (int ir = 0; ir < 16; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      const int64_t i = i0 + wr + ir * 4 + (lane >> 4), j = j0 + wc + jr * 16 + (lane & 15);
      if (i < m && j <= i) {
        const double v = C[i * m + j] - acc[ir][jr];
        C[i * m + j] = v;
        C[j * m + i] = v;
      }
    }
}

// A[i][i] += d: the caller's diag_add on the sampled covariance, in one addition
__global__ void post_shift_kernel(double* __restrict__ A, int64_t lda, double d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i * lda + i] += d;
}

// ------------------------------------------------------- held-out log density
// The residual rows in place: R (pad_rows x ldr, ldr = round_up(m, 128)) holds ystar's rows
// [0, rows) in its columns [0, m); R[r, j] -= mean[j] there, zero in columns [m, ldr) and in the
// padding rows. One thread per pair of columns: every row starts 16-byte aligned, so each access
// of R is one 16-byte load or store; mean (the handle's out) is 16-byte aligned too.
__global__ __launch_bounds__(256) void post_resid_kernel(double* __restrict__ R, int64_t ldr,
                                                         const double* __restrict__ mean, int64_t m,
                                                         int64_t rows) {
  const int64_t row = blockIdx.y;
  const int64_t j = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (j >= ldr) return;
  double2* p = reinterpret_cast<double2*>(R + row * ldr + j);
  double2 v = {0.0, 0.0};
  if (row < rows && j < m) {
    v = *p;
    if (j + 1 < m) {
      const double2 mu = *reinterpret_cast<const double2*>(mean + j);
      v.x -= mu.x;
      v.y -= mu.y;
    } else {
      v.x -= mean[j];
      v.y = 0.0;
    }
  }
  *p = v;
}

// logp[r] = base - 0.5 * s2[r]: one multiplication (exact) and one subtraction; base = res[0] is
// the factorisation's own reduction at residual 0, -1/2 logdet - (m / 2) log 2 pi. NaN when the
// status word res[3] says a pivot failed, and when the row's s2 is not finite: an Inf in ystar
// need not meet a zero of the factor on its way through the sweep, and would end as -Inf.
__global__ void post_logp_kernel(const double* __restrict__ res, const double* __restrict__ s2,
                                 int64_t rows, double* __restrict__ logp) {
  #pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const double half = 0.5 * s2[r];
  const bool ok = res[3] == (double)STATUS_NONE && half < __builtin_inf();
  logp[r] = ok ? res[0] - half : __builtin_nan("");
}

// ------------------------------------------------------------- launches
// The right-looking sweep of one chunk's rows (g.Vt) against a factor (g.L, g.dinv, g.z): the
// plan's panel and update launches in order
void post_sweep(lfm_ctx* ctx, PostArgs g, const ResidentPlan& P, const PostChunk& c) {
  hipStream_t st = ctx->stream;
  const double prow = (double)c.panel_grid * 64;
  for (const PostPanel& s : P.panels) {
    g.K0 = s.K0;
    g.w = s.w;
    g.tj0 = s.tj0;
    hipEvent_t ev;
    prof_begin(ctx, K_POST_PANEL, &ev);
    hipLaunchKernelGGL(post_panel_kernel, dim3((unsigned)c.panel_grid), dim3(256), 0, st, g);
    prof_end(ctx, K_POST_PANEL, ev, prow * NB * NB * s.w * s.w, 2.0 * prow * NB * s.w * 8);
    if (s.ntj > 0) {
      prof_begin(ctx, K_POST_UPDATE, &ev);
      hipLaunchKernelGGL(post_update_kernel, dim3((unsigned)c.tiles, (unsigned)s.ntj), dim3(256),
                         0, st, g);
      prof_end(ctx, K_POST_UPDATE, ev, 2.0 * c.pad_rows * NB * s.ntj * NB * s.w,
               2.0 * c.pad_rows * NB * s.ntj * 8);
    }
  }
}

}  // namespace

int post_sigma(lfm_ctx* ctx, const HypDev& h, const double* x, const double* d_y,
               const double* d_v, int64_t n, double diag_add, double* L, int64_t Mp) {
  int r = launch_gram_direct<double>(ctx, h, x, n, x, n, diag_add, 0.0, LFM_UPLO_LOWER, L, Mp);
  if (r) return r;
  if (d_v)
    hipLaunchKernelGGL(post_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, L, Mp, d_v, n);
  return launch_augment(ctx, h, x, d_y, nullptr, n, L, Mp, Mp);
}

void post_factor_ready(lfm_ctx* ctx, double* L, int64_t ldl, int64_t n, int64_t Np, double* z,
                       double* dinv, unsigned z_grid, unsigned dinv_grid) {
  hipLaunchKernelGGL(post_z_kernel, dim3(z_grid), dim3(256), 0, ctx->stream, L, ldl, n, Np, z);
  hipLaunchKernelGGL(post_dinv_kernel, dim3(dinv_grid), dim3(128), 0, ctx->stream, L, ldl, dinv);
}

int post_chunk(lfm_ctx* ctx, const PostArgs& g, const ResidentPlan& P, const PostChunk& c,
               const HypDev& h, const double* x, const double* t, double* out) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(post_pad_kernel, dim3(1, (unsigned)c.pad_rows), dim3(256), 0, st, g.Vt, P.Np,
                     P.n, c.rows);
  int r = launch_gram_direct<double>(ctx, h, t + c.q0 * 3, c.rows, x, P.n, 0.0, 0.0,
                                     LFM_UPLO_FULL, g.Vt, P.Np);
  if (r) return r;
  post_sweep(ctx, g, P, c);
  hipLaunchKernelGGL(post_finish_kernel, dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, st,
                     h, t, c.q0, c.rows, P.m, g.s2, g.sz, out, out + P.m);
  return hip_fail(ctx, hipGetLastError(), "resident posterior: chunk launches");
}

int post_cov(lfm_ctx* ctx, const HypDev& h, const ResidentPlan& P, const double* t,
             const double* Vt, double* cov) {
  int r = launch_gram_direct<double>(ctx, h, t, P.m, t, P.m, 0.0, 0.0, LFM_UPLO_LOWER, cov, P.m);
  if (r) return r;
  hipLaunchKernelGGL(post_cov_kernel, dim3((unsigned)P.cov_tiles, (unsigned)P.cov_tiles),
                     dim3(256), 0, ctx->stream, Vt, P.Np, cov, P.m);
  return hip_fail(ctx, hipGetLastError(), "post_cov_kernel");
}

int post_shift_factor(lfm_ctx* ctx, double* A, int64_t m, int64_t Mp, double diag_add,
                      const double* d_loc) {
  hipLaunchKernelGGL(post_shift_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                     ctx->stream, A, Mp, diag_add, m);
  return scale_factor(ctx, A, m, Mp, d_loc);
}

int post_logp_pass(lfm_ctx* ctx, const PostArgs& a, const PostLogpPlan& P, const PostChunk& c,
                   const double* mean, double* lp) {
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(post_resid_kernel, dim3((unsigned)P.resid_grid, (unsigned)c.pad_rows),
                     dim3(256), 0, st, a.Vt, P.Np, mean, P.m, c.rows);
  post_sweep(ctx, a, P.rows, c);
  hipLaunchKernelGGL(post_logp_kernel, dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, st,
                     ctx->result, a.s2, c.rows, lp);
  return hip_fail(ctx, hipGetLastError(), "held-out log density: pass launches");
}

}  // namespace lfm
