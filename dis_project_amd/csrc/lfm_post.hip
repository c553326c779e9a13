// lfm_post.hip — the resident posterior (include/lfm.h lfm_post_*): factor a large model once,
// predict many times.
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
#include "lfm_api_internal.h"
#include "lfm_chol_dev.h"

using namespace lfm;

struct lfm_post {
  lfm_ctx* owner = nullptr;  // the creating context: takes lfm_post_set_chunk's message
  int device = 0;
  int64_t n = 0, Np = 0, Mp = 0, G = 0;
  int64_t chunk = 0;         // 0: post_default_chunk(Np)
  double l = 0.0;
  // fixed at creation
  double* L = nullptr;       // Mp x Mp, Mp = round_up(n + 1, 128): the factor, lower triangle
  double* dinv = nullptr;    // Np / 128 x 8 inverses of L's 16 x 16 diagonal blocks
  double* z = nullptr;       // [Np], zero from n
  double* x = nullptr;       // [n x 3]
  double* par = nullptr;     // D, S, B
  // grown by the predicts (ResidentPlan's byte counts)
  double *vt = nullptr, *acc = nullptr, *t = nullptr, *out = nullptr, *cov = nullptr;
  size_t vt_cap = 0, acc_cap = 0, t_cap = 0, out_cap = 0, cov_cap = 0;
  // grown by the samples (SamplePlan's byte counts): the covariance's factor, Z and X
  double *smat = nullptr, *sz = nullptr, *sx = nullptr;
  size_t smat_cap = 0, sz_cap = 0, sx_cap = 0;
  // grown by the log densities (PostLogpPlan's byte counts): the inverses of the covariance
  // factor's diagonal blocks, the sweep's zero z and one pass's results
  double *sdinv = nullptr, *szero = nullptr, *lp = nullptr;
  size_t sdinv_cap = 0, szero_cap = 0, lp_cap = 0;
};

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
struct PostArgs {
  double* Vt;         // the chunk's rows x Np
  int64_t ldv;
  const double* L;
  int64_t ldl;
  const double* dinv;
  const double* z;
  int64_t K0;         // the super-panel's first column
  int w;              // its width in block columns
  int tj0;            // update: first block column to the right
  double* s2;         // per-row sum v^2 over the columns solved so far
  double* sz;         // per-row sum v z
};

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

// ------------------------------------------------------------------ host
int grow(lfm_ctx* ctx, double** p, size_t* cap, size_t bytes, const char* what) {
  if (bytes <= *cap) return LFM_OK;
  // every call ends synchronised: nothing in flight reads the old allocation
  if (*p) hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc((void**)p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return set_err(ctx, LFM_E_OOM, std::string("out of device memory: ") + what + " needs " +
                                       std::to_string(bytes) + " bytes");
  }
  *cap = bytes;
  return LFM_OK;
}

void release(lfm_post* q) {
  for (double* p : {q->L, q->dinv, q->z, q->x, q->par, q->vt, q->acc, q->t, q->out, q->cov,
                    q->smat, q->sz, q->sx, q->sdinv, q->szero, q->lp})
    if (p) hipFree(p);
  delete q;
}

int post_fit(lfm_ctx* ctx, lfm_post* q, const double* x, const double* y, const double* diag_vec,
             double diag_add, const lfm_hyp* hyp) {
  const int64_t n = q->n, G = q->G, Np = q->Np, Mp = q->Mp;
  auto alloc = [&](double** p, size_t count, const char* what) {
    size_t cap = 0;
    return grow(ctx, p, &cap, count * sizeof(double), what);
  };
  int r = alloc(&q->L, (size_t)Mp * Mp, "the resident factor");
  if (!r) r = alloc(&q->dinv, (size_t)(Np / NB) * NB * IB, "the diagonal inverses");
  if (!r) r = alloc(&q->z, (size_t)Np, "z");
  if (!r) r = alloc(&q->x, (size_t)n * 3, "x");
  if (!r) r = alloc(&q->par, (size_t)G * 3, "the hyperparameters");
  // y and the variances are only read while S is built: the ctx's staging
  if (!r) r = ctx->xin.reserve(ctx, (size_t)n * 2 * sizeof(double));
  if (!r) r = ctx->hpin.reserve(ctx, 64 * sizeof(double));
  if (r) return r;
  hipStream_t st = ctx->stream;
  double* d_y = ctx->xin;
  double* d_v = d_y + n;
  hipMemcpyAsync(q->x, x, n * 3 * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(d_y, y, n * 8, hipMemcpyHostToDevice, st);
  if (diag_vec) hipMemcpyAsync(d_v, diag_vec, n * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(q->par, hyp->true_d, G * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(q->par + G, hyp->true_s, G * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(q->par + 2 * G, hyp->true_b, G * 8, hipMemcpyHostToDevice, st);
  r = hip_fail(ctx, hipGetLastError(), "resident posterior: upload");
  if (r) return r;
  const HypDev h{q->par, q->par + G, q->par + 2 * G, (int)G, q->l};
  r = launch_gram_direct<double>(ctx, h, q->x, n, q->x, n, diag_add, 0.0, LFM_UPLO_LOWER, q->L, Mp);
  if (r) return r;
  if (diag_vec)
    hipLaunchKernelGGL(post_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q->L,
                       Mp, d_v, n);
  r = launch_augment(ctx, h, q->x, d_y, nullptr, n, q->L, Mp, Mp);
  if (r) return r;
  r = chol_factor_solve(ctx, q->L, Mp, n, Mp, 0, ctx->result, CHOL_RESIDENT);
  if (r) return r;
  hipLaunchKernelGGL(post_z_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, q->L, Mp,
                     n, Np, q->z);
  hipLaunchKernelGGL(post_dinv_kernel, dim3((unsigned)(Np / NB)), dim3(128), 0, st, q->L, Mp,
                     q->dinv);
  r = hip_fail(ctx, hipGetLastError(), "post_dinv_kernel");
  if (r) return r;
  double* hres = ctx->hpin;
  hipMemcpyAsync(hres, ctx->result, 5 * sizeof(double), hipMemcpyDeviceToHost, st);
  r = finish(ctx);
  if (r) return r;
  return status_code(ctx, hres[3], hres[4]);
}

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

// The launches of one chunk, exactly as the plan lists them
int post_chunk(lfm_ctx* ctx, lfm_post* q, const ResidentPlan& P, const PostChunk& c,
               const HypDev& h) {
  hipStream_t st = ctx->stream;
  const int64_t Np = P.Np;
  hipLaunchKernelGGL(post_pad_kernel, dim3(1, (unsigned)c.pad_rows), dim3(256), 0, st, q->vt, Np,
                     q->n, c.rows);
  int r = launch_gram_direct<double>(ctx, h, q->t + c.q0 * 3, c.rows, q->x, q->n, 0.0, 0.0,
                                     LFM_UPLO_FULL, q->vt, Np);
  if (r) return r;
  PostArgs g{};
  g.Vt = q->vt;
  g.ldv = Np;
  g.L = q->L;
  g.ldl = q->Mp;
  g.dinv = q->dinv;
  g.z = q->z;
  g.s2 = q->acc;
  g.sz = q->acc + P.vt_rows;
  post_sweep(ctx, g, P, c);
  hipLaunchKernelGGL(post_finish_kernel, dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, st,
                     h, q->t, c.q0, c.rows, P.m, g.s2, g.sz, q->out, q->out + P.m);
  return hip_fail(ctx, hipGetLastError(), "resident posterior: chunk launches");
}

// One predict with the covariance when the plan has it, left on the device: mean in q->out [m],
// var in q->out + m (marginals only), cov in q->cov (m x m, dense). Nothing is downloaded.
int post_enqueue(lfm_ctx* ctx, lfm_post* q, const ResidentPlan& P, const double* t) {
  const bool cov = P.cov_bytes != 0;
  int r = grow(ctx, &q->vt, &q->vt_cap, P.vt_bytes, "the solve workspace");
  if (!r) r = grow(ctx, &q->acc, &q->acc_cap, P.acc_bytes, "the row accumulators");
  if (!r) r = grow(ctx, &q->t, &q->t_cap, P.t_bytes, "the test inputs");
  if (!r) r = grow(ctx, &q->out, &q->out_cap, P.out_bytes, "mean / var");
  if (!r && cov) r = grow(ctx, &q->cov, &q->cov_cap, P.cov_bytes, "the covariance");
  if (r) return r;
  hipStream_t st = ctx->stream;
  const int64_t G = q->G, m = P.m;
  const HypDev h{q->par, q->par + G, q->par + 2 * G, (int)G, q->l};
  hipMemcpyAsync(q->t, t, P.t_bytes, hipMemcpyHostToDevice, st);
  for (const PostChunk& c : P.chunks) {
    r = post_chunk(ctx, q, P, c, h);
    if (r) return r;
  }
  if (cov) {
    // one chunk (the plan rejected anything else): its Vt is whole
    r = launch_gram_direct<double>(ctx, h, q->t, m, q->t, m, 0.0, 0.0, LFM_UPLO_LOWER, q->cov, m);
    if (r) return r;
    hipLaunchKernelGGL(post_cov_kernel, dim3((unsigned)P.cov_tiles, (unsigned)P.cov_tiles),
                       dim3(256), 0, st, q->vt, P.Np, q->cov, m);
    r = hip_fail(ctx, hipGetLastError(), "post_cov_kernel");
  }
  return r;
}

// A[i][i] += d: the caller's diag_add on the sampled covariance, in one addition
__global__ void post_shift_kernel(double* __restrict__ A, int64_t lda, double d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i * lda + i] += d;
}

// The first steps of a sample and of a log density, in stream order: the predict with the
// covariance (mean in q->out, cov in q->cov), cov into the Mp-stride matrix q->smat, diag_add on
// its diagonal in one addition, the augmented row with residual 0 and the factorisation, which
// leaves L in q->smat's lower triangle, the status in ctx->result[3] and
// ctx->result[0] = -1/2 logdet - (m / 2) log 2 pi. q->smat holds Mp x Mp doubles.
int post_scale_factor(lfm_ctx* ctx, lfm_post* q, const ResidentPlan& P, int64_t Mp, const double* t,
                      double diag_add) {
  int r = post_enqueue(ctx, q, P, t);
  if (r) return r;
  hipStream_t st = ctx->stream;
  const int64_t m = P.m;
  hipError_t e = hipMemcpy2DAsync(q->smat, Mp * 8, q->cov, m * 8, m * 8, m,
                                  hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return hip_fail(ctx, e, "the covariance into the factor's stride");
  hipLaunchKernelGGL(post_shift_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st,
                     q->smat, Mp, diag_add, m);
  return scale_factor(ctx, q->smat, m, Mp, q->out);
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

}  // namespace
}  // namespace lfm

extern "C" {

int lfm_post_create(lfm_ctx* ctx, const double* x, const double* y, int64_t n,
                    const double* diag_vec, double diag_add, const lfm_hyp* hyp, lfm_post** out) {
  int r = validate_x(ctx, x, n);
  if (r) return r;
  if (out) *out = nullptr;
  if (!y || !out) return set_err(ctx, LFM_E_ARG, "y / out is NULL");
  if (!hyp) return set_err(ctx, LFM_E_ARG, "hyp is NULL");
  if (hyp->num_genes < 1 || hyp->num_genes > (1 << 20))
    return set_err(ctx, LFM_E_ARG, "num_genes must be in [1, 2^20]");
  if (!hyp->true_d || !hyp->true_s || !hyp->true_b)
    return set_err(ctx, LFM_E_ARG, "hyp true_d / true_s / true_b must not be NULL");
  r = check_mean_shape(ctx, n, hyp);
  if (r) return r;
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // schedule 1, shared
  lfm_post* q = new lfm_post;
  q->owner = ctx;
  q->device = ctx->device;
  q->n = n;
  q->G = hyp->num_genes;
  q->Np = round_up(n, NB);
  q->Mp = round_up(n + 1, NB);
  q->l = hyp->l;
  r = post_fit(ctx, q, x, y, diag_vec, diag_add, hyp);
  if (r) {
    hipStreamSynchronize(ctx->stream);
    release(q);
    return r;
  }
  *out = q;
  return LFM_OK;
}

int lfm_post_destroy(lfm_post* post) {
  if (!post) return LFM_E_ARG;
  DeviceGuard g(post->device);
  release(post);
  return LFM_OK;
}

int lfm_post_set_chunk(lfm_post* post, int64_t rows) {
  if (!post) return LFM_E_ARG;
  if (rows < 0 || rows % 128 != 0)
    return set_err(post->owner, LFM_E_ARG, "the chunk must be a multiple of 128 rows (0: default)");
  post->chunk = rows;
  return LFM_OK;
}

int lfm_post_predict_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double* mean,
                         double* var, double* cov) {
  if (!ctx) return LFM_E_ARG;
  if (!post) return set_err(ctx, LFM_E_ARG, "post is NULL");
  if (ctx->device != post->device)
    return set_err(ctx, LFM_E_ARG, "the handle belongs to another device than this ctx");
  if (!t || !mean) return set_err(ctx, LFM_E_ARG, "t / mean is NULL");
  if (!var && !cov) return set_err(ctx, LFM_E_ARG, "one of var / cov must be given");
  lfm_post* q = post;
  const ResidentPlan P = plan_post(q->n, q->G, m, q->chunk, cov != nullptr);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // no factorisation: shared
  int r = post_enqueue(ctx, q, P, t);
  if (r) return r;
  hipStream_t st = ctx->stream;
  hipMemcpyAsync(mean, q->out, (size_t)m * 8, hipMemcpyDeviceToHost, st);
  if (cov)
    hipMemcpyAsync(cov, q->cov, P.cov_bytes, hipMemcpyDeviceToHost, st);
  else
    hipMemcpyAsync(var, q->out + m, (size_t)m * 8, hipMemcpyDeviceToHost, st);
  r = finish(ctx);
  if (r) return r;
  if (cov && var)
    for (int64_t i = 0; i < m; ++i) var[i] = cov[i * m + i];  // diag(cov), bit for bit
  return LFM_OK;
}

int lfm_post_sample_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                        uint64_t seed, int64_t sample0, int64_t nsamp, double* mean,
                        double* out) {
  if (!ctx) return LFM_E_ARG;
  if (!post) return set_err(ctx, LFM_E_ARG, "post is NULL");
  if (ctx->device != post->device)
    return set_err(ctx, LFM_E_ARG, "the handle belongs to another device than this ctx");
  if (!t || !out) return set_err(ctx, LFM_E_ARG, "t / out is NULL");
  lfm_post* q = post;
  const ResidentPlan P = plan_post(q->n, q->G, m, q->chunk, true);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  const SamplePlan S = plan_sample(m, nsamp, sample0);
  if (S.reject) return set_err(ctx, LFM_E_ARG, S.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // CHOL_RESIDENT is schedule 1: shared
  int r = grow(ctx, &q->smat, &q->smat_cap, S.mat_bytes, "the covariance's factor");
  if (!r) r = grow(ctx, &q->sz, &q->sz_cap, S.z_bytes, "the normals");
  if (!r) r = grow(ctx, &q->sx, &q->sx_cap, S.x_bytes, "the samples");
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  r = post_scale_factor(ctx, q, P, S.Mp, t, diag_add);
  if (r) return r;
  hipStream_t st = ctx->stream;
  r = sample_draw(ctx, S, q->smat, q->out, seed, q->sz, q->sx);
  if (r) return r;
  if (mean) hipMemcpyAsync(mean, q->out, (size_t)m * 8, hipMemcpyDeviceToHost, st);
  return sample_finish(ctx, S, q->sx, out, mean);
}

int lfm_post_log_prob_f64(lfm_ctx* ctx, lfm_post* post, const double* t, int64_t m, double diag_add,
                          const double* ystar, int64_t k, double* mean, double* logp) {
  if (!ctx) return LFM_E_ARG;
  if (!post) return set_err(ctx, LFM_E_ARG, "post is NULL");
  if (ctx->device != post->device)
    return set_err(ctx, LFM_E_ARG, "the handle belongs to another device than this ctx");
  if (!t || !ystar || !logp) return set_err(ctx, LFM_E_ARG, "t / ystar / logp is NULL");
  lfm_post* q = post;
  const PostLogpPlan P = plan_post_logp(q->n, q->G, m, k, q->chunk);
  if (P.reject) return set_err(ctx, LFM_E_ARG, P.why);
  DeviceGuard g(ctx->device);
  DeviceTenancy tenancy(ctx, false);  // CHOL_RESIDENT is schedule 1: shared
  // the predict's Vt and accumulators serve the residual rows once the covariance is formed:
  // grown to the larger of the two uses before the predict, which then finds them large enough
  int r = grow(ctx, &q->vt, &q->vt_cap, P.vt_bytes, "the solve workspace");
  if (!r) r = grow(ctx, &q->acc, &q->acc_cap, P.acc_bytes, "the row accumulators");
  if (!r) r = grow(ctx, &q->smat, &q->smat_cap, P.mat_bytes, "the covariance's factor");
  if (!r) r = grow(ctx, &q->sdinv, &q->sdinv_cap, P.dinv_bytes, "its diagonal inverses");
  if (!r) r = grow(ctx, &q->szero, &q->szero_cap, P.zero_bytes, "the zero z");
  if (!r) r = grow(ctx, &q->lp, &q->lp_cap, P.logp_bytes, "the log densities");
  if (!r) r = ctx->hpin.reserve(ctx, 1 << 16);
  if (r) return r;
  r = post_scale_factor(ctx, q, P.pred, P.Mp, t, diag_add);
  if (r) return r;
  hipStream_t st = ctx->stream;
  // the factor as the sweep reads it: row m, which holds L^{-1} 0, becomes the identity row its
  // neighbours are and its zeros become the sweep's z; then the diagonal blocks' inverses. The
  // sweep reads the factor's 16 x 16 diagonal blocks through these inverses alone (built from
  // their lower triangles) and everything else strictly below them, so the input entries the
  // factorisation leaves above the diagonal are never read.
  hipLaunchKernelGGL(post_z_kernel, dim3((unsigned)P.z_grid), dim3(256), 0, st, q->smat, P.Mp, m,
                     P.Np, q->szero);
  hipLaunchKernelGGL(post_dinv_kernel, dim3((unsigned)P.dinv_grid), dim3(128), 0, st, q->smat, P.Mp,
                     q->sdinv);
  PostArgs a{};
  a.Vt = q->vt;
  a.ldv = P.Np;
  a.L = q->smat;
  a.ldl = P.Mp;
  a.dinv = q->sdinv;
  a.z = q->szero;
  a.s2 = q->acc;
  a.sz = q->acc + P.rows.vt_rows;
  for (const PostChunk& c : P.rows.chunks) {
    hipError_t e = hipMemcpy2DAsync(q->vt, P.Np * 8, ystar + c.q0 * m, m * 8, m * 8, c.rows,
                                    hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "upload ystar");
    hipLaunchKernelGGL(post_resid_kernel, dim3((unsigned)P.resid_grid, (unsigned)c.pad_rows),
                       dim3(256), 0, st, q->vt, P.Np, q->out, m, c.rows);
    post_sweep(ctx, a, P.rows, c);
    hipLaunchKernelGGL(post_logp_kernel, dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, st,
                       ctx->result, a.s2, c.rows, q->lp);
    r = hip_fail(ctx, hipGetLastError(), "held-out log density: pass launches");
    if (r) return r;
    hipMemcpyAsync(logp + c.q0, q->lp, (size_t)c.rows * 8, hipMemcpyDeviceToHost, st);
  }
  if (mean) hipMemcpyAsync(mean, q->out, (size_t)m * 8, hipMemcpyDeviceToHost, st);
  double* hres = ctx->hpin;
  hipMemcpyAsync(hres, ctx->result, 5 * sizeof(double), hipMemcpyDeviceToHost, st);
  r = finish(ctx);
  if (r) return r;
  r = status_code(ctx, hres[3], hres[4]);
  if (r == LFM_E_NOT_PD) {
    std::fill(logp, logp + k, std::nan(""));
    if (mean) std::fill(mean, mean + m, std::nan(""));
  }
  return r;
}

}  // extern "C"
