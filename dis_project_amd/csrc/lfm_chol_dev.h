// lfm_chol_dev.h — the device primitives the factorisation's kernels (lfm_chol.hip) share with
// the resident posterior's (lfm_post.hip): the fp64 MFMA wrappers, the coherent / plain 16-byte
// load, the wave-level LDS fence and gemm_accumulate, the LDS-staged panel product every
// trailing update runs on. Device code only; included by .hip units.
#pragma once

#include <cstdint>

#include "lfm_chol.h"

namespace lfm {

typedef double double4v __attribute__((ext_vector_type(4)));

// LDS row stride of a staged K stage: KS + LDP doubles. ds_read_b64 banks by (a / 4) mod 64
// per 32-lane half: the MFMA fragment reads (16 rows x 4 k, and 4 rows x 4 k) are conflict-free
// at a stride of 18 (and 66 for the chain's 64-deep stages); at 17 the 16-row reads were 2-way
// conflicted. Measured: -0.57 ms per C2 evaluation (scripts/ab_lib.py, 5 rounds), same bits.
static constexpr int LDP = 2;

__device__ __forceinline__ double4v mfma16(double a, double b, double4v c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// v_mfma_f64_4x4x4_4b_f64: four independent 4x4x4 blocks, g = (lane >> 2) & 3; lane maps
// (scripts/probe_mfma4_layout.py): A_g[i][k] at lane 16k + 4g + i, B_g[k][j] at lane
// 16k + 4g + j, D_g[i][j] at lane 16i + 4g + j.
__device__ __forceinline__ double mfma4(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// Orders one wave's LDS writes before its following LDS reads (and vice versa): LDS
// operations of a wave complete in order; the asm keeps the compiler from reordering.
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Two doubles; COH: device-coherent loads that bypass the CU's vector L1, which may hold stale
// lines of data another CU wrote (write-through) in the same launch: one 16-B nontemporal load
// (global_load_dwordx4 nt, L2-served like sc1).
typedef double double2v __attribute__((ext_vector_type(2)));
template <bool COH>
__device__ __forceinline__ double2 ld2(const double* p) {
  if (COH) {
    double2 v;
    const double2v t = __builtin_nontemporal_load(reinterpret_cast<const double2v*>(p));
    v.x = t.x;
    v.y = t.y;
    return v;
  }
  return *reinterpret_cast<const double2*>(p);
}

// acc[ir][jr] (C[wr + ir*4 + (lane>>4)][wc + jr*16 + (lane&15)] of a TR x 128 block; waves
// as 2 x 2) += sum_k Pi[i][k] Pj[j][k], k < kd. pi: row i0 of the i panel (k contiguous,
// row stride ldi). pj: BT = false, row j0 of the j panel (k contiguous, row stride ldj);
// BT = true, a K-major panel: element (k, j) at pj[k * ldj + j]. The SYRK callers hold -C in
// acc (negated once at load / store instead of per fragment). sP: LDS staging, (TR + ST) rows
// of KB + LDP doubles: rows [0, TR) panel i, rows [TR, TR + ST) panel j (j-major).
// Every thread of the (256-thread) workgroup must call it.
// KS: depth of one LDS stage (16 in the bulk kernels; 64 where one workgroup per CU has no
// neighbours to hide the global-load latency behind — the side stream's chain kernel).
template <int TR, bool BT = false, bool COH = false, int KS = KB>
__device__ __forceinline__ void gemm_accumulate(const double* __restrict__ pi, int64_t ldi,
                                                const double* __restrict__ pj, int64_t ldj,
                                                int kd, double (&acc)[TR / 8][4],
                                                double (*__restrict__ sP)[KS + LDP]) {
  constexpr int IRN = TR / 8;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: lane offsets are recomputed, not held live
  const int lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * (TR / 2), wc = (w & 1) * 64;
  const int li = lane & 15, lk = lane >> 4, l3 = lane & 3;
  // staging: TR rows of panel i and 128 rows of panel j, KS doubles each; a row is CH double2
  // chunks, thread tid moves chunk (tid % CH) of rows tid / CH + RP u. K-major j panel:
  // thread tid moves the double2 (k = idx >> 6, j = 2 (idx & 63)) of idx = tid + 256u and
  // stores it transposed.
  static_assert(KS % 16 == 0 && KS <= 64, "stage depth");
  constexpr int CH = KS / 2, RP = 256 / CH;
  constexpr int NUI = TR / RP, NUJ = ST / RP, NU = NUI + NUJ;
  const int srow = tid / CH, sch = tid % CH;
  const double* gi = pi + srow * ldi + 2 * sch;
  const double* gj = BT ? pj + (tid >> 6) * ldj + 2 * (tid & 63) : pj + srow * ldj + 2 * sch;
  const int li32 = (int)(RP * ldi);
  const int lj32 = BT ? (int)(4 * ldj) : (int)(RP * ldj);
  double2 pre[NU];
  auto gload = [&](int k0) {
    // row offsets recomputed per call (opaque stride) rather than held as live 64-bit pointers
    int l32 = li32, m32 = lj32;
    asm volatile("" : "+v"(l32), "+v"(m32));
#pragma unroll
    for (int u = 0; u < NUI; ++u) pre[u] = ld2<COH>(gi + u * l32 + k0);
    const double* gjk = BT ? gj + (int64_t)k0 * ldj : gj + k0;
#pragma unroll
    for (int u = 0; u < NUJ; ++u) pre[NUI + u] = ld2<COH>(gjk + u * m32);
  };
  gload(0);
  for (int k0 = 0; k0 < kd; k0 += KS) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NUI; ++u) {
      double* d = &sP[srow + RP * u][2 * sch];
      d[0] = pre[u].x;
      d[1] = pre[u].y;
    }
#pragma unroll
    for (int u = 0; u < NUJ; ++u) {
      if (BT) {
        const int kr = (tid >> 6) + 4 * u, jc = 2 * (tid & 63);
        sP[TR + jc][kr] = pre[NUI + u].x;
        sP[TR + jc + 1][kr] = pre[NUI + u].y;
      } else {
        double* d = &sP[TR + srow + RP * u][2 * sch];
        d[0] = pre[NUI + u].x;
        d[1] = pre[NUI + u].y;
      }
    }
    __syncthreads();
    if (k0 + KS < kd) gload(k0 + KS);
    {
#pragma unroll 1
      for (int kk = 0; kk < KS; kk += 4) {
        double bb[4];
#pragma unroll
        for (int jr = 0; jr < 4; ++jr) bb[jr] = sP[TR + wc + jr * 16 + li][kk + lk];
#pragma unroll
        for (int h = 0; h < IRN / 8; ++h) {
          double a[8];
#pragma unroll
          for (int ir = 0; ir < 8; ++ir) a[ir] = sP[wr + (h * 8 + ir) * 4 + l3][kk + lk];
#pragma unroll
          for (int ir = 0; ir < 8; ++ir)
#pragma unroll
            for (int jr = 0; jr < 4; ++jr)
              acc[h * 8 + ir][jr] = mfma4(a[ir], bb[jr], acc[h * 8 + ir][jr]);
        }
      }
    }
  }
}

}  // namespace lfm
