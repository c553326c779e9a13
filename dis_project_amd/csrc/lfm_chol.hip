// lfm_chol.hip — blocked right-looking fp64 Cholesky + solve + logdet on gfx950.
//
// Replaces the arithmetic behind gpjax 0.8.2 GaussianDistribution.log_prob as called
// at src/objectives.py:76-78 (cola Cholesky -> jnp.linalg.cholesky -> LAPACK dpotrf,
// triangular solves, logdet = 2 sum log L_ii):
//     log N(y; m, S) = -1/2 ( n log 2pi + logdet S + r^T S^{-1} r ),  r = y - m.
//
// The factor is stored row-major, lower triangle, leading dimension lda = Mp
// (Mp = n+1 rounded up to 128). Row n holds r (written by augment_kernel), so the
// factorisation of the augmented matrix [[S, .], [r^T, 1]] yields z = L^{-1} r in
// row n: no separate triangular solve pass (quad = ||z||^2). Rows > n are identity.
//
// Per block column k (NB = 128):
//   potrf_diag_kernel  one workgroup factors the 128x128 diagonal block in LDS, 16 columns
//                      at a time: the 16x16 diagonal sub-block is factored and inverted
//                      in registers by every wave (cross-lane v_readlane broadcasts), the
//                      rows below are solved against that inverse, and the rank-16 update
//                      of the rest runs on v_mfma_f64_16x16x4_f64. It also writes the eight
//                      16x16 diagonal inverses (dinv) for the panel solve, the logdet
//                      partial and the first failing pivot. Columns >= n take a unit pivot.
//   trsm_kernel        rows below the block: X = A_ik L_kk^{-T} by blocked substitution,
//                      16 columns at a time, on fp64 MFMA (L_kk from L2, dinv blocks).
//   syrk_kernel        trailing lower triangle, 128x128 tiles: C -= P P^T on fp64 MFMA —
//                      the only O(n^3) kernel.
// Look-ahead: the SYRK of block column k is split into the next block column (k+1) and
// the rest. A high-priority side stream runs syrk(next) -> potrf(k+1) -> trsm(k+1) while
// the main stream runs syrk(rest) of step k, so the latency-bound panel work of step k+1
// hides behind the bulk of step k's trailing update.
// finalize_kernel reduces logdet + ||z||^2 to the scalar MLL.
// This unit is the device code alone; the host code that plans and issues the launches
// (chol_factor_solve, both schedules) is lfm_chol_sched.hip, over the plan of lfm_host.cpp.
#include <cstdint>

#include "lfm_chol.h"
#include "lfm_chol_dev.h"

namespace lfm {

// The tile constants shared with the scheduling unit (NB, IB, ST, KB, SLAB_WGS, WBULK, WBORD,
// SUPERTILE, TALL_SPLIT), the launch argument structs and the LDS sizes: lfm_chol.h. The MFMA
// wrappers, the staged stride LDP, ld2, wave_lds_fence and gemm_accumulate, shared with the
// resident posterior's kernels: lfm_chol_dev.h.
// Bulk trailing update (step_kernel's update units): K depth of one LDS stage (32: 130 VGPRs +
// 64 AGPRs, 2 waves / SIMD)
static constexpr int STEP_KS = 16;
constexpr int PANEL_TIMEOUT = STATUS_TIMEOUT;  // status: a bounded device-side wait ran out
// Which wait ran out first (status[1], reported in LFM_E_TIMEOUT's message): 1 tall unit on the
// chain, 2 tall unit on its ahead units, 5 chain input wait, 6 chain grid barrier, 7 fused panel
// wait (3 and 4 are unused).
__device__ __forceinline__ void timeout_at(int* status, int why) {
  atomicMin(status, PANEL_TIMEOUT);
  atomicCAS(status + 1, 0, why);
}

// Value of v held by lane `src` (0..15, compile-time) of each 16-lane row, broadcast to the
// row: DPP row_newbcast (VGPR to VGPR; no SGPR round trip as with v_readlane).
template <int SRC>
__device__ __forceinline__ double row_bcast_t(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, 0x150 + SRC, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), 0x150 + SRC, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// src folds to a constant in the fully unrolled callers
__device__ __forceinline__ double row_bcast(double v, int src) {
  switch (src) {
    case 0: return row_bcast_t<0>(v);
    case 1: return row_bcast_t<1>(v);
    case 2: return row_bcast_t<2>(v);
    case 3: return row_bcast_t<3>(v);
    case 4: return row_bcast_t<4>(v);
    case 5: return row_bcast_t<5>(v);
    case 6: return row_bcast_t<6>(v);
    case 7: return row_bcast_t<7>(v);
    case 8: return row_bcast_t<8>(v);
    case 9: return row_bcast_t<9>(v);
    case 10: return row_bcast_t<10>(v);
    case 11: return row_bcast_t<11>(v);
    case 12: return row_bcast_t<12>(v);
    case 13: return row_bcast_t<13>(v);
    case 14: return row_bcast_t<14>(v);
    default: return row_bcast_t<15>(v);
  }
}

// As row_bcast with one v_mov_b64_dpp (gfx90a+ 64-bit DPP, row_newbcast) instead of two
// 32-bit moves; the compiler keeps the DPP hazards.
template <int SRC>
__device__ __forceinline__ double row_bcast64_t(double v) {
  return __builtin_amdgcn_mov_dpp(v, 0x150 + SRC, 0xf, 0xf, false);
}
__device__ __forceinline__ double row_bcast64(double v, int src) {
  switch (src) {
    case 0: return row_bcast64_t<0>(v);
    case 1: return row_bcast64_t<1>(v);
    case 2: return row_bcast64_t<2>(v);
    case 3: return row_bcast64_t<3>(v);
    case 4: return row_bcast64_t<4>(v);
    case 5: return row_bcast64_t<5>(v);
    case 6: return row_bcast64_t<6>(v);
    case 7: return row_bcast64_t<7>(v);
    case 8: return row_bcast64_t<8>(v);
    case 9: return row_bcast64_t<9>(v);
    case 10: return row_bcast64_t<10>(v);
    case 11: return row_bcast64_t<11>(v);
    case 12: return row_bcast64_t<12>(v);
    case 13: return row_bcast64_t<13>(v);
    case 14: return row_bcast64_t<14>(v);
    default: return row_bcast64_t<15>(v);
  }
}

// Pins 16 register values at this point of the instruction stream (no instructions): the
// updates before it are issued before the ones after it. Keeps a right-looking sweep
// right-looking (the scheduler otherwise regroups the FMAs per element, a dependent chain of
// c FMAs for element c).
__device__ __forceinline__ void pin16(double (&p)[16]) {
  asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]),
               "+v"(p[6]), "+v"(p[7]), "+v"(p[8]), "+v"(p[9]), "+v"(p[10]), "+v"(p[11]),
               "+v"(p[12]), "+v"(p[13]), "+v"(p[14]), "+v"(p[15]));
}

// ---------------------------------------------------------------- potrf
// One double, write-through (COH) or plain.
template <bool COH>
__device__ __forceinline__ void st1(double* p, double v) {
  if (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// Two doubles at base + off (bytes, 16-B aligned) in one 16-B write-through (sc1) vector store:
// the wide form of st1<true> (an 8-B sc1 store is one fabric write, ≈2.7x the 16-B time per
// byte, MI355X_MICROARCH.md). base must be wave-uniform (a kernel argument or derived from one):
// it becomes the buffer resource. Range: off + 16 <= 2^31 - 1 (num_records); a store past it is
// dropped without a fault, so the helper serves the per-block workspaces only (the inverse,
// X_D, the chain workspace: at most 4 W^2 doubles = 13 MB at W = 640), never the matrix.
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st2_wt(double* base, unsigned off, double a, double b) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
  const double2v v = {a, b};
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), r, off, 0, 16 /* sc1 */);
}
template <bool COH>
__device__ __forceinline__ double ld1(const double* p) {
  if (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x * y, y, 1.5);
  y = y * fma(-0.5 * x * y, y, 1.5);
  return y;
}

// One 256-thread workgroup, the 128x128 diagonal block in LDS, 16 columns per step:
//  (1) wave 0 factors the 16x16 diagonal sub-block in registers (lane = row);
//  (2) every wave solves rows below against it by substitution (lane = row; the L_D
//      entries are wave-uniform LDS reads);
//  (3) the rank-16 update of the trailing lower triangle on fp64 MFMA.
// After the loop the eight 16x16 diagonal inverses (dinv, for trsm_kernel) are built by
// the four waves, and logdet / the first failing pivot are reduced.
// PH: bit 0 = phase 1, bit 1 = phase 2, bit 2 = phase 3, bit 3 = global load / store of
// the block. The product path always runs PH = 15, in the
// chain kernel with bit 5 (the block load in one batch) and bit 7 (64-bit DPP broadcasts in
// the leaf), in its light mode also bit 4 (device-coherent block loads) and bit 6 (no block
// store: nothing reads it but row n).
// only the 36 lower 16x16 blocks of the 128x128 block, each 16 x 17 (padded) doubles
// (MB_DOUBLES): 78 KB, so the kernel fits on a CU beside one SYRK workgroup (look-ahead overlap)

template <int PH>
__device__ __forceinline__ void potrf_block(double* __restrict__ Mb, double* __restrict__ A,
                                            int64_t lda, int64_t kb, int64_t npiv,
                                            double* __restrict__ dinv,
                                            double* __restrict__ parts, int k,
                                            int* __restrict__ status,
                                            double* __restrict__ Li = nullptr,
                                            unsigned long long* __restrict__ pst = nullptr) {
  // pst (diagnostics, NULL: off): s_memrealtime after the load (0), panel iterations 0, 3, 6
  // (1-3), the loop (4), inverse block row 6 (5) and 7 (6), the block store (7)
  auto pstamp = [&](int p) {
    if (pst && threadIdx.x == 0) pst[p] = __builtin_amdgcn_s_memrealtime();
  };
  __shared__ double pvs[NB];  // unscaled pivots
  __shared__ double ipv[NB];  // 1 / L_cc
  __shared__ double red[4];
  __shared__ int redi[4];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: the callers' loops do not hoist and hold its index math
  const int lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
#define MS(r, q) Mb[((((r) >> 4) * (((r) >> 4) + 1) / 2) + ((q) >> 4)) * (IB * (IB + 1)) + \
                    ((r) & 15) * (IB + 1) + ((q) & 15)]

  // block load: row r, 16-B chunks of the lower 16x16 blocks; two batches of 16 loads per
  // thread in flight (64 VGPRs), so the kernel fits in one bulk-SYRK workgroup's registers
  // (PH bit 5, the chain kernel with one workgroup per CU: all 32 at once)
  constexpr int LB = (PH & 32) ? 32 : 16;
#pragma unroll
  for (int hb = 0; hb < 32 / LB; ++hb) {
    double2 v[LB];
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int idx = tid + 256 * (u + LB * hb), r = idx >> 6, c2 = idx & 63;
      if ((2 * c2) >> 4 <= r >> 4)
        v[u] = (PH & 8) ? ld2<(PH & 16) != 0>(&A[(kb + r) * lda + kb + 2 * c2])
                        : double2{(r == 2 * c2) ? 2.0 : 0.0, (r == 2 * c2 + 1) ? 2.0 : 0.0};
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int idx = tid + 256 * (u + LB * hb), r = idx >> 6, c2 = idx & 63;
      if ((2 * c2) >> 4 <= r >> 4) {
        MS(r, 2 * c2) = v[u].x;
        MS(r, 2 * c2 + 1) = v[u].y;
      }
    }
  }
  __syncthreads();

  // Look-ahead over the eight 16-column panels: after the rows below panel ib are solved,
  // wave 0 applies panel ib to the next diagonal 16x16 block alone and factors it (the serial
  // leaf) while waves 1-3 apply panel ib to the rest of the trailing triangle.
  // leaf: wave 0 factors diagonal block cb in registers (lane = row)
  auto leaf = [&](int cb) {
    const int c0 = cb * IB;
    double d[IB], pv[IB], yv[IB];
#pragma unroll
    for (int q = 0; q < IB; ++q) d[q] = (lane < IB && q <= lane) ? MS(c0 + li, c0 + q) : 0.0;
    // PH bit 7: 64-bit DPP moves (v_mov_b64_dpp, one instruction per broadcast) instead of
    // two 32-bit ones
    if constexpr ((PH & 128) != 0) {
      // pipelined: column c's update of column c + 1 first, then the pivot chain of c + 1
      // (broadcast, rsqrt, Newton) is issued ahead of c's remaining updates, whose latency it
      // hides; the same operations per element in the same order (bit-identical)
      double dc = row_bcast64(d[0], 0);
      if (kb + c0 >= npiv) dc = 1.0;
      double y = rsqrt_1nr(dc);
#pragma unroll
      for (int c = 0; c < IB; ++c) {
        pv[c] = dc;
        yv[c] = y;
        d[c] = (lane == c) ? dc * y : d[c] * y;
        if (c + 1 < IB) {
          d[c + 1] = fma(-d[c], row_bcast64(d[c], c + 1), d[c + 1]);
          double dn = row_bcast64(d[c + 1], c + 1);
          if (kb + c0 + c + 1 >= npiv) dn = 1.0;
          // rsqrt_1nr(dn) = r * fma(-0.5 dn * r, r, 1.5), its dependent steps spread over the
          // remaining updates in four chunks (scheduling fences keep the interleave: the wave
          // issues in order, so a dependent step stalls it unless independent work sits between)
          const double r = __builtin_amdgcn_rsq(dn);
          const double hh = -0.5 * dn;
          const int REM = IB - c - 2, K = (REM + 3) / 4;
          double t1 = 0.0, t2 = 0.0, yn = 0.0;
#pragma unroll
          for (int part = 0; part < 4; ++part) {
            // a chunk's broadcasts first, then its FMAs (each FMA would otherwise wait on the
            // broadcast issued just before it)
            double bq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // K <= 4 (REM <= 14)
              const int q = c + 2 + part * K + i;
              if (i < K && q < IB) bq[i] = row_bcast64(d[c], q);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int q = c + 2 + part * K + i;
              if (i < K && q < IB) d[q] = fma(-d[c], bq[i], d[q]);
            }
            if (part == 0) t1 = hh * r;
            if (part == 1) t2 = fma(t1, r, 1.5);
            if (part == 2) yn = r * t2;
            __builtin_amdgcn_sched_barrier(0);
          }
          dc = dn;
          y = yn;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < IB; ++c) {
        double dc = row_bcast(d[c], c);
        if (kb + c0 + c >= npiv) dc = 1.0;
        const double y = rsqrt_1nr(dc);
        pv[c] = dc;
        yv[c] = y;
        d[c] = (lane == c) ? dc * y : d[c] * y;
#pragma unroll
        for (int q = c + 1; q < IB; ++q) d[q] = fma(-d[c], row_bcast(d[c], q), d[q]);
      }
    }
    if (lane < IB) {
#pragma unroll
      for (int q = 0; q < IB; ++q)
        if (q <= lane) MS(c0 + lane, c0 + q) = d[q];
    }
    // the pivots are wave-uniform after the broadcasts: lane c keeps pivot c
    double pvl = 0.0, yvl = 0.0;
#pragma unroll
    for (int c = 0; c < IB; ++c) {
      pvl = (lane == c) ? pv[c] : pvl;
      yvl = (lane == c) ? yv[c] : yvl;
    }
    if (lane < IB) {
      pvs[c0 + lane] = pvl;
      ipv[c0 + lane] = yvl;
    }
  };
  // one 16x16 tile (i0, j0) -= panel c0 rows i0 x rows j0 (fp64 MFMA), in LDS
  // (block offsets from wave-uniform block indices: scalar address math; the lane parts
  // (lk + 4 r) * 17 + li and li * 17 + 4 ks + lk are fixed per lane)
  auto tile_update = [&](int i0, int j0, int c0) {
    const int bi = __builtin_amdgcn_readfirstlane(i0 >> 4);
    const int bj = __builtin_amdgcn_readfirstlane(j0 >> 4);
    const int bc = __builtin_amdgcn_readfirstlane(c0 >> 4);
    double* C = Mb + (bi * (bi + 1) / 2 + bj) * (IB * (IB + 1));
    const double* Pa = Mb + (bi * (bi + 1) / 2 + bc) * (IB * (IB + 1));
    const double* Pb = Mb + (bj * (bj + 1) / 2 + bc) * (IB * (IB + 1));
    double4v acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = C[(lk + 4 * r) * (IB + 1) + li];
#pragma unroll
    for (int ks = 0; ks < IB / 4; ++ks)
      acc = mfma16(-Pa[li * (IB + 1) + ks * 4 + lk], Pb[li * (IB + 1) + ks * 4 + lk], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(lk + 4 * r) * (IB + 1) + li] = acc[r];
  };
  // lower 16x16 tiles of a triangle of side nrb, enumerated row by row: tile t -> (row, column)
  auto tri_tile = [](int t, int* ti, int* tj) {
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    *ti = r;
    *tj = t - r * (r + 1) / 2;
  };
  // With Li (the full inverse is wanted), waves 1-3 build it in the time the look-ahead leaves
  // them: Dinv_I (16x16 inverse of L_II, forward substitution, lane = column) and the blocks
  // Linv_IJ = -Dinv_I sum_{K=J}^{I-1} L_IK Linv_KJ of block row I (fp64 MFMA; the 16x16
  // accumulator layout is the B-operand layout of the next product).
#define LI(r, q) Li[((((r) >> 4) * (((r) >> 4) + 1) / 2) + ((q) >> 4)) * (IB * (IB + 1)) + \
                    ((r) & 15) * (IB + 1) + ((q) & 15)]
  // PH bit 9: p <- p L^-T (16 columns, right-looking), pinned column by column, column c + 1
  // of L (and its 1 / L_cc) loaded while column c is applied (the pins are scheduling
  // boundaries). Ld: the 16x16 block (row stride 17), y: 1 / L_cc.
  auto sweep_pinned = [](double (&p)[IB], const double* Ld, const double* y) {
    double lc[IB], ln[IB], yc = y[0], yn = 0.0;
#pragma unroll
    for (int q = 1; q < IB; ++q) lc[q] = Ld[q * (IB + 1)];
#pragma unroll
    for (int c = 0; c < IB; ++c) {
      if (c + 1 < IB) {
        yn = y[c + 1];
#pragma unroll
        for (int q = c + 2; q < IB; ++q) ln[q] = Ld[q * (IB + 1) + c + 1];
      }
      p[c] = p[c] * yc;
#pragma unroll
      for (int q = c + 1; q < IB; ++q) p[q] = fma(-p[c], lc[q], p[q]);
      pin16(p);
      yc = yn;
#pragma unroll
      for (int q = c + 2; q < IB; ++q) lc[q] = ln[q];
    }
  };
  auto dinv_block = [&](int I) {
    const int c0 = I * IB;
    const int bd = __builtin_amdgcn_readfirstlane(I);
    const double* Ld = Mb + (bd * (bd + 1) / 2 + bd) * (IB * (IB + 1));
    double x[IB];
#pragma unroll
    for (int r = 0; r < IB; ++r) x[r] = (li == r) ? 1.0 : 0.0;
    // right-looking (the same terms in the same order per element as the left-looking sum,
    // one dependent FMA + multiply per step instead of r)
    if constexpr ((PH & 512) != 0) {
      sweep_pinned(x, Ld, ipv + c0);
    } else {
#pragma unroll
      for (int r = 0; r < IB; ++r) {
        x[r] = x[r] * ipv[c0 + r];
#pragma unroll
        for (int q = r + 1; q < IB; ++q) x[q] = fma(-Ld[q * (IB + 1) + r], x[r], x[q]);
      }
    }
    if (lane < IB) {
#pragma unroll
      for (int r = 0; r < IB; ++r) LI(c0 + r, c0 + lane) = x[r];
    }
  };
  auto linv_block = [&](int I, int J) {
    I = __builtin_amdgcn_readfirstlane(I);  // wave-uniform block indices: scalar offsets
    J = __builtin_amdgcn_readfirstlane(J);
    auto blk = [&](int bi, int bj) { return (bi * (bi + 1) / 2 + bj) * (IB * (IB + 1)); };
    double4v sacc = {0, 0, 0, 0};
    for (int K = J; K < I; ++K) {
      const double* a = Mb + blk(I, K);
      const double* b = Li + blk(K, J);
#pragma unroll
      for (int ks = 0; ks < IB / 4; ++ks)
        sacc = mfma16(a[li * (IB + 1) + 4 * ks + lk], b[(4 * ks + lk) * (IB + 1) + li], sacc);
    }
    const double* d = Li + blk(I, I);
    double4v o = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < IB / 4; ++ks) o = mfma16(d[li * (IB + 1) + 4 * ks + lk], sacc[ks], o);
    double* out = Li + blk(I, J);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(lk + 4 * r) * (IB + 1) + li] = -o[r];
  };
  if ((PH & 1) && w == 0) leaf(0);
  __syncthreads();
  pstamp(0);
#pragma unroll 1
  for (int ib = 0; ib < NB / IB; ++ib) {
    const int c0 = ib * IB;
    // (2) rows below: x_c = (p_c - sum_{q<c} x_q L[c][q]) / L_cc, swept right-looking: once
    // x_c is known it is subtracted from every later p_q at once. Each p_q still accumulates
    // its terms in increasing c (bit-identical to the left-looking sum), but the dependent
    // chain per column is one FMA and one multiply instead of c FMAs.
    const int nr = NB - c0 - IB;
    if ((PH & 2) && w * 64 < nr) {
      const bool act = tid < nr;
      const int row = c0 + IB + (act ? tid : 0);
      double p[IB];
#pragma unroll
      for (int q = 0; q < IB; ++q) p[q] = MS(row, c0 + q);
      const int bd = __builtin_amdgcn_readfirstlane(c0 >> 4);
      const double* Ld = Mb + (bd * (bd + 1) / 2 + bd) * (IB * (IB + 1));  // L[c0.., c0..]
      if constexpr ((PH & 512) != 0) {
        sweep_pinned(p, Ld, ipv + c0);
      } else {
#pragma unroll
        for (int c = 0; c < IB; ++c) {
          p[c] = p[c] * ipv[c0 + c];
#pragma unroll
          for (int q = c + 1; q < IB; ++q) p[q] = fma(-p[c], Ld[q * (IB + 1) + c], p[q]);
        }
      }
      if (act) {
#pragma unroll
        for (int q = 0; q < IB; ++q) MS(row, c0 + q) = p[q];
      }
    }
    __syncthreads();
    if (nr == 0) break;
    // (3) wave 0: next diagonal block, then its leaf; waves 1-3: the other trailing tiles
    const int nrb = nr / IB;
    // the early panels' wide trailing triangles: wave 0 takes its last k0 tiles after the leaf
    // (28 tiles -> 4, 21 -> 2, 15 -> 1), so the four waves reach the barrier together
    const int ntiles = nrb * (nrb + 1) / 2;
    const int k0 = max(0, (ntiles - 11) / 4);
    if (w == 0) {
      if (PH & 4) {
        tile_update(c0 + IB, c0 + IB, c0);
        wave_lds_fence();
      }
      if (PH & 1) leaf(ib + 1);
      if (PH & 4) {
        for (int tc = ntiles - k0; tc < ntiles; ++tc) {
          int ti, tj;
          tri_tile(tc, &ti, &tj);
          tile_update(c0 + IB + ti * IB, c0 + IB + tj * IB, c0);
        }
      }
    } else if (PH & 4) {
      const int wu = __builtin_amdgcn_readfirstlane(w);  // wave-uniform: scalar tile walk
      for (int t = wu; t < ntiles - k0; t += 6) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int tc = t + 3 * u;
          if (tc >= ntiles - k0) break;
          int ti, tj;
          tri_tile(tc, &ti, &tj);
          tile_update(c0 + IB + ti * IB, c0 + IB + tj * IB, c0);
        }
      }
    }
    if (Li && w > 0) {
      // Dinv_ib (L_ib,ib final since leaf(ib)); block row ib - 1 (Dinv_{ib-1} from last pass)
      if (w == 1) dinv_block(ib);
      else
        for (int J = w - 2; J < ib - 1; J += 2) linv_block(ib - 1, J);
    }
    __syncthreads();
    if (ib == 0 || ib == 3 || ib == 6) pstamp(ib == 0 ? 1 : ib == 3 ? 2 : 3);
  }
  pstamp(4);
  if (Li) {
    // remaining: Dinv_7 with block row 6, then block row 7
    constexpr int L7 = NB / IB - 1;
    if (w == 0) dinv_block(L7);
    else
      for (int J = w - 1; J < L7 - 1; J += 3) linv_block(L7 - 1, J);
    __syncthreads();
    pstamp(5);
    for (int J = w; J < L7; J += 4) linv_block(L7, J);
    pstamp(6);
  }
#undef LI
  // inverses of the eight 16x16 diagonal blocks: wave w builds blocks w and w + 4,
  // lane c (< 16) column c by forward substitution; dinv[ib][r][c] = X[r][c]
  // (not needed with Li: the caller uses the full inverse)
#pragma unroll
  for (int h = 0; h < (Li ? 0 : 2); ++h) {
    const int ib = w + 4 * h, c0 = ib * IB;
    double x[IB];
#pragma unroll
    for (int r = 0; r < IB; ++r) {
      double sacc = (li == r) ? 1.0 : 0.0;
#pragma unroll
      for (int q = 0; q < r; ++q) sacc = fma(-MS(c0 + r, c0 + q), x[q], sacc);
      x[r] = sacc * ipv[c0 + r];
    }
    if (lane < IB) {
#pragma unroll
      for (int r = 0; r < IB; ++r) {
        dinv[(ib * IB + r) * IB + lane] = x[r];
      }
    }
  }
  // block store (lower triangle incl. diagonal)
  if ((PH & 8) && !(PH & 64)) {
#pragma unroll 8
    for (int u = 0; u < 32; ++u) {
      const int idx = tid + 256 * u, r = idx >> 6, c2 = idx & 63;
      if (2 * c2 <= r) {
        double2 v;
        v.x = MS(r, 2 * c2);
        v.y = MS(r, 2 * c2 + 1);  // past the diagonal: scratch (the upper triangle is unused)
        *reinterpret_cast<double2*>(&A[(kb + r) * lda + kb + 2 * c2]) = v;
      }
    }
  }
  pstamp(7);
  // logdet partial = 1/2 sum log(pivot) over real pivots; first non-positive pivot
  double lg = 0.0;
  int bad = STATUS_NONE;
  if (tid < NB && kb + tid < npiv) {
    const double dp = pvs[tid];
    lg = 0.5 * log(dp);
    if (!(dp > 0.0)) bad = (int)(kb + tid);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lg += __shfl_xor(lg, o);
    bad = min(bad, __shfl_xor(bad, o));
  }
  if (lane == 0) {
    red[w] = lg;
    redi[w] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    parts[k] = red[0] + red[1] + red[2] + red[3];
    const int b = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
    if (b != STATUS_NONE) atomicMin(status, b);
  }
#undef MS
}

// out[k][j] = Linv[j][k] (the transposed inverse of the factored block: upper triangular,
// zeros below the diagonal), ld ldo, from Li (packed 16x16 blocks, built by potrf_block).
template <bool COH = false>
__device__ __forceinline__ void store_inverse_t(const double* __restrict__ Li,
                                                double* __restrict__ out, int64_t ldo) {
#define LI(r, q) Li[((((r) >> 4) * (((r) >> 4) + 1) / 2) + ((q) >> 4)) * (IB * (IB + 1)) + \
                    ((r) & 15) * (IB + 1) + ((q) & 15)]
  __syncthreads();
#pragma unroll 8
  for (int u = 0; u < NB * (NB / 2) / 256; ++u) {
    const int idx = threadIdx.x + 256 * u;
    const int k = idx / (NB / 2), j = 2 * (idx % (NB / 2));
    double2 v;
    v.x = j >= k ? LI(j, k) : 0.0;
    v.y = j + 1 >= k ? LI(j + 1, k) : 0.0;
    if (COH) {
      st2_wt(out, (unsigned)((k * ldo + j) * 8), v.x, v.y);
    } else {
      *reinterpret_cast<double2*>(&out[k * ldo + j]) = v;
    }
  }
#undef LI
}

// (256, 4): at most 128 VGPRs, so the factor fits in the registers one bulk-SYRK workgroup frees
// The block lives in dynamic LDS (MB_DOUBLES doubles, set at launch) so the occupancy target
// (4 waves / SIMD) holds at compile time and caps the kernel at 128 VGPRs.
template <int PH>
__global__ __launch_bounds__(256, 4) void potrf_diag_kernel(double* __restrict__ A, int64_t lda,
                                                           int64_t kb, int64_t npiv,
                                                           double* __restrict__ dinv,
                                                           double* __restrict__ parts, int k,
                                                           int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double Mb[];
  __builtin_amdgcn_s_setprio(3);  // critical path: win issue slots over co-resident SYRK waves
  potrf_block<PH>(Mb, A, lda, kb, npiv, dinv, parts, k, status);
}

// ------------------------------------------------------------ trsm (v2)
// Rows [s, Mp) of block column kb, 64 rows per workgroup, 16 rows per wave:
//   X_cb = (A_cb - sum_{q < cb} X_q L_{cb,q}^T) * Dinv_cb^T,  cb = 0..7 (16 columns each).
// The wave's rows live in LDS; the L_{cb,q} fragments (the factored diagonal block, shared
// by every workgroup, L2-resident) for column block cb+1 are loaded while cb computes,
// and the K chain is split over two accumulators.
// The solve proper on 64 rows already in LDS (sA, visible to every wave of the workgroup).
__device__ __forceinline__ void trsm_rows(double (*__restrict__ sA)[NB + 1],
                                          double* __restrict__ A, int64_t lda, int64_t r0,
                                          int64_t kb, const double* __restrict__ dinv) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int wr = w * IB;
  const double* Lrow = A + (kb + li) * lda + kb + lk;  // L[li][lk]
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
        bf[nxt][st] = Lrow[(int64_t)(cb + 1) * IB * lda + st * 4];
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
    double4v z = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < IB / 4; ++ks) z = mfma16(sA[wr + li][cb * IB + ks * 4 + lk], dv[cur][ks], z);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[wr + lk + 4 * r][cb * IB + li] = z[r];
    wave_lds_fence();
  }
  // the wave's 16 rows back to HBM
  for (int idx = lane; idx < IB * (NB / 2); idx += 64) {
    const int r = idx / (NB / 2), q2 = idx - r * (NB / 2);
    double2 v;
    v.x = sA[wr + r][2 * q2];
    v.y = sA[wr + r][2 * q2 + 1];
    *reinterpret_cast<double2*>(&A[(r0 + wr + r) * lda + kb + 2 * q2]) = v;
  }
}

__global__ __launch_bounds__(256) void trsm_kernel_v2(double* __restrict__ A, int64_t lda, int64_t s,
                                                   int64_t kb, const double* __restrict__ dinv) {
  __shared__ double sA[64][NB + 1];
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  const int64_t r0 = s + (int64_t)blockIdx.x * 64;
  for (int idx = tid; idx < 64 * (NB / 2); idx += 256) {
    const int r = idx / (NB / 2), q2 = idx - r * (NB / 2);
    const double2 v = *reinterpret_cast<const double2*>(&A[(r0 + r) * lda + kb + 2 * q2]);
    sA[r][2 * q2] = v.x;
    sA[r][2 * q2 + 1] = v.y;
  }
  trsm_rows(sA, A, lda, r0, kb, dinv);
}

// ----------------------------------------------------------------- syrk
// Trailing update of the lower triangle: for 128x128 tiles (ti >= tj) of rows/cols
// starting at s:  C[i][j] -= sum_q P[i][q] P[j][q],  P = A[:, kb:kb+NB].
// 4 waves as 2x2, each a 64x64 block of C held in registers. The product runs on
// v_mfma_f64_4x4x4_4b_f64 (72.7 TFLOP/s measured on MI355X, against 49 for
// v_mfma_f64_16x16x4_f64; scripts/probe_mfma.py). Lane maps (scripts/probe_mfma4_layout.py),
// with g = (lane >> 2) & 3 the block: A_g[i][k] at lane 16k + 4g + i, B_g[k][j] at lane
// 16k + 4g + j, D_g[i][j] at lane 16i + 4g + j. A is replicated over the four blocks
// (rows ir*4 + i) and each block owns 4 of 16 columns (jr*16 + 4g + j), so accumulator
// acc[ir][jr] holds C[ir*4 + (lane >> 4)][jr*16 + (lane & 15)]: 16 consecutive columns per
// 16 lanes, as the 16x16 layout. Per K step of 4: 16 A + 4 B fragments, 64 MFMAs.
// The K dimension (NB) is staged KB columns at a time through LDS, the next stage
// prefetched into registers while the current one feeds the MFMAs.
// mode 0: every lower tile; 1: only tile column 0 (the next block column, look-ahead);
// 2: every lower tile with tile column >= 1 (the rest).
// KD: depth of the update (columns kb .. kb+KD of A). CIO = false (diagnostics only) skips
// the C tile's HBM read and write.
// Lower tiles (tile row ti >= tile column tj, 128-wide tile columns) of the trailing matrix
// starting at row/column s, restricted to tile columns [tj_lo, tj_hi); T tile rows in all.
// Bands of at most 8 columns (look-ahead / in-panel updates) are enumerated column by
// column; otherwise tj_hi must be T and the band is a triangle. Update depth kd (multiple
// of KB): columns kb .. kb + kd of A. TR = tile rows (128, or 64 for latency-critical bands).
// DB: double-buffered LDS stages (one barrier per K step instead of two).
// The product itself is gemm_accumulate (lfm_chol_dev.h).

// gemm_accumulate on v_mfma_f64_16x16x4_f64: the same staging and the same products, acc as
// TR / 32 x 4 blocks of 16 x 16 (acc[rb][jr][r] = C[wr + 16 rb + 4 r + (lane >> 4)][wc + 16 jr
// + (lane & 15)] — element for element the map of gemm_accumulate's acc[4 rb + r][jr]). Per
// 4-deep k step a wave issues 2 TR / 64 A and 4 B fragment reads and 2 TR / 16 MFMAs of 2048
// flops (against 12 reads and 32 MFMAs of 512 flops on the 4x4x4 blocks).
template <int TR, bool BT = false, bool COH = false, int KS = KB, int CW = ST>
__device__ __forceinline__ void gemm_accumulate16(const double* __restrict__ pi, int64_t ldi,
                                                  const double* __restrict__ pj, int64_t ldj,
                                                  int kd, double4v (&acc)[TR / 32][CW / 32],
                                                  double (*__restrict__ sP)[KS + LDP]) {
  constexpr int RB = TR / 32, JB = CW / 32;  // 16 x 16 blocks per wave: RB rows, JB columns
  constexpr int CPR = CW / 2;                 // K-major j panel: double2 chunks per k row
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: lane offsets are recomputed, not held live
  const int lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * (TR / 2), wc = (w & 1) * (CW / 2);
  const int li = lane & 15, lk = lane >> 4;
  static_assert(KS % 16 == 0 && KS <= 64, "stage depth");
  constexpr int CH = KS / 2, RP = 256 / CH;
  constexpr int NUI = TR / RP, NUJ = CW / RP, NU = NUI + NUJ;
  static_assert(BT ? KS * CPR == 256 * NUJ : true, "K-major staging");
  const int srow = tid / CH, sch = tid % CH;
  const double* gi = pi + srow * ldi + 2 * sch;
  const double* gj = BT ? pj + (tid / CPR) * ldj + 2 * (tid % CPR) : pj + srow * ldj + 2 * sch;
  const int li32 = (int)(RP * ldi);
  const int lj32 = BT ? (int)((256 / CPR) * ldj) : (int)(RP * ldj);
  double2 pre[NU];
  auto gload = [&](int k0) {
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
        const int kr = tid / CPR + (256 / CPR) * u, jc = 2 * (tid % CPR);
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
#pragma unroll 1
    for (int kk = 0; kk < KS; kk += 4) {
      double bb[JB], a[RB];
#pragma unroll
      for (int jr = 0; jr < JB; ++jr) bb[jr] = sP[TR + wc + jr * 16 + li][kk + lk];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) a[rb] = sP[wr + rb * 16 + li][kk + lk];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int jr = 0; jr < JB; ++jr) acc[rb][jr] = mfma16(a[rb], bb[jr], acc[rb][jr]);
    }
  }
}

// C tile loads of the trailing update: device-coherent or nontemporal (the C stores likewise)
template <bool COH>
__device__ __forceinline__ double ldc(const double* p) {
  if (COH) return ld1<true>(p);
  return __builtin_nontemporal_load(p);
}

// The tile body of syrk_unit: C (TR x 128 at row i0, column j0) -= panel rows i0.. x rows j0..
// over depth kd; CLOAD = false: C starts from zero (not read).
// GEN: C is not read but generated from the gram tables (GramGen, a tile inside one gene pair
// of an aligned grid layout): the tile's Toeplitz windows and row / column tables staged in
// sP first, then gram_grid_aligned_kernel's arithmetic per element (bit-identical Sigma).
template <bool CIO, int TR, int KS, bool LDCOH, bool CLOAD, bool GEN = false>
__device__ __forceinline__ void syrk_tile(double* __restrict__ A, int64_t lda, Panel P, int kd,
                                          int64_t i0, int64_t j0, bool diag, bool coh,
                                          double (*__restrict__ sP)[KS + LDP],
                                          const GramGen* gen = nullptr) {
  constexpr int IRN = TR / 8;  // 4-row groups per wave (2 x 2 waves, TR/2 rows each)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * (TR / 2), wc = (w & 1) * 64;
  const int li = lane & 15, lk = lane >> 4;
  double* Cb = A + (i0 + wr + lk) * lda + j0 + wc + li;  // C[wr + lk][wc + li]
  const int ld4 = (int)(4 * lda);  // row-group stride (elements); 60 * ld4 < 2^31 for lda < 2^23

  double4v acc4[IRN / 4][4];
#define ACC(ir, jr) acc4[(ir) >> 2][jr][(ir) & 3]
  if constexpr (GEN) {
    constexpr int WIN = ST + TR - 1;
    static_assert(4 * WIN + 3 * TR + 3 * ST <= (TR + ST) * (KS + LDP), "gram windows in sP");
    double* sWk = &sP[0][0];
    double* sXk = sWk + WIN;
    double* sWj = sXk + WIN;
    double* sXj = sWj + WIN;
    double* sPk = sXj + WIN;  // rows: Pt[k][tau], Et[j][tau], Qt[j][tau]
    double* sEj = sPk + TR;
    double* sQj = sEj + TR;
    double* sPj = sQj + TR;   // columns: Pt[j][tau'], Et[k][tau'], Qt[k][tau']
    double* sEk = sPj + ST;
    double* sQk = sEk + ST;
    const int Tn = gen->Tn, G = gen->G;
    const int64_t Wd = 2 * (int64_t)Tn - 1;
    const double* Wt = gen->tab;
    const double* Xt = Wt + (int64_t)G * Wd;
    const double* Pt = Xt + (int64_t)G * Wd;
    const double* Et = Pt + (int64_t)G * Tn;
    const double* Qt = Et + (int64_t)G * Tn;
    const double* Cm = Qt + (int64_t)G * Tn;
    const int j = gen->bg[i0 / Tn], k = gen->bg[j0 / Tn];
    const int tau0 = (int)(i0 % Tn), tp0 = (int)(j0 % Tn);
    const int dmin = tp0 - tau0 - (TR - 1);
    for (int e = tid; e < WIN; e += 256) {
      const int64_t d = dmin + e;
      sWk[e] = Wt[(int64_t)k * Wd + (Tn - 1) + d];
      sXk[e] = Xt[(int64_t)k * Wd + (Tn - 1) + d];
      sWj[e] = Wt[(int64_t)j * Wd + (Tn - 1) - d];
      sXj[e] = Xt[(int64_t)j * Wd + (Tn - 1) - d];
    }
    if (tid < TR) {
      sPk[tid] = Pt[(int64_t)k * Tn + tau0 + tid];
      sEj[tid] = Et[(int64_t)j * Tn + tau0 + tid];
      sQj[tid] = Qt[(int64_t)j * Tn + tau0 + tid];
    }
    if (tid < ST) {
      sPj[tid] = Pt[(int64_t)j * Tn + tp0 + tid];
      sEk[tid] = Et[(int64_t)k * Tn + tp0 + tid];
      sQk[tid] = Qt[(int64_t)k * Tn + tp0 + tid];
    }
    const double Cjk = Cm[(int64_t)j * G + k];
    __syncthreads();
#pragma unroll
    for (int ir = 0; ir < IRN; ++ir)
#pragma unroll
      for (int jr = 0; jr < 4; ++jr) {
        const int rl = wr + ir * 4 + lk, cl = wc + jr * 16 + li, e = cl - rl + (TR - 1);
        double v = sWk[e] + sWj[e];
        v = fma(-sXk[e], sPk[rl], v);
        v = fma(-sXj[e], sPj[cl], v);
        v = fma(-(sEk[cl] * sEj[rl]), sQk[cl] + sQj[rl], v);
        v = Cjk * v;
        if (i0 + rl == j0 + cl) v = (v + gen->da1) + gen->da2;
        ACC(ir, jr) = -v;
        if (jr == 3) __builtin_amdgcn_sched_barrier(0);  // one row group's reads at a time
      }
    __syncthreads();  // the windows are read: sP is the K stages' again
  } else {
#pragma unroll
    for (int ir = 0; ir < IRN; ++ir)
#pragma unroll
      for (int jr = 0; jr < 4; ++jr)
        ACC(ir, jr) = (CIO && CLOAD) ? -ldc<LDCOH>(&Cb[ir * ld4 + jr * 16]) : 0.0;
  }
  gemm_accumulate16<TR, false, LDCOH, KS>(P.p + (i0 - P.r0) * P.ld, P.ld,
                                          P.p + (j0 - P.r0) * P.ld, P.ld, kd, acc4, sP);

  int ld4s = ld4;
  asm volatile("" : "+v"(ld4s));  // recompute store addresses instead of keeping 64 pointers live
#pragma unroll
  for (int ir = 0; ir < IRN; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) {
      const int64_t row = i0 + wr + ir * 4 + lk, col = j0 + wc + jr * 16 + li;
      if (CIO && (!diag || col <= row)) {
        // coh: device-coherent (write-through) stores, read by another XCD in flight
        if (coh)
          __hip_atomic_store(&Cb[ir * ld4s + jr * 16], -ACC(ir, jr), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        else
          __builtin_nontemporal_store(-ACC(ir, jr), &Cb[ir * ld4s + jr * 16]);
      }
      if (!CIO && ACC(ir, jr) == 1.2345e300) Cb[0] = 0.0;  // keep the MFMAs live
    }
#undef ACC
}

// Unit b of a band / triangle enumeration -> (TR-row slab ti, 128-column tile tj), relative
// to the trailing matrix: tile columns [tj_lo, tj_hi), tile rows from ti0 (bands) / the
// triangle over tile columns [tj_lo, T). Host mirror of the triangle: rest_unit_tile
// (lfm_host.cpp).
template <int TR>
__device__ __forceinline__ void unit_tile(int T, int tj_lo, int tj_hi, int64_t b, int ti0,
                                          int* ti_out, int* tj_out) {
  constexpr int SUB = ST / TR;  // row tiles per 128 rows
  int ti, tj;  // ti in TR-row units
  if (tj_hi - tj_lo <= kBandMaxCols && ti0 >= tj_hi) {
    // rectangular band (every row below the band's columns): row by row, so consecutive units
    // share a row panel and the band's few column panels stay in L2
    const int nb = tj_hi - tj_lo;
    const int64_t r = b / (nb * SUB);
    const int rem = (int)(b - r * nb * SUB);
    tj = tj_lo + rem / SUB;
    ti = SUB * (ti0 + (int)r) + rem % SUB;
  } else if (tj_hi - tj_lo <= kBandMaxCols) {
    // band: tile columns [tj_lo, tj_hi), tile rows max(tj, ti0) .. T - 1
    tj = tj_lo;
    while (b >= (int64_t)SUB * max(0, T - max(tj, ti0))) {
      b -= (int64_t)SUB * max(0, T - max(tj, ti0));
      ++tj;
    }
    ti = SUB * max(tj, ti0) + (int)b;
  } else {
    // triangle of 128-tiles over tile columns [tj_lo, T), SUB row slabs of TR rows per tile;
    // groups of SUPERTILE tile rows are enumerated in order (so a launch can skip the first
    // ones: b offset), within a group Q x Q supertiles in turn, tiles row by row within those:
    // consecutive units (one XCD's co-resident workgroups) then share row and column panels
    const int sub = (int)(b % SUB);
    b /= SUB;
    int a = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((int64_t)(a + 1) * (a + 2) / 2 <= b) ++a;
    while ((int64_t)a * (a + 1) / 2 > b) --a;
    constexpr int Q = SUPERTILE;
    if constexpr (Q > 1) {
      const int R = a / Q, r0 = R * Q, qr = min(Q, T - tj_lo - r0);
      const int64_t off = b - (int64_t)r0 * (r0 + 1) / 2;
      const int64_t full = (int64_t)R * qr * Q;
      int lr, lc;
      if (off < full) {
        const int C = (int)(off / (qr * Q)), t = (int)(off % (qr * Q));
        lr = t / Q;
        lc = C * Q + t % Q;
      } else {
        const int d = (int)(off - full);
        lr = (int)((sqrt(8.0 * (double)d + 1.0) - 1.0) * 0.5);
        while ((lr + 1) * (lr + 2) / 2 <= d) ++lr;
        while (lr * (lr + 1) / 2 > d) --lr;
        lc = r0 + d - lr * (lr + 1) / 2;
      }
      tj = lc + tj_lo;
      ti = SUB * (r0 + lr + tj_lo) + sub;
    } else {
      tj = (int)(b - (int64_t)a * (a + 1) / 2) + tj_lo;
      ti = SUB * (a + tj_lo) + sub;
    }
  }
  *ti_out = ti;
  *tj_out = tj;
}

// One TR x 128 work unit of a band / triangle launch: C -= P_i P_j^T over panel depth kd,
// C the lower part of the trailing matrix of A starting at row / column s. b = the unit's
// index in the enumeration (unit_tile).
// Returns whether the unit's tile lies in the leading coh_lim x coh_lim tiles of the trailing
// matrix (stores then write through to memory: device-coherent, for an in-flight reader).
// LDCOH: C and panel loads device-coherent too (a reader of data written in the same launch).
template <bool CIO, int TR, bool COH = false, int KS = KB, bool LDCOH = false>
__device__ __forceinline__ bool syrk_unit(double* __restrict__ A, int64_t lda, int64_t s, Panel P,
                                          int kd, int T, int tj_lo, int tj_hi, int64_t b, int ti0,
                                          double (*__restrict__ sP)[KS + LDP], int coh_lim = 0,
                                          int64_t pad_after = INT64_MAX,
                                          int64_t pad_end = INT64_MAX,
                                          int64_t zero_from = INT64_MAX,
                                          const GramGen* gen = nullptr) {
  int ti, tj;  // ti in TR-row units
  unit_tile<TR>(T, tj_lo, tj_hi, b, ti0, &ti, &tj);

  const int64_t i0 = s + (int64_t)ti * TR, j0 = s + (int64_t)tj * ST;
  const bool diag = i0 < j0 + ST;  // the tile reaches the diagonal: keep col <= row only
  const bool in_lead = (i0 - s) / ST < coh_lim && (j0 - s) / ST < coh_lim;
  // rows in (pad_after, pad_end) are identity padding of the augmented matrix (their panel
  // entries are zero): nothing reads their update
  if (i0 > pad_after && i0 < pad_end && !in_lead) return false;
  const bool coh = COH || in_lead;
  // rows >= zero_from are zeros no update has written yet (the bordered matrix's border rows
  // entering the window; never initialised in memory): a tile body that does not load C. (A
  // per-element load-or-zero choice makes hipcc branch around every load and wait on each, +7 %
  // per evaluation; a selected base pointer costs 2 VGPRs, occupancy 4 -> 3 waves / SIMD.)
  if (i0 >= zero_from)
    syrk_tile<CIO, TR, KS, LDCOH, false>(A, lda, P, kd, i0, j0, diag, coh, sP);
  else if (gen && i0 + TR <= gen->n)
    syrk_tile<CIO, TR, KS, LDCOH, false, true>(A, lda, P, kd, i0, j0, diag, coh, sP, gen);
  else
    syrk_tile<CIO, TR, KS, LDCOH, true>(A, lda, P, kd, i0, j0, diag, coh, sP);
  return in_lead;
}

// XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so
// XCD x is given the contiguous range [lo_x, hi_x) of the enumeration: the workgroups resident
// on one XCD then share panel rows instead of striding over them.
__device__ __forceinline__ void xcd_range(int64_t nunits, int x, int64_t* lo, int64_t* hi) {
  const int64_t q = nunits / 8, r = nunits % 8;
  *lo = x * q + min((int64_t)x, r);
  *hi = *lo + q + (x < r ? 1 : 0);
}

// Trailing update (mode by tile-column range, see syrk_unit); skip: units of the triangle
// enumeration left out at its start (tile rows already updated elsewhere).
template <bool CIO, int TR>
__global__ __launch_bounds__(256, TR == 64 ? SLAB_WGS : 2) void syrk_kernel(
    double* __restrict__ A, int64_t lda, int64_t s, Panel P, int kd, int T, int tj_lo, int tj_hi,
    int prio, int xcd_remap, int ti0, int64_t skip) {
  __shared__ double sP[TR + ST][KB + LDP];
  if (prio) __builtin_amdgcn_s_setprio(2);  // look-ahead bands: ahead of the bulk update
  int64_t b = blockIdx.x;
  if (xcd_remap && tj_hi - tj_lo > 8) {
    int64_t lo, hi;
    xcd_range(gridDim.x, (int)(b % 8), &lo, &hi);
    b = lo + b / 8;
  }
  syrk_unit<CIO, TR>(A, lda, s, P, kd, T, tj_lo, tj_hi, b + skip, ti0, sP);
}

// Device-side waits are bounded in TIME, on the 100 MHz constant clock (s_memrealtime), not
// in polls: `limit` ticks (ctx->knobs.wait_ticks, LFM_DEVICE_WAIT_MS; 2 s by default), so a wait
// starved by another tenant of the GPU ends after a known time whatever the poll rate, and the
// call re-runs on schedule 1 (lfm_ctx.hip). limit = 0 fails at once (the LFM_DEBUG_SPIN_LIMIT
// test knob). A wait also ends as soon as another wait of the call has recorded a timeout
// (`status`), so one stall drains the whole factorisation within one bound.
__device__ __forceinline__ unsigned long long wall_ticks() { return __builtin_amdgcn_s_memrealtime(); }

// Bounded relaxed / acquire spin on a device counter: true once *p >= target, false after
// `limit` ticks or once *status records a timeout (the caller records PANEL_TIMEOUT).
template <bool ACQ = true, int SLEEP = 2>
__device__ __forceinline__ bool spin_until(const unsigned* p, unsigned target, unsigned limit,
                                           const int* status = nullptr) {
  auto ready = [&] {
    return __hip_atomic_load(p, ACQ ? __ATOMIC_ACQUIRE : __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT) >= target;
  };
  if (ready()) return true;
  if (limit == 0) return false;
  const unsigned long long t0 = wall_ticks();
  for (unsigned it = 1; !ready(); ++it) {
    if ((it & 15) == 0) {
      if (wall_ticks() - t0 > limit) return false;
      if (status &&
          __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == PANEL_TIMEOUT)
        return false;
    }
    __builtin_amdgcn_s_sleep(SLEEP);
  }
  return true;
}

// One main-stream launch per super-panel step s (schedule 3): step s's trailing update from
// X_s (the next diagonal block excluded: chain_kernel applies it), then X_{s+1}. Roles of
// 64 x 128 units in blockIdx order (each segment padded to a multiple of 8 workgroups,
// XCD-contiguous within it):
//   ahead the next super-panel's columns below its diagonal block; each unit bumps
//         a_done[tile row]
//   rest  the remaining trailing triangle (optionally split around the tall units)
//   tall  X_{s+1} = A21 Bd_{s+1} for the rows below the next diagonal block: a unit waits for
//         the side stream's factor (chain_done) and for its rows' `ahead` units.
// Workgroups are dispatched in order per XCD, so a waiting `tall` unit never holds a slot an
// unfinished `ahead` unit of its XCD still needs; waits are bounded (status PANEL_TIMEOUT).
// Its arguments: StepArgs (lfm_chol.h).

// Diagnostics: atomic max of the 100 MHz clock (or of its bitwise NOT: the earliest start)
__device__ __forceinline__ void stamp_max(unsigned long long* p, bool negate = false) {
  if (p && threadIdx.x == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __hip_atomic_fetch_max(p, negate ? ~t : t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Unit of workgroup b (offset within its role's segment) of a step launch: *u, and *end (u >=
// *end: padding). Ahead and rest units are dealt to the XCDs in contiguous ranges (panel
// sharing in each XCD's L2); the tall units round-robin, so every XCD gets the same mix of
// depths, deepest first (contiguous ranges gave one XCD all the deepest column block and made
// it the launch's last by a whole unit: profiles/r03_unit_trace_*).
__device__ __forceinline__ void tall_or_xcd_range(int seg, int64_t cnt, int64_t b, int64_t* u,
                                                  int64_t* end) {
  if (seg == 2) {
    // workgroup b runs on XCD x = b % 8 at position p = b / 8 of its queue: group j = (p / S)
    // 8 + x, piece p % S (the segment is padded to 8 S workgroups: lfm_host.h tall_grid)
    constexpr int S = TALL_SPLIT;
    const int64_t p = b / 8;
    *u = S * ((p / S) * 8 + b % 8) + p % S;
    *end = cnt;
    return;
  }
  int64_t lo, hi;
  xcd_range(cnt, (int)(b % 8), &lo, &hi);
  *u = lo + b / 8;
  *end = hi;
}

__device__ __forceinline__ void bump_after_stores(unsigned* ctr) {
  __builtin_amdgcn_s_waitcnt(0);  // this thread's write-through stores have completed
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


// tall unit u (row slab rb, column block cb, its part hf of TALL_SPLIT) of step s + 1:
// deepest column blocks first (longest units), so the launch ends on short ones; the split
// halves a unit's width so the launch's last round drains in shorter pieces
// Returns false when its device-side wait ran out (the workgroup then stops claiming units).
__device__ __forceinline__ bool tall_unit(const StepArgs& g, int64_t u, double (*sP)[KB + LDP],
                                          unsigned long long* const st,
                                          unsigned long long t_unit) {
  auto add_dur = [&](int slot) {
    if (threadIdx.x == 0)
      __hip_atomic_fetch_add(st + slot, __builtin_amdgcn_s_memrealtime() - t_unit,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  constexpr int TCW = NB / TALL_SPLIT;  // output columns per tall unit
  const int64_t nrb = g.nt / (g.tw * TALL_SPLIT);
  const int cb = g.tw - 1 - (int)(u / (nrb * TALL_SPLIT));
  const int64_t rq = u % (nrb * TALL_SPLIT);
  const int64_t rb = rq / TALL_SPLIT;
  const int c0 = cb * NB + (int)(rq % TALL_SPLIT) * TCW;  // first output column in X_{s+1}
  const int64_t i0 = g.tr0 + rb * 64;
  if (i0 > g.n && i0 < g.pad_end) return true;  // identity padding rows: their X is never read
  {
    __shared__ int ok;
    // relaxed polling and device-coherent operand loads below instead of an acquire fence:
    // an agent-scope acquire invalidates this XCD's L2 under the running bulk units
    if (threadIdx.x == 0) {
      int why = 0;
      bool good = !g.chain_done || spin_until<false>(g.chain_done, 1u, g.spin, g.status);
      if (!good) why = 1;
      // rows past step s's update (bordered: the border rows that entered the window with
      // super-panel s + 1, zero in every earlier panel column) have no ahead unit to wait for
      if (good && g.a_done && (i0 - g.s0) / ST < g.T) {
        good = spin_until<false>(&g.a_done[(i0 - g.s0) / ST], (unsigned)(2 * g.wn), g.spin,
                                 g.status);
        if (!good) why = 2;
      }
      if (!good) timeout_at(g.status, why);
      ok = good;
    }
    __syncthreads();
    if (!ok) return false;
    if (st) stamp_max(st + 2);
  }
  const int W = g.tw * NB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (i0 >= g.copy_from) {
    // border rows: X = e_{row - copy_from} Bd, the row of Bd (written through by the chain)
    const double* src = g.Bd + (i0 - g.copy_from) * W + c0;
    double* dst = g.X + (i0 - g.tr0) * W + c0;
#pragma unroll 4
    for (int u = 0; u < 64 * TCW / 2 / 256; ++u) {
      const int idx = tid + 256 * u, r = idx / (TCW / 2), c2 = 2 * (idx % (TCW / 2));
      *reinterpret_cast<double2*>(&dst[r * W + c2]) = ld2<true>(&src[(int64_t)r * W + c2]);
    }
    if (st) {
      __syncthreads();
      stamp_max(st + 3);
      add_dur(6);
    }
    return true;
  }
  const int wr = (wv >> 1) * 32, wc = (wv & 1) * (TCW / 2);
  const int li = lane & 15, lk = lane >> 4;
  constexpr int JR = TCW / 32;  // 16-column blocks per wave
  double4v acc4[2][JR];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int jr = 0; jr < JR; ++jr) acc4[rb][jr] = (double4v){0.0, 0.0, 0.0, 0.0};
  gemm_accumulate16<64, true, true, KB, TCW>(g.A + i0 * g.lda + g.tk0, g.lda, g.Bd + c0, W,
                                             NB * (cb + 1), acc4, sP);
#define ACC(ir, jr) acc4[(ir) >> 2][jr][(ir) & 3]
  double* Xb = g.X + (i0 - g.tr0 + wr + lk) * W + c0 + wc + li;
#pragma unroll
  for (int ir = 0; ir < 8; ++ir)
#pragma unroll
    for (int jr = 0; jr < JR; ++jr) {
      Xb[(ir * 4) * W + jr * 16] = ACC(ir, jr);
      if (i0 + wr + ir * 4 + lk == g.n) g.zvec[g.tk0 + c0 + wc + jr * 16 + li] = ACC(ir, jr);
    }
#undef ACC
  if (st) {
    __syncthreads();
    stamp_max(st + 3);
    add_dur(6);
  }
  return true;
}

// ran (diagnostics, NULL: off): thread 0 records role << 32 | unit of the unit it runs
template <int TR>
__device__ __forceinline__ void step_body(const StepArgs& g, unsigned long long* ran = nullptr) {
  constexpr int SUB = ST / TR;  // units per 128-row tile
  __shared__ double sPbuf[(64 + ST) * (STEP_KS + LDP)];
  double (*sP)[KB + LDP] = reinterpret_cast<double (*)[KB + LDP]>(sPbuf);
  double (*sPu)[STEP_KS + LDP] = reinterpret_cast<double (*)[STEP_KS + LDP]>(sPbuf);
  const int64_t b = blockIdx.x;
  // roles in blockIdx order: ahead (1), rest (2), tall (3), each padded to a multiple of 8
  const int cnt[3] = {g.na, g.nr, g.nt};
  const int64_t width[2] = {pad8(g.na), pad8(g.nr)};
  int seg = 0;
  int64_t base = 0;
  while (seg < 2 && b >= base + width[seg]) {
    base += width[seg];
    ++seg;
  }
  int64_t lo, hi;
  tall_or_xcd_range(seg, cnt[seg], b - base, &lo, &hi);
  const int64_t u = lo;
  if (u >= hi) return;
  const int role = seg + 1;
  if (ran && threadIdx.x == 0) *ran = ((unsigned long long)role << 32) | (unsigned long long)u;
  unsigned long long* const st = g.stamps;
  if (st) stamp_max(st, true);
  // diagnostics: summed unit durations per role (rest [5], tall [6], ahead [7]; 100 MHz)
  const unsigned long long t_unit = st ? __builtin_amdgcn_s_memrealtime() : 0;
  auto add_dur = [&](int slot) {
    if (threadIdx.x == 0)
      __hip_atomic_fetch_add(st + slot, __builtin_amdgcn_s_memrealtime() - t_unit,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  if (role == 1) {
    // device-coherent stores + a counter bump once they have completed: the tall units read
    // these rows with device-coherent loads (no L2 writeback / invalidate on either side)
    syrk_unit<true, TR, true, STEP_KS>(g.A, g.lda, g.s0, g.px, g.kd, g.T, 0, g.wn, u, g.wn, sPu,
                                       0, g.n, g.pad_end, g.zero_from,
                                       g.gen.tab ? &g.gen : nullptr);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    // 128-tile row of the unit (the band's enumeration order, syrk_unit)
    const int trow = g.wn + (int)(u / (SUB * g.wn));
    if (threadIdx.x == 0 && g.a_done)
      __hip_atomic_fetch_add(&g.a_done[trow], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0 && g.xready && trow < g.wn + g.lead)
      __hip_atomic_fetch_add(g.xready, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st) {
      stamp_max(st + 1);
      stamp_max(st + 3);
      add_dur(7);
    }
    return;
  }
  if (role == 2) {
    unsigned long long c0 = 0, r0 = 0;
    if (st) {
      c0 = __builtin_amdgcn_s_memtime();
      r0 = __builtin_amdgcn_s_memrealtime();
    }
    const bool lead = syrk_unit<true, TR, false, STEP_KS>(g.A, g.lda, g.s0, g.px, g.kd, g.T,
                                                          g.wn, g.T, u + g.rest_off, 0, sPu,
                                                          g.xready ? g.wn + g.lead : 0, g.n,
                                                          g.pad_end, g.zero_from,
                                                          g.gen.tab ? &g.gen : nullptr);
    if (lead) bump_after_stores(g.xready);
    if (st) {
      __syncthreads();
      stamp_max(st + 1);
      stamp_max(st + 3);
      if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(st + 4, __builtin_amdgcn_s_memtime() - c0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(st + 5, __builtin_amdgcn_s_memrealtime() - r0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    return;
  }
  tall_unit(g, u, sP, st, t_unit);
}

// Diagnostics (lfm_debug_trace): per workgroup {entry, exit} (s_memrealtime), the hardware
// id (HW_ID | XCC_ID << 32) and the launch tag | role << 32 | unit (role 0: padding)
template <int TR>
__device__ __forceinline__ void step_traced(const StepArgs& g) {
  __shared__ unsigned long long t0;  // in LDS: nothing held in registers across the body
  __shared__ unsigned long long ran;  // role << 32 | unit (0: padding, or nothing left to claim)
  if (threadIdx.x == 0) {
    t0 = __builtin_amdgcn_s_memrealtime();
    ran = 0;
  }
  __syncthreads();
  step_body<TR>(g, &ran);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t b = blockIdx.x;
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long* r = g.trace + 4 * b;
    r[0] = t0;
    r[1] = __builtin_amdgcn_s_memrealtime();
    r[2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
    r[3] = (g.trace_tag << 40) | ran;
  }
}

// (256, 4): 128 VGPRs, 4 waves / SIMD (the zero-C tile body would otherwise take 134)
__global__ __launch_bounds__(256, 4) void step_kernel(StepArgs g) { step_body<64>(g); }
// The side-CU helper's launches (rest units only): the same body under its own name, so
// traces and counters keep the main-stream step launches apart
__global__ __launch_bounds__(256, 4) void helper_update_kernel(StepArgs g) { step_body<64>(g); }
// Both with the unit trace (lfm_debug_trace on): separate symbols, so the product kernels'
// code is the untraced body
__global__ __launch_bounds__(256, 4) void step_kernel_traced(StepArgs g) { step_traced<64>(g); }
__global__ __launch_bounds__(256, 4) void helper_update_kernel_traced(StepArgs g) {
  step_traced<64>(g);
}

// ---------------------------------------------------------- fused panel
// One block column of the look-ahead chain in one launch (w = 1 steps):
//   workgroups 0, 1   apply the pending rank-pkd update (panel columns pkb .. pkb + pkd) to the
//                     two 64-row slabs of the 128 x 128 diagonal block; workgroup 0 then waits
//                     for both and factors the block (potrf_block);
//   workgroups >= 2   each apply the pending update to 64 rows below the block, keep them in
//                     LDS, wait for the factor and solve them (trsm_rows).
// This replaces band-SYRK -> potrf -> trsm (three dependent launches) and their dispatch gaps.
// Order across workgroups: device-scope release / acquire on sync[1] (diagonal slabs written,
// +1 each) and sync[0] (factor written, = epoch). Workgroup 0 is dispatched first, so waiting
// workgroups never hold the slots it needs; a bounded wait still ends every workgroup (status
// PANEL_TIMEOUT) rather than hang.
static_assert(MB_DOUBLES >= 64 * (NB + 1) && MB_DOUBLES >= (64 + ST) * (KB + LDP), "LDS union");

__device__ __forceinline__ bool wait_counter(unsigned* p, unsigned target, unsigned limit,
                                             const int* status) {
  __shared__ int ok;
  if (threadIdx.x == 0) ok = spin_until<true>(p, target, limit, status);
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok;
}

__global__ __launch_bounds__(256) void panel_kernel(double* __restrict__ A, int64_t lda,
                                                    int64_t kb, int64_t pkb, int pkd,
                                                    int64_t npiv, double* __restrict__ dinv,
                                                    double* __restrict__ parts, int k,
                                                    int* __restrict__ status,
                                                    unsigned* __restrict__ sync, unsigned epoch,
                                                    unsigned spin) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 64;
  const int li = lane & 15, lk = lane >> 4;
  const int b = blockIdx.x;
  const int64_t i0 = b < 2 ? kb + 64 * b : kb + NB + 64 * (int64_t)(b - 2);
  double* Cb = A + (i0 + wr + lk) * lda + kb + wc + li;  // C[wr + lk][wc + li]
  const int ld4 = (int)(4 * lda);
  double acc[8][4];
#pragma unroll
  for (int ir = 0; ir < 8; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) acc[ir][jr] = -Cb[ir * ld4 + jr * 16];
  if (pkd > 0)
    gemm_accumulate<64>(A + i0 * lda + pkb, lda, A + kb * lda + pkb, lda, pkd, acc,
                        reinterpret_cast<double (*)[KB + LDP]>(smem));
  if (b < 2) {
    // diagonal slab back to the matrix (the part above the diagonal is scratch)
#pragma unroll
    for (int ir = 0; ir < 8; ++ir)
#pragma unroll
      for (int jr = 0; jr < 4; ++jr) Cb[ir * ld4 + jr * 16] = -acc[ir][jr];
    __threadfence();
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(&sync[1], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (b == 1) return;
    if (!wait_counter(&sync[1], 2u * epoch, spin, status)) {
      if (tid == 0) {
        timeout_at(status, 7);
        __hip_atomic_store(&sync[0], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    potrf_block<15>(smem, A, lda, kb, npiv, dinv, parts, k, status);
    __threadfence();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&sync[0], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // rows below the block: the solve's 64 x 129 LDS image (aliases the staging buffer)
  double (*sA)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(smem);
  __syncthreads();
#pragma unroll
  for (int ir = 0; ir < 8; ++ir)
#pragma unroll
    for (int jr = 0; jr < 4; ++jr) sA[wr + ir * 4 + lk][wc + jr * 16 + li] = -acc[ir][jr];
  if (!wait_counter(&sync[0], epoch, spin, status)) {
    if (tid == 0) timeout_at(status, 7);
    return;
  }
  trsm_rows(sA, A, lda, i0, kb, dinv);
}

// ---------------------------------------------------- schedule 3 chain (side stream)
// One launch per super-panel s on the side stream's own CUs (gridDim.x workgroups, one per
// CU, all co-resident): the whole factorisation of the diagonal block in the workspace,
// phases separated by grid barriers instead of kernel boundaries:
//   P0  Wk top = A[D] - X_{s-1}[D rows] X_{s-1}[D rows]^T (step s - 1's update of the block,
//       64 x 128 units), Wk bottom = identity
//   per block column c: potrf (workgroup 0) | panel solve of the rows below in Wk (64-row
//       units, D rows and identity rows) | update of the block's later columns (band units)
// and finally z (row n, when it falls in the block) and chain_done[s] = 1. Wk bottom ends as
// Bd = L11^{-T}, which the main stream's tall units multiply with. Its arguments: ChainArgs
// (lfm_chol.h); dynamic LDS: CHAIN_LDS, the factor block and its inverse (packed 16x16 blocks).

// Grid barrier over the chain kernel's co-resident workgroups: release, count, acquire.
// Bounded: on timeout (or a timeout already recorded in *status) it returns false at once.
__device__ __forceinline__ bool grid_sync(unsigned* bar, unsigned target, int* status,
                                          unsigned limit) {
  __shared__ int ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const bool good = spin_until<true, 1>(bar, target, limit, status);
    if (!good) timeout_at(status, 6);
    ok = good;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok;
}

// Light grid barrier: no cache maintenance. Valid when every value another workgroup wrote
// before the barrier was stored write-through (agent-scope relaxed stores) and is read after it
// with device-coherent loads: the s_waitcnt orders this thread's stores before the arrival.
__device__ __forceinline__ bool grid_sync_light(unsigned* bar, unsigned target, int* status,
                                                unsigned limit) {
  __shared__ int ok;
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool good = spin_until<false, 1>(bar, target, limit, status);
    if (!good) timeout_at(status, 6);
    ok = good;
  }
  __syncthreads();
  return ok;
}


constexpr int CKS = 64;  // chain kernel GEMM stage depth
static_assert(2 * MB_DOUBLES >= (64 + ST) * (CKS + LDP), "chain LDS union");

// Small-tile GEMM for the chain's latency-bound phases: one 32 x 32 output tile per
// workgroup, so a 128-row block spreads over 16 workgroups instead of two 64 x 128 units
// (one CU's fp64 MFMA rate is 1/256 of the chip's: a 64 x 128 x 128 unit alone is ~7 us).
//   v[q] = sum_{k < kd} P[r][k] Q[k][c],  element (r, c) = ((tid + 256 q) >> 5, & 31)
// P: row-major, k contiguous (row r at pi + r ldi). Q: BT, K-major (element (k, c) at
// pj[k ldj + c]); !BT, j-major (element (k, c) at pj[c ldj + k]). kd: multiple of 128.
// Stages of 128 k are loaded with 16 coalesced 16-B loads per thread (the next stage is
// prefetched into registers while the current one is multiplied); the four waves each take
// 32 k of a stage and their partial tiles are summed through LDS at the end.
// LDS: smem[0, 2 * 32 * G32K) (operands) and then [0, 4 * 32 * 33) (partials, aliased).
constexpr int G32K = 129;  // LDS row stride of a 128-deep operand row (130: same time, A/B)
static_assert(2 * MB_DOUBLES >= 2 * 32 * G32K + 4 * 1024 && 2 * MB_DOUBLES >= 4 * 32 * 33,
              "gemm32 LDS (+ the in-chain solve's parked output tiles)");
template <bool BT, bool COH = false, bool PAIR = false>
__device__ __forceinline__ void gemm32(const double* __restrict__ pi, int64_t ldi,
                                       const double* __restrict__ pj, int64_t ldj, int kd,
                                       double (&v)[4], double* __restrict__ smem) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: index math is redone per call, not hoisted and held
  const int lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  double* sA = smem;             // [32][G32K]: P rows
  double* sB = smem + 32 * G32K;  // [32][G32K]: Q columns (j-major)
  double4v acc4[2][2];  // 16 x 16 blocks: acc4[rb][jr][r] = element (16 rb + 4 r + lk, 16 jr + li)
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) acc4[rb][0] = acc4[rb][1] = (double4v){0.0, 0.0, 0.0, 0.0};
#define ACC(ir, jr) acc4[(ir) >> 2][jr][(ir) & 3]
  double2 pre[16];
  auto gload = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u;
      pre[u] = ld2<COH>(pi + (idx >> 6) * ldi + k0 + 2 * (idx & 63));
      pre[8 + u] = BT ? ld2<COH>(pj + (int64_t)(k0 + (idx >> 4)) * ldj + 2 * (idx & 15))
                      : ld2<COH>(pj + (idx >> 6) * ldj + k0 + 2 * (idx & 63));
    }
  };
  if (kd > 0) gload(0);
  for (int k0 = 0; k0 < kd; k0 += 128) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u;
      double* d = sA + (idx >> 6) * G32K + 2 * (idx & 63);
      d[0] = pre[u].x;
      d[1] = pre[u].y;
      if (BT) {
        const int kr = idx >> 4, c = 2 * (idx & 15);
        sB[c * G32K + kr] = pre[8 + u].x;
        sB[(c + 1) * G32K + kr] = pre[8 + u].y;
      } else {
        double* e = sB + (idx >> 6) * G32K + 2 * (idx & 63);
        e[0] = pre[8 + u].x;
        e[1] = pre[8 + u].y;
      }
    }
    __syncthreads();
    if (k0 + 128 < kd) gload(k0 + 128);
#pragma unroll
    for (int kk = 32 * w; kk < 32 * w + 32; kk += 4) {
      const double b0 = sB[li * G32K + kk + lk], b1 = sB[(16 + li) * G32K + kk + lk];
      const double a0 = sA[li * G32K + kk + lk], a1 = sA[(16 + li) * G32K + kk + lk];
      acc4[0][0] = mfma16(a0, b0, acc4[0][0]);
      acc4[0][1] = mfma16(a0, b1, acc4[0][1]);
      acc4[1][0] = mfma16(a1, b0, acc4[1][0]);
      acc4[1][1] = mfma16(a1, b1, acc4[1][1]);
    }
  }
  __syncthreads();  // operand reads done: the partials alias them
  double* red = smem;  // [4][32][33]
#pragma unroll
  for (int ir = 0; ir < 8; ++ir)
#pragma unroll
    for (int jr = 0; jr < 2; ++jr) red[(w * 32 + ir * 4 + lk) * 33 + jr * 16 + li] = ACC(ir, jr);
#undef ACC
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // PAIR: v[2h], v[2h + 1] = elements e, e + 1 with e = 2 tid + 512 h (one 16-B store each)
    const int e = PAIR ? 2 * tid + 512 * (q >> 1) + (q & 1) : tid + 256 * q, r = e >> 5, c = e & 31;
    v[q] = red[r * 33 + c] + red[(32 + r) * 33 + c] + red[(64 + r) * 33 + c] +
           red[(96 + r) * 33 + c];
  }
  __syncthreads();  // partials read: smem is free for the next call
}
// Every phase runs in 32 x 32 output tiles (gemm32) over all gridDim.x workgroups: one CU's
// fp64 rate is 1/256 of the chip's, so the latency-bound chain spreads each product thin.
// LIGHT (w = 1): every value one workgroup hands to another is stored write-through and
// loaded device-coherently, so the barriers, the input wait and the completion flag need no
// cache maintenance (an agent-scope fence costs ~1.7-3.5 us).
template <bool LIGHT>
__global__ __launch_bounds__(256) void chain_kernel(ChainArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int G = gridDim.x, wg = blockIdx.x, tid = threadIdx.x;
  const int W = g.w * NB;
  double* Aw = g.Wk - (g.Kc * W + g.Kc);  // the workspace with the matrix's row / column numbers
  unsigned nbar = 0;
  auto stamp = [&](int p) {
    if (g.stamps && wg == 0 && tid == 0 && p < 16) g.stamps[p] = __builtin_amdgcn_s_memrealtime();
  };
  auto sync = [&]() {
    return (LIGHT ? grid_sync_light : grid_sync)(g.bar, G * ++nbar, g.status, g.spin >> 2);
  };
  stamp(0);
  // the block's inputs come from the main stream's launch in flight: wait for its count
  if (g.xready) {
    __shared__ int okx;
    if (tid == 0) {
      okx = spin_until<false>(g.xready, g.xtarget, g.spin, g.status);
      if (!okx) timeout_at(g.status, 5);
    }
    __syncthreads();
    // one agent-scope acquire so the inputs below come through plain, cached loads (LIGHT:
    // device-coherent loads instead)
    if (!LIGHT) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (!okx) return;
  }
  stamp(14);
  if (g.kd > 0) {
    // PX in 32 x 32 tiles (K = 32 (cb + 1) rounded up to 128: Bd is upper triangular)
    const int nc = g.kd / 32, nu = (W / 32) * nc;
    for (int u = wg; u < nu; u += G) {
      const int cb = u % nc, rb = u / nc;
      const int kd = min(g.kd, (32 * (cb + 1) + 127) / 128 * 128);
      double v[4];
      gemm32<true, LIGHT, LIGHT>(g.A + (g.Kc + 32 * rb) * g.lda + g.K0p, g.lda, g.Bdp + 32 * cb,
                                 g.kd, kd, v, smem);
      if (LIGHT) {
        // element pairs, one 16-B write-through store each (xd: W x kd doubles, < 2^31 B)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = 2 * tid + 512 * h;
          st2_wt(g.xd, (unsigned)(((32 * rb + (e >> 5)) * g.kd + 32 * cb + (e & 31)) * 8), v[2 * h],
                 v[2 * h + 1]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = tid + 256 * q;
          g.xd[(int64_t)(32 * rb + (e >> 5)) * g.kd + 32 * cb + (e & 31)] = v[q];
        }
      }
    }
    if (!sync()) return;
  }
  stamp(13);
  // P0: pending update of the block into the workspace, 32 x 32 lower tiles:
  // Wk[D] = A[D] - X X^T
  {
    const int nt = W / 32, ntile = nt * (nt + 1) / 2;
    for (int u = wg; u < ntile; u += G) {
      int ti = 0;
      while ((ti + 1) * (ti + 2) / 2 <= u) ++ti;
      const int tj = u - ti * (ti + 1) / 2;
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      if (g.kd > 0)
        gemm32<false, LIGHT, LIGHT>(g.xd + (int64_t)32 * ti * g.kd, g.kd,
                                    g.xd + (int64_t)32 * tj * g.kd, g.kd, g.kd, v, smem);
      if (LIGHT) {
        // element pairs: one 16-B device-coherent load and one 16-B write-through store each
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = 2 * tid + 512 * h;
          const int il = 32 * ti + (e >> 5), jl = 32 * tj + (e & 31);
          const double2 a = ld2<true>(&g.A[(g.Kc + il) * g.lda + g.Kc + jl]);
          st2_wt(g.Wk, (unsigned)((il * W + jl) * 8), a.x - v[2 * h], a.y - v[2 * h + 1]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = tid + 256 * q;
          const int64_t i = g.Kc + 32 * ti + (e >> 5), j = g.Kc + 32 * tj + (e & 31);
          Aw[i * W + j] = g.A[i * g.lda + j] - v[q];
        }
      }
    }
    // identity border (w = 1: Bd overwrites it whole, nothing reads it)
    for (int64_t idx = (int64_t)wg * 256 + tid; idx < (LIGHT ? 0 : (int64_t)W * W / 2);
         idx += (int64_t)G * 256) {
      const int r = (int)(idx / (W / 2)), c = 2 * (int)(idx % (W / 2));
      double2 v;
      v.x = (r == c) ? 1.0 : 0.0;
      v.y = (r == c + 1) ? 1.0 : 0.0;
      *reinterpret_cast<double2*>(&g.Wk[(int64_t)(W + r) * W + c]) = v;
    }
  }
  stamp(1);
  bool ok = sync();
  stamp(2);
  for (int c = 0; c < g.w && ok; ++c) {
    const int64_t kb = g.Kc + (int64_t)c * NB, r0 = kb + NB;
    // workgroup 0: factor block c and its full inverse; transposed into Bd directly when it is
    // the only block (w = 1: Bd = L11^{-T}), else into linv for the panel solve below
    if (wg == 0) {
      double* Li = smem + MB_DOUBLES;
      potrf_block<(LIGHT ? 127 : 47) | 128 | 512>(smem, Aw, W, kb, g.n, g.dinv, g.parts,
                                                  (int)(kb / NB), g.status, Li,
                                                  g.stamps && g.w == 1 ? g.stamps + 5 : nullptr);
      stamp(3 + 3 * c);
      store_inverse_t<LIGHT>(Li, g.w == 1 ? g.Wk + (int64_t)W * W : g.linv, g.w == 1 ? W : NB);
      stamp(4 + 3 * c);
    }
    if (g.w == 1) break;
    ok = sync();
    if (!ok) break;
    // panel solve of every workspace row below block c as a GEMM: X = A_c Linv_c^T
    const int64_t rows = g.Kc + 2 * W - r0;
    {
      // 32-row units, one workgroup each (the solve is in place: a unit owns its rows), the
      // four 32-column output tiles parked in LDS past gemm32's operands until all are formed
      double* park = smem + 2 * 32 * G32K;
      for (int64_t u = wg; u < rows / 32; u += G) {
        const int64_t ra = r0 + 32 * u;
#pragma unroll 1
        for (int jc = 0; jc < 4; ++jc) {
          double v[4];
          gemm32<true>(Aw + ra * W + kb, W, g.linv + 32 * jc, NB, NB, v, smem);
#pragma unroll
          for (int q = 0; q < 4; ++q) park[jc * 1024 + tid + 256 * q] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int jc = 0; jc < 4; ++jc)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            Aw[(ra + (e >> 5)) * W + kb + 32 * jc + (e & 31)] = park[jc * 1024 + e];
          }
        __syncthreads();
      }
    }
    ok = sync();
    stamp(5 + 3 * c);
    if (!ok || c + 1 == g.w) break;
    const int hi = g.w - 1 - c;
    {
      // band update in 32 x 32 tiles: columns r0 .. r0 + 128 hi, every row below (diagonal
      // tiles whole: their upper part is never read)
      const int R32 = (int)(rows / 32), J32 = 4 * hi;
      int nt = 0;
      for (int jt = 0; jt < J32; ++jt) nt += R32 - jt;
      for (int u = wg; u < nt; u += G) {
        int jt = 0, rem = u;
        while (rem >= R32 - jt) {
          rem -= R32 - jt;
          ++jt;
        }
        const int it = jt + rem;
        const int64_t ra = r0 + 32 * it, ca = r0 + 32 * jt;
        double v[4];
        gemm32<false>(Aw + ra * W + kb, W, Aw + ca * W + kb, W, NB, v, smem);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = tid + 256 * q;
          Aw[(ra + (e >> 5)) * W + ca + (e & 31)] -= v[q];
        }
      }
    }
    ok = sync();
  }
  if (wg == 0) {
    if (g.n >= g.Kc && g.n < g.Kc + W) {
      const int r = (int)(g.n - g.Kc);
      // LIGHT (w = 1): row n of the factor from LDS (the block was not stored back)
      for (int c = tid; c < W; c += 256)
        g.zvec[g.Kc + c] = !LIGHT ? g.Wk[(int64_t)r * W + c]
                           : c <= r ? smem[(((r >> 4) * ((r >> 4) + 1) / 2) + (c >> 4)) *
                                               (IB * (IB + 1)) + (r & 15) * (IB + 1) + (c & 15)]
                                    : 0.0;
    }
    // LIGHT: Bd went out write-through and its readers load it device-coherently; zvec, parts
    // and status are read by later launches only
    if (LIGHT) __builtin_amdgcn_s_waitcnt(0);
    else __threadfence();
    __syncthreads();
    stamp(15);
    if (tid == 0)
      __hip_atomic_store(g.done, 1u, LIGHT ? __ATOMIC_RELAXED : __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Start-up check for schedule 3: can gridDim.x chain-sized workgroups (CHAIN_LDS each, so one
// per CU) be resident together on the side stream's CUs? Each arrives at a counter and waits
// (bounded, ~0.1 s) for all; ok[0] = 1 when every one saw the full count.
__global__ __launch_bounds__(256) void coresident_kernel(unsigned* bar, int* ok) {
  extern __shared__ double pad[];
  if (threadIdx.x == 0) {
    pad[0] = 0.0;
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned it = 0;
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x &&
           ++it < (1u << 20))
      __builtin_amdgcn_s_sleep(2);
    if (it >= (1u << 20)) atomicExch(ok, 0);
  }
}

// ------------------------------------------------------------- finalize
// z = L^{-1} r: columns c < zsplit from zvec (schedule 3 keeps the panels out of A), the rest
// from row n of the factor.
__global__ __launch_bounds__(1024) void finalize_kernel(const double* __restrict__ A, int64_t lda,
                                                        int64_t n, const double* __restrict__ parts,
                                                        int nparts, const int* __restrict__ status,
                                                        int negative, double* __restrict__ out,
                                                        const double* __restrict__ zvec,
                                                        int64_t zsplit) {
  __shared__ double red[2][16];
  const int tid = threadIdx.x;
  double q = 0.0, ld = 0.0;
  for (int64_t c = tid; c < n; c += 1024) {
    const double z = c < zsplit ? zvec[c] : A[n * lda + c];
    q += z * z;
  }
  for (int k = tid; k < nparts; k += 1024) ld += parts[k];
  for (int o = 32; o > 0; o >>= 1) {
    q += __shfl_xor(q, o);
    ld += __shfl_xor(ld, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = q;
    red[1][tid >> 6] = ld;
  }
  __syncthreads();
  if (tid == 0) {
    double Q = 0.0, LD = 0.0;
    for (int i = 0; i < 16; ++i) {
      Q += red[0][i];
      LD += red[1][i];
    }
    const double logdet = 2.0 * LD;
    const double two_pi = 6.283185307179586476925;
    double mll = -0.5 * ((double)n * log(two_pi) + logdet + Q);
    mll *= negative ? -1.0 : 1.0;
    if (status[0] != STATUS_NONE) mll = __builtin_nan("");
    out[0] = mll;
    out[1] = logdet;
    out[2] = Q;
    out[3] = (double)status[0];
    out[4] = (double)status[1];
  }
}

__global__ void status_init_kernel(int* st) {
  st[0] = STATUS_NONE;
  st[1] = 0;  // which wait timed out first (timeout_at)
}

// The kernel templates as the host launches them (lfm_chol_sched.hip), instantiated here by
// naming them, after every other kernel and in this order. Explicit instantiation definitions
// (`template __global__ void ...;`) would do, but the compiler emits those ahead of the other
// kernels, and with the code object laid out that way an N = 16384 evaluation measured 0.14 ms
// (0.5 %) slower, the kernels' own code being identical. The one host function
// of this unit: it returns the i-th of them (lfm_chol.h).
const void* chol_kernel_template(int i) {
  static const void* const k[6] = {reinterpret_cast<const void*>(&potrf_diag_kernel<15>),
                                   reinterpret_cast<const void*>(&syrk_kernel<true, 64>),
                                   reinterpret_cast<const void*>(&syrk_kernel<true, 128>),
                                   reinterpret_cast<const void*>(&syrk_kernel<false, 64>),
                                   reinterpret_cast<const void*>(&chain_kernel<false>),
                                   reinterpret_cast<const void*>(&chain_kernel<true>)};
  return k[i];
}

}  // namespace lfm
