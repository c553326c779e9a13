// lfm_chol.h — what crosses between the factorisation's kernels (lfm_chol.hip) and the host
// code that schedules them (lfm_chol_sched.hip): the tile constants, the launch argument
// structs, the dynamic LDS sizes and the kernels themselves.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>

#include "lfm_math.h"

namespace lfm {

static constexpr int NB = 128;       // panel width (block column)
static constexpr int IB = 16;        // inner block of the diagonal factor / panel solve
static constexpr int ST = 128;       // SYRK output tile edge
static constexpr int KB = 16;        // SYRK K-step staged through LDS
// schedule 1's 64-row SYRK (syrk_kernel<., 64>): workgroups per CU in its launch bounds
static constexpr int SLAB_WGS = 3;
// schedule-3 MLL bulk super-panel width in block columns
static constexpr int WBULK = 5;
// the same for the gradient's bordered factorisation (its window keeps every step full width)
static constexpr int WBORD = 4;
// rest-triangle enumeration: tile rows in groups of Q, Q x Q supertiles within a group
static constexpr int SUPERTILE = 6;
// tall units (X_{s+1} = A21 Bd) in 64 x (128 / TALL_SPLIT) pieces
static constexpr int TALL_SPLIT = 2;
static constexpr int STATUS_NONE = INT_MAX;

// Doubles of a packed 128 x 128 lower-triangular block in LDS (16 x 16 blocks, row stride
// IB + 1: potrf_block's MS)
constexpr int MB_DOUBLES = (NB / IB) * (NB / IB + 1) / 2 * IB * (IB + 1);
// dynamic LDS of panel_kernel (the block, then a union of its other uses) and of chain_kernel
// (the factor block and its inverse)
constexpr size_t PANEL_LDS = (size_t)MB_DOUBLES * sizeof(double);
constexpr size_t CHAIN_LDS = 2 * (size_t)MB_DOUBLES * sizeof(double);

// Source of a trailing update's panel rows: matrix row r (k = 0 at the panel's first column)
// starts at p + (r - r0) * ld. The factor's own block column: {A + kb, lda, 0}; a separate
// panel buffer holding rows r0 .. : {X, ldx, r0}.
struct Panel {
  const double* p;
  int64_t ld, r0;
};

// One launch of step_kernel / helper_update_kernel (lfm_chol.hip step_body): the units of its
// three roles, ahead, rest and tall.
struct StepArgs {
  double* A;
  int64_t lda;
  int64_t s0;     // trailing matrix of step s starts at row / column s0 = K1
  Panel px;       // X_s (rows from s0)
  int kd, T, wn;  // depth W_s, trailing 128-tiles, next width in tiles
  int na, nr, nt;  // units per role
  int64_t tr0;    // tall: first row (K1 of step s + 1), W_{s+1} = tw * 128, K0_{s+1} = tk0
  int64_t tk0;
  int tw;
  const double* Bd;
  double* X;      // X_{s+1}, ld tw * 128, row tr0 first
  int64_t n;
  double* zvec;
  unsigned* a_done;  // [T] per tile row of step s (NULL: no wait)
  const unsigned* chain_done;  // NULL: no wait
  int* status;
  // inputs of chain(s + 2), which starts while this launch runs: the rest units of its block
  // (lead x lead leading tiles of the rest triangle) and the ahead units of its rows (tile
  // rows < wn + lead) write through to memory and bump *xready when done
  unsigned* xready;  // NULL: no chain waits on this launch
  int lead;
  unsigned spin;     // time bound of every device-side wait, ticks (PANEL_TIMEOUT past it)
  unsigned long long* stamps;  // diagnostics (NULL: off): [8] launch stamps, lfm_diag.h
  int64_t pad_end;   // rows in (n, pad_end) are skipped identity padding (INT64_MAX: every
                     // row past n; n + 1: none)
  // bordered matrix (the gradient's inverse): border row Mp + i is e_i in the first Mp columns
  // and zero after until the window reaches it, so it is never initialised in memory —
  // update units of rows >= zero_from start from C = 0, and the tall units of rows >=
  // copy_from (= Mp + K0: A21 is the identity there) copy Bd's row (row - copy_from)
  int64_t zero_from;
  int64_t copy_from;
  GramGen gen;       // gen.tab != NULL: the first step's update units generate Sigma (fused gram)
  int64_t rest_off;  // rest units of this launch are [rest_off, rest_off + nr) of the step's
                     // enumeration (the side-CU helper launch takes the tail of it)
  unsigned long long* trace;  // diagnostics (NULL: off): 4 words per workgroup (lfm_debug_trace)
  unsigned long long trace_tag;  // launch tag, bits 40+ of each record's last word
};

// One launch of chain_kernel: the factorisation of super-panel s's diagonal block.
struct ChainArgs {
  const double* A;
  int64_t lda;
  int64_t Kc;         // first row / column of the super-panel
  int w;              // width in 128-column blocks
  double* Wk;         // 2W x W, ld W
  int kd;             // W_{s-1}: depth of the pending update (0: none)
  int64_t n;
  double* dinv;
  double* linv;       // 128 x 128: transposed inverse of the current diagonal block (w > 1)
  double* parts;
  int* status;
  double* zvec;
  unsigned* bar;      // grid barrier counter (zeroed per call)
  unsigned* done;     // chain_done[s]
  unsigned long long* stamps;  // diagnostics (NULL: off): s_memrealtime per phase, [16]
  const unsigned* xready;  // NULL: inputs ready at launch; else wait for *xready >= xtarget and
  unsigned xtarget;        // read A[D] and the panel rows with device-coherent loads
  // PX (kd > 0): the block's rows of X_{s-1} = A[D rows, K0p .. K0p + kd) Bd_{s-1} are formed
  // here (into xd, ld kd) instead of waiting for the main stream's tall units
  int64_t K0p;             // first column of super-panel s - 1
  const double* Bdp;       // Bd_{s-1}: kd x kd, ld kd
  double* xd;              // W x kd scratch
  unsigned spin;           // time bound of the input wait, ticks (grid barriers: spin / 4)
};

// The kernels (lfm_chol.hip; the templates are instantiated there for what the host launches)
template <int PH>
__global__ __launch_bounds__(256, 4) void potrf_diag_kernel(double* __restrict__ A, int64_t lda,
                                                           int64_t kb, int64_t npiv,
                                                           double* __restrict__ dinv,
                                                           double* __restrict__ parts, int k,
                                                           int* __restrict__ status);
__global__ __launch_bounds__(256) void trsm_kernel_v2(double* __restrict__ A, int64_t lda,
                                                      int64_t s, int64_t kb,
                                                      const double* __restrict__ dinv);
template <bool CIO, int TR>
__global__ __launch_bounds__(256, TR == 64 ? SLAB_WGS : 2) void syrk_kernel(
    double* __restrict__ A, int64_t lda, int64_t s, Panel P, int kd, int T, int tj_lo, int tj_hi,
    int prio, int xcd_remap, int ti0, int64_t skip);
__global__ __launch_bounds__(256, 4) void step_kernel(StepArgs g);
__global__ __launch_bounds__(256, 4) void helper_update_kernel(StepArgs g);
__global__ __launch_bounds__(256, 4) void step_kernel_traced(StepArgs g);
__global__ __launch_bounds__(256, 4) void helper_update_kernel_traced(StepArgs g);
__global__ __launch_bounds__(256) void panel_kernel(double* __restrict__ A, int64_t lda,
                                                    int64_t kb, int64_t pkb, int pkd,
                                                    int64_t npiv, double* __restrict__ dinv,
                                                    double* __restrict__ parts, int k,
                                                    int* __restrict__ status,
                                                    unsigned* __restrict__ sync, unsigned epoch,
                                                    unsigned spin);
template <bool LIGHT>
__global__ __launch_bounds__(256) void chain_kernel(ChainArgs g);
__global__ __launch_bounds__(256) void coresident_kernel(unsigned* bar, int* ok);
__global__ __launch_bounds__(1024) void finalize_kernel(const double* __restrict__ A, int64_t lda,
                                                        int64_t n, const double* __restrict__ parts,
                                                        int nparts, const int* __restrict__ status,
                                                        int negative, double* __restrict__ out,
                                                        const double* __restrict__ zvec,
                                                        int64_t zsplit);
__global__ void status_init_kernel(int* st);
// The six template instances the host launches (potrf_diag_kernel<15>, syrk_kernel<true, 64>,
// <true, 128>, <false, 64>, chain_kernel<false>, <true>): lfm_chol.hip instantiates them by
// naming them in this function
const void* chol_kernel_template(int i);

}  // namespace lfm
