// lfm_small.hip — the small-N path on gfx950: one workgroup per problem (n <= SMALL_MAX), the
// whole problem in LDS. Configs 1 and 5 of BASELINE.json (N = 35, 28) and the reference's
// training workflow over them:
//   small_mll_kernel(_args)   CustomConjMLL(negative).step (src/objectives.py:21-78) of every
//                             problem of a batch in one launch (the ablation farm of
//                             src/notebook.py:33-75);
//   small_grad_kernel(_args)  its value and gradient with respect to the constrained
//                             parameters (jax.value_and_grad at src/trainer.py:126);
//   small_fit_kernel          JaxTrainer.fit (src/trainer.py:162-228): every problem's Adam steps
//                             run inside the kernel, one workgroup per problem;
//   small_post_kernel, small_post_cov_kernel
//                             latent_predict / multi_gene_predict (src/model.py:420-514) of every
//                             problem at its own test inputs (lfm_batch_posterior_f64).
#include "lfm_bijectors.h"
#include "lfm_dual.h"
#include <mutex>

namespace lfm {

// ------------------------------------------------------- small-N batch
// One workgroup per problem: Sigma (+ residual row) built and factored in LDS.
// Used for n <= SMALL_MAX (configs 1 and 5: N = 35, 28).

// Factor of the augmented (n + 1)-row matrix on one wave (small_mll_kernel, n + 1 <= 64): lane
// r holds row r (row n: the residual) in registers as a window d[q] = A[r][c + q] over the
// columns from the current one c on, right-looking. Column c: every lane scales its entry into
// L[r][c] and puts it in colbuf[r] (LDS); every lane then reads L[c + q][c] back (all reads
// issued at once) and updates and shifts its window in one step, d[q - 1] = d[q] - L[r][c]
// L[c + q][c]. The pivot of column c + 1 is lane c + 1's new d[0], which that lane forms from
// its own L[c + 1][c] without the LDS round trip, so its reciprocal square root (v_rsq_f64 and
// one Newton step, as the large factor's leaf) is issued alongside column c's update. The
// window narrows as columns retire (W = 64 or 32, then 24, 16, 12, 8: small_next_w), so a
// column costs about as many fused multiply-adds as it has live entries; the column loops stay rolled
// (fully unrolled, the straight-line code was instruction-fetch bound). Per element the terms
// are summed in the same order (k = 0, 1, ...) as before. colbuf: >= 128 doubles, zero from
// index 64 on. Lane r ends with its pivot (r < n) and residual entry z[r] = L[n][r].
struct SmallFactor {
  int n, r;
  bool act;
  double* colbuf;
  double dc, y;      // the current column's pivot input and 1 / sqrt of it
  double mp, mz;     // this lane's pivot and z entry (one wave: mp = the pivot input d_r)
  double inv;        // one wave, LDL^T columns: 1 / dc
  double q;          // one wave: this row's sum of L[r][c]^2 (lane n: r^T Sigma^{-1} r)
  int bad;
};
// 1 / d to the last bit or so: v_rcp_f64 and two Newton steps (the sweep's reciprocal)
__device__ __forceinline__ double rcp_2nr(double d) {
  double v = __builtin_amdgcn_rcp(d);
  v = fma(v, fma(-d, v, 1.0), v);
  return fma(v, fma(-d, v, 1.0), v);
}
__device__ __forceinline__ double swap_halves(double v) {
  // lane i < 32 gets lane i + 32's value and lane i + 32 lane i's (v_permlane32_swap_b32)
  const long long b = __double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false,
                                                   false);
  const bool low = (threadIdx.x & 32) == 0;
  const unsigned l = low ? lo[1] : lo[0], h = low ? hi[1] : hi[0];
  return __longlong_as_double(((long long)h << 32) | l);
}
// An LDS hand-off between the lanes of ONE wave (the form of HIP's __syncwarp): a release and an
// acquire fence at wavefront scope around a wave barrier. Every lane's LDS stores before it are
// ordered before every lane's LDS reads after it, and every read before it before every store
// after it (the next step's overwrite of a buffer the other lanes were reading). On gfx950 both
// fences are empty (a wave's LDS operations are performed in issue order) and the wave barrier
// only fences code motion, so the ISA is unchanged; what it adds over a bare compiler fence is the
// language-level ordering the reads rely on.
__device__ __forceinline__ void wave_lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// window widths of the phases: 64 48 32 24 16 12 8
template <int W>
constexpr int small_next_w() {
  return W == 64 ? 48 : W == 48 ? 32 : W == 32 ? 24 : W == 24 ? 16 : W == 16 ? 12 : 8;
}
template <int W>
__device__ __forceinline__ void small_factor_next(double (&d)[W], int c, SmallFactor& f);
template <int W>
__device__ __forceinline__ void small_factor_phase(double (&d)[W], int c, SmallFactor& f) {
  // phase W: the columns while more than the next width of them remain (the last phase: all)
  constexpr int WN = small_next_w<W>();
  const int cend = W > 8 ? max(c, f.n - WN) : f.n;
#pragma unroll 1
  for (; c < cend; ++c) {
    if (!(f.dc > 0.0) && f.bad == 0) f.bad = c + 1;
    const double lc = f.r == c ? f.dc * f.y : d[0] * f.y;  // L[r][c]; lane c: the pivot
    if (f.r == c) f.mp = f.dc;  // logdet = sum log d_c (L_cc^2 = d_c)
    f.q = fma(lc, lc, f.q);
    // the next pivot: lane c + 1's d[1] - L[c + 1][c]^2 (past the last column: unused)
    const double dn = rdl(fma(-lc, lc, d[1]), c + 1);
    const double yn = rsqrt_1nr(dn);
    wave_lds_handoff();  // the previous column's reads of colbuf before this column's stores
    f.colbuf[f.r] = (f.act && f.r > c) ? lc : 0.0;
    wave_lds_handoff();  // every lane's store before the reads
    // the column comes back in chunks of at most 32, every read of a chunk issued before its
    // first use (sched_barrier: the scheduler would otherwise sink the reads to their uses and
    // expose the LDS latency two or three reads at a time)
    constexpr int CH = W > 32 ? 32 : W;
#pragma unroll
    for (int q0 = 1; q0 < W; q0 += CH) {
      double col[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u)
        if (q0 + u < W) col[u] = f.colbuf[c + q0 + u];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < CH; ++u)
        if (q0 + u < W) d[q0 + u - 1] = fma(-lc, col[u], d[q0 + u]);
    }
    d[W - 1] = 0.0;
    f.dc = dn;
    f.y = yn;
  }
  if constexpr (W > 8)
    if (c < f.n) small_factor_next<WN>(*reinterpret_cast<double(*)[WN]>(&d[0]), c, f);
}
// Windows of 32 and narrower: LDL^T (Sigma = L D L^T, unit L), software-pipelined by one
// column. The trailing matrix is the same Schur complement as Cholesky's, so the two meet at a
// phase boundary; what changes is what goes through LDS: a column's UNSCALED entries u_r (lane r's
// window d[0]) instead of L[r][c] = u_r / sqrt(d_c). A lane scales its own multiplier,
// l_r = u_r / d_c, so no reciprocal (square root) of the pivot sits between a column's last
// update and its store. Column c: l_r, the next column's entry d[1] - l_r u_{c+1} first, stored;
// column c + 1's reads issued; then the next pivot's reciprocal (v_rcp_f64 and two Newton steps,
// uniform: lane c + 1's entry by v_readlane) and the rest of column c's multiply-adds, all under
// that LDS round trip. logdet = sum log d_c; the residual row's sum of u_n^2 / d_c is
// r^T Sigma^{-1} r (the window does not keep that row's diagonal: it narrows past it).
// On entry col[q - 1] = u_{c + q} (q = 1 .. W - 1, reads possibly in flight), f.inv = 1 / d_c.
template <int W>
__device__ __forceinline__ void small_pipe_col(double (&d)[W], double (&cur)[W - 1],
                                               double (&nxt)[W - 1], int c, SmallFactor& f) {
  // column c's reads complete here, before column c + 1's are issued (lgkmcnt counts in order)
#pragma unroll
  for (int q = 0; q < W - 1; ++q) asm volatile("" : "+v"(cur[q]));
  if (!(f.dc > 0.0) && f.bad == 0) f.bad = c + 1;
  if (f.r == c) f.mp = f.dc;
  const double l = d[0] * f.inv;             // l_r = u_r / d_c (lanes <= c: dead rows)
  f.q = fma(l, d[0], f.q);                   // u_r^2 / d_c = L[r][c]^2
  const double d0 = fma(-l, cur[0], d[1]);   // u_r of column c + 1
  // (past the last column, c + 1 = n: unused; lanes past n store zeros) one basic block, so
  // column c's update cannot be moved past column c + 1's head
  wave_lds_handoff();  // column c's reads (completed above) before column c + 1's stores
  f.colbuf[f.r] = (f.act && f.r > c + 1) ? d0 : 0.0;
  wave_lds_handoff();  // every lane's store before column c + 1's reads
#pragma unroll
  for (int q = 1; q < W; ++q) nxt[q - 1] = f.colbuf[c + 1 + q];
  __builtin_amdgcn_sched_barrier(0);  // column c + 1's reads issued before column c's update
  const double dn = rdl(d0, c + 1);   // d_{c + 1}
  const double invn = rcp_2nr(dn);
  d[0] = d0;
#pragma unroll
  for (int q = 2; q < W; ++q) d[q - 1] = fma(-l, cur[q - 1], d[q]);
  d[W - 1] = 0.0;
  // the update is done here, ahead of column c + 1's wait for its reads
#pragma unroll
  for (int q = 0; q < W - 1; ++q) asm volatile("" : "+v"(d[q]));
  f.dc = dn;
  f.inv = invn;
}
template <int W>
__device__ __forceinline__ void small_factor_pipe(double (&d)[W], double (&col)[W - 1], int c,
                                                  SmallFactor& f) {
  constexpr int WN = small_next_w<W>();
  const int cend = W > 8 ? max(c, f.n - WN) : f.n;
  double alt[W - 1];
  // two columns an iteration, the column buffers alternating (no register copies)
#pragma unroll 1
  for (; c + 1 < cend; c += 2) {
    small_pipe_col<W>(d, col, alt, c, f);
    small_pipe_col<W>(d, alt, col, c + 1, f);
  }
  if (c < cend) {
    small_pipe_col<W>(d, col, alt, c, f);
    ++c;
#pragma unroll
    for (int q = 0; q < W - 1; ++q) col[q] = alt[q];
  }
  if constexpr (W > 8)
    if (c < f.n)
      small_factor_pipe<WN>(*reinterpret_cast<double(*)[WN]>(&d[0]),
                            *reinterpret_cast<double(*)[WN - 1]>(&col[0]), c, f);
}
// the phase of window W from column c: LDL^T pipelined for W <= 32 (its first column's entries
// stored and read back here), Cholesky (small_factor_phase) above
template <int W>
__device__ __forceinline__ void small_factor_next(double (&d)[W], int c, SmallFactor& f) {
  if constexpr (W <= 32) {
    f.inv = rcp_2nr(f.dc);
    wave_lds_handoff();  // the previous phase's reads of colbuf before these stores
    f.colbuf[f.r] = (f.act && f.r > c) ? d[0] : 0.0;
    wave_lds_handoff();
    double col[W - 1];
#pragma unroll
    for (int q = 1; q < W; ++q) col[q - 1] = f.colbuf[c + q];
    small_factor_pipe<W>(d, col, c, f);
  } else {
    small_factor_phase<W>(d, c, f);
  }
}
// n + 1 <= 32, the columns while more than 16 remain: LDL^T with each row on TWO lanes (lane i
// slots 0..15 of row i's window, lane i + 32 slots 16..31), so a column's read-back is 16 values
// a lane instead of up to 31 — the column step is bound by the wave's LDS read rate
// (r05_ubench_lds_chain.txt). Column c: l = u_i / d_c (u_i: the low lane's slot 0, the high
// lane gets it by v_permlane32_swap); the low lanes store u_i; each half reads its 16 entries
// u_{c + 16 hi + k}; slots shift down one with d[q - 1] = d[q] - l u_{c + q}, the high lane's
// updated slot 16 crossing to the low lane's slot 15. The same arithmetic as the one-lane LDL^T
// columns. On return the low lanes' 16 slots are the one-lane window of width 16 at column c.
__device__ __forceinline__ int small_factor_two(double (&a)[16], SmallFactor& f) {
  const int hi = (int)((threadIdx.x >> 5) & 1), i = (int)(threadIdx.x & 31);  // any wave
  const bool act = i < f.n + 1;
  if (hi) f.colbuf[32 + i] = 0.0;  // entries past the rows (the high half reads up to c + 31)
  int c = 0;
  f.inv = rcp_2nr(f.dc);
#pragma unroll 1
  for (; f.n - c > 16; ++c) {
    if (!(f.dc > 0.0) && f.bad == 0) f.bad = c + 1;
    if (hi == 0 && i == c) f.mp = f.dc;
    const double part = swap_halves(a[0]);
    const double u = hi ? part : a[0];  // row i's column-c entry
    const double l = u * f.inv;
    f.q = fma(l, u, f.q);
    wave_lds_handoff();  // the previous column's reads before this column's stores
    if (hi == 0) f.colbuf[i] = (act && i > c) ? u : 0.0;
    wave_lds_handoff();  // every lane's store before the reads
    double col[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k] = f.colbuf[c + 16 * hi + k];
    __builtin_amdgcn_sched_barrier(0);  // every read issued before the first use
    const double t = swap_halves(fma(-l, col[0], a[0]));  // the high lane's slot 16, updated
#pragma unroll
    for (int k = 1; k < 16; ++k) a[k - 1] = fma(-l, col[k], a[k]);
    a[15] = hi ? 0.0 : t;
    f.dc = rdl(a[0], c + 1);  // d_{c + 1}: row c + 1's new slot 0 (a low lane)
    f.inv = rcp_2nr(f.dc);
  }
  return c;
}
// Lane r < n ends with d_r (its pivot: logdet = sum log d_r); every lane with the quadratic form
// r^T Sigma^{-1} r = sum_c L[n][c]^2 (lane n's sum).
template <int MR>
__device__ __forceinline__ void small_factor_regs(const double* __restrict__ sm, int ld, int n,
                                                  int M, double* colbuf, double* piv_r,
                                                  double* quad, int* bad_out) {
  SmallFactor f;
  f.n = n;
  f.r = threadIdx.x & 63;  // one wave, whichever it is
  f.act = f.r < M;
  f.colbuf = colbuf;
  f.mp = f.mz = f.q = 0.0;
  f.bad = 0;
  if constexpr (MR == 32) {
    // two lanes a row while more than 16 columns remain, then the one-lane phases from W = 16
    // (the high lanes are rows past n there: inactive)
    const int hi = f.r >> 5, i = f.r & 31;
    double d[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int q = 16 * hi + u;
      d[u] = (i < M && q <= i && q < n) ? sm[i * ld + q] : 0.0;
    }
    f.dc = rdl(d[0], 0);
    const int c = small_factor_two(d, f);
    f.y = rsqrt_1nr(f.dc);
    if (c < n) small_factor_next<16>(d, c, f);
  } else {
    double d[MR];
#pragma unroll
    for (int q = 0; q < MR; ++q) d[q] = (f.act && q <= f.r && q < n) ? sm[f.r * ld + q] : 0.0;
    f.dc = rdl(d[0], 0);
    f.y = rsqrt_1nr(f.dc);
    small_factor_next<MR>(d, 0, f);
  }
  *piv_r = f.mp;
  *quad = rdl(f.q, n);
  *bad_out = f.bad;
}

// The same factor for 64 < n + 1 <= 128: rows on two waves (thread r, r < 128, holds row r),
// the window up to 128 columns wide (small_next_w2: 128 96 64 48 32 24 16 12 8). Column c's
// entries and the next pivot's input (lane c + 1's d[1] - L[c + 1][c]^2, in slot 255) go through
// one of two alternating LDS buffers with ONE workgroup barrier per column (a wave can be at most
// one column ahead, so the buffer it writes is never the one another wave still reads); the
// reads come back in chunks of 16 (the window and all its column values would not fit the
// registers). Every thread of the workgroup calls it (waves 2 and 3 only keep the barrier count).
template <int W>
constexpr int small_next_w2() {
  return W == 128 ? 96 : W == 96 ? 64 : small_next_w<W>();
}
template <int W>
__device__ __forceinline__ void small_factor2_phase(double (&d)[W], int c, SmallFactor& f) {
  constexpr int WN = small_next_w2<W>();
  const int cend = W > 8 ? max(c, f.n - WN) : f.n;
#pragma unroll 1
  for (; c < cend; ++c) {
    if (!(f.dc > 0.0) && f.bad == 0) f.bad = c + 1;
    const double lc = f.r == c ? f.dc * f.y : d[0] * f.y;  // L[r][c]; lane c: the pivot
    if (f.r == c) f.mp = lc;
    double* buf = f.colbuf + (c & 1) * 256;
    if (f.r < 128) buf[f.r] = (f.act && f.r > c) ? lc : 0.0;
    if (f.r == c + 1) buf[255] = fma(-lc, lc, d[1]);  // the next pivot's input
    __syncthreads();
    if (f.r == c) f.mz = buf[f.n];  // L[n][c] = z[c], from the residual row's lane
    const double dn = buf[255];
#pragma unroll
    for (int q0 = 1; q0 < W; q0 += 16) {
      double col[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (q0 + u < W) col[u] = buf[c + q0 + u];
      __builtin_amdgcn_sched_barrier(0);  // the chunk's reads issued before its first use
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (q0 + u < W) d[q0 + u - 1] = fma(-lc, col[u], d[q0 + u]);
    }
    d[W - 1] = 0.0;
    f.dc = dn;
    f.y = rsqrt_1nr(dn);
  }
  if constexpr (W > 8)
    if (c < f.n) small_factor2_phase<WN>(*reinterpret_cast<double(*)[WN]>(&d[0]), c, f);
}
__device__ __forceinline__ void small_factor_regs2(const double* __restrict__ sm, int ld, int n,
                                                   int M, double* colbuf, double* piv_r,
                                                   double* z_r, int* bad_out) {
  SmallFactor f;
  f.n = n;
  f.r = threadIdx.x;
  f.act = f.r < M;
  f.colbuf = colbuf;
  // the buffers' tails past the rows read as zeros (window entries past the last column)
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    if (i >= 128) colbuf[i] = colbuf[256 + i] = 0.0;
  }
  double d[128];
#pragma unroll
  for (int q = 0; q < 128; ++q) d[q] = (f.act && q <= f.r && q < n) ? sm[f.r * ld + q] : 0.0;
  f.dc = sm[0];
  f.y = rsqrt_1nr(f.dc);
  f.mp = f.mz = 0.0;
  f.bad = 0;
  __syncthreads();  // windows loaded, buffer tails zero
  small_factor2_phase<128>(d, 0, f);
  *piv_r = f.mp;
  *z_r = f.mz;
  *bad_out = f.bad;
}

// SmallMap / small_map, one problem's LDS map (the MLL, gradient, fit and posterior kernels'),
// and every launch size derived from it: lfm_small_plan.h

// The MLL from a two-wave factor (every thread: pr / zr its row's pivot and z entry, rows < n):
// per-wave sums, then wave 0's + wave 1's in that order; returned to every thread.
__device__ __forceinline__ double small_mll_2wave(double pr, double zr, int bad, int n,
                                                  int negative, double* red) {
  const int tid = threadIdx.x;
  double ldp = 0.0, qp = 0.0;
  if (tid < n) {
    ldp = log(pr);
    qp = zr * zr;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ldp += __shfl_xor(ldp, o);
    qp += __shfl_xor(qp, o);
  }
  __syncthreads();  // every thread is past the factor's last reads of the column buffers
  if (tid == 0 || tid == 64) {
    red[tid >> 6] = ldp;
    red[2 + (tid >> 6)] = qp;
  }
  __syncthreads();
  const double two_pi = 6.283185307179586476925;
  double mll = -0.5 * ((double)n * log(two_pi) + 2.0 * (red[0] + red[1]) + (red[2] + red[3]));
  mll *= negative ? -1.0 : 1.0;
  if (bad) mll = __builtin_nan("");
  return mll;
}

// x, y and (grid problems) the times and block genes into the problem's LDS map; every thread
// calls it, a barrier follows before use
__device__ __forceinline__ void small_stage(const SmallProb& P, const SmallMap& m) {
  const int tid = threadIdx.x, n = m.n;
  for (int i = tid; i < 3 * n; i += 256) m.xs[i] = P.x[i];
  for (int i = tid; i < n; i += 256) m.ys[i] = P.y[i];
  if (P.T > 0) {
    for (int i = tid; i < P.T; i += 256) m.tms[i] = P.times[i];
    for (int i = tid; i < n / P.T; i += 256) m.bgs[i] = P.bg[i];
  }
}

// Sigma = (K + jitter I) + obs_stddev^2 I (objectives.py:66-73) in the lower triangle of A and
// the residual r = y - m (model.py:124-149) in row n; every thread of the workgroup calls it (the
// hyperparameters, x and y already in LDS; it ends without a barrier).
__device__ __forceinline__ void small_sigma(const SmallProb& P, const SmallMap& m, const HypDev& h,
                                            int tabs) {
  double* sm = m.A;
  const int n = m.n, ld = m.ld, G = m.G;
  const int tid = threadIdx.x;
  const double* xs = m.xs;
  const double* ys = m.ys;
  const double jitter = m.hyp[3 * G + 2], sd = m.hyp[3 * G + 1];
  const double noise = sd * sd;  // objectives.py:66
  if (P.T > 0) {
    // grid layout: the per-gene tables of lfm_gram.hip (tables_kernel) in LDS, then each lower
    // element with gram_grid_kernel's operations (~10 FMAs instead of 2 erf + 3 exp)
    double* gt = m.gt;
    const int T = P.T, W = 2 * T - 1;
    const int nt = (int)(2 * (int64_t)G * W + 3 * (int64_t)G * T + (int64_t)G * G);
    for (int q = tid; q < nt; q += 256) gt[q] = grid_table_entry(h, T, P.dt, m.tms, q);
    __syncthreads();
    const double* Wt = gt;
    const double* Xt = Wt + G * W;
    const double* Pt = Xt + G * W;
    const double* Et = Pt + G * T;
    const double* Qt = Et + G * T;
    const double* Cm = Qt + G * T;
    const int np = n * (n + 1) / 2;  // the lower triangle, row by row
    for (int q = tid; q < np; q += 256) {
      int i = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
      while (i * (i + 1) / 2 > q) --i;
      while ((i + 1) * (i + 2) / 2 <= q) ++i;
      const int c = q - i * (i + 1) / 2;
      const int bi = i / T, tau = i - bi * T, j = m.bgs[bi];
      const int bc = c / T, tp = c - bc * T, k = m.bgs[bc];
      const int d = tp - tau;
      double v = Wt[k * W + (T - 1) + d] + Wt[j * W + (T - 1) - d];
      v = fma(-Xt[k * W + (T - 1) + d], Pt[k * T + tau], v);
      v = fma(-Xt[j * W + (T - 1) - d], Pt[j * T + tp], v);
      v = fma(-(Et[k * T + tp] * Et[j * T + tau]), Qt[k * T + tp] + Qt[j * T + tau], v);
      v = Cm[j * G + k] * v;
      if (i == c) v = (v + jitter) + noise;
      sm[i * ld + c] = v;
    }
  } else if (tabs) {
    // n <= 63 (the launch's LDS holds the tables): gene-gene pairs from KxxTab, the same bits
    // as kernel_ref with a third of its transcendentals; pairs with a latent row direct
    double* gam = m.ktab;  // [G], 2 G unused
    double* qr = gam + 3 * G;
    double* pr = qr + n;
    const KxxTab t{gam, pr, qr, G};
    small_tables(h, xs, n, G, gam, pr, qr);
    const int np = n * (n + 1) / 2;  // the lower triangle, row by row
    for (int q = tid; q < np; q += 256) {
      int i = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
      while (i * (i + 1) / 2 > q) --i;
      while ((i + 1) * (i + 2) / 2 <= q) ++i;
      const int c = q - i * (i + 1) / 2;
      const double* xa = xs + 3 * i;
      const double* xb = xs + 3 * c;
      double v;
      if (flag_int(xa[2]) == 1 && flag_int(xb[2]) == 1)
        v = kxx_tab(h, t, xa[0], gene_index(xa[1], G), i, xb[0], gene_index(xb[1], G), c);
      else
        v = kernel_ref(h, xa[0], xa[1], xa[2], xb[0], xb[1], xb[2]);
      if (i == c) v = (v + jitter) + noise;
      sm[i * ld + c] = v;
    }
  } else {
    for (int idx = tid; idx < n * n; idx += 256) {
      const int i = idx / n, c = idx - i * n;
      if (c <= i) {
        const double* xa = xs + 3 * i;
        const double* xb = xs + 3 * c;
        double v = kernel_ref(h, xa[0], xa[1], xa[2], xb[0], xb[1], xb[2]);
        if (i == c) v = (v + jitter) + noise;
        sm[i * ld + c] = v;
      }
    }
  }
  const int64_t bs = n / G;
  for (int c = tid; c < n; c += 256) sm[n * ld + c] = ys[c] - mean_at(h, xs, c, bs);
}

__device__ __forceinline__ void small_body(const SmallProb P, int negative,
                                           double* __restrict__ out, int* __restrict__ status,
                                           int tabs) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, M = n + 1, G = P.G;
  const int tid = threadIdx.x;
  SmallMap m;
  small_map(sm, n, G, P.T, tabs, 0, 0, &m);
  const int ld = m.ld;
  double* red = m.red;  // [8] reduction scratch + [1] flag
  // hyperparameters staged in LDS (they may live in pinned host memory: read once), with x and
  // y, so that no later phase waits on HBM
  double* hyp = m.hyp;
  double* colbuf = m.colbuf;
  for (int i = tid; i < 3 * G; i += 256) hyp[i] = P.dsb[i];
  if (tid < 3) hyp[3 * G + tid] = P.sc[tid];
  small_stage(P, m);
  __syncthreads();
  const HypDev h{hyp, hyp + G, hyp + 2 * G, G, hyp[3 * G]};
  small_sigma(P, m, h, tabs);
  if (tid == 0) red[8] = 0.0;
  __syncthreads();
  if (M <= 64) {
    // one wave, the augmented matrix in registers (small_factor_regs); no workgroup barrier
    // (256-thread barriers were ~60 % of the kernel at n = 28, two per column)
    if (tid >= 64) return;
    const int r = tid;
    double pr, qp;
    int bad;
    colbuf[64 + r] = 0.0;
    if (M <= 32)
      small_factor_regs<32>(sm, ld, n, M, colbuf, &pr, &qp, &bad);
    else
      small_factor_regs<64>(sm, ld, n, M, colbuf, &pr, &qp, &bad);
    double ldp = r < n ? log(pr) : 0.0;
    for (int o = 32; o > 0; o >>= 1) ldp += __shfl_xor(ldp, o);
    if (r == 0) {
      const double two_pi = 6.283185307179586476925;
      double mll = -0.5 * ((double)n * log(two_pi) + ldp + qp);
      mll *= negative ? -1.0 : 1.0;
      if (bad) mll = __builtin_nan("");
      out[blockIdx.x] = mll;
      // the status word lands after the result: the host may take it as the problem's
      // completion (lfm_batch_mll_f64)
      __threadfence_system();
      if (status) status[blockIdx.x] = bad;
    }
    return;
  }
  if (M <= 128) {
    // two waves (64 < n + 1 <= 128): the same right-looking register window, one barrier a
    // column
    double pr, zr;
    int bad;
    small_factor_regs2(sm, ld, n, M, colbuf, &pr, &zr, &bad);
    const double mll = small_mll_2wave(pr, zr, bad, n, negative, red);
    if (tid == 0) {
      out[blockIdx.x] = mll;
      __threadfence_system();  // the result before the status word (lfm_batch_mll_f64)
      if (status) status[blockIdx.x] = bad;
    }
    return;
  }
  // n = SMALL_MAX = 128 (129 rows with the residual): column by column in LDS, every thread
  for (int c = 0; c < n; ++c) {
    const double d = sm[c * ld + c];
    const double piv = sqrt(d);
    const double inv = 1.0 / piv;
    for (int r = c + 1 + tid; r < M; r += 256) sm[r * ld + c] *= inv;
    if (tid == 0) {
      sm[c * ld + c] = piv;
      if (!(d > 0.0) && red[8] == 0.0) red[8] = (double)(c + 1);
    }
    __syncthreads();
    const int w = M - c - 1;
    for (int idx = tid; idx < w * w; idx += 256) {
      const int r = c + 1 + idx / w, q = c + 1 + idx % w;
      if (q <= r) sm[r * ld + q] -= sm[r * ld + c] * sm[q * ld + c];
    }
    __syncthreads();
  }
  double ldp = 0.0, qp = 0.0;
  for (int c = tid; c < n; c += 256) {
    ldp += log(sm[c * ld + c]);
    const double z = sm[n * ld + c];
    qp += z * z;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ldp += __shfl_xor(ldp, o);
    qp += __shfl_xor(qp, o);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = ldp;
    red[4 + (tid >> 6)] = qp;
  }
  __syncthreads();
  if (tid == 0) {
    const double LD = 2.0 * (red[0] + red[1] + red[2] + red[3]);
    const double Q = red[4] + red[5] + red[6] + red[7];
    const double two_pi = 6.283185307179586476925;
    double mll = -0.5 * ((double)n * log(two_pi) + LD + Q);
    mll *= negative ? -1.0 : 1.0;
    int st = 0;
    if (red[8] != 0.0) {
      mll = __builtin_nan("");
      st = (int)red[8];  // 1-based failing pivot
    }
    out[blockIdx.x] = mll;
    __threadfence_system();  // the result before the status word (lfm_batch_mll_f64)
    if (status) status[blockIdx.x] = st;
  }
}

__global__ __launch_bounds__(256) void small_mll_kernel(const SmallProb* __restrict__ probs,
                                                        int negative, double* __restrict__ out,
                                                        int* __restrict__ status, int tabs) {
  small_body(probs[blockIdx.x], negative, out, status, tabs);
}

// The same with the problem table and the hyperparameters in the kernel arguments (a resident
// batch of at most SMALL_ARG_PROBS problems and SMALL_ARG_HYP hyperparameters): no dependent
// load of the table from HBM and no read of pinned host memory before the gram.
__global__ __launch_bounds__(256) void small_mll_kernel_args(SmallArgs a) {
  SmallProb P = a.probs[blockIdx.x];
  P.dsb = a.hyp + a.dsb_off[blockIdx.x];
  P.sc = a.hyp + a.sc_off[blockIdx.x];
  small_body(P, a.negative, a.out, a.status, a.tabs);
}

// ------------------------------------------------ value and gradient (one workgroup)
// What jax.value_and_grad(loss) computes at trainer.py:126 for CustomConjMLL(negative).step,
// before the bijectors' chain rule (the large-N path's algebra, lfm_grad.hip):
//     d log N(y; m, S) / d theta = 1/2 tr(W dS/dtheta) + alpha^T dm/dtheta,
//     alpha = S^{-1} r,  W = alpha alpha^T - S^{-1},
// for n <= 127 (n + 1 <= 128 rows of the augmented matrix in registers):
//   1. Sigma and r in LDS (small_sigma: the MLL kernel's arithmetic);
//   2. the sweep operator on [[Sigma, r], [r^T, 0]] (below): -Sigma^{-1} and alpha in one pass
//      — on half a wave (n + 1 <= 32, two lanes a row), one wave
//      (n + 1 <= 64; waves 1-3 meanwhile build the grid layout's derivative tables,
//      grad_table_entry) or four waves (n + 1 <= 128, one barrier a step);
//      Its pivots and last entry would give the MLL too, through other roundings than the MLL
//      kernel's: the value comes from that kernel's own factor instead (wave 1 beside a one-wave
//      sweep, every wave before the four-wave one), so that it is lfm_batch_mll_f64's bit for bit;
//   3. W = alpha alpha^T - Sigma^{-1} written by the sweep's last pass (small_sweep_w*): into wb
//      (one wave) or A's lower triangle (four waves), diag(W) into wd;
//   4. 1/2 tr(W dS/d{D, S, l}): grid problems one wave per gene-block pair (its rows share gene
//      j, its columns gene k: the derivative tables as grad_grid_kernel reads them, the gene-pair
//      constant applied to the wave's sums); other layouts one lane per pair with the dual-number
//      kernel (kernel_grad), reduced per gene across the wave. Per-wave partial sums, combined in
//      a fixed order: the gradient is bit-reproducible from run to run;
//   5. tr(W) (d / d obs_stddev = obs_stddev tr W) and the mean terms of m_i = (B/D)[i // (n/G)]
//      flag_i (model.py:124-149), the sign of CustomConjMLL(negative); NaN on a failed factor.
// Every thread calls it, with the hyperparameters (hyp), x and y in LDS; on return (after a
// barrier) m.gout holds the gradient and the MLL is returned to every thread.

// The gradient's factorisation for n + 1 <= 64 (one wave): the sweep operator (Goodnight 1979;
// Gauss-Jordan elimination of a symmetric matrix without pivoting, stable for SPD input) on the
// augmented [[Sigma, r], [r^T, 0]], swept on its first n indices, leaves [[-Sigma^{-1}, alpha],
// [alpha^T, -r^T Sigma^{-1} r]] with alpha = Sigma^{-1} r, and its pivots are the factor's
// (L_kk^2, the Schur complements), so logdet = sum log d_k. One sweep replaces the factor, the
// triangular inverse and the X^T X products (round 5: 10 + 14 + 2.2 us a step at n = 28).
// Lane i holds row i, ROTATED so that the column being swept is always slot 0: after step k,
// slot q holds column (q + k + 1) mod MR, and the swept column enters at slot MR - 1. Step k:
// every lane puts its slot 0 (A[i][k] = A[k][i]) into buf[i] and buf[i + MR]; row k comes back
// as buf[k + q]; then
//   lane i != k: g = A[i][k] / d,  A[i][j] -= g A[k][j],  A[i][k] = g
//   lane k:      A[k][j] /= d,                             A[k][k] = -1 / d.
// On return slot q holds column (q + n) mod MR: alpha_i = a[0], column j < n sits at slot
// j + MR - n. buf: >= 4 MR + 2 doubles of LDS, 16-B aligned.
template <int MR>
__device__ __forceinline__ void small_sweep_regs(const double* __restrict__ A, int ld, int n,
                                                 double* buf, double (&a)[MR], double* logdet,
                                                 int* bad_out) {
  using dbl2 = double __attribute__((ext_vector_type(2)));
  // the row comes back in chunks: the whole row at MR = 32, 16 at a time at MR = 64 (registers),
  // 16 B a read: from buf when it starts at an even index, else from bufS (buf shifted by one)
  constexpr int CH = MR == 32 ? 32 : 16;
  double* bufS = buf + 2 * MR;
  const int i = threadIdx.x;  // wave 0
  const int M = n + 1;
#pragma unroll
  for (int q = 0; q < MR; ++q) {
    double v = 0.0;
    if (i < M && q < M && !(i == n && q == n)) v = q <= i ? A[i * ld + q] : A[q * ld + i];
    a[q] = v;
  }
  double mypiv = 1.0;  // lane k keeps d_k (its log is taken once, after the sweep)
  int bad = 0;
  asm volatile("" ::: "memory");  // the rows are loaded before the buffers are written
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    wave_lds_handoff();  // step k - 1's reads of the row buffers before step k's stores
    if (i < MR) {
      buf[i] = a[0];
      buf[i + MR] = a[0];
      bufS[i + 1] = a[0];
      bufS[i + 1 + MR] = a[0];
    }
    wave_lds_handoff();  // every lane's stores before the row's reads
    // row k from its pivot on: r[u] = buf[k + u] (r[0] = d), 16 B a read from buf when k is
    // even, else from bufS (buf shifted by one); the pivot's read is the oldest, so its
    // arithmetic starts while the rest of the row is in flight
    const double* src = (k & 1) ? bufS + 1 : buf;  // src[k + 2 p] is 16-B aligned
    double row[CH];
#pragma unroll
    for (int u = 0; u < CH; u += 2) {
      const dbl2 v = *reinterpret_cast<const dbl2*>(src + k + u);
      row[u] = v.x;
      row[u + 1] = v.y;
    }
    __builtin_amdgcn_sched_barrier(0);
    const double d = row[0];
    if (!(d > 0.0) && bad == 0) bad = k + 1;
    const bool piv = i == k;
    if (piv) mypiv = d;
    // 1 / d: v_rcp_f64 and two Newton steps
    double invd = __builtin_amdgcn_rcp(d);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    const double g = piv ? -invd : a[0] * invd;  // lane k: -g = 1 / d scales its row
    const double keep = piv ? 0.0 : 1.0;
    // slot q takes row entry q (r index q within the chunk starting at q0)
#pragma unroll
    for (int q0 = 0; q0 < MR; q0 += CH) {
      if (q0 > 0) {
#pragma unroll
        for (int u = 0; u < CH; u += 2) {
          const dbl2 v = *reinterpret_cast<const dbl2*>(src + k + q0 + u);
          row[u] = v.x;
          row[u + 1] = v.y;
        }
        __builtin_amdgcn_sched_barrier(0);  // the chunk's reads issued before its first use
      }
#pragma unroll
      for (int u = 0; u < CH; ++u)
        if (q0 + u >= 1) a[q0 + u - 1] = fma(-g, row[u], a[q0 + u] * keep);
    }
    a[MR - 1] = g;
  }
  // logdet = sum_k log d_k, one log per lane, then the wave's sum
  double lp = i < n ? log(mypiv) : 0.0;
  for (int o = 32; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
  *logdet = lp;
  *bad_out = bad;
}

// W = alpha alpha^T - Sigma^{-1} from the sweep's rows (lane i: row i of -Sigma^{-1} and alpha_i):
// alpha into al, W's rows into A (its Sigma is dead; the reduction reads the strictly lower
// part), diag(W) into wd.
template <int MR>
__device__ __forceinline__ void small_sweep_w(const double (&a)[MR], int n, double* wb,
                                              double* alS, double* al, double* wd) {
  constexpr int LDW = MR | 1;
  const int i = threadIdx.x;  // wave 0
  // alpha at alS[MR - n + j] (slot q of every row holds column j = q - (MR - n)), so that
  // every read and store below has a compile-time offset; alpha also into al
  wave_lds_handoff();  // the sweep's last reads of its row buffers (alS) before these stores
  if (i < n) {
    al[i] = a[0];
    alS[MR - n + i] = a[0];
  }
  wave_lds_handoff();  // alpha in LDS before every lane reads it back
  double alj[MR];
#pragma unroll
  for (int q = 1; q < MR; ++q) alj[q] = alS[q];
  __builtin_amdgcn_sched_barrier(0);
  // lane i's row (lanes past row n - 1 write the dead row n); the slots before column 0 hold
  // the padding columns' products, never read
  const double ai = a[0];
  double* row = wb + min(i, n) * LDW - 1;
#pragma unroll
  for (int q = 1; q < MR; ++q) row[q] = fma(ai, alj[q], a[q]);
  wave_lds_handoff();  // the rows stored before the diagonal is read back
  if (i < n) wd[i] = row[MR - n + i];
}

// The sweep for n + 1 <= 32 with each row on TWO lanes (half the fused multiply-adds a step):
// lane i holds slots 0..15 of row i, lane i + 32 slots 16..31 of row i, rotated as in
// small_sweep_regs. Step k: the low lanes put their slot 0 (A[i][k]) into the buffers; each half
// reads its 16 row entries (16 B a read) and A[i][k], d from the buffer; the high lane also forms
// the new value of slot 16, which moves to the low lane's slot 15 (v_permlane32_swap), and takes
// the swept column into slot 31. On return slot q holds column (q + n) mod 32, as before.

__device__ __forceinline__ void small_sweep_half(const double* __restrict__ A, int ld, int n,
                                                 double* buf, double (&a)[16], double* logdet,
                                                 int* bad_out) {
  using dbl2 = double __attribute__((ext_vector_type(2)));
  constexpr int MR = 32;
  double* bufS = buf + 2 * MR;
  const int lane = threadIdx.x;  // wave 0
  const int i = lane & 31, hi = lane >> 5;
  const int M = n + 1;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int q = hi * 16 + u;
    double v = 0.0;
    if (i < M && q < M && !(i == n && q == n)) v = q <= i ? A[i * ld + q] : A[q * ld + i];
    a[u] = v;
  }
  double mypiv = 1.0;
  int bad = 0;
  asm volatile("" ::: "memory");  // the rows are loaded before the buffers are written
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    wave_lds_handoff();  // step k - 1's reads of the row buffers before step k's stores
    if (hi == 0) {
      buf[i] = a[0];
      buf[i + MR] = a[0];
      bufS[i + 1] = a[0];
      bufS[i + 1 + MR] = a[0];
    }
    wave_lds_handoff();  // every lane's stores before the row's reads
    const int s0 = k + hi * 16;  // this half's row entries buf[s0 + u], u = 0..15
    const double* src = (s0 & 1) ? bufS + 1 : buf;
    const double d = buf[k];
    const double aik = buf[i];  // A[i][k]: the low lane's slot 0, for both halves
    double row[16];
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
      const dbl2 v = *reinterpret_cast<const dbl2*>(src + s0 + u);
      row[u] = v.x;
      row[u + 1] = v.y;
    }
    __builtin_amdgcn_sched_barrier(0);  // every read issued before the pivot's arithmetic
    if (!(d > 0.0) && bad == 0) bad = k + 1;
    const bool piv = i == k;
    if (piv) mypiv = d;
    double invd = __builtin_amdgcn_rcp(d);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    const double g = piv ? -invd : aik * invd;
    const double keep = piv ? 0.0 : 1.0;
    // the high lane's old slot 16 -> the low lane's new slot 15
    const double t = swap_halves(fma(-g, row[0], a[0] * keep));
#pragma unroll
    for (int u = 1; u < 16; ++u) a[u - 1] = fma(-g, row[u], a[u] * keep);
    a[15] = hi ? g : t;
  }
  double lp = (hi == 0 && i < n) ? log(mypiv) : 0.0;
  for (int o = 32; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
  *logdet = lp;
  *bad_out = bad;
}

// small_sweep_w for the two-lane rows of small_sweep_half.
__device__ __forceinline__ void small_sweep_w_half(const double (&a)[16], int n, double* wb,
                                                   double* alS, double* al, double* wd) {
  constexpr int MR = 32, LDW = MR | 1;
  const int lane = threadIdx.x;
  const int i = lane & 31, hi = lane >> 5;
  wave_lds_handoff();  // the sweep's last reads of its row buffers (alS) before these stores
  if (hi == 0 && i < n) {
    al[i] = a[0];
    alS[MR - n + i] = a[0];
  }
  wave_lds_handoff();  // alpha in LDS before every lane reads it back
  const double ai = al[min(i, max(n - 1, 0))];
  double alj[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) alj[u] = alS[hi * 16 + u];
  __builtin_amdgcn_sched_barrier(0);
  double* row = wb + min(i, n) * LDW - 1 + hi * 16;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (hi || u > 0) row[u] = fma(ai, alj[u], a[u]);
  wave_lds_handoff();  // both halves' stores before the diagonal is read back
  if (hi == 0 && i < n) wd[i] = wb[i * LDW - 1 + MR - n + i];
}

// The sweep for 64 < n + 1 <= 128 on the four waves: row r = (wave & 1) 64 + lane, the
// wave's column half h = wave >> 1 holding slots 64 h .. 64 h + 63 of that row, rotated as in
// small_sweep_regs (slot q holds column (q + k) mod 128 before step k). One workgroup barrier a
// step: the h = 0 lanes put their slot 0 (A[r][k]) into the step parity's row buffer, then every
// lane reads d, A[r][k] and its 64 row entries; the h = 1 lane's old slot 64 becomes the h = 0
// lane's new slot 63 through the parity's crossing buffer, read after the next step's barrier
// (double-buffered by step parity: a wave is never more than one step ahead). Every thread of
// the workgroup calls it. On return slot q holds column (q + n) mod 128, slot 63 included.
__device__ __forceinline__ void small_sweep4(const double* __restrict__ A, int ld, int n,
                                             double* buf, double (&a)[64], double* logdet,
                                             int* bad_out) {
  using dbl2 = double __attribute__((ext_vector_type(2)));
  constexpr int MR = 128;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = (wv & 1) * 64 + lane, h = wv >> 1;
  const int M = n + 1;
  double* cross = buf + 2 * 520;  // [parity][128]
  double* wsum = cross + 2 * 128;
#pragma unroll
  for (int u = 0; u < 64; ++u) {
    const int q = h * 64 + u;
    double v = 0.0;
    if (r < M && q < M && !(r == n && q == n)) v = q <= r ? A[r * ld + q] : A[q * ld + r];
    a[u] = v;
  }
  double mypiv = 1.0;
  int bad = 0;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    double* B = buf + (k & 1) * 520;
    double* BS = B + 2 * MR;
    if (h == 0) {
      B[r] = a[0];
      B[r + MR] = a[0];
      BS[r + 1] = a[0];
      BS[r + 1 + MR] = a[0];
    }
    __syncthreads();
    if (h == 0 && k > 0) a[63] = cross[((k - 1) & 1) * 128 + r];
    const int s0 = k + h * 64;  // this half's row entries B[s0 + u], u = 0..63
    const double* src = (s0 & 1) ? BS + 1 : B;
    const double d = B[k];
    const double aik = B[r];
    double row[16];
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
      const dbl2 v = *reinterpret_cast<const dbl2*>(src + s0 + u);
      row[u] = v.x;
      row[u + 1] = v.y;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!(d > 0.0) && bad == 0) bad = k + 1;
    const bool piv = r == k;
    if (piv && h == 0) mypiv = d;
    double invd = __builtin_amdgcn_rcp(d);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    invd = fma(invd, fma(-d, invd, 1.0), invd);
    const double g = piv ? -invd : aik * invd;
    const double keep = piv ? 0.0 : 1.0;
    // the h = 1 lane's old slot 64: the h = 0 lane's new slot 63
    if (h == 1) cross[(k & 1) * 128 + r] = fma(-g, row[0], a[0] * keep);
#pragma unroll
    for (int q0 = 0; q0 < 64; q0 += 16) {
      if (q0 > 0) {
#pragma unroll
        for (int u = 0; u < 16; u += 2) {
          const dbl2 v = *reinterpret_cast<const dbl2*>(src + s0 + q0 + u);
          row[u] = v.x;
          row[u + 1] = v.y;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (q0 + u >= 1) a[q0 + u - 1] = fma(-g, row[u], a[q0 + u] * keep);
    }
    a[63] = h ? g : 0.0;  // h = 0: fetched after the next barrier
  }
  __syncthreads();
  if (h == 0) a[63] = cross[((n - 1) & 1) * 128 + r];
  // logdet = sum_k log d_k: the h = 0 waves' sums, wave 0's then wave 1's
  double lp = (h == 0 && r < n) ? log(mypiv) : 0.0;
  for (int o = 32; o > 0; o >>= 1) lp += __shfl_xor(lp, o);
  if (lane == 0 && h == 0) wsum[wv] = lp;
  __syncthreads();
  *logdet = wsum[0] + wsum[1];
  *bad_out = bad;
}

// W = alpha alpha^T - Sigma^{-1} from small_sweep4's rows: alpha into al, W's strictly lower
// part into A (its Sigma is dead since the sweep's loads), diag(W) into wd. Every thread calls it.
__device__ __forceinline__ void small_sweep4_w(const double (&a)[64], int n, double* A, int ld,
                                               double* al, double* wd) {
  constexpr int MR = 128;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = (wv & 1) * 64 + lane, h = wv >> 1;
  if (h == 0 && r < n) al[r] = a[0];
  __syncthreads();
  const double ar = al[min(r, n - 1)];
#pragma unroll
  for (int u = 0; u < 64; ++u) {
    const int j = h * 64 + u - (MR - n);  // the column slot h 64 + u holds (j < 0: none)
    if (j >= 0 && j <= r && r < n) {
      const double w = fma(ar, al[j], a[u]);
      if (j == r) wd[r] = w;
      else A[r * ld + j] = w;
    }
  }
}

// genes up to which the gradient's grid reduction keeps per-thread, per-gene sums
constexpr int SMALL_RED_G = 8;

// (i, c), c <= i, of lower-triangle element q (row by row)
__device__ __forceinline__ void tri_index(int q, int* i_out, int* c_out) {
  int i = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > q) --i;
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  *i_out = i;
  *c_out = q - i * (i + 1) / 2;
}

__device__ __forceinline__ double small_value_grad(const SmallProb P, const SmallMap m,
                                                  int negative, int* bad_out) {
  double* A = m.A;
  const int n = m.n, M = n + 1, ld = m.ld, G = m.G;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const HypDev h{m.hyp, m.hyp + G, m.hyp + 2 * G, G, m.hyp[3 * G]};
  const double sd = m.hyp[3 * G + 1];
  const double sign = negative ? -1.0 : 1.0;
  const int nacc = 2 * G + 1;
  small_sigma(P, m, h, 1);
  for (int t = tid; t < 4 * nacc; t += 256) m.accw[t] = 0.0;
  __syncthreads();
  if (M > 64) {
    // every wave takes part in the sweep below (small_sweep4, one barrier a step): the
    // derivative tables first, by every thread
    if (P.T > 0) {
      const int ngg = (int)grad_tables_doubles(G, P.T);
      for (int q = tid; q < ngg; q += 256) m.gg[q] = grad_table_entry(h, P.T, P.dt, m.tms, q);
    }
    __syncthreads();  // Sigma and r are read by every wave
    // the value: the MLL kernel's own two-wave factor and sums on the same Sigma (A is only
    // read), so that value[p] is lfm_batch_mll_f64's out[p] bit for bit (include/lfm.h); the
    // sweep's pivots give the same number through other roundings. Its column buffers are the
    // sweep's, which is past a barrier from here
    double fmll;
    int fbad;
    {
      double pr, zr;
      small_factor_regs2(A, ld, n, M, m.colbuf, &pr, &zr, &fbad);
      fmll = small_mll_2wave(pr, zr, fbad, n, negative, m.red);
    }
    __syncthreads();  // every thread has read the sums in red and is past the column buffers
    // the four-wave sweep: alpha and -Sigma^{-1}; W from its rows
    double a[64];
    double logdet;
    int bad;
    small_sweep4(A, ld, n, m.colbuf, a, &logdet, &bad);
    small_sweep4_w(a, n, A, ld, m.al, m.wd);
    if (tid == 0) {
      m.red[0] = bad ? __builtin_nan("") : fmll;
      m.red[1] = (double)(bad ? bad : fbad);
    }
  } else if (wv == 0) {
    // one wave: the sweep (small_sweep_regs) gives the MLL's logdet and quadratic form, alpha
    // and -Sigma^{-1} at once; W is written straight from its rows
    auto sweep = [&](auto& a) {
      double logdet;
      int bad;
      small_sweep_regs(A, ld, n, m.colbuf, a, &logdet, &bad);
      small_sweep_w(a, n, m.wb, m.colbuf, m.al, m.wd);
      if (lane == 0) m.red[1] = (double)bad;
    };
    if (M <= 32) {
      // each row on two lanes (small_sweep_half)
      double a[16];
      double logdet;
      int bad;
      small_sweep_half(A, ld, n, m.colbuf, a, &logdet, &bad);
      small_sweep_w_half(a, n, m.wb, m.colbuf, m.al, m.wd);
      if (lane == 0) m.red[1] = (double)bad;
    } else {
      double a[64];
      sweep(a);
    }
  } else {
    if (wv == 1) {
      // The value, beside wave 0's sweep: the MLL kernel's own one-wave factor (small_body's
      // operations on the same Sigma, which both waves only read; a column buffer of its own,
      // m.fcol), so that value[p] is lfm_batch_mll_f64's out[p] bit for bit (include/lfm.h). The
      // sweep's pivots give the same number through other roundings.
      double pr, qp;
      int fbad;
      m.fcol[64 + lane] = 0.0;
      if (M <= 32)
        small_factor_regs<32>(A, ld, n, M, m.fcol, &pr, &qp, &fbad);
      else
        small_factor_regs<64>(A, ld, n, M, m.fcol, &pr, &qp, &fbad);
      double ldp = lane < n ? log(pr) : 0.0;
      for (int o = 32; o > 0; o >>= 1) ldp += __shfl_xor(ldp, o);
      if (lane == 0) {
        const double two_pi = 6.283185307179586476925;
        double mll = -0.5 * ((double)n * log(two_pi) + ldp + qp);
        mll *= negative ? -1.0 : 1.0;
        if (fbad) mll = __builtin_nan("");
        m.red[0] = mll;
        m.red[3] = (double)fbad;
      }
    }
    if (P.T > 0) {
      const int ngg = (int)grad_tables_doubles(G, P.T);
      for (int q = tid - 64; q < ngg; q += 192)
        m.gg[q] = grad_table_entry(h, P.T, P.dt, m.tms, q);
    }
  }
  __syncthreads();
  // one wave: a failure seen by either the sweep or the factor fails the problem
  if (M <= 64 && tid == 0) {
    if (m.red[1] != 0.0) m.red[0] = __builtin_nan("");
    else if (m.red[3] != 0.0) m.red[1] = m.red[3];
  }
  // (W was written by the sweep: small_sweep_w / _half on one wave, small_sweep4_w on four)
  const int np = n * (n + 1) / 2;
  __syncthreads();
  double* aw = m.accw + wv * nacc;  // this wave's partial sums: [0,G) D  [G,2G) S  [2G] l
  // W's strictly lower part: W[i][c] = Wrow[i ldw + c] (one wave: the sweep's row buffer; two
  // waves: A's lower triangle)
  const int ldw = M <= 64 ? small_wb_ld(n) : ld;
  const double* Wrow = M <= 64 ? m.wb + (small_sweep_mr(n) - n - 1) : A;
  if (P.T > 0) {
    const int T = P.T, Wd = 2 * T - 1, nblk = n / T;
    const int nW = G * Wd, nT = G * T;
    const double* Tt = m.gg;           // six Toeplitz tables, table w at Tt + w nW
    const double* Pt = m.gg + 6 * nW;  // eight time tables, table w at Pt + w nT
    // element (i, c), c <= i, of gene block pair (bi, bc): the bracket V of kxx / (D_j + D_k) and
    // its derivatives in D_j, D_k, l, from the derivative tables (grad_grid_kernel's reads)
    auto elem = [&](int bi, int bc, int tau, int tp, int j, int k, double& V, double& Vj,
                    double& Vk, double& Vl) {
      const int d = tp - tau;
      const int kd = k * Wd + (T - 1) + d, jd = j * Wd + (T - 1) - d;
      const double Wk = Tt[kd], Xk = Tt[nW + kd], WkD = Tt[2 * nW + kd], XkD = Tt[3 * nW + kd];
      const double Wkl = Tt[4 * nW + kd], Xkl = Tt[5 * nW + kd];
      const double Wj = Tt[jd], Xj = Tt[nW + jd], WjD = Tt[2 * nW + jd], XjD = Tt[3 * nW + jd];
      const double Wjl = Tt[4 * nW + jd], Xjl = Tt[5 * nW + jd];
      const int kr = k * T + tau, jr = j * T + tau, jc = j * T + tp, kc = k * T + tp;
      const double Pk = Pt[kr], PkD = Pt[nT + kr], Pkl = Pt[2 * nT + kr];
      const double Ej = Pt[3 * nT + jr], EjD = Pt[4 * nT + jr];
      const double Qj = Pt[5 * nT + jr], QjD = Pt[6 * nT + jr], Qjl = Pt[7 * nT + jr];
      const double Pj = Pt[jc], PjD = Pt[nT + jc], Pjl = Pt[2 * nT + jc];
      const double Ek = Pt[3 * nT + kc], EkD = Pt[4 * nT + kc];
      const double Qk = Pt[5 * nT + kc], QkD = Pt[6 * nT + kc], Qkl = Pt[7 * nT + kc];
      const double EE = Ek * Ej, QQ = Qk + Qj;
      V = Wk + Wj - Xk * Pk - Xj * Pj - EE * QQ;
      Vk = WkD - XkD * Pk - Xk * PkD - EkD * Ej * QQ - EE * QkD;
      Vj = WjD - XjD * Pj - Xj * PjD - Ek * EjD * QQ - EE * QjD;
      Vl = Wkl - Xkl * Pk - Xk * Pkl + Wjl - Xjl * Pj - Xj * Pjl - EE * (Qkl + Qjl);
    };
    if (G <= SMALL_RED_G) {
      // every lower element by one thread (np / 256 rounds, no idle lanes), its contributions
      // to the 2G + 1 sums scaled by its gene pair's constants and kept per thread and gene
      // (predicated: the genes are run-time), then one DPP sum per accumulator and wave
      double accD[SMALL_RED_G], accS[SMALL_RED_G], accl = 0.0;
#pragma unroll
      for (int g = 0; g < SMALL_RED_G; ++g) accD[g] = accS[g] = 0.0;

      for (int q = tid; q < np; q += 256) {
        int i, c;
        tri_index(q, &i, &c);
        const int bi = i / T, bc = c / T;
        const int tau = i - bi * T, tp = c - bc * T;
        const int j = m.bgs[bi], k = m.bgs[bc];
        double V, Vj, Vk, Vl;
        elem(bi, bc, tau, tp, j, k, V, Vj, Vk, Vl);
        const double w = i == c ? 0.5 * m.wd[i] : Wrow[i * ldw + c];
        const double iDD = 1.0 / (h.D[j] + h.D[k]);
        const double Cm = h.S[j] * h.S[k] * h.l * kSqrtPi * 0.5 * iDD;
        const double cV = Cm * (w * V);
        const double dj = Cm * (w * Vj) - cV * iDD, dk = Cm * (w * Vk) - cV * iDD;
        const double sj = cV / h.S[j], sk = cV / h.S[k];
        accl += cV / h.l + Cm * (w * Vl);
#pragma unroll
        for (int g = 0; g < SMALL_RED_G; ++g) {
          accD[g] += (j == g ? dj : 0.0) + (k == g ? dk : 0.0);
          accS[g] += (j == g ? sj : 0.0) + (k == g ? sk : 0.0);
        }
      }
#pragma unroll
      for (int g = 0; g < SMALL_RED_G; ++g) {
        if (g < G) {
          const double sD = wave_sum_dpp(accD[g]), sS = wave_sum_dpp(accS[g]);
          if (lane == 63) {
            aw[g] = sD;
            aw[G + g] = sS;
          }
        }
      }
      const double sl = wave_sum_dpp(accl);
      if (lane == 63) aw[2 * G] = sl;
    } else {
      const int nbp = nblk * (nblk + 1) / 2;
      for (int bp = wv; bp < nbp; bp += 4) {
        int bi, bc;
        tri_index(bp, &bi, &bc);
        const int j = m.bgs[bi], k = m.bgs[bc];
        double sV = 0.0, sVj = 0.0, sVk = 0.0, sVl = 0.0;
        for (int e = lane; e < T * T; e += 64) {
          const int tau = e / T, tp = e - tau * T;
          const int i = bi * T + tau, c = bc * T + tp;
          if (c > i) continue;
          double V, Vj, Vk, Vl;
          elem(bi, bc, tau, tp, j, k, V, Vj, Vk, Vl);
          const double w = i == c ? 0.5 * m.wd[i] : Wrow[i * ldw + c];
          sV += w * V;
          sVj += w * Vj;
          sVk += w * Vk;
          sVl += w * Vl;
        }
        sV = wave_sum_dpp(sV);
        sVj = wave_sum_dpp(sVj);
        sVk = wave_sum_dpp(sVk);
        sVl = wave_sum_dpp(sVl);
        if (lane == 0) {
          const double l = h.l, iDD = 1.0 / (h.D[j] + h.D[k]);
          const double Cm = h.S[j] * h.S[k] * l * kSqrtPi * 0.5 * iDD;
          aw[j] += Cm * (sVj - sV * iDD);
          aw[k] += Cm * (sVk - sV * iDD);
          aw[G + j] += Cm * sV / h.S[j];
          aw[G + k] += Cm * sV / h.S[k];
          aw[2 * G] += Cm * (sV / l + sVl);
        }
      }
    }
  } else {
    const double* xs = m.xs;
    for (int q0 = wv * 64; q0 < np; q0 += 256) {
      const int q = q0 + lane;
      PairGrad o{0.0, 0.0, 0.0, 0.0, 0.0};
      int jr = -1, kc = -1;
      if (q < np) {
        int i, c;
        tri_index(q, &i, &c);
        const double w = i == c ? 0.5 * m.wd[i] : Wrow[i * ldw + c];
        const double* xa = xs + 3 * i;
        const double* xb = xs + 3 * c;
        kernel_grad(h, xa[0], xa[1], xa[2], xb[0], xb[1], xb[2], w, o);
        jr = gene_index(xa[1], G);
        kc = gene_index(xb[1], G);
      }
      for (int g = 0; g < G; ++g) {
        const double sD = wave_sum_dpp((jr == g ? o.dDr : 0.0) + (kc == g ? o.dDc : 0.0));
        const double sS = wave_sum_dpp((jr == g ? o.dSr : 0.0) + (kc == g ? o.dSc : 0.0));
        if (lane == 0) {
          aw[g] += sD;
          aw[G + g] += sS;
        }
      }
      const double sl = wave_sum_dpp(o.dl);
      if (lane == 0) aw[2 * G] += sl;
    }
  }
  __syncthreads();
  const bool failed = m.red[1] != 0.0;
  const double nan = __builtin_nan("");
  if (tid < G) {
    const int g = tid;
    const double* acc = m.accw;
    const double aD = ((acc[g] + acc[nacc + g]) + acc[2 * nacc + g]) + acc[3 * nacc + g];
    const double aS =
        ((acc[G + g] + acc[nacc + G + g]) + acc[2 * nacc + G + g]) + acc[3 * nacc + G + g];
    const int bs = n / G;
    double af = 0.0;  // sum over mean block g of alpha_i flag_i (model.py:145-149)
    for (int i = g * bs; i < (g + 1) * bs; ++i) af += m.al[i] * (double)flag_int(m.xs[3 * i + 2]);
    const double D = h.D[g], B = h.B[g];
    m.gout[g] = failed ? nan : sign * (aD - B / (D * D) * af);
    m.gout[G + g] = failed ? nan : sign * aS;
    m.gout[2 * G + g] = failed ? nan : sign * (af / D);
  }
  if (wv == 3) {
    // tr W by the last wave (n <= 127: two entries a lane), summed across it by DPP
    double tr = (lane < n ? m.wd[lane] : 0.0) + (lane + 64 < n ? m.wd[lane + 64] : 0.0);
    tr = wave_sum_dpp(tr);
    if (lane == 63) {
      const double* acc = m.accw;
      const double al_ =
          ((acc[2 * G] + acc[nacc + 2 * G]) + acc[2 * nacc + 2 * G]) + acc[3 * nacc + 2 * G];
      m.gout[3 * G] = failed ? nan : sign * al_;
      m.gout[3 * G + 1] = failed ? nan : sign * sd * tr;
      m.gout[3 * G + 2] = 0.0;  // jitter: a static field (model.py:64), no gradient
    }
  }
  *bad_out = (int)m.red[1];
  const double v = m.red[0];
  __syncthreads();
  return v;
}

// small_value_grad for the fit's step loop, a call of its own: scalar arguments only (the map is
// rebuilt from the dynamic LDS base), so the sweep's register rows are allocated without the
// loop's state beside them (inlined into the loop they spilled)
__device__ __noinline__ double small_value_grad_step(int n, int G, int T, double dt,
                                                     int negative, int* bad_out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  SmallProb P{};  // what small_value_grad reads of it: the sizes (x, y, times, genes are in LDS)
  P.n = n;
  P.G = G;
  P.T = T;
  P.dt = dt;
  SmallMap m;
  small_map(sm, n, G, T, 1, 1, 1, &m);
  return small_value_grad(P, m, negative, bad_out);
}

// value and gradient of one problem of a batch: hyperparameters from dsb / sc (kernel arguments
// or pinned host memory), out[b], the gradient into grad at the problem's packed offsets, then
// (after a system-scope fence) its status word: the host's completion signal
__device__ __forceinline__ void small_grad_one(const SmallProb& P, int negative, int dsb_off,
                                               int sc_off, double* __restrict__ out,
                                               double* __restrict__ grad,
                                               int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, G = P.G, tid = threadIdx.x;
  SmallMap m;
  small_map(sm, n, G, P.T, 1, 1, 0, &m);
  for (int i = tid; i < 3 * G; i += 256) m.hyp[i] = P.dsb[i];
  if (tid < 3) m.hyp[3 * G + tid] = P.sc[tid];
  small_stage(P, m);
  __syncthreads();
  int bad;
  const double v = small_value_grad(P, m, negative, &bad);
  for (int i = tid; i < 3 * G; i += 256) grad[dsb_off + i] = m.gout[i];
  if (tid < 3) grad[sc_off + tid] = m.gout[3 * G + tid];
  if (tid == 0) out[blockIdx.x] = v;
  __threadfence_system();
  __syncthreads();
  if (tid == 0 && status) status[blockIdx.x] = bad;
}

__global__ __launch_bounds__(256) void small_grad_kernel(const SmallProb* __restrict__ probs,
                                                         const int* __restrict__ offs, int nprob,
                                                         int negative, double* __restrict__ out,
                                                         double* __restrict__ grad,
                                                         int* __restrict__ status) {
  const int b = blockIdx.x;
  small_grad_one(probs[b], negative, offs[b], offs[nprob + b], out, grad, status);
}

__global__ __launch_bounds__(256) void small_grad_kernel_args(SmallArgs a) {
  const int b = blockIdx.x;
  SmallProb P = a.probs[b];
  P.dsb = a.hyp + a.dsb_off[b];
  P.sc = a.hyp + a.sc_off[b];
  small_grad_one(P, a.negative, a.dsb_off[b], a.sc_off[b], a.out, a.grad, a.status);
}

// ------------------------------------------------------------- the fit (one workgroup)
// JaxTrainer.fit (trainer.py:162-228) of every problem of a batch, each workgroup stepping its
// problem through nsteps Adam steps without leaving the kernel. Per step, as trainer.py:105-132
// and the host restatement (dis_project_amd/trainer.py, which the tests hold it to):
//   constrain (fit_constrain, lfm_bijectors.h)
//   value and gradient (small_value_grad), history[s] = the value
//   the chain rule, optax.adam and after_epoch of every trainable parameter (fit_update,
//     lfm_bijectors.h) with c1 = 1 - b1^count, c2 = 1 - b2^count from the host (bias[2 s],
//     bias[2 s + 1]: adam_bias, lfm_host.cpp)
// The jitter slot holds the static jitter (constrained) and is never updated.
__global__ __launch_bounds__(256) void small_fit_kernel(SmallFitLaunch a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const SmallProb P = a.probs[b];
  const int n = P.n, G = P.G, nh = 3 * G + 3;
  SmallMap m;
  small_map(sm, n, G, P.T, 1, 1, 1, &m);
  const int od = a.offs[b], os = a.offs[a.nprob + b];
  for (int i = tid; i < nh; i += 256) {
    const int gi = i < 3 * G ? od + i : os + (i - 3 * G);
    m.raw[i] = a.raw[gi];
    m.mu[i] = a.mu[gi];
    m.nu[i] = a.nu[gi];
  }
  small_stage(P, m);
  __syncthreads();
  for (int i = tid; i < nh; i += 256) m.hyp[i] = fit_constrain(i, G, m.raw[i]);
  __syncthreads();
  int first_bad = 0;
  // The loop's scalars read from the arguments once: left to itself the compiler re-reads the
  // argument block inside the step loop, several scalar loads and their waits a step.
  AdamOpt opt = a.opt;
  int negative = a.negative;
  asm volatile("" : "+s"(opt.lr), "+s"(opt.b1), "+s"(opt.b2), "+s"(opt.eps), "+s"(opt.eps_root),
                    "+s"(opt.step0), "+s"(opt.spe), "+s"(opt.fix), "+s"(negative));
  for (int64_t s = 0; s < a.nsteps; ++s) {
    int bad;
    const double v = small_value_grad_step(n, G, P.T, P.dt, negative, &bad);
    if (bad && !first_bad) first_bad = (int)s + 1;
    if (tid == 0) a.history[s * a.nprob + b] = v;
    // the update, after_epoch on the unconstrained leaves, and the next step's constrained model,
    // each parameter by its own thread (one barrier a step); 3G + 2 > 256 parameters (G >= 85)
    // take a second pass
    auto update = [&](int i) {
      const FitSlot u = fit_update(opt, i, G, s, m.raw[i], m.gout[i], m.mu[i], m.nu[i],
                                   a.bias[2 * s], a.bias[2 * s + 1]);
      m.mu[i] = u.mu;
      m.nu[i] = u.nu;
      m.raw[i] = u.x;
      m.hyp[i] = fit_constrain(i, G, u.x);
    };
    if (tid < nh - 1) update(tid);
    if (nh - 1 > 256 && tid + 256 < nh - 1) update(tid + 256);
    __syncthreads();
  }
  for (int i = tid; i < nh; i += 256) {
    const int gi = i < 3 * G ? od + i : os + (i - 3 * G);
    a.raw[gi] = m.raw[i];
    a.mu[gi] = m.mu[i];
    a.nu[gi] = m.nu[i];
  }
  if (tid == 0) a.status[b] = first_bad;
}

static void small_attr(const void* f) {
  hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SMALL_LDS_BYTES);
}

int launch_small_grad(lfm_ctx* ctx, SmallArgs* a, const SmallProb* d_probs, const int* d_offs,
                      int nprob, size_t lds, int negative, double* out, double* grad, int* status) {
  static std::once_flag once;
  std::call_once(once, [] {
    small_attr(reinterpret_cast<const void*>(&small_grad_kernel));
    small_attr(reinterpret_cast<const void*>(&small_grad_kernel_args));
  });
  if (lds > SMALL_LDS_BYTES)
    return set_err(ctx, LFM_E_ARG, "small gradient batch: LDS past 160 KB");
  hipEvent_t ev;
  prof_begin(ctx, K_SMALL_GRAD, &ev, ctx->stream);
  if (a) {
    a->negative = negative;
    a->out = out;
    a->grad = grad;
    a->status = status;
    hipLaunchKernelGGL(small_grad_kernel_args, dim3(nprob), dim3(256), lds, ctx->stream, *a);
  } else {
    hipLaunchKernelGGL(small_grad_kernel, dim3(nprob), dim3(256), lds, ctx->stream, d_probs,
                       d_offs, nprob, negative, out, grad, status);
  }
  prof_end(ctx, K_SMALL_GRAD, ev, 0, 0, ctx->stream);
  return hip_fail(ctx, hipGetLastError(), "small_grad_kernel");
}

int launch_small_fit(lfm_ctx* ctx, const SmallFitLaunch& f, size_t lds) {
  if (lds > SMALL_LDS_BYTES) return set_err(ctx, LFM_E_ARG, "small fit batch: LDS past 160 KB");
  static std::once_flag once;
  std::call_once(once, [] { small_attr(reinterpret_cast<const void*>(&small_fit_kernel)); });
  hipEvent_t ev;
  prof_begin(ctx, K_SMALL_GRAD, &ev, ctx->stream);
  hipLaunchKernelGGL(small_fit_kernel, dim3(f.nprob), dim3(256), lds, ctx->stream, f);
  prof_end(ctx, K_SMALL_GRAD, ev, 0, 0, ctx->stream);
  return hip_fail(ctx, hipGetLastError(), "small_fit_kernel");
}

// ------------------------------------------- batched posterior predictors (small problems)
// latent_predict / multi_gene_predict (src/model.py:420-514) of every problem of a resident
// batch at its own test inputs t (what src/utils.py:144-172 and notebook.py:91-110 call per
// fitted model):
//     S = K(x,x) + diag(diag_vec) + diag_add I = L L^T,  V = L^{-1} K(x,t),  z = L^{-1} (y - m(x)),
//     mean = m(t) + V^T z,   var = diag K(t,t) - sum_k V_k^2,   cov = K(t,t) - V^T V.
// small_post_kernel, grid (problem, split): every workgroup of a problem builds Sigma with
// small_sigma's arithmetic (noise and jitter zero: the caller's diagonal is added after it) and
// factors it column by column in LDS, which leaves L below A's diagonal, 1 / L_ii in invd and
// z in A's row n. It then takes every gridDim.y-th pass of `unit` test columns: the panel
// K(x, t_pass) is filled into LDS by the whole workgroup, then thread c forward-substitutes
// column c against L (L's entries are broadcast reads, the column is the thread's own: no barrier
// inside the substitution) and sums mean and var over k = 0 .. n - 1 in that order. A test
// point's mean / var / V column depend on that point's row of t alone (mean_function's block
// position j // (m / G) apart), not on unit, the split count or m.
// small_post_cov_kernel, one workgroup per 16 x 16 tile of the lower triangles of all the
// problems' covariances: cov_ij = k(t_i, t_j) - sum_k V_ki V_kj from V in HBM (the same sums in
// the same order: diag(cov) is var bit for bit), written to (i, j) and (j, i).
// Not positive definite: status[p] = 1 + the failing column, the problem's outputs NaN.
__global__ __launch_bounds__(256) void small_post_kernel(SmallPostLaunch a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int p = blockIdx.x, split = blockIdx.y, tid = threadIdx.x;
  const SmallProb P = a.probs[p];
  const PostProb pq = a.pp[p];
  const int n = P.n, M = n + 1, G = P.G;
  const int unit = min(a.unit, small_post_cols(n, G, P.T));  // a power of two
  if ((int64_t)split * unit >= pq.m) return;  // no pass of this problem left for this split
  const int tabs = M <= 64;
  SmallMap m;
  double* invd = sm + small_map(sm, n, G, P.T, tabs, 0, 0, &m);
  double* panel = invd + n;
  const int ld = m.ld;
  double* A = m.A;
  const double* dsb = a.hyp + a.offs[p];
  for (int i = tid; i < 3 * G; i += 256) m.hyp[i] = dsb[i];
  if (tid == 0) {
    m.hyp[3 * G] = a.hyp[a.offs[a.nprob + p]];  // l
    m.hyp[3 * G + 1] = 0.0;                     // small_sigma's noise and jitter: none
    m.hyp[3 * G + 2] = 0.0;
    m.red[8] = 0.0;
  }
  small_stage(P, m);
  __syncthreads();
  const HypDev h{m.hyp, m.hyp + G, m.hyp + 2 * G, G, m.hyp[3 * G]};
  small_sigma(P, m, h, tabs);
  __syncthreads();
  const double dadd = a.dadd[p];
  for (int c = tid; c < n; c += 256) {
    const double dv = a.dv ? a.dv[pq.dv_off + c] : 0.0;
    A[c * ld + c] = (A[c * ld + c] + dv) + dadd;
  }
  __syncthreads();
  // right-looking Cholesky of the n + 1 augmented rows, row r on threads r and r + 128 (the
  // columns of its update alternate between them); the diagonal keeps d_c, invd 1 / sqrt(d_c)
  {
    const int r = tid & 127, half = tid >> 7;
    for (int c = 0; c < n; ++c) {
      const double d = A[c * ld + c];
      const double y = 1.0 / sqrt(d);
      if (half == 0 && r > c && r < M) A[r * ld + c] *= y;
      if (tid == 0) {
        invd[c] = y;
        if (!(d > 0.0) && m.red[8] == 0.0) m.red[8] = (double)(c + 1);
      }
      __syncthreads();
      if (r > c && r < M) {
        const double lrc = A[r * ld + c];
        const int qe = min(r, n - 1);
        for (int q = c + 1 + half; q <= qe; q += 2)
          A[r * ld + q] = fma(-lrc, A[q * ld + c], A[r * ld + q]);
      }
      __syncthreads();
    }
  }
  const int bad = (int)m.red[8];
  if (split == 0 && tid == 0) a.status[p] = bad;
  const double* z = A + n * ld;
  const double* tp = a.t + 3 * pq.t_off;
  const int64_t bs = pq.m / G;  // mean_function's block of the test inputs
  const double nan = __builtin_nan("");
  const int lu = __ffs(unit) - 1;
  for (int64_t j0 = (int64_t)split * unit; j0 < pq.m; j0 += (int64_t)gridDim.y * unit) {
    if (!bad) {
      for (int e = tid; e < n * unit; e += 256) {
        const int i = e >> lu, c = e & (unit - 1);
        const int64_t j = j0 + c;
        if (j < pq.m) {
          const double* xi = m.xs + 3 * i;
          const double* tj = tp + 3 * j;
          panel[e] = kernel_ref(h, xi[0], xi[1], xi[2], tj[0], tj[1], tj[2]);
        }
      }
    }
    __syncthreads();
    const int64_t j = j0 + tid;
    if (tid < unit && j < pq.m) {
      double mean = nan, var = nan;
      if (!bad) {
        double macc = 0.0, vacc = 0.0;
        for (int i = 0; i < n; ++i) {
          const double* Li = A + i * ld;
          double s = panel[i * unit + tid];
          for (int k = 0; k < i; ++k) s = fma(-Li[k], panel[k * unit + tid], s);
          const double v = s * invd[i];
          panel[i * unit + tid] = v;
          macc = fma(v, z[i], macc);
          vacc = fma(v, v, vacc);
          if (a.V) a.V[pq.v_off + (int64_t)i * pq.m + j] = v;
        }
        const double* tj = tp + 3 * j;
        mean = mean_at(h, tp, j, bs) + macc;
        var = kernel_ref(h, tj[0], tj[1], tj[2], tj[0], tj[1], tj[2]) - vacc;
      }
      a.mean[pq.t_off + j] = mean;
      if (a.var) a.var[pq.t_off + j] = var;
    }
    __syncthreads();  // the pass's columns are done before the next pass fills the panel
  }
}

__global__ __launch_bounds__(256) void small_post_cov_kernel(SmallPostLaunch a) {
  __shared__ double Vi[SMALL_GRAD_MAX * 16], Vj[SMALL_GRAD_MAX * 16];
  const int tid = threadIdx.x;
  // the problem of this tile: the last one whose first tile is not past it
  int lo = 0, hi = a.nprob - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.pp[mid].tile0 <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const int p = lo;
  const PostProb pq = a.pp[p];
  const int n = a.probs[p].n, G = a.probs[p].G, mt = pq.m;
  int ti, tj;
  tri_index((int)blockIdx.x - pq.tile0, &ti, &tj);
  const int bad = a.status[p];
  const double* V = a.V + pq.v_off;
  if (!bad) {
    for (int e = tid; e < n * 16; e += 256) {
      const int k = e >> 4, c = e & 15;
      const int ci = ti * 16 + c, cj = tj * 16 + c;
      Vi[e] = ci < mt ? V[(int64_t)k * mt + ci] : 0.0;
      Vj[e] = cj < mt ? V[(int64_t)k * mt + cj] : 0.0;
    }
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  const int i = ti * 16 + ty, j = tj * 16 + tx;
  if (i >= mt || j > i) return;
  double v = __builtin_nan("");
  if (!bad) {
    const double* dsb = a.hyp + a.offs[p];
    const HypDev h{dsb, dsb + G, dsb + 2 * G, G, a.hyp[a.offs[a.nprob + p]]};
    double acc = 0.0;
    for (int k = 0; k < n; ++k) acc = fma(Vi[k * 16 + ty], Vj[k * 16 + tx], acc);
    const double* xi = a.t + 3 * (pq.t_off + i);
    const double* xj = a.t + 3 * (pq.t_off + j);
    v = kernel_ref(h, xi[0], xi[1], xi[2], xj[0], xj[1], xj[2]) - acc;
  }
  double* cov = a.cov + pq.cov_off;
  cov[(int64_t)i * mt + j] = v;
  cov[(int64_t)j * mt + i] = v;
}

int launch_small_post(lfm_ctx* ctx, const SmallPostLaunch& f, size_t lds) {
  if (lds > SMALL_LDS_BYTES)
    return set_err(ctx, LFM_E_ARG, "small posterior batch: LDS past 160 KB");
  static std::once_flag once;
  std::call_once(once, [] { small_attr(reinterpret_cast<const void*>(&small_post_kernel)); });
  hipEvent_t ev;
  prof_begin(ctx, K_SMALL_POST, &ev, ctx->stream);
  hipLaunchKernelGGL(small_post_kernel, dim3(f.nprob, f.nsplit), dim3(256), lds, ctx->stream, f);
  if (f.cov)
    hipLaunchKernelGGL(small_post_cov_kernel, dim3(f.ntiles), dim3(256), 0, ctx->stream, f);
  prof_end(ctx, K_SMALL_POST, ev, 0, 0, ctx->stream);
  return hip_fail(ctx, hipGetLastError(), "small_post_kernel");
}

// the MLL kernels' LDS limit raised to a CU's (SMALL_LDS_BYTES), once per process (before any
// launch or stream capture that uses them)
void small_batch_attrs() {
  static std::once_flag once;
  std::call_once(once, [] {
    small_attr(reinterpret_cast<const void*>(&small_mll_kernel));
    small_attr(reinterpret_cast<const void*>(&small_mll_kernel_args));
  });
}

int launch_small_args(lfm_ctx* ctx, SmallArgs& a, int nprob, const SmallMllPlan& plan) {
  const size_t lds = plan.lds_bytes;
  if (lds > SMALL_LDS_BYTES || nprob > SMALL_ARG_PROBS)
    return set_err(ctx, LFM_E_ARG, "small batch (kernel arguments): past its limits");
  a.tabs = plan.tabs;
  small_batch_attrs();
  hipEvent_t ev;
  prof_begin(ctx, K_SMALL, &ev, ctx->stream);
  hipLaunchKernelGGL(small_mll_kernel_args, dim3(nprob), dim3(256), lds, ctx->stream, a);
  prof_end(ctx, K_SMALL, ev, 0, 0, ctx->stream);
  return hip_fail(ctx, hipGetLastError(), "small_mll_kernel_args");
}

int launch_small_batch(lfm_ctx* ctx, const SmallProb* d_probs, int nprob, const SmallMllPlan& plan,
                       int negative, double* d_out, int* d_status) {
  const size_t lds = plan.lds_bytes;
  if (lds > SMALL_LDS_BYTES)
    return set_err(ctx, LFM_E_ARG, "small batch: LDS past 160 KB (n <= 128, grid tables <= "
                                   "SMALL_GRID_TAB_MAX)");
  small_batch_attrs();
  hipEvent_t ev;
  prof_begin(ctx, K_SMALL, &ev, ctx->stream);
  hipLaunchKernelGGL(small_mll_kernel, dim3(nprob), dim3(256), lds, ctx->stream,
                     d_probs, negative, d_out, d_status, plan.tabs);
  prof_end(ctx, K_SMALL, ev, 0, 0, ctx->stream);
  return hip_fail(ctx, hipGetLastError(), "small_mll_kernel");
}

}  // namespace lfm
