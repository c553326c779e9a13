// lfm_host.cpp — host-only logic of liblfm (lfm_host.h): plain C++, compiled into liblfm.so and
// into the host sanitizer check (tests/native/host_check.cpp).
#include "lfm_host.h"

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstring>

namespace lfm {

GridLayout detect_grid(const double* x, int64_t n, int64_t G) {
  GridLayout L;
  if (!x || n < 1 || G < 1 || n > INT_MAX || G > INT_MAX) return L;
  const int g0 = gene_index(x[1], (int)G);
  int64_t T = 1;
  while (T < n && gene_index(x[3 * T + 1], (int)G) == g0) ++T;
  if (n % T != 0) return L;
  const int64_t nblk = n / T;
  L.times.resize(T);
  for (int64_t t = 0; t < T; ++t) L.times[t] = x[3 * t];
  L.block_gene.resize(nblk);
  for (int64_t b = 0; b < nblk; ++b) {
    const int gb = gene_index(x[3 * b * T + 1], (int)G);
    L.block_gene[b] = gb;
    for (int64_t t = 0; t < T; ++t) {
      const double* r = x + 3 * (b * T + t);
      if (r[2] != 1.0) return GridLayout();                    // all rows gene rows (flag 1)
      if (gene_index(r[1], (int)G) != gb) return GridLayout(); // one gene per block
      if (std::memcmp(&r[0], &L.times[t], sizeof(double)) != 0) return GridLayout();  // shared
    }
  }
  const double t0 = L.times[0];
  const double dt = T > 1 ? (L.times[T - 1] - t0) / (double)(T - 1) : 0.0;
  double scale = 1.0;
  for (double t : L.times) scale = std::max(scale, std::fabs(t));
  for (int64_t t = 0; t < T; ++t)
    if (!(std::fabs(L.times[t] - (t0 + (double)t * dt)) <= 1e-12 * scale)) return GridLayout();
  L.T = (int)T;
  L.nblk = (int)nblk;
  L.t0 = t0;
  L.dt = dt;
  L.ok = true;
  return L;
}

std::vector<std::pair<int64_t, int>> plan_steps(int64_t nblk, int64_t Mp, int nb, bool bordered,
                                                bool s3, int wbulk, int64_t w4min,
                                                int64_t w2min, int w0) {
  std::vector<std::pair<int64_t, int>> steps;
  for (int64_t k = 0; k < nblk;) {
    const int64_t m = bordered ? Mp + nb : Mp - k * nb;
    int w = 1;
    // the first bulk super-panel stays 4 wide: its chain runs beside the shallow first update
    const int wk = steps.size() == 1 ? 4 : wbulk;
    if (m >= w4min && k + wk <= nblk) w = wk;
    else if (m >= w4min && k + 4 <= nblk) w = 4;
    else if (m >= w2min && k + 2 <= nblk) w = 2;
    if (k == 0 && s3) w = (w0 == 2 && nblk >= 2) ? 2 : 1;
    steps.emplace_back(k, w);
    k += w;
  }
  return steps;
}

void rest_unit_tile(int64_t b, int T, int tj_lo, int Q, int* ti_out, int* tj_out) {
  constexpr int SUB = 2;  // 64-row slabs per 128-row tile
  const int sub = (int)(b % SUB);
  b /= SUB;
  int a = (int)((std::sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((int64_t)(a + 1) * (a + 2) / 2 <= b) ++a;
  while ((int64_t)a * (a + 1) / 2 > b) --a;
  int tj, ti;
  if (Q > 1) {
    const int R = a / Q, r0 = R * Q, qr = std::min(Q, T - tj_lo - r0);
    const int64_t off = b - (int64_t)r0 * (r0 + 1) / 2;
    const int64_t full = (int64_t)R * qr * Q;
    int lr, lc;
    if (off < full) {
      const int C = (int)(off / (qr * Q)), t = (int)(off % (qr * Q));
      lr = t / Q;
      lc = C * Q + t % Q;
    } else {
      const int d = (int)(off - full);
      lr = (int)((std::sqrt(8.0 * (double)d + 1.0) - 1.0) * 0.5);
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
  *ti_out = ti;
  *tj_out = tj;
}

int64_t helper_units(int kd, int na, int nr, int nt, int wnext, int nb, int cus, int side_cus,
                     double tc, double dmin) {
  if (kd <= 0 || side_cus <= 0 || cus <= side_cus) return 0;
  const double t = 154.0 * kd / 640.0 + 4.0;  // one depth-kd unit, us (step timeline)
  const double o = 0.9;
  const double sm = 4.0 * (cus - side_cus), sh = 4.0 * side_cus;
  const double tall_eq = (double)nt * (wnext + 1) / 2.0 * nb / kd;
  const double units = (double)na + nr + tall_eq;
  const double d0 = units * t / (sm * o);
  if (d0 < dmin) return 0;
  const double x = o * (d0 - tc) / (t * (1.0 / sh + 1.0 / sm));
  return std::max<int64_t>(0, std::min<int64_t>((int64_t)x, nr / 2));
}

int64_t helper_clamp(int64_t hu, int nr, int T, int wn, int lead, int Q) {
  // a rest region of at most 8 tile columns is enumerated on the device as a band, column by
  // column (lfm_chol.hip unit_tile), not as this triangle: no helper there (its tail would be
  // the last columns, lead tiles included)
  if (hu <= 0 || T - wn <= kBandMaxCols) return 0;
  Q = std::max(Q, 1);
  const int64_t r0e = std::min<int64_t>((int64_t)(lead + Q - 1) / Q * Q, (int64_t)T - wn);
  hu = std::min<int64_t>(hu, (int64_t)nr - r0e * (r0e + 1));  // 2 slabs per triangle tile
  if (hu <= 0) return 0;
  for (int64_t b = nr - hu; b < nr; ++b) {
    int ti, tj;
    rest_unit_tile(b, T, wn, Q, &ti, &tj);
    if (ti / 2 < wn + lead && tj < wn + lead) return 0;
  }
  return hu;
}

namespace {
// Algorithmic flops (profiling) of rest units [b0, b1) of a step's update: 2 kd per updated
// lower element of their tiles, rows past n (identity padding) excluded
double units_alg(const S3Params& p, int64_t s0, int T, int wn, int kd, int64_t b0, int64_t b1) {
  double a = 0.0;
  for (int64_t b = b0; b < b1; ++b) {
    int ti, tj;
    rest_unit_tile(b, T, wn, p.supertile, &ti, &tj);
    const int64_t i0 = s0 + (int64_t)ti * 64, j0 = s0 + (int64_t)tj * p.st;
    for (int64_t r = i0; r < i0 + 64 && (p.bordered || r <= p.n); ++r)
      a += (double)std::max<int64_t>(0, std::min<int64_t>(p.st, r - j0 + 1));
  }
  return a * 2.0 * kd;
}

// Flops of one step-kernel launch: the update of step u with nr_main of its rest units (u NULL:
// none) and the tall units of step t (NULL: none); alg_adjust: algorithmic flops of the update
// done elsewhere (the helper's tail, a kernel class of its own).
// issued: every 64 x 128 unit in full (padding rows included), tall units as GEMMs with the
// triangular inverse; algorithmic: the update of the unpadded augmented trailing matrix (rows
// s0 .. n, residual row n included: it is the forward substitution) less the next diagonal
// block (the chain's), and the triangular solve of the rows below the next super-panel (rows
// .. n) against its W' x W' factor
void launch_flops(const S3Params& p, const S3Step* u, int64_t nr_main, const S3Step* t,
                  double alg_adjust, double* alg_out, double* issued_out) {
  const int NB = p.nb, ST = p.st;
  const int na = u ? u->na : 0, kd = u ? u->w * NB : 0;
  const int nr = u ? (int)nr_main : 0, nt = t ? t->nt : 0, tw = t ? t->tw : 0;
  *issued_out = ((double)na + nr) * 64 * ST * 2.0 * kd +
                (double)nt * 64 * (ST / p.tall_split) * NB * (tw + 1);
  double alg = 0.0;
  if (na + nr > 0) {
    // bordered: the whole Mp-row window is algorithmic (Cholesky + inverse = Mp^3)
    const double m = p.bordered ? (double)p.Mp : (double)(p.n - u->K1);
    const double d = std::min<double>(u->wn * NB, m);
    alg += 2.0 * kd * (m * (m + 1) / 2 + (p.bordered ? 0.0 : m) - d * (d + 1) / 2);
  }
  if (nt > 0) {
    const double W2 = (double)tw * NB;
    const int64_t rows = p.bordered ? t->tk0 + p.Mp - t->tr0 : p.n + 1 - t->tr0;
    alg += (double)std::max<int64_t>(0, rows) * W2 * W2;
  }
  *alg_out = alg - alg_adjust;
}
}  // namespace

S3Plan plan_s3(const std::vector<std::pair<int64_t, int>>& steps, const S3Params& p) {
  S3Plan P;
  P.params = p;
  P.step_list = steps;
  const int S = (int)steps.size(), NB = p.nb, ST = p.st;
  const int64_t n = p.n, Mp = p.Mp;
  // the trailing matrix of a step whose super-panel ends at column K1: rows / columns [K1, Mp)
  // (MLL), or the Mp-row window [K1, K1 + Mp) the identity border has reached (bordered: rows
  // Mp + j are zero in panel columns < j; the window size is constant)
  auto rows_end = [&](int64_t K1) { return p.bordered ? K1 + Mp : Mp; };
  P.S = S;
  int wmax = 1;
  for (const auto& st : steps) wmax = std::max(wmax, st.second);
  const int64_t Wmax = P.Wmax = (int64_t)wmax * NB, Tmax = P.Tmax = Mp / ST + 1;
  // two workspaces: chain(s + 1) starts while the tall units of step s still read Bd_s
  P.wk_bytes = (size_t)4 * Wmax * Wmax * sizeof(double);
  P.xbuf_bytes = (size_t)2 * Mp * Wmax * sizeof(double);
  P.zvec_bytes = (size_t)Mp * sizeof(double);
  P.linv_bytes = (size_t)NB * NB * sizeof(double);
  P.xd_bytes = (size_t)Wmax * Wmax * sizeof(double);
  P.nflags = (size_t)S * (3 + Tmax);
  P.flags_bytes = P.nflags * sizeof(unsigned);
  P.chain_done = 0;
  P.a_done = (size_t)S;
  P.bars = P.a_done + (size_t)S * Tmax;  // grid barrier counters of chain(s)
  P.xready = P.bars + S;                 // inputs of chain(s) landed (s >= 1)
  // MLL: rows past n are identity padding whose updates nothing reads; bordered: none is
  // skipped (the border rows have real entries in the padding columns, which are eliminated
  // too, so the padding rows' X must exist)
  P.pad_end = p.bordered ? n + 1 : INT64_MAX;
  P.zsplit = n;  // finalize: z columns below zsplit come from zvec
  P.nevents = chol_events(S);
  P.steps.resize(S);
  for (int s = 0; s < S; ++s) {
    S3Step& q = P.steps[s];
    q.w = steps[s].second;
    q.kd = q.w * NB;
    q.K0 = steps[s].first * NB;
    q.K1 = (steps[s].first + steps[s].second) * NB;
    q.wn = s + 1 < S ? steps[s + 1].second : 0;
    q.T = (int)((rows_end(q.K1) - q.K1) / ST);
    // update of step s (trailing matrix from K1), excluding the next diagonal block (none after
    // the last super-panel: the bordered mode's final update of its border block)
    q.na = 2 * q.wn * (q.T - q.wn);
    q.nr = (q.T - q.wn) * (q.T - q.wn + 1);  // two 64-row units per tile of the triangle
    // tall units of step s: rows [K1, rows_end) x w column blocks
    q.nt = (int)((rows_end(q.K1) - q.K1) / 64 * q.w * p.tall_split);
    q.tr0 = q.K0 + (int64_t)q.w * NB;
    q.tk0 = q.K0;
    q.tw = q.w;
    if (p.bordered) q.zero_from = q.copy_from = Mp + q.K0;
    q.gen = p.fused && s == 0;
    // launch s writes the inputs of chain(s + 2): the block's tiles (leading rest units,
    // w (w + 1) 64-row slabs) and its rows of the columns of super-panel s + 1 (leading ahead
    // units, 2 w w_{s+1} slabs); chain(s + 2) forms X_{s+1} of its rows
    if (s + 2 < S) q.lead = steps[s + 2].second;
    if (s >= 2) q.xtarget = (unsigned)(q.w * (q.w + 1) + 2 * q.w * steps[s - 1].second);
    q.nr_main = q.nr;
    q.f_done = P.chain_done + s;
    q.f_adone = P.a_done + (size_t)s * Tmax;
    q.f_bar = P.bars + s;
    q.f_xready = P.xready + s;
    q.wk_off = (size_t)(s & 1) * 2 * Wmax * Wmax;
    q.bd_off = q.wk_off + (size_t)((int64_t)q.w * NB * q.w * NB);
    q.x_off = (size_t)(s & 1) * Mp * Wmax;
    q.ugrid = pad8(q.na) + pad8(q.nr);
    q.tgrid = tall_grid(q.nt, p.tall_split);
    launch_flops(p, &q, q.nr, nullptr, 0.0, &q.upd_alg, &q.upd_issued);
    launch_flops(p, nullptr, 0, &q, 0.0, &q.tall_alg, &q.tall_issued);
    // chain(s), algorithmic: the block's factor W^3 / 3, its pending update from X_{s-1} (the
    // block's lower elements x 2 kd) and its rows of X_{s-1} (W kd^2); issued adds the block
    // inverse (W^3) and the padded 32 x 32 tiles
    const double W = q.w * NB, kd = s > 0 ? steps[s - 1].second * NB : 0;
    q.chain_alg = W * W * W / 3.0 + W * (W + 1) * kd + W * kd * kd;
    q.chain_issued = W * W * W / 3.0 + W * W * W + W * W * kd + 2.0 * W * kd * kd;
  }
  bool tail_marked = false;
  for (int s = 0; s < S; ++s) {
    S3Step& q = P.steps[s];
    if (s + 1 == S) {  // the last super-panel: only the bordered mode updates past it
      q.grid = p.bordered ? q.ugrid : 0;
      q.step_alg = q.upd_alg;
      q.step_issued = q.upd_issued;
      break;
    }
    const S3Step& nx = P.steps[s + 1];
    // Side-CU helper: the tail of this step's rest units, sized to end with the main launch
    // (helper_units), never a lead tile of chain(s + 2) (helper_clamp)
    if (p.helper && s >= 1 && s + 2 < S)
      q.hu = helper_clamp(helper_units(q.w * NB, q.na, q.nr, nx.nt / p.tall_split, nx.w, NB,
                                       p.cus, p.side_cus, p.helper_tc, p.helper_min),
                          q.nr, q.T, q.wn, q.lead, p.supertile);
    q.nr_main = (int)(q.nr - q.hu);
    if (p.prof && q.hu > 0)
      q.helper_alg = units_alg(p, q.K1, q.T, q.wn, q.w * NB, q.nr_main, q.nr);
    q.helper_issued = (double)q.hu * 64 * ST * 2.0 * (q.w * NB);
    q.hgrid = pad8((int)q.hu);
    q.grid = pad8(q.na) + pad8(q.nr_main) + nx.tgrid;
    launch_flops(p, &q, q.nr_main, &nx, q.helper_alg, &q.step_alg, &q.step_issued);
    // overlapped: the next evaluation may start once the launches before this evaluation's
    // tail have run (its first step below ovl_at trailing rows)
    if (!tail_marked && s >= 1 && rows_end(q.K1) - q.K1 < p.ovl_at) q.ovl_mark = tail_marked = true;
  }
  return P;
}

bool plan_s3_keep(S3Plan& kept, const std::vector<std::pair<int64_t, int>>& steps,
                  const S3Params& p) {
  if (kept.params == p && kept.step_list == steps) return false;
  kept = plan_s3(steps, p);
  return true;
}

// ------------------------------------------------------------ the small-problem path
SmallDims small_dims(const std::vector<SmallShape>& shapes) {
  SmallDims d;
  for (const SmallShape& s : shapes) {
    d.maxn = std::max(d.maxn, s.n);
    d.maxg = std::max(d.maxg, s.G);
    if (s.T) d.gridtab = std::max(d.gridtab, (int)small_grid_extra(s.n, s.G, s.T));
  }
  return d;
}

SmallMllPlan plan_small_mll(const SmallDims& d) {
  const int tabs = d.maxn + 1 <= 64;
  return {(small_map(nullptr, d.maxn, d.maxg, 0, tabs, 0, 0, nullptr) + (size_t)d.gridtab) *
              sizeof(double),
          tabs};
}

size_t small_grad_lds(const std::vector<SmallShape>& shapes, int fit) {
  size_t mx = 0;
  for (const SmallShape& s : shapes) {
    if (s.n > SMALL_GRAD_MAX) return 0;
    mx = std::max(mx, small_map(nullptr, s.n, s.G, s.T, 1, 1, fit, nullptr));
  }
  return mx * sizeof(double) > SMALL_LDS_BYTES ? 0 : mx * sizeof(double);
}

SmallPack plan_small_pack(const std::vector<SmallShape>& shapes, bool hyp_inline) {
  SmallPack P;
  P.at.reserve(shapes.size());
  size_t off = 0;
  for (const SmallShape& s : shapes) {
    const size_t n = (size_t)s.n, nh = hyp_inline ? 3 * (size_t)s.G + 3 : 0;
    const size_t grid = off + 4 * n + nh;
    P.at.push_back({off, off + 3 * n, off + 4 * n, grid - (nh ? 3 : 0), grid});
    off = grid + (s.T ? (size_t)s.T + ((size_t)s.n / s.T + 1) / 2 : 0);
    P.bound += 4 * n + nh + (size_t)small_grid_doubles(s.n);
  }
  return P;
}

BatchLayout batch_layout(int64_t nhyp, int64_t nprob) {
  BatchLayout L;
  L.out = (size_t)nhyp;
  L.status = L.out + (size_t)nprob;
  L.grad = L.status + (size_t)nprob;
  L.bytes = (L.grad + (size_t)nhyp) * sizeof(double);
  return L;
}

FitLayout fit_layout(int64_t nhyp, int64_t nprob, int64_t nsteps) {
  FitLayout L;
  L.mu = (size_t)nhyp;
  L.nu = 2 * (size_t)nhyp;
  L.bias = 3 * (size_t)nhyp;
  L.hist = L.bias + 2 * (size_t)nsteps;
  L.status = L.hist + (size_t)nsteps * nprob;
  L.bytes = L.status * sizeof(double) + (size_t)nprob * sizeof(int);
  return L;
}

void adam_bias(const lfm_adam* opt, int64_t step0, int64_t nsteps, double* out) {
  for (int64_t s = 0; s < nsteps; ++s) {
    const double count = (double)(step0 + s + 1);
    out[2 * s] = 1.0 - std::pow(opt->b1, count);
    out[2 * s + 1] = 1.0 - std::pow(opt->b2, count);
  }
}

PostPlan plan_small_post(const std::vector<SmallShape>& shapes, int64_t nhyp, const int64_t* m,
                         bool has_dv, bool has_cov) {
  auto rejected = [](PostPlan::Reject why) {
    PostPlan R;
    R.reject = why;
    return R;
  };
  const size_t np = shapes.size();
  PostPlan P;
  P.pp.resize(np);
  // nsplit for either unit: which one holds is known once every problem's passes are counted
  int64_t ntiles = 0, wg64 = 0, split64 = 1, split256 = 1;
  size_t lds = 0;
  for (size_t p = 0; p < np; ++p) {
    const SmallShape& s = shapes[p];
    if (m[p] < 1 || m[p] % s.G != 0 || m[p] > (1 << 20)) return rejected(PostPlan::BAD_M);
    const int cols = small_post_cols(s.n, s.G, s.T);
    if (!cols) return rejected(PostPlan::NO_FIT);
    const int64_t tb = (m[p] + 15) / 16;
    P.pp[p] = PostProb{P.sm, P.sv, P.sc, (int)m[p], (int)P.sn, (int)ntiles, 0};
    P.sm += m[p];
    P.sn += s.n;
    P.sv += has_cov ? s.n * m[p] : 0;
    P.sc += has_cov ? m[p] * m[p] : 0;
    ntiles += has_cov ? tb * (tb + 1) / 2 : 0;
    wg64 += (m[p] + 63) / 64;
    if (P.sm > ((int64_t)1 << 28) || P.sc > ((int64_t)1 << 29) || ntiles > INT_MAX / 2)
      return rejected(PostPlan::TOO_LARGE);
    const int u64 = std::min(64, cols);
    split64 = std::max(split64, (m[p] + u64 - 1) / u64);
    split256 = std::max(split256, (m[p] + cols - 1) / cols);
    lds = std::max(lds, small_post_base(s.n, s.G, s.T) + (size_t)s.n * cols);
  }
  P.unit = wg64 <= 4096 ? 64 : 256;
  P.nsplit = (int)std::min<int64_t>(P.unit == 64 ? split64 : split256, 1024);
  P.ntiles = (int)ntiles;
  P.lds_bytes = lds * sizeof(double);
  P.dadd = (size_t)nhyp;
  P.dv = P.dadd + np;
  P.t = P.dv + (has_dv ? (size_t)P.sn : 0);
  P.table = P.t + 3 * (size_t)P.sm;
  P.in_bytes = P.table * sizeof(double) + np * sizeof(PostProb);
  P.mean = P.in_bytes / sizeof(double);
  P.var = P.mean + (size_t)P.sm;
  P.V = P.var + (size_t)P.sm;
  P.cov = P.V + (size_t)P.sv;
  P.status = P.cov + (size_t)P.sc;
  P.all_bytes = P.status * sizeof(double) + np * sizeof(int);
  return P;
}

namespace {
// flock, restarted when a signal interrupts the wait; 0 or the errno of the failure
int flock_retry(int fd, int op) {
  for (;;) {
    if (::flock(fd, op) == 0) return 0;
    if (errno != EINTR) return errno;
  }
}

// flock needs no write access: a file another user created (mode 0666 less their umask) is
// opened read-only rather than dropping to in-process locking
int open_lock_file(const std::string& p) {
  int fd = ::open(p.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
  if (fd < 0 && errno == EACCES) fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
  return fd;
}
}  // namespace

bool TenancyLock::open(const std::string& path) {
  std::lock_guard<std::mutex> lk(open_mu_);
  if (opened_) return ok_;
  opened_ = true;
  path_ = path;
  if (path.size() < 5 || path.compare(path.size() - 5, 5, ".lock") != 0) return ok_ = false;
  fd_ = open_lock_file(path);
  turn_ = open_lock_file(path.substr(0, path.size() - 5) + ".turn");
  if (fd_ < 0 || turn_ < 0) {
    if (fd_ >= 0) ::close(fd_);
    if (turn_ >= 0) ::close(turn_);
    fd_ = turn_ = -1;
    return ok_ = false;
  }
  return ok_ = true;
}

std::string TenancyLock::path() {
  std::lock_guard<std::mutex> lk(open_mu_);
  return path_;
}

// The first flock failure (ENOLCK on a filesystem without locks, EBADF, ...) turns the
// cross-process part off for good: logged once with the cause, so a later schedule-3 stall
// beside another process can be traced to the missing lock; the in-process lock still holds.
bool TenancyLock::files() const { return fd_ >= 0 && err_.load(std::memory_order_acquire) == 0; }

void TenancyLock::fail(int e, const char* what) {
  int expected = 0;
  if (err_.compare_exchange_strong(expected, e))
    std::fprintf(stderr,
                 "liblfm: flock(%s) on %s failed: %s; the schedule-3 tenancy lock is in-process "
                 "only from now on (another process on this GPU can stall schedule 3)\n",
                 what, path_.c_str(), std::strerror(e));
}

void TenancyLock::lock_exclusive() {
  rw_.lock();
  if (files()) {
    std::lock_guard<std::mutex> tl(turn_mu_);
    // readers arriving from now on wait at the turnstile, then the readers already in drain
    if (int e = flock_retry(turn_, LOCK_EX)) return fail(e, "turnstile, exclusive");
    if (int e = flock_retry(fd_, LOCK_EX)) fail(e, "lock, exclusive");
    else fd_held_ = true;
    if (int e = flock_retry(turn_, LOCK_UN)) fail(e, "turnstile, release");
  }
}

void TenancyLock::unlock_exclusive() {
  if (fd_held_) {
    fd_held_ = false;
    if (int e = flock_retry(fd_, LOCK_UN)) fail(e, "lock, release");
  }
  rw_.unlock();
}

void TenancyLock::lock_shared() {
  rw_.lock_shared();
  if (fd_ < 0) return;
  if (files()) {
    std::lock_guard<std::mutex> tl(turn_mu_);
    // behind any writer waiting in another process
    if (int e = flock_retry(turn_, LOCK_EX)) fail(e, "turnstile, shared");
    else if (int e2 = flock_retry(turn_, LOCK_UN)) fail(e2, "turnstile, release");
  }
  // every shared holder is counted, whatever the file lock's state: the LOCK_SH taken by the
  // first is released by the last (sh_held_), also if a failure turned the files off between
  std::lock_guard<std::mutex> fl(fd_mu_);
  if (readers_++ == 0 && files()) {
    if (int e = flock_retry(fd_, LOCK_SH)) fail(e, "lock, shared");
    else sh_held_ = true;
  }
}

void TenancyLock::unlock_shared() {
  if (fd_ >= 0) {
    std::lock_guard<std::mutex> fl(fd_mu_);
    if (--readers_ == 0 && sh_held_) {
      sh_held_ = false;
      if (int e = flock_retry(fd_, LOCK_UN)) fail(e, "lock, release");
    }
  }
  rw_.unlock_shared();
}

TenancyLock::~TenancyLock() {
  if (fd_ >= 0) ::close(fd_);
  if (turn_ >= 0) ::close(turn_);
}

// ------------------------------------------------- resident posterior (lfm_post.hip)
int64_t post_default_chunk(int64_t Np) {
  const int64_t fit = (int64_t)(POST_VT_BUDGET / ((size_t)Np * sizeof(double)));
  return std::min(POST_CHUNK_MAX, std::max<int64_t>(fit / 128 * 128, 128));
}

ResidentPlan plan_post(int64_t n, int64_t G, int64_t m, int64_t chunk, bool want_cov) {
  ResidentPlan P;
  P.n = n;
  P.Np = (n + 127) / 128 * 128;
  P.m = m;
  P.chunk = chunk ? chunk : post_default_chunk(P.Np);
  auto rejected = [&](int code, const std::string& why) {
    P.reject = code;
    P.why = why;
    return P;
  };
  if (m < 1 || G < 1 || m % G != 0)
    return rejected(ResidentPlan::BAD_M,
                    "m must be >= 1 and divisible by num_genes (mean_function, model.py:145-149)");
  if (want_cov && m > P.chunk)
    return rejected(ResidentPlan::COV_CHUNK,
                    "the covariance needs m within one chunk: m = " + std::to_string(m) +
                        " is above the limit of " + std::to_string(P.chunk) +
                        " test rows (lfm_post_set_chunk; cov = NULL takes any m)");
  if (P.chunk < 128 || P.chunk % 128 != 0)
    return rejected(ResidentPlan::BAD_CHUNK, "the chunk must be a positive multiple of 128 rows");
  for (int64_t q0 = 0; q0 < m; q0 += P.chunk) {
    PostChunk c;
    c.q0 = q0;
    c.rows = std::min(P.chunk, m - q0);
    c.pad_rows = (c.rows + 127) / 128 * 128;
    c.panel_grid = (int)((c.rows + 63) / 64);
    c.tiles = (int)(c.pad_rows / 128);
    P.vt_rows = std::max(P.vt_rows, c.pad_rows);
    P.chunks.push_back(c);
  }
  const int nblk = (int)(P.Np / 128);
  for (int b = 0; b < nblk; b += POST_W) {
    PostPanel s;
    s.w = std::min(POST_W, nblk - b);
    s.K0 = (int64_t)b * 128;
    s.K1 = s.K0 + (int64_t)s.w * 128;
    s.tj0 = b + s.w;
    s.ntj = nblk - s.tj0;
    P.panels.push_back(s);
  }
  P.vt_bytes = (size_t)P.vt_rows * P.Np * sizeof(double);
  P.acc_bytes = 2 * (size_t)P.vt_rows * sizeof(double);
  P.t_bytes = (size_t)m * 3 * sizeof(double);
  P.out_bytes = 2 * (size_t)m * sizeof(double);
  if (want_cov) {
    P.cov_bytes = (size_t)m * m * sizeof(double);
    P.cov_tiles = (int)((m + 127) / 128);
  }
  return P;
}

// ------------------------------------------------- joint samples (lfm_sample.hip)
SamplePlan plan_sample(int64_t n, int64_t nsamp, int64_t sample0) {
  SamplePlan P;
  P.n = n;
  P.nsamp = nsamp;
  P.sample0 = sample0;
  auto rejected = [&](int code, const std::string& why) {
    P.reject = code;
    P.why = why;
    return P;
  };
  if (n < 1 || n > (int64_t)1 << 30)
    return rejected(SamplePlan::BAD_N, "n must be in [1, 2^30]");
  if (nsamp < 1) return rejected(SamplePlan::BAD_NSAMP, "nsamp must be >= 1");
  if (sample0 < 0) return rejected(SamplePlan::BAD_SAMPLE0, "sample0 must be >= 0");
  if (sample0 > INT64_MAX - nsamp)
    return rejected(SamplePlan::RANGE, "sample0 + nsamp overflows 2^63");
  if (nsamp > SAMPLE_MAX_NSAMP)
    return rejected(SamplePlan::TOO_MANY,
                    "nsamp = " + std::to_string(nsamp) + " is above the limit of " +
                        std::to_string(SAMPLE_MAX_NSAMP) +
                        " samples a call (continue the draw with sample0)");
  P.Np = (n + 127) / 128 * 128;
  P.Mp = (n + 1 + 127) / 128 * 128;
  P.ldz = P.Np;
  P.zrows = (nsamp + 127) / 128 * 128;
  P.mat_bytes = (size_t)P.Mp * P.Mp * sizeof(double);
  P.z_bytes = (size_t)P.zrows * P.ldz * sizeof(double);
  P.x_bytes = (size_t)nsamp * n * sizeof(double);
  P.tiles_i = (int)(P.zrows / 128);
  P.tiles_j = (int)(P.Np / 128);
  P.pairs = P.zrows * (P.ldz / 2);
  P.randn_grid = (int)std::min<int64_t>((P.pairs + 255) / 256, SAMPLE_RANDN_GRID);
  return P;
}

// ------------------------- held-out log density on the resident posterior (lfm_post.hip)
PostLogpPlan plan_post_logp(int64_t n, int64_t G, int64_t m, int64_t k, int64_t chunk) {
  PostLogpPlan P;
  P.m = m;
  P.k = k;
  auto rejected = [&](int code, const std::string& why) {
    P.reject = code;
    P.why = why;
    P.pred = ResidentPlan();
    return P;
  };
  P.pred = plan_post(n, G, m, chunk, true);
  if (P.pred.reject) return rejected(P.pred.reject, P.pred.why);  // the codes are plan_post's
  if (k < 1) return rejected(PostLogpPlan::BAD_K, "k must be >= 1 held-out vector");
  if (k > LOGP_MAX_K)
    return rejected(PostLogpPlan::TOO_MANY,
                    "k = " + std::to_string(k) + " is above the limit of " +
                        std::to_string(LOGP_MAX_K) +
                        " held-out vectors a call (split the rows of ystar over calls)");
  P.Np = (m + 127) / 128 * 128;
  P.Mp = (m + 1 + 127) / 128 * 128;
  P.pass = std::min(P.pred.chunk, post_default_chunk(P.Np));
  P.rows = plan_post(m, 1, k, P.pass, false);
  P.mat_bytes = (size_t)P.Mp * P.Mp * sizeof(double);
  P.dinv_bytes = (size_t)(P.Np / 128) * 128 * 16 * sizeof(double);
  P.zero_bytes = (size_t)P.Np * sizeof(double);
  P.vt_bytes = std::max(P.pred.vt_bytes, P.rows.vt_bytes);
  P.acc_bytes = std::max(P.pred.acc_bytes, P.rows.acc_bytes);
  P.logp_bytes = (size_t)P.rows.vt_rows * sizeof(double);
  P.dinv_grid = (int)(P.Np / 128);
  P.z_grid = (int)((P.Np + 255) / 256);
  P.resid_grid = (int)((P.Np / 2 + 255) / 256);
  return P;
}

// ------------------------------ leave-one-out CV (lfm_loo.hip)
LooPlan plan_loo(int64_t n) {
  LooPlan P;
  P.n = n;
  auto rejected = [&](int code, const std::string& why) {
    P = LooPlan();
    P.n = n;
    P.reject = code;
    P.why = why;
    return P;
  };
  if (n < 1 || n > (int64_t)1 << 30) return rejected(LooPlan::BAD_N, "n must be in [1, 2^30]");
  P.Np = (n + 127) / 128 * 128;
  P.Mp = (n + 1 + 127) / 128 * 128;
  P.ld = 2 * P.Mp;
  P.tiles = P.Np / 128;
  // ld^2 doubles within size_t (and ptrdiff_t), the product's 1-D grid within a launch's 2^31 - 1
  // and the scale kernel's grid rows within 65535
  const uint64_t ld = (uint64_t)P.ld, cap = (uint64_t)INT64_MAX / sizeof(double);
  if (ld > cap / ld || P.tiles * (P.tiles + 1) / 2 > (int64_t)INT32_MAX || P.Np / 64 > 65535)
    return rejected(LooPlan::TOO_LARGE,
                    "n = " + std::to_string(n) + " is too large for the bordered matrix of the "
                    "leave-one-out call");
  P.mat_bytes = (size_t)(ld * ld) * sizeof(double);
  P.bt = P.Mp * P.ld + P.Mp;
  P.a = P.bt + n * P.ld;
  P.bs = 0;
  P.w = P.Mp;
  P.mu = 0;
  P.var = P.Np;
  P.sc = 2 * P.Np;
  P.b = 3 * P.Np;
  P.u = 4 * P.Np;
  P.val = 5 * P.Np;
  P.vec = 5 * P.Np + 2;
  P.vec_bytes = (size_t)P.vec * sizeof(double);
  P.product_grid = P.tiles * (P.tiles + 1) / 2;
  P.scale_tiles = P.Np / 64;
  P.u_grid = (n + 63) / 64;
  return P;
}

// ------------------- mid-size resident batch (lfm_mbatch.hip; its kernels: lfm_mid.hip)
namespace {
// a region's size rounded up to 16 bytes: in doubles, and in bytes
int64_t even(int64_t d) { return (d + 1) / 2 * 2; }
size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// The factorisation's launches: one per block column k of the largest problem, its units the row
// blocks from k on.
void push_columns(std::vector<MidLaunch>& v, unsigned gx, int maxnb) {
  for (int k = 0; k < maxnb; ++k) v.push_back({MID_COLUMN, k, gx, (unsigned)(maxnb - k)});
}

// The sizes of a table entry for an n x n problem and, from `at`, the regions the factorisation
// works in: the augmented matrix S, the factor L, W behind it if the entry has one, and the
// inverses of the factor's diagonal blocks. Returns the first double past them.
int64_t factor_regions(MidProb& m, int64_t n, int64_t at, bool has_W) {
  m.n = (int)n;
  m.nb = mid_blocks(m.n);
  m.Mp = m.nb * MID_TILE;
  const int64_t mat = (int64_t)m.Mp * m.Mp;
  m.S = at;
  m.L = m.S + mat;
  m.dinv = m.L + mat;
  if (has_W) {
    m.W = m.dinv;
    m.dinv = m.W + mat;
  }
  return m.dinv + (int64_t)m.nb * MID_TILE * MID_TILE;
}
}  // namespace

int64_t mid_problem_doubles(int64_t n) {
  const int64_t nb = mid_blocks((int)n), Mp = nb * MID_TILE;
  return even(3 * n) + even(n) + 3 * Mp * Mp + nb * MID_TILE * MID_TILE +
         even((int64_t)mid_tiles((int)nb) * MID_PART);
}

MidPlan plan_mid(const std::vector<MidShape>& shapes) {
  MidPlan P;
  auto rejected = [&](int code, const std::string& why) {
    P.reject = code;
    P.why = why;
    return P;
  };
  if (shapes.empty()) return rejected(MidPlan::EMPTY, "lfm_mbatch: no problems");
  if ((int64_t)shapes.size() > MID_MAX_PROBS)
    return rejected(MidPlan::TOO_MANY, "lfm_mbatch: at most " + std::to_string(MID_MAX_PROBS) +
                                           " problems per batch");
  for (size_t q = 0; q < shapes.size(); ++q) {
    const MidShape& s = shapes[q];
    if (s.n < 1 || s.n > MID_MAX_N)
      return rejected(MidPlan::BAD_N, "lfm_mbatch: problem " + std::to_string(q) + " has n = " +
                                          std::to_string(s.n) + ", outside [1, " +
                                          std::to_string(MID_MAX_N) + "] (LFM_MID_MAX_N)");
    if (s.G < 1 || s.G > s.n || s.n % s.G != 0)
      return rejected(MidPlan::BAD_G, "lfm_mbatch: problem " + std::to_string(q) +
                                          " needs num_genes in [1, n] dividing n "
                                          "(mean_function, model.py:145-149)");
  }
  P.nprob = (int64_t)shapes.size();
  for (const MidShape& s : shapes) P.nhyp += 3 * s.G + 3;
  P.hyp = 0;
  P.out = even(P.nhyp);
  P.grad = P.out + even(P.nprob);
  int64_t at = P.grad + even(P.nhyp);
  int64_t hv = 0, hs = P.nhyp - 3 * P.nprob;  // the vectors first, then the scalars
  P.probs.reserve(shapes.size());
  for (const MidShape& s : shapes) {
    MidProb m{};
    m.G = (int)s.G;
    m.hv = hv;
    m.hs = hs;
    hv += 3 * s.G;
    hs += 3;
    m.x = at;
    m.y = m.x + even(3 * s.n);
    m.part = factor_regions(m, s.n, m.y + even(s.n), true);
    at = m.part + even((int64_t)mid_tiles(m.nb) * MID_PART);
    P.maxnb = std::max(P.maxnb, m.nb);
    P.probs.push_back(m);
  }
  P.maxtiles = mid_tiles(P.maxnb);
  P.doubles = at;
  P.status = (size_t)at * sizeof(double);
  P.table = P.status + up16((size_t)P.nprob * sizeof(int));
  P.bytes = P.table + (size_t)P.nprob * sizeof(MidProb);
  // the launches: their count depends on the largest problem alone
  const unsigned gx = (unsigned)P.nprob;
  P.value.push_back({MID_FILL, 0, gx, (unsigned)P.maxtiles});
  push_columns(P.value, gx, P.maxnb);
  P.value.push_back({MID_VALUE, 0, gx, 1u});
  P.value_grad = P.value;  // the same launches first: the same value bits
  P.value_grad.push_back({MID_INVERT, 0, gx, (unsigned)P.maxnb});
  P.value_grad.push_back({MID_SINV, 0, gx, (unsigned)P.maxtiles});
  P.value_grad.push_back({MID_PAIRS, 0, gx, (unsigned)P.maxtiles});
  P.value_grad.push_back({MID_GRAD, 0, gx, 1u});
  return P;
}

MidPostPlan plan_mid_post(const std::vector<MidShape>& shapes, const int64_t* m, bool has_dv,
                          bool want_cov) {
  MidPostPlan P;
  auto rejected = [&](int code, size_t q, const std::string& why) {
    P.reject = code;
    P.why = "lfm_mbatch_posterior_f64: problem " + std::to_string(q) + " has m = " +
            std::to_string(m[q]) + why;
    return P;
  };
  for (size_t q = 0; q < shapes.size(); ++q) {
    if (m[q] < 1) return rejected(MidPostPlan::NO_ROWS, q, ", needs m >= 1");
    if (m[q] % shapes[q].G != 0)
      return rejected(MidPostPlan::BAD_M, q, ", no multiple of num_genes = " +
                                                 std::to_string(shapes[q].G) +
                                                 " (mean_function, model.py:145-149)");
    if (m[q] > MID_MAX_M)
      return rejected(MidPostPlan::TOO_MANY_ROWS, q, ", past " + std::to_string(MID_MAX_M) +
                                                         " (LFM_MID_MAX_M); use lfm_post_* for "
                                                         "more test rows on one model");
  }
  P.nprob = (int64_t)shapes.size();
  for (size_t q = 0; q < shapes.size(); ++q) {
    P.sn += shapes[q].n;
    P.sm += m[q];
    P.sc += m[q] * m[q];
  }
  int64_t at = 0;
  P.dadd = at;
  at += even(P.nprob);
  if (has_dv) {
    P.dv = at;
    at += even(P.sn);
  }
  P.t = at;
  at += even(3 * P.sm);
  P.pp.reserve(shapes.size());
  int64_t on = 0, om = 0, oc = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    const int nb = mid_blocks((int)shapes[q].n);
    MidPostProb e{};
    e.m = (int)m[q];
    e.mb = (e.m + MID_TILE - 1) / MID_TILE;
    e.dv = has_dv ? P.dv + on : -1;
    e.t = P.t + 3 * om;
    e.V = at;
    at += (int64_t)e.mb * MID_TILE * nb * MID_TILE;
    e.mean = om;  // within the packed outputs: their bases are added below
    e.var = om;
    e.cov = want_cov ? oc : -1;
    on += shapes[q].n;
    om += m[q];
    oc += m[q] * m[q];
    P.maxnb = std::max(P.maxnb, nb);
    P.maxmb = std::max(P.maxmb, e.mb);
    P.maxunits = std::max(P.maxunits, e.mb * nb);
    P.pp.push_back(e);
  }
  P.mean = at;
  at += even(P.sm);
  P.var = at;
  at += even(P.sm);
  if (want_cov) {
    P.cov = at;
    at += even(P.sc);
  }
  for (MidPostProb& e : P.pp) {
    e.mean += P.mean;
    e.var += P.var;
    if (want_cov) e.cov += P.cov;
  }
  P.maxtiles = mid_tiles(P.maxnb);
  P.maxcov = mid_tiles(P.maxmb);
  P.doubles = at;
  P.table = (size_t)at * sizeof(double);
  P.bytes = P.table + (size_t)P.nprob * sizeof(MidPostProb);
  const unsigned gx = (unsigned)P.nprob;
  P.launches.push_back({MID_POST_FILL, 0, gx, (unsigned)(P.maxtiles + P.maxunits)});
  push_columns(P.launches, gx, P.maxnb);
  P.launches.push_back({MID_SOLVE, 0, gx, (unsigned)P.maxmb});
  if (want_cov) P.launches.push_back({MID_COV, 0, gx, (unsigned)P.maxcov});
  return P;
}

MidFitPlan plan_mid_fit(const std::vector<MidShape>& shapes, int64_t nsteps) {
  MidFitPlan F;
  auto rejected = [&](int code, const std::string& why) {
    F.reject = code;
    F.why = why;
    return F;
  };
  const MidPlan P = plan_mid(shapes);
  if (P.reject) return rejected(MidFitPlan::BAD_BATCH, P.why);
  if (nsteps < 1) return rejected(MidFitPlan::NO_STEPS, "lfm_mbatch_fit_f64: nsteps = " +
                                                            std::to_string(nsteps) + ", needs >= 1");
  if (nsteps > MID_FIT_MAX_STEPS)
    return rejected(MidFitPlan::TOO_MANY_STEPS,
                    "lfm_mbatch_fit_f64: nsteps = " + std::to_string(nsteps) + ", past " +
                        std::to_string(MID_FIT_MAX_STEPS) + " a call; resume with step0");
  F.nprob = P.nprob;
  F.nhyp = P.nhyp;
  F.nsteps = nsteps;
  F.raw = 0;
  F.mu = F.raw + even(F.nhyp);
  F.nu = F.mu + even(F.nhyp);
  F.bias = F.nu + even(F.nhyp);
  F.hist = F.bias + 2 * nsteps;
  F.doubles = F.hist + even(nsteps * F.nprob);
  F.first_bad = (size_t)F.doubles * sizeof(double);
  F.bytes = F.first_bad + up16((size_t)F.nprob * sizeof(int));
  const unsigned gx = (unsigned)F.nprob;
  F.per_step = P.value_grad.size() + 1;
  F.launches.reserve(1 + (size_t)nsteps * F.per_step);
  F.launches.push_back({MID_CONSTRAIN, 0, gx, 1u});
  for (int64_t s = 0; s < nsteps; ++s) {
    F.launches.insert(F.launches.end(), P.value_grad.begin(), P.value_grad.end());
    F.launches.push_back({MID_ADAM, (int)s, gx, 1u});
  }
  return F;
}

size_t mid_draw_problem_bytes(int64_t m, bool has_ystar, int64_t nsamp) {
  const int64_t nq = mid_blocks((int)m), Mq = nq * MID_TILE;
  const int64_t cb = (m + MID_TILE - 1) / MID_TILE, sb = (nsamp + MID_TILE - 1) / MID_TILE;
  int64_t d = 2 * Mq * Mq + nq * MID_TILE * MID_TILE + 2;
  if (has_ystar) d += m;
  if (nsamp > 0) d += (int64_t)MID_TILE * MID_TILE * sb * cb + nsamp * m;
  return (size_t)d * 8 + sizeof(uint64_t) + sizeof(MidProb) + sizeof(MidDrawProb);
}

MidDrawPlan plan_mid_draw(const std::vector<MidShape>& shapes, const int64_t* m, bool has_cov_add,
                          bool has_ystar, int64_t nsamp, int64_t sample0) {
  MidDrawPlan P;
  const std::string who = "lfm_mbatch_predictive_f64: ";
  auto rejected = [&](int code, const std::string& why) {
    P.reject = code;
    P.why = who + why;
    return P;
  };
  if (!has_cov_add) return rejected(MidDrawPlan::NO_COV_ADD, "cov_add is NULL");
  if (nsamp < 0) return rejected(MidDrawPlan::BAD_NSAMP, "nsamp must be >= 0");
  if (!has_ystar && nsamp == 0)
    return rejected(MidDrawPlan::NOTHING, "nothing asked for: give ystar and logp, or nsamp > 0");
  if (nsamp > MID_DRAW_MAX_NSAMP)
    return rejected(MidDrawPlan::TOO_MANY,
                    "nsamp = " + std::to_string(nsamp) + " is above the limit of " +
                        std::to_string(MID_DRAW_MAX_NSAMP) +
                        " samples a call (continue the draw with sample0)");
  if (sample0 < 0) return rejected(MidDrawPlan::BAD_SAMPLE0, "sample0 must be >= 0");
  if (sample0 > INT64_MAX - nsamp)
    return rejected(MidDrawPlan::RANGE, "sample0 + nsamp overflows 2^63");
  for (size_t q = 0; q < shapes.size(); ++q) {
    const std::string pm = "problem " + std::to_string(q) + " has m = " + std::to_string(m[q]);
    if (m[q] < 1) return rejected(MidDrawPlan::NO_ROWS, pm + ", needs m >= 1");
    if (m[q] % shapes[q].G != 0)
      return rejected(MidDrawPlan::BAD_M, pm + ", no multiple of num_genes = " +
                                              std::to_string(shapes[q].G) +
                                              " (mean_function, model.py:145-149)");
    if (m[q] > MID_MAX_N)
      return rejected(MidDrawPlan::TOO_MANY_ROWS,
                      pm + ", past " + std::to_string(MID_MAX_N) +
                          " (LFM_MID_MAX_N: the covariance goes through the mid-size "
                          "factorisation); use lfm_post_* for a larger m on one model");
  }
  P.nprob = (int64_t)shapes.size();
  P.nsamp = nsamp;
  P.sample0 = sample0;
  for (size_t q = 0; q < shapes.size(); ++q) P.sm += m[q];
  const int64_t sb = (nsamp + MID_TILE - 1) / MID_TILE;
  int64_t at = 0;
  P.cadd = at;
  at += even(P.nprob);
  P.out = at;
  at += even(P.nprob);
  if (has_ystar) {
    P.ystar = at;
    at += even(P.sm);
  }
  P.probs.reserve(shapes.size());
  P.dp.reserve(shapes.size());
  int64_t om = 0, oc = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    MidProb e{};
    e.G = (int)shapes[q].G;
    at = factor_regions(e, m[q], at, false);
    MidDrawProb d{};
    d.m = e.n;
    d.cb = (e.n + MID_TILE - 1) / MID_TILE;
    d.sb = (int)sb;
    d.cov = oc;
    d.mean = om;
    d.ystar = has_ystar ? P.ystar + om : -1;
    d.Z = -1;
    d.X = -1;
    if (nsamp > 0) {
      d.Z = at;
      at += (int64_t)MID_TILE * MID_TILE * sb * d.cb;
      d.X = nsamp * om;  // within the packed samples: their base is added below
    }
    om += m[q];
    oc += m[q] * m[q];
    P.maxnq = std::max(P.maxnq, e.nb);
    P.maxcb = std::max(P.maxcb, d.cb);
    P.probs.push_back(e);
    P.dp.push_back(d);
  }
  if (nsamp > 0) {
    P.X = at;
    at += even(nsamp * P.sm);
    for (MidDrawProb& d : P.dp) d.X += P.X;
  }
  P.maxsb = (int)sb;
  P.maxtiles = mid_tiles(P.maxnq);
  P.doubles = at;
  P.seeds = (size_t)at * sizeof(double);
  P.table = P.seeds + up16((size_t)P.nprob * sizeof(uint64_t));
  P.dtable = P.table + up16((size_t)P.nprob * sizeof(MidProb));
  P.bytes = P.dtable + (size_t)P.nprob * sizeof(MidDrawProb);
  const unsigned gx = (unsigned)P.nprob;
  P.launches.push_back({MID_DRAW_SCALE, 0, gx, (unsigned)P.maxtiles});
  push_columns(P.launches, gx, P.maxnq);
  if (has_ystar) P.launches.push_back({MID_VALUE, 0, gx, 1u});
  if (nsamp > 0) {
    // 64 sb x 64 cb / 2 pairs of the largest problem, 256 a workgroup
    const int64_t wgs = 8 * sb * P.maxcb;
    P.launches.push_back(
        {MID_DRAW_RANDN, 0, gx, (unsigned)std::min<int64_t>(wgs, MID_DRAW_RANDN_GY)});
    P.launches.push_back({MID_DRAW_PRODUCT, 0, gx, (unsigned)(sb * P.maxcb)});
  }
  return P;
}

}  // namespace lfm
