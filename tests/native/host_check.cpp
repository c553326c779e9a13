// host_check.cpp — the host-side code of liblfm (dis_project_amd/csrc/lfm_host.cpp) and the
// C++ oracle (oracle/lfm_cpu.cpp) under AddressSanitizer + UBSan: built and run
// by `make -C tests/native asan` (tests/test_host_asan.py). Exits non-zero on the first failed
// check; the sanitizers abort on any memory / UB error.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <string>
#include <thread>
#include <vector>

#include "../../dis_project_amd/csrc/lfm_host.h"

extern "C" {
int lfm_cpu_gram(const double* x, int64_t n, int64_t G, const double* D, const double* S,
                 double l, double diag_add, double* K, int64_t ldk, int threads);
int lfm_cpu_gram_rows_f32(const double* x, int64_t n, int64_t G, const double* D,
                          const double* S, double l, double diag_add, const int64_t* rows,
                          int64_t nrows, float* out, int threads);
int64_t lfm_cpu_potrf(double* A, int64_t n, int64_t lda, int threads);
double lfm_cpu_mll(const double* x, const double* y, int64_t n, int64_t G, const double* D,
                   const double* S, const double* B, double l, double obs_stddev, double jitter,
                   int negative, int threads, double* work, double* info);
}

static int failures = 0;
#define CHECK(c, ...)                                     \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

using namespace lfm;

// every (64-row slab, 128-column tile) of the rest triangle exactly once
static void check_enumeration() {
  int cases = 0;
  for (int Q : {1, 2, 6}) {
    for (int T = 1; T <= 40; ++T) {
      for (int lo = 0; lo < T && lo <= 6; ++lo) {
        const int m = T - lo;
        const int64_t units = (int64_t)m * (m + 1);  // 2 slabs per tile of the m-tile triangle
        std::set<std::pair<int, int>> seen;
        for (int64_t b = 0; b < units; ++b) {
          int ti, tj;
          rest_unit_tile(b, T, lo, Q, &ti, &tj);
          const int tr = ti / 2;
          CHECK(tj >= lo && tj <= tr && tr < T, "Q=%d T=%d lo=%d b=%lld -> (%d,%d)", Q, T, lo,
                (long long)b, ti, tj);
          CHECK(seen.insert({ti, tj}).second, "duplicate unit Q=%d T=%d lo=%d b=%lld", Q, T, lo,
                (long long)b);
        }
        CHECK((int64_t)seen.size() == units, "coverage Q=%d T=%d lo=%d", Q, T, lo);
        ++cases;
      }
    }
  }
  std::printf("enumeration: %d (Q, T, tj_lo) cases bijective\n", cases);
}

// the side-CU helper's tail never holds a lead tile; the cap is the first unit past them
static void check_helper_clamp() {
  std::mt19937_64 rng(7);
  int cases = 0, capped = 0;
  for (int it = 0; it < 4000; ++it) {
    const int Q = (int)(rng() % 2) ? 6 : 1 + (int)(rng() % 4);
    const int T = 2 + (int)(rng() % 130);
    const int wn = 1 + (int)(rng() % 5);
    if (T - wn <= kBandMaxCols) continue;  // band enumeration: no helper (checked below)
    const int lead = 1 + (int)(rng() % 5);
    const int nr = (T - wn) * (T - wn + 1);
    const int64_t want = (int64_t)(rng() % (nr + 1));
    const int64_t hu = helper_clamp(want, nr, T, wn, lead, Q);
    CHECK(hu >= 0 && hu <= want, "hu out of range");
    for (int64_t b = nr - hu; b < nr; ++b) {
      int ti, tj;
      rest_unit_tile(b, T, wn, Q, &ti, &tj);
      CHECK(!(ti / 2 < wn + lead && tj < wn + lead), "lead tile in the helper's tail T=%d wn=%d "
            "lead=%d Q=%d b=%lld", T, wn, lead, Q, (long long)b);
    }
    capped += hu < want;
    ++cases;
  }
  // band-enumerated rest regions (<= 8 tile columns) never get a helper
  for (int T = 2; T <= 40; ++T)
    for (int wn = 1; wn < T && wn <= 5; ++wn)
      if (T - wn <= kBandMaxCols)
        CHECK(helper_clamp((T - wn) * (T - wn + 1) / 2, (T - wn) * (T - wn + 1), T, wn, 1, 6) == 0,
              "band region T=%d wn=%d got a helper", T, wn);
  CHECK(helper_units(640, 100, 5000, 200, 5, 128, 256, 32, 700, 1200) >= 0, "helper_units");
  CHECK(helper_units(640, 100, 5000, 200, 5, 128, 256, 32, 700, 1200) <= 2500, "helper half");
  CHECK(helper_units(640, 0, 10, 0, 5, 128, 256, 32, 700, 1200) == 0, "no helper for short");
  CHECK(helper_units(640, 100, 5000, 200, 5, 128, 256, 0, 700, 1200) == 0, "no side CUs");
  std::printf("helper clamp: %d cases (%d capped)\n", cases, capped);
}

static std::vector<double> grid_x(int G, int T, int R, const std::vector<int>& genes) {
  std::vector<double> x;
  for (int r = 0; r < R; ++r)
    for (int g = 0; g < G; ++g)
      for (int t = 0; t < T; ++t) {
        x.push_back(T > 1 ? 12.0 * t / (T - 1) : 0.0);
        x.push_back((double)genes[g]);
        x.push_back(1.0);
      }
  return x;
}

static void check_detect_grid() {
  std::vector<int> g8 = {0, 1, 2, 3, 4, 5, 6, 7};
  auto x = grid_x(8, 64, 1, g8);
  GridLayout L = detect_grid(x.data(), 8 * 64, 8);
  CHECK(L.ok && L.T == 64 && L.nblk == 8 && L.block_gene[7] == 7, "plain grid");
  auto x3 = grid_x(8, 16, 3, g8);  // replicate-major
  L = detect_grid(x3.data(), 3 * 8 * 16, 8);
  CHECK(L.ok && L.T == 16 && L.nblk == 24 && L.block_gene[8] == 0, "replicates");
  std::vector<int> shuf = {3, 1, 7, 0, 2, 6, 5, 4};
  auto xs = grid_x(8, 32, 1, shuf);
  L = detect_grid(xs.data(), 8 * 32, 8);
  CHECK(L.ok && L.block_gene[0] == 3 && L.block_gene[2] == 7, "shuffled genes");
  // negative / out-of-range / NaN gene indices follow the gather semantics
  std::vector<int> odd = {-1, 0, 9, 1};
  auto xo = grid_x(4, 8, 1, odd);
  L = detect_grid(xo.data(), 32, 4);
  CHECK(L.ok && L.block_gene[0] == 3 && L.block_gene[2] == 3, "wrapped / clamped genes");
  auto xn = x;
  xn[3 * 5 + 2] = 0.0;  // a latent (flag 0) row
  CHECK(!detect_grid(xn.data(), 8 * 64, 8).ok, "flag 0 row");
  xn = x;
  xn[3 * 70] += 1e-3;  // non-shared times in block 1
  CHECK(!detect_grid(xn.data(), 8 * 64, 8).ok, "times differ");
  xn = x;
  xn[3 * 10] = 100.0;  // non-uniform grid
  for (int b = 0; b < 8; ++b) xn[3 * (b * 64 + 10)] = 100.0;
  CHECK(!detect_grid(xn.data(), 8 * 64, 8).ok, "non-uniform");
  CHECK(!detect_grid(x.data(), 8 * 64 - 3, 8).ok, "ragged n");
  xn = x;
  xn[3 * 70 + 1] = std::nan("");  // NaN gathers gene 0: not block 1's gene
  CHECK(!detect_grid(xn.data(), 8 * 64, 8).ok, "NaN gene inside a block");
  xn = x;
  xn[3 * 3 + 1] = std::nan("");  // ... but block 0's
  CHECK(detect_grid(xn.data(), 8 * 64, 8).ok, "NaN gene gathers gene 0");
  CHECK(!detect_grid(nullptr, 0, 8).ok && !detect_grid(x.data(), 0, 8).ok, "empty");
  L = detect_grid(x.data(), 1, 8);
  CHECK(L.ok && L.T == 1 && L.nblk == 1, "single row");
  std::printf("detect_grid: ok\n");
}

static void check_plan() {
  int cases = 0;
  for (bool s3 : {false, true})
    for (bool bordered : {false, true})
      for (int64_t nblk : {1, 2, 3, 5, 9, 17, 33, 65, 129, 130}) {
        const int64_t Mp = nblk * 128;
        auto st = plan_steps(nblk, Mp, 128, bordered, s3, 5, 6144, 5120);
        int64_t k = 0;
        for (size_t i = 0; i < st.size(); ++i) {
          CHECK(st[i].first == k, "contiguous");
          CHECK(st[i].second == 1 || st[i].second == 2 || st[i].second == 4 ||
                    st[i].second == 5, "width");
          if (s3 && i == 0) CHECK(st[i].second == 1, "schedule 3 starts at width 1");
          k += st[i].second;
        }
        CHECK(k == nblk, "covers every block column");
        ++cases;
      }
  std::printf("plan_steps: %d cases\n", cases);
}

// ---- schedule 3's launch plan (plan_s3) ----
static constexpr int kST = 128, kSplit = 2, kQ = 6;  // lfm_chol.h ST, TALL_SPLIT, SUPERTILE

static S3Params s3_params(int64_t n, int64_t Mp, bool bordered, int side_cus, int helper,
                          bool prof) {
  S3Params p;
  p.n = n;
  p.Mp = Mp;
  p.bordered = bordered;
  p.prof = prof;
  p.st = kST;
  p.tall_split = kSplit;
  p.supertile = kQ;
  p.cus = 256;
  p.side_cus = side_cus;
  p.helper = helper;
  return p;
}

// Lead units among rest units [b0, b1) of a step's enumeration, as the device finds them
// (syrk_unit in_lead: tile row and column < wn + lead): the triangle through the enumeration
// mirror, a band region (<= kBandMaxCols columns) column by column as unit_tile's band branch
static int64_t lead_rest_units(int T, int wn, int lead, int64_t b0, int64_t b1) {
  static std::map<std::tuple<int, int, int, int64_t, int64_t>, int64_t> memo;
  const auto key = std::make_tuple(T, wn, lead, b0, b1);
  const auto it = memo.find(key);
  if (it != memo.end()) return it->second;
  int64_t cnt = 0;
  if (T - wn > kBandMaxCols) {
    for (int64_t b = b0; b < b1; ++b) {
      int ti, tj;
      rest_unit_tile(b, T, wn, kQ, &ti, &tj);
      cnt += ti / 2 < wn + lead && tj < wn + lead;
    }
  } else {
    int64_t b = 0;
    for (int tj = wn; tj < T; ++tj)
      for (int ti = 2 * tj; ti < 2 * T; ++ti, ++b)
        cnt += b >= b0 && b < b1 && ti / 2 < wn + lead && tj < wn + lead;
    CHECK(b == (int64_t)(T - wn) * (T - wn + 1), "band enumeration size");
  }
  return memo[key] = cnt;
}

static void check_s3_plan(const std::vector<std::pair<int64_t, int>>& steps, const S3Params& p,
                          const S3Plan& P, const char* tag) {
  const int S = P.S;
  const int64_t rows = p.bordered ? 2 * p.Mp : p.Mp;  // of the matrix
  CHECK(S == (int)steps.size() && (int)P.steps.size() == S && S >= 1, "%s: steps", tag);
  // the plan names its inputs (a context reuses its last plan while they hold)
  S3Params other = p;
  other.n += 1;
  CHECK(P.params == p && !(P.params == other) && P.step_list == steps, "%s: plan inputs", tag);
  // flag layout: four regions, disjoint, in order, ending at nflags
  CHECK(P.chain_done == 0 && P.a_done == P.chain_done + S &&
            P.bars == P.a_done + (size_t)S * P.Tmax && P.xready == P.bars + S &&
            P.nflags == P.xready + S && P.flags_bytes == P.nflags * sizeof(unsigned),
        "%s: flag regions", tag);
  CHECK(P.nevents == chol_events(S) && P.nevents >= (size_t)3 * S + 3, "%s: events", tag);
  CHECK(P.pad_end == (p.bordered ? p.n + 1 : INT64_MAX) && P.zsplit == p.n, "%s: pad_end", tag);
  CHECK(P.zvec_bytes >= (size_t)p.Mp * 8 && P.linv_bytes >= 128 * 128 * 8, "%s: zvec", tag);
  int marks = 0;
  double alg = 0.0;
  for (int s = 0; s < S; ++s) {
    const S3Step& q = P.steps[s];
    const int64_t W = (int64_t)q.w * 128, end = p.bordered ? q.K1 + p.Mp : p.Mp;
    CHECK(q.K0 == steps[s].first * 128 && q.w == steps[s].second && q.K1 == q.K0 + W &&
              q.kd == W && W <= P.Wmax, "%s s=%d: columns", tag, s);
    CHECK(q.wn == (s + 1 < S ? steps[s + 1].second : 0), "%s s=%d: wn", tag, s);
    // flags of the step: each index inside its region
    CHECK(q.f_done >= P.chain_done && q.f_done < P.a_done, "%s s=%d: chain_done", tag, s);
    CHECK(q.f_adone >= P.a_done && q.f_adone + P.Tmax <= P.bars && q.T <= P.Tmax,
          "%s s=%d: a_done row", tag, s);
    CHECK(q.f_bar >= P.bars && q.f_bar < P.xready, "%s s=%d: bars", tag, s);
    CHECK(q.f_xready >= P.xready && q.f_xready < P.nflags, "%s s=%d: xready", tag, s);
    // buffers: the chain's 2W x W workspace, Bd_s (W x W), X_s (rows [K1, end) x W), the
    // chain's W x kd_{s-1} rows of X_{s-1}
    CHECK((q.wk_off + 2 * W * W) * 8 <= P.wk_bytes && q.bd_off == q.wk_off + (size_t)(W * W),
          "%s s=%d: workspace", tag, s);
    CHECK((q.x_off + (size_t)((end - q.K1) * W)) * 8 <= P.xbuf_bytes, "%s s=%d: X buffer", tag, s);
    if (s > 0) {
      CHECK((size_t)(W * P.steps[s - 1].kd) * 8 <= P.xd_bytes, "%s s=%d: xd", tag, s);
      CHECK(q.wk_off != P.steps[s - 1].wk_off && q.x_off != P.steps[s - 1].x_off,
            "%s s=%d: buffers alternate", tag, s);
    }
    // the matrix: the trailing tiles, the tall rows and the panel columns
    CHECK(q.K1 <= p.Mp && q.K1 + (int64_t)128 * q.T <= rows && q.T >= 0, "%s s=%d: tiles", tag, s);
    CHECK(q.tk0 == q.K0 && q.tr0 == q.K1 && q.tw == q.w && q.tk0 + W <= p.Mp,
          "%s s=%d: tall columns", tag, s);
    CHECK(q.nt % (q.w * kSplit) == 0 && q.tr0 + 64 * (int64_t)(q.nt / (q.w * kSplit)) <= rows &&
              q.nt == (end - q.K1) / 64 * q.w * kSplit, "%s s=%d: tall rows", tag, s);
    CHECK(q.zero_from == (p.bordered ? p.Mp + q.K0 : INT64_MAX) && q.copy_from == q.zero_from,
          "%s s=%d: border rows", tag, s);
    // units: the ahead band has 2 wn units per tile row (a_done's target), the rest triangle
    // two per tile; main and helper make up the whole enumeration
    CHECK(q.na == 2 * q.wn * (q.T - q.wn) && q.nr == (q.T - q.wn) * (q.T - q.wn + 1),
          "%s s=%d: unit counts", tag, s);
    for (int trow = q.wn; q.wn > 0 && trow < q.T; ++trow) {
      int cnt = 0;
      for (int u = 0; u < q.na; ++u) cnt += q.wn + u / (2 * q.wn) == trow;
      if (cnt != 2 * q.wn) CHECK(false, "%s s=%d: a_done row %d gets %d", tag, s, trow, cnt);
    }
    CHECK(q.hu >= 0 && q.hu <= q.nr / 2 && q.nr_main + q.hu == q.nr, "%s s=%d: helper share", tag, s);
    if (s == 0 || s + 2 >= S || !p.helper) CHECK(q.hu == 0, "%s s=%d: helper where none", tag, s);
    CHECK(q.lead == (s + 2 < S ? steps[s + 2].second : 0), "%s s=%d: lead", tag, s);
    if (q.hu > 0)
      CHECK(lead_rest_units(q.T, q.wn, q.lead, q.nr_main, q.nr) == 0,
            "%s s=%d: lead tile in the helper's tail", tag, s);
    if (s + 2 < S) {
      // chain(s + 2) waits for the lead units of launch s: all of them run in the main launch
      CHECK(q.T - q.wn >= q.lead, "%s s=%d: lead block outside the trailing matrix", tag, s);
      int64_t ahead = 0;
      for (int u = 0; u < q.na; ++u) ahead += q.wn + u / (2 * q.wn) < q.wn + q.lead;
      const int64_t rest = lead_rest_units(q.T, q.wn, q.lead, 0, q.nr_main);
      CHECK(rest == (int64_t)q.lead * (q.lead + 1), "%s s=%d: %lld lead rest units", tag, s,
            (long long)rest);
      CHECK((unsigned)(ahead + rest) == P.steps[s + 2].xtarget,
            "%s s=%d: %lld lead units, chain(s + 2) waits for %u", tag, s,
            (long long)(ahead + rest), P.steps[s + 2].xtarget);
    }
    if (s < 2) CHECK(q.xtarget == 0, "%s s=%d: xtarget without a wait", tag, s);
    // grids: the padded segments
    const int64_t tnext = s + 1 < S ? tall_grid(P.steps[s + 1].nt, kSplit) : 0;
    CHECK(q.ugrid == pad8(q.na) + pad8(q.nr) && q.tgrid == tall_grid(q.nt, kSplit) &&
              q.tgrid >= q.nt && q.tgrid % (8 * kSplit) == 0 && q.hgrid == pad8((int)q.hu),
          "%s s=%d: segment grids", tag, s);
    if (s + 1 < S)
      CHECK(q.grid == pad8(q.na) + pad8(q.nr_main) + tnext, "%s s=%d: grid", tag, s);
    else
      CHECK(q.grid == (p.bordered ? q.ugrid : 0), "%s s=%d: last grid", tag, s);
    marks += q.ovl_mark;
    alg += q.chain_alg + q.helper_alg + q.step_alg;
    CHECK(q.step_issued >= 0 && q.chain_issued >= q.chain_alg, "%s s=%d: issued flops", tag, s);
  }
  alg += P.steps[0].tall_alg;  // X_0's launch
  CHECK(marks <= 1, "%s: %d overlap tail marks", tag, marks);
  // The algorithmic flops of all launches are NOT checked against the closed form of the
  // factorisation ((n + 1)^3 / 3, bordered Mp^3): the per-launch formulas are approximations
  // whose sum depends on the step widths (16512 rows, MLL: 1.5051e12 against 1.5006e12, 0.3 %;
  // bordered 4.64e12 .. 4.75e12 against 4.50e12). They are pinned by the golden plans below.
  CHECK(std::isfinite(alg) && alg > 0, "%s: algorithmic flops", tag);
}

// The device-ordered launches of a plan, in issue order, one line each — what the kernels are
// given, pointers as offsets into their buffers (-1: null), INT64_MAX as "max":
//   E events / M bytes of flags cleared / T the overlap tail mark / R the buffers reserved
//   C grid Kc w kd K0p xtarget Wk Bdp bar done xready                      chain_kernel
//   L|H grid s0 kd T wn na nr nt tr0 tk0 tw lead rest_off zero_from copy_from pad_end
//       px.p px.ld px.r0 Bd X a_done chain_done xready gen                 step / helper launch
//   F class algorithmic issued                                 flops per kernel class, hexfloat
static std::string s3_launch_text(const S3Plan& P, const S3Params& p) {
  std::string out;
  char buf[512];
  auto num = [](int64_t v) { return v == INT64_MAX ? std::string("max") : std::to_string(v); };
  double fl[3][2] = {{0, 0}, {0, 0}, {0, 0}};  // chains, step launches, helpers
  // u: the step whose update the launch carries (NULL: none), t: whose tall units
  auto step = [&](const char* k, int64_t grid, const S3Step* u, const S3Step* t, int nr,
                  int64_t roff, bool device_ordered, double alg, double issued) {
    if (grid == 0) return;
    const bool h = k[0] == 'H';
    const S3Step* l = u && u->lead && device_ordered ? &P.steps[(u - P.steps.data()) + 2] : nullptr;
    std::snprintf(buf, sizeof(buf),
                  "%s %lld %s %d %d %d %d %d %d %s %s %d %d %s %s %s %s %lld %lld %lld %lld %lld "
                  "%lld %lld %lld %d\n",
                  k, (long long)grid, num(u ? u->K1 : 0).c_str(), u ? u->kd : 0, u ? u->T : 0,
                  u ? u->wn : 0, u && !h ? u->na : 0, nr, t && !h ? t->nt : 0,
                  num(t ? t->tr0 : 0).c_str(), num(t ? t->tk0 : 0).c_str(), t ? t->tw : 0,
                  l ? u->lead : 0, num(roff).c_str(), num(u ? u->zero_from : INT64_MAX).c_str(),
                  num(t ? t->copy_from : INT64_MAX).c_str(), num(P.pad_end).c_str(),
                  u ? (long long)u->x_off : -1LL, u ? (long long)u->kd : 0LL,
                  u ? (long long)u->K1 : 0LL, t ? (long long)t->bd_off : -1LL,
                  t ? (long long)t->x_off : -1LL, u && device_ordered ? (long long)u->f_adone : -1LL,
                  t ? (long long)t->f_done : -1LL, l && !h ? (long long)l->f_xready : -1LL,
                  (int)(u && u->gen));
    out += buf;
    fl[h ? 2 : 1][0] += alg;
    fl[h ? 2 : 1][1] += issued;
  };
  auto chain = [&](int s) {
    const S3Step& q = P.steps[s];
    const S3Step* prev = s > 0 ? &P.steps[s - 1] : nullptr;
    std::snprintf(buf, sizeof(buf), "C %d %lld %d %d %lld %u %lld %lld %lld %lld %lld\n", p.side_cus,
                  (long long)q.K0, q.w, prev ? prev->kd : 0, prev ? (long long)prev->K0 : 0LL,
                  q.xtarget, (long long)q.wk_off, prev ? (long long)prev->bd_off : -1LL,
                  (long long)q.f_bar, (long long)q.f_done, s >= 2 ? (long long)q.f_xready : -1LL);
    out += buf;
    fl[0][0] += q.chain_alg;
    fl[0][1] += q.chain_issued;
  };
  out += "E " + std::to_string(P.nevents) + "\nM " + std::to_string(P.flags_bytes) + "\n";
  const S3Step* st = P.steps.data();
  bool marked = false;
  chain(0);
  step("L", st[0].tgrid, nullptr, &st[0], 0, 0, true, st[0].tall_alg, st[0].tall_issued);
  for (int s = 0; s + 1 < P.S; ++s) {
    chain(s + 1);
    if (st[s].ovl_mark) out += "T\n", marked = true;
    step("L", st[s].grid, &st[s], &st[s + 1], st[s].nr_main, 0, true, st[s].step_alg,
         st[s].step_issued);
    if (st[s].hu > 0)
      step("H", st[s].hgrid, &st[s], &st[s + 1], (int)st[s].hu, st[s].nr_main, true,
           st[s].helper_alg, st[s].helper_issued);
  }
  if (p.bordered)
    step("L", st[P.S - 1].ugrid, &st[P.S - 1], nullptr, st[P.S - 1].nr, 0, false,
         st[P.S - 1].upd_alg, st[P.S - 1].upd_issued);
  if (!marked) out += "T\n";
  std::snprintf(buf, sizeof(buf), "R %zu %zu %zu %zu %zu %zu\n", P.wk_bytes, P.xbuf_bytes,
                P.zvec_bytes, P.linv_bytes, P.xd_bytes, P.flags_bytes);
  out += buf;
  const int cls[3] = {4, 6, 12};  // lfm_internal.h K_POTRF, K_SYRK, K_SIDE_SYRK
  for (int c = 0; c < 3; ++c) {
    std::snprintf(buf, sizeof(buf), "F %d %a %a\n", cls[c], fl[c][0], fl[c][1]);
    out += buf;
  }
  return out;
}

// The launches of the parent of the commit that introduced plan_s3 (its chol_factor_solve,
// built with every HIP call stubbed out), device-ordered, profiler on, overlapped (so the tail
// mark shows), 256 CUs of which 32 are the side stream's, default knobs:
// the benchmark's N = 16384 MLL with the fused gram ...
static const char kGolden16384[] = R"(E 177
M 30856
C 32 0 1 0 0 0 0 -1 7598 0 -1
L 512 0 0 0 0 0 0 512 128 0 1 0 0 max max max -1 0 0 16384 0 -1 0 -1 0
C 32 128 4 128 0 0 819200 16384 7599 1 -1
L 18480 128 128 128 4 992 15500 1984 640 128 4 5 0 max max max 0 128 128 1081344 10567680 58 1 7658 1
C 32 640 5 512 128 70 0 1081344 7600 2 7658
L 16368 640 512 124 5 1190 12790 2380 1280 640 5 5 0 max max max 10567680 512 640 409600 0 188 2 7659 0
H 1496 640 512 124 5 0 1490 0 1280 640 5 5 12790 max max max 10567680 512 640 409600 0 188 2 -1 0
C 32 1280 5 640 640 80 819200 409600 7601 3 7659
L 15128 1280 640 119 5 1140 11690 2280 1920 1280 5 5 0 max max max 0 640 1280 1228800 10567680 318 3 7660 0
H 1424 1280 640 119 5 0 1420 0 1920 1280 5 5 11690 max max max 0 640 1280 1228800 10567680 318 3 -1 0
C 32 1920 5 640 1280 80 0 1228800 7602 4 7660
L 14008 1920 640 114 5 1090 10720 2180 2560 1920 5 5 0 max max max 10567680 640 1920 409600 0 448 4 7661 0
H 1272 1920 640 114 5 0 1270 0 2560 1920 5 5 10720 max max max 10567680 640 1920 409600 0 448 4 -1 0
C 32 2560 5 640 1920 80 819200 409600 7603 5 7661
L 12920 2560 640 109 5 1040 9794 2080 3200 2560 5 5 0 max max max 0 640 2560 1228800 10567680 578 5 7662 0
H 1128 2560 640 109 5 0 1126 0 3200 2560 5 5 9794 max max max 0 640 2560 1228800 10567680 578 5 -1 0
C 32 3200 5 640 2560 80 0 1228800 7604 6 7662
L 11888 3200 640 104 5 990 8912 1980 3840 3200 5 5 0 max max max 10567680 640 3200 409600 0 708 6 7663 0
H 992 3200 640 104 5 0 988 0 3840 3200 5 5 8912 max max max 10567680 640 3200 409600 0 708 6 -1 0
C 32 3840 5 640 3200 80 819200 409600 7605 7 7663
L 10912 3840 640 99 5 940 8073 1880 4480 3840 5 5 0 max max max 0 640 3840 1228800 10567680 838 7 7664 0
H 864 3840 640 99 5 0 857 0 4480 3840 5 5 8073 max max max 0 640 3840 1228800 10567680 838 7 -1 0
C 32 4480 5 640 3840 80 0 1228800 7606 8 7664
L 9968 4480 640 94 5 890 7278 1780 5120 4480 5 5 0 max max max 10567680 640 4480 409600 0 968 8 7665 0
H 736 4480 640 94 5 0 732 0 5120 4480 5 5 7278 max max max 10567680 640 4480 409600 0 968 8 -1 0
C 32 5120 5 640 4480 80 819200 409600 7607 9 7665
L 9048 5120 640 89 5 840 6527 1680 5760 5120 5 5 0 max max max 0 640 5120 1228800 10567680 1098 9 7666 0
H 616 5120 640 89 5 0 613 0 5760 5120 5 5 6527 max max max 0 640 5120 1228800 10567680 1098 9 -1 0
C 32 5760 5 640 5120 80 0 1228800 7608 10 7666
L 8200 5760 640 84 5 790 5819 1580 6400 5760 5 5 0 max max max 10567680 640 5760 409600 0 1228 10 7667 0
H 504 5760 640 84 5 0 501 0 6400 5760 5 5 5819 max max max 10567680 640 5760 409600 0 1228 10 -1 0
C 32 6400 5 640 5760 80 819200 409600 7609 11 7667
L 7392 6400 640 79 5 740 5155 1480 7040 6400 5 5 0 max max max 0 640 6400 1228800 10567680 1358 11 7668 0
H 400 6400 640 79 5 0 395 0 7040 6400 5 5 5155 max max max 0 640 6400 1228800 10567680 1358 11 -1 0
C 32 7040 5 640 6400 80 0 1228800 7610 12 7668
L 6920 7040 640 74 5 690 4830 1380 7680 7040 5 5 0 max max max 10567680 640 7040 409600 0 1488 12 7669 0
C 32 7680 5 640 7040 80 819200 409600 7611 13 7669
L 6080 7680 640 69 5 640 4160 1280 8320 7680 5 5 0 max max max 0 640 7680 1228800 10567680 1618 13 7670 0
C 32 8320 5 640 7680 80 0 1228800 7612 14 7670
L 5320 8320 640 64 5 590 3540 1180 8960 8320 5 5 0 max max max 10567680 640 8320 409600 0 1748 14 7671 0
C 32 8960 5 640 8320 80 819200 409600 7613 15 7671
L 4608 8960 640 59 5 540 2970 1080 9600 8960 5 5 0 max max max 0 640 8960 1228800 10567680 1878 15 7672 0
C 32 9600 5 640 8960 80 0 1228800 7614 16 7672
L 3944 9600 640 54 5 490 2450 980 10240 9600 5 5 0 max max max 10567680 640 9600 409600 0 2008 16 7673 0
C 32 10240 5 640 9600 80 819200 409600 7615 17 7673
L 3304 10240 640 49 5 440 1980 880 10880 10240 5 2 0 max max max 0 640 10240 1228800 10567680 2138 17 7674 0
C 32 10880 2 640 10240 26 0 1228800 7616 18 7674
T
L 2312 10880 640 44 2 168 1806 336 11136 10880 2 2 0 max max max 10567680 640 10880 65536 0 2268 18 7675 0
C 32 11136 2 256 10880 14 819200 65536 7617 19 7675
L 2120 11136 256 42 2 160 1640 320 11392 11136 2 2 0 max max max 0 256 11136 884736 10567680 2398 19 7676 0
C 32 11392 2 256 11136 14 0 884736 7618 20 7676
L 1944 11392 256 40 2 152 1482 304 11648 11392 2 1 0 max max max 10567680 256 11392 65536 0 2528 20 7677 0
C 32 11648 1 256 11392 6 819200 65536 7619 21 7677
L 1648 11648 256 38 1 74 1406 148 11776 11648 1 1 0 max max max 0 256 11648 835584 10567680 2658 21 7678 0
C 32 11776 1 128 11648 4 0 835584 7620 22 7678
L 1552 11776 128 37 1 72 1332 144 11904 11776 1 1 0 max max max 10567680 128 11776 16384 0 2788 22 7679 0
C 32 11904 1 128 11776 4 819200 16384 7621 23 7679
L 1480 11904 128 36 1 70 1260 140 12032 11904 1 1 0 max max max 0 128 11904 835584 10567680 2918 23 7680 0
C 32 12032 1 128 11904 4 0 835584 7622 24 7680
L 1408 12032 128 35 1 68 1190 136 12160 12032 1 1 0 max max max 10567680 128 12032 16384 0 3048 24 7681 0
C 32 12160 1 128 12032 4 819200 16384 7623 25 7681
L 1344 12160 128 34 1 66 1122 132 12288 12160 1 1 0 max max max 0 128 12160 835584 10567680 3178 25 7682 0
C 32 12288 1 128 12160 4 0 835584 7624 26 7682
L 1248 12288 128 33 1 64 1056 128 12416 12288 1 1 0 max max max 10567680 128 12288 16384 0 3308 26 7683 0
C 32 12416 1 128 12288 4 819200 16384 7625 27 7683
L 1184 12416 128 32 1 62 992 124 12544 12416 1 1 0 max max max 0 128 12416 835584 10567680 3438 27 7684 0
C 32 12544 1 128 12416 4 0 835584 7626 28 7684
L 1128 12544 128 31 1 60 930 120 12672 12544 1 1 0 max max max 10567680 128 12544 16384 0 3568 28 7685 0
C 32 12672 1 128 12544 4 819200 16384 7627 29 7685
L 1064 12672 128 30 1 58 870 116 12800 12672 1 1 0 max max max 0 128 12672 835584 10567680 3698 29 7686 0
C 32 12800 1 128 12672 4 0 835584 7628 30 7686
L 984 12800 128 29 1 56 812 112 12928 12800 1 1 0 max max max 10567680 128 12800 16384 0 3828 30 7687 0
C 32 12928 1 128 12800 4 819200 16384 7629 31 7687
L 928 12928 128 28 1 54 756 108 13056 12928 1 1 0 max max max 0 128 12928 835584 10567680 3958 31 7688 0
C 32 13056 1 128 12928 4 0 835584 7630 32 7688
L 872 13056 128 27 1 52 702 104 13184 13056 1 1 0 max max max 10567680 128 13056 16384 0 4088 32 7689 0
C 32 13184 1 128 13056 4 819200 16384 7631 33 7689
L 824 13184 128 26 1 50 650 100 13312 13184 1 1 0 max max max 0 128 13184 835584 10567680 4218 33 7690 0
C 32 13312 1 128 13184 4 0 835584 7632 34 7690
L 744 13312 128 25 1 48 600 96 13440 13312 1 1 0 max max max 10567680 128 13312 16384 0 4348 34 7691 0
C 32 13440 1 128 13312 4 819200 16384 7633 35 7691
L 696 13440 128 24 1 46 552 92 13568 13440 1 1 0 max max max 0 128 13440 835584 10567680 4478 35 7692 0
C 32 13568 1 128 13440 4 0 835584 7634 36 7692
L 656 13568 128 23 1 44 506 88 13696 13568 1 1 0 max max max 10567680 128 13568 16384 0 4608 36 7693 0
C 32 13696 1 128 13568 4 819200 16384 7635 37 7693
L 608 13696 128 22 1 42 462 84 13824 13696 1 1 0 max max max 0 128 13696 835584 10567680 4738 37 7694 0
C 32 13824 1 128 13696 4 0 835584 7636 38 7694
L 544 13824 128 21 1 40 420 80 13952 13824 1 1 0 max max max 10567680 128 13824 16384 0 4868 38 7695 0
C 32 13952 1 128 13824 4 819200 16384 7637 39 7695
L 504 13952 128 20 1 38 380 76 14080 13952 1 1 0 max max max 0 128 13952 835584 10567680 4998 39 7696 0
C 32 14080 1 128 13952 4 0 835584 7638 40 7696
L 464 14080 128 19 1 36 342 72 14208 14080 1 1 0 max max max 10567680 128 14080 16384 0 5128 40 7697 0
C 32 14208 1 128 14080 4 819200 16384 7639 41 7697
L 432 14208 128 18 1 34 306 68 14336 14208 1 1 0 max max max 0 128 14208 835584 10567680 5258 41 7698 0
C 32 14336 1 128 14208 4 0 835584 7640 42 7698
L 368 14336 128 17 1 32 272 64 14464 14336 1 1 0 max max max 10567680 128 14336 16384 0 5388 42 7699 0
C 32 14464 1 128 14336 4 819200 16384 7641 43 7699
L 336 14464 128 16 1 30 240 60 14592 14464 1 1 0 max max max 0 128 14464 835584 10567680 5518 43 7700 0
C 32 14592 1 128 14464 4 0 835584 7642 44 7700
L 312 14592 128 15 1 28 210 56 14720 14592 1 1 0 max max max 10567680 128 14592 16384 0 5648 44 7701 0
C 32 14720 1 128 14592 4 819200 16384 7643 45 7701
L 280 14720 128 14 1 26 182 52 14848 14720 1 1 0 max max max 0 128 14720 835584 10567680 5778 45 7702 0
C 32 14848 1 128 14720 4 0 835584 7644 46 7702
L 232 14848 128 13 1 24 156 48 14976 14848 1 1 0 max max max 10567680 128 14848 16384 0 5908 46 7703 0
C 32 14976 1 128 14848 4 819200 16384 7645 47 7703
L 208 14976 128 12 1 22 132 44 15104 14976 1 1 0 max max max 0 128 14976 835584 10567680 6038 47 7704 0
C 32 15104 1 128 14976 4 0 835584 7646 48 7704
L 184 15104 128 11 1 20 110 40 15232 15104 1 1 0 max max max 10567680 128 15104 16384 0 6168 48 7705 0
C 32 15232 1 128 15104 4 819200 16384 7647 49 7705
L 168 15232 128 10 1 18 90 36 15360 15232 1 1 0 max max max 0 128 15232 835584 10567680 6298 49 7706 0
C 32 15360 1 128 15232 4 0 835584 7648 50 7706
L 120 15360 128 9 1 16 72 32 15488 15360 1 1 0 max max max 10567680 128 15360 16384 0 6428 50 7707 0
C 32 15488 1 128 15360 4 819200 16384 7649 51 7707
L 104 15488 128 8 1 14 56 28 15616 15488 1 1 0 max max max 0 128 15488 835584 10567680 6558 51 7708 0
C 32 15616 1 128 15488 4 0 835584 7650 52 7708
L 96 15616 128 7 1 12 42 24 15744 15616 1 1 0 max max max 10567680 128 15616 16384 0 6688 52 7709 0
C 32 15744 1 128 15616 4 819200 16384 7651 53 7709
L 80 15744 128 6 1 10 30 20 15872 15744 1 1 0 max max max 0 128 15744 835584 10567680 6818 53 7710 0
C 32 15872 1 128 15744 4 0 835584 7652 54 7710
L 48 15872 128 5 1 8 20 16 16000 15872 1 1 0 max max max 10567680 128 15872 16384 0 6948 54 7711 0
C 32 16000 1 128 15872 4 819200 16384 7653 55 7711
L 40 16000 128 4 1 6 12 12 16128 16000 1 1 0 max max max 0 128 16000 835584 10567680 7078 55 7712 0
C 32 16128 1 128 16000 4 0 835584 7654 56 7712
L 32 16128 128 3 1 4 6 8 16256 16128 1 1 0 max max max 10567680 128 16128 16384 0 7208 56 7713 0
C 32 16256 1 128 16128 4 819200 16384 7655 57 7713
L 32 16256 128 2 1 2 2 4 16384 16256 1 0 0 max max max 0 128 16256 835584 10567680 7338 57 -1 0
R 13107200 169082880 132096 131072 3276800 30856
F 4 0x1.2ea38aaaaaa9ep+33 0x1.1a2d555555561p+34
F 6 0x1.42658b8fp+40 0x1.4d838p+40
F 12 0x1.1ac6871p+36 0x1.633cp+36
)";
// ... N = 2560 with LFM_W4_MIN=1024, MLL (fused gram) ...
static const char kGolden2560[] = R"(E 30
M 900
C 32 0 1 0 0 0 0 -1 207 0 -1
L 80 0 0 0 0 0 0 80 128 0 1 0 0 max max max -1 0 0 16384 0 -1 0 -1 0
C 32 128 4 128 0 0 819200 16384 208 1 -1
L 656 128 128 20 4 128 272 256 640 128 4 5 0 max max max 0 128 128 1081344 1720320 9 1 218 1
C 32 640 5 512 128 70 0 1081344 209 2 218
T
L 472 640 512 16 5 110 132 220 1280 640 5 5 0 max max max 1720320 512 640 409600 0 31 2 219 0
C 32 1280 5 640 640 80 819200 409600 210 3 219
L 240 1280 640 11 5 60 42 120 1920 1280 5 1 0 max max max 0 640 1280 1228800 1720320 53 3 220 0
C 32 1920 1 640 1280 12 0 1228800 211 4 220
L 80 1920 640 6 1 10 30 20 2048 1920 1 1 0 max max max 1720320 640 1920 16384 0 75 4 221 0
C 32 2048 1 128 1920 4 819200 16384 212 5 221
L 48 2048 128 5 1 8 20 16 2176 2048 1 1 0 max max max 0 128 2048 835584 1720320 97 5 222 0
C 32 2176 1 128 2048 4 0 835584 213 6 222
L 40 2176 128 4 1 6 12 12 2304 2176 1 1 0 max max max 1720320 128 2176 16384 0 119 6 223 0
C 32 2304 1 128 2176 4 819200 16384 214 7 223
L 32 2304 128 3 1 4 6 8 2432 2304 1 1 0 max max max 0 128 2304 835584 1720320 141 7 224 0
C 32 2432 1 128 2304 4 0 835584 215 8 224
L 32 2432 128 2 1 2 2 4 2560 2432 1 0 0 max max max 1720320 128 2432 16384 0 163 8 -1 0
R 13107200 27525120 21504 131072 3276800 900
F 4 0x1.298f555555557p+30 0x1.202aaaaaaaaa9p+31
F 6 0x1.213e8p+32 0x1.7bcp+32
F 12 0x0p+0 0x0p+0
)";
// ... and the same size bordered (the gradient's inverse)
static const char kGolden2560b[] = R"(E 21
M 600
C 32 0 1 0 0 0 0 -1 138 0 -1
L 96 0 0 0 0 0 0 84 128 0 1 0 0 max 2688 2561 -1 0 0 16384 0 -1 0 -1 0
C 32 128 4 128 0 0 524288 16384 139 1 -1
L 784 128 128 21 4 136 306 336 640 128 4 4 0 2688 2816 2561 0 128 128 786432 1376256 6 1 146 0
C 32 640 4 512 128 52 0 786432 140 2 146
T
L 784 640 512 21 4 136 306 336 1152 640 4 4 0 2816 3328 2561 1376256 512 640 262144 0 28 2 147 0
C 32 1152 4 512 640 52 524288 262144 141 3 147
L 784 1152 512 21 4 136 306 336 1664 1152 4 4 0 3328 3840 2561 0 512 1152 786432 1376256 50 3 148 0
C 32 1664 4 512 1152 52 0 786432 142 4 148
L 784 1664 512 21 4 136 306 336 2176 1664 4 4 0 3840 4352 2561 1376256 512 1664 262144 0 72 4 149 0
C 32 2176 4 512 1664 52 524288 262144 143 5 149
L 784 2176 512 21 4 136 306 336 2688 2176 4 0 0 4352 4864 2561 0 512 2176 786432 1376256 94 5 -1 0
L 464 2688 512 21 0 0 462 0 0 0 0 0 0 4864 max 2561 1376256 512 2688 -1 -1 -1 -1 -1 0
R 8388608 22020096 21504 131072 2097152 600
F 4 0x1.3fc3fffffffffp+30 0x1.30fffffffffffp+31
F 6 0x1.441f5p+34 0x1.678p+34
F 12 0x0p+0 0x0p+0
)";

static void check_s3_golden() {
  struct Case { int64_t n; bool bordered; int64_t w4min; bool fused; const char* want; };
  const Case cases[] = {{16384, false, 6144, true, kGolden16384},
                        {2560, false, 1024, true, kGolden2560},
                        {2560, true, 1024, false, kGolden2560b}};
  for (const Case& c : cases) {
    const int64_t Mp = (c.n + 1 + 127) / 128 * 128;
    const int64_t cols = c.bordered ? Mp / 128 : (c.n + 127) / 128;
    const auto steps = plan_steps(cols, Mp, 128, c.bordered, true, c.bordered ? 4 : 5, c.w4min,
                                  5120, 1);
    S3Params p = s3_params(c.n, Mp, c.bordered, 32, 1, true);
    p.fused = c.fused;
    const std::string got = s3_launch_text(plan_s3(steps, p), p);
    if (got != c.want) {
      size_t i = 0;
      while (i < got.size() && got[i] == c.want[i]) ++i;
      const size_t b = got.rfind('\n', i) + 1;
      CHECK(false, "golden plan n=%lld%s differs at byte %zu: got '%s'", (long long)c.n,
            c.bordered ? " bordered" : "", i, got.substr(b, got.find('\n', i) - b).c_str());
    }
  }
  std::printf("plan_s3: 3 golden plans reproduced\n");
}

// A kept plan is reused while its inputs hold and rebuilt when any of them changes
static void check_s3_keep() {
  const int64_t n = 2560, Mp = 2688;
  const auto steps = plan_steps(20, Mp, 128, false, true, 5, 1024, 5120, 1);
  const S3Params p = s3_params(n, Mp, false, 32, 1, false);
  S3Plan kept;
  CHECK(plan_s3_keep(kept, steps, p) && kept.S == (int)steps.size(), "first call builds");
  const S3Step* data = kept.steps.data();
  CHECK(!plan_s3_keep(kept, steps, p) && kept.steps.data() == data, "same inputs: reused");
  // every field of the parameters, and the step list, invalidates
  std::vector<S3Params> changed(15, p);
  changed[0].n -= 1;
  changed[1].Mp += 128;
  changed[2].bordered = true;
  changed[3].fused = true;
  changed[4].prof = true;
  changed[5].nb = 64;
  changed[6].st = 64;
  changed[7].tall_split = 1;
  changed[8].supertile = 1;
  changed[9].cus = 304;
  changed[10].side_cus = 8;
  changed[11].helper = 0;
  changed[12].helper_tc = 701;
  changed[13].helper_min = 1201;
  changed[14].ovl_at = 1024;
  for (size_t i = 0; i < changed.size(); ++i) {
    CHECK(plan_s3_keep(kept, steps, changed[i]), "changed parameter %zu: not rebuilt", i);
    CHECK(kept.params == changed[i] && plan_s3_keep(kept, steps, p), "back to the first inputs");
  }
  const auto steps2 = plan_steps(20, Mp, 128, false, true, 5, 6144, 5120, 1);
  CHECK(steps2 != steps && plan_s3_keep(kept, steps2, p) && kept.step_list == steps2,
        "changed step list: rebuilt");
  CHECK(s3_launch_text(kept, p) == s3_launch_text(plan_s3(steps2, p), p), "kept plan = fresh plan");
  std::printf("plan_s3: kept plan reused and invalidated\n");
}

static void check_s3_plans() {
  int cases = 0;
  const int64_t knobs[3][2] = {{6144, 5120}, {1024, 5120}, {(int64_t)1 << 30, 1024}};
  for (int64_t nblk : {1, 2, 3, 5, 9, 17, 33, 65, 129, 130})
    for (int64_t dn : {1, 128, 129})
      for (bool bordered : {false, true})
        for (int w0 : {1, 2})
          for (const auto& kn : knobs)
            for (int side_cus : {8, 32})
              for (int helper : {0, 1}) {
                const int64_t Mp = nblk * 128, n = Mp - dn;
                if (n <= 0) continue;
                const int64_t cols = bordered ? Mp / 128 : (n + 127) / 128;
                const auto steps =
                    plan_steps(cols, Mp, 128, bordered, true, bordered ? 4 : 5, kn[0], kn[1], w0);
                // the helpers' algorithmic flops (a loop over their units' rows) on a subset
                const S3Params p =
                    s3_params(n, Mp, bordered, side_cus, helper, w0 == 1 && side_cus == 32);
                char tag[128];
                std::snprintf(tag, sizeof(tag), "n=%lld Mp=%lld %s w0=%d w4min=%lld side=%d helper=%d",
                              (long long)n, (long long)Mp, bordered ? "bordered" : "mll", w0,
                              (long long)kn[0], side_cus, helper);
                check_s3_plan(steps, p, plan_s3(steps, p), tag);
                ++cases;
              }
  std::printf("plan_s3: %d plans\n", cases);
}

static void check_oracle() {
  const int G = 4, T = 24, n = G * T;
  std::vector<int> g4 = {0, 1, 2, 3};
  auto x = grid_x(G, T, 1, g4);
  std::vector<double> D = {0.3, 0.5, 0.7, 0.9}, S = {1.0, 0.8, 1.2, 0.9}, B = {0.05, 0.02, 0.07, 0.1};
  std::vector<double> y(n);
  std::mt19937_64 rng(3);
  std::normal_distribution<double> nd(0, 0.5);
  for (int i = 0; i < n; ++i) y[i] = B[i / T] / D[i / T] + nd(rng);
  std::vector<double> info(8), work((size_t)n * n);
  const double v1 = lfm_cpu_mll(x.data(), y.data(), n, G, D.data(), S.data(), B.data(), 2.5, 1.0,
                                1e-4, 0, 2, nullptr, info.data());
  const double v2 = lfm_cpu_mll(x.data(), y.data(), n, G, D.data(), S.data(), B.data(), 2.5, 1.0,
                                1e-4, 1, 2, work.data(), nullptr);
  CHECK(std::isfinite(v1) && v2 == -v1, "mll / negative");
  std::vector<double> K((size_t)n * n, 0.0);
  CHECK(lfm_cpu_gram(x.data(), n, G, D.data(), S.data(), 2.5, 0.0, K.data(), n, 2) == 0, "gram");
  std::vector<int64_t> rows = {0, 5, n - 1};
  std::vector<float> R(rows.size() * n, 0.0f);
  CHECK(lfm_cpu_gram_rows_f32(x.data(), n, G, D.data(), S.data(), 2.5, 0.0, rows.data(),
                              (int64_t)rows.size(), R.data(), 2) == 0, "gram rows");
  for (size_t q = 0; q < rows.size(); ++q)
    for (int64_t j = 0; j <= rows[q]; ++j)
      CHECK(R[q * n + j] == (float)K[rows[q] * n + j], "rows vs gram");
  int64_t bad = n;
  CHECK(lfm_cpu_gram_rows_f32(x.data(), n, G, D.data(), S.data(), 2.5, 0.0, &bad, 1, R.data(),
                              1) == 1, "row out of range refused");
  for (int i = 0; i < n; ++i) K[(size_t)i * n + i] += 1.0;
  CHECK(lfm_cpu_potrf(K.data(), n, n, 2) == -1, "potrf of K + I");
  std::printf("oracle: mll %.10f\n", v1);
}

// The device tenancy lock (TenancyLock, lfm_ctx.hip DeviceTenancy). Two objects on one path
// stand for two processes (flock is per open file description).
static void check_tenancy() {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) {
    return std::chrono::duration<double, std::milli>(clk::now() - t).count();
  };
  char dir[] = "/tmp/lfm_tenancy_XXXXXX";
  CHECK(mkdtemp(dir) != nullptr, "mkdtemp");
  const std::string path = std::string(dir) + "/lfm_gpu_test.lock";
  TenancyLock a, b;
  CHECK(a.open(path) && b.open(path), "open");
  CHECK(a.path() == path, "path");
  TenancyLock bad;
  CHECK(!bad.open(std::string(dir) + "/no_suffix"), "a path without .lock is refused");

  // exclusive: mutual exclusion over threads
  {
    int counter = 0;
    std::vector<std::thread> ts;
    for (int t = 0; t < 4; ++t)
      ts.emplace_back([&] {
        for (int i = 0; i < 2000; ++i) {
          a.lock_exclusive();
          const int v = counter;
          counter = v + 1;
          a.unlock_exclusive();
        }
      });
    for (auto& t : ts) t.join();
    CHECK(counter == 8000, "exclusive sections overlapped: %d", counter);
  }
  // shared: two readers inside at once
  {
    std::atomic<int> inside{0};
    std::atomic<bool> both{false};
    auto reader = [&] {
      a.lock_shared();
      ++inside;
      const auto t0 = clk::now();
      while (inside.load() < 2 && ms_since(t0) < 2000) std::this_thread::yield();
      if (inside.load() == 2) both = true;
      a.unlock_shared();
    };
    std::thread r1(reader), r2(reader);
    r1.join();
    r2.join();
    CHECK(both.load(), "two shared holders were not admitted together");
  }
  // another "process" holding it exclusively: a shared request waits for the release
  {
    std::atomic<bool> held{false};
    std::thread w([&] {
      b.lock_exclusive();
      held = true;
      std::this_thread::sleep_for(std::chrono::milliseconds(200));
      b.unlock_exclusive();
    });
    while (!held.load()) std::this_thread::yield();
    const auto t0 = clk::now();
    a.lock_shared();
    const double waited = ms_since(t0);
    a.unlock_shared();
    w.join();
    CHECK(waited >= 150.0, "shared request did not wait for the other writer (%.1f ms)", waited);
  }
  // turnstile: while a writer of another "process" waits for this process's reader, a second
  // reader of this process queues behind the writer instead of joining the first reader
  {
    std::atomic<bool> r1_in{false}, w_waiting{false};
    std::atomic<double> w_at{0.0}, r2_at{0.0};
    const auto t0 = clk::now();
    std::thread r1([&] {
      a.lock_shared();
      r1_in = true;
      std::this_thread::sleep_for(std::chrono::milliseconds(300));
      a.unlock_shared();
    });
    while (!r1_in.load()) std::this_thread::yield();
    std::thread w([&] {
      w_waiting = true;
      b.lock_exclusive();
      w_at = ms_since(t0);
      std::this_thread::sleep_for(std::chrono::milliseconds(100));
      b.unlock_exclusive();
    });
    while (!w_waiting.load()) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(80));  // the writer is queued now
    std::thread r2([&] {
      a.lock_shared();
      r2_at = ms_since(t0);
      a.unlock_shared();
    });
    r1.join();
    w.join();
    r2.join();
    CHECK(w_at.load() >= 250.0, "writer got in before the reader left (%.1f ms)", w_at.load());
    CHECK(r2_at.load() >= w_at.load() + 80.0,
          "second reader overtook the waiting writer (writer %.1f, reader %.1f ms)", w_at.load(),
          r2_at.load());
  }
  // a flock failure (here EBADF: the lock file's descriptor swapped for an O_PATH one, which
  // flock refuses) is recorded, not ignored: the lock turns in-process only and says so once,
  // and the in-process part still excludes
  {
    const std::string p2 = std::string(dir) + "/lfm_gpu_fail.lock";
    TenancyLock c;
    CHECK(c.open(p2), "open p2");
    int lock_fd = -1;
    for (int fd = 0; fd < 1024; ++fd) {
      char link[64], target[512];
      std::snprintf(link, sizeof(link), "/proc/self/fd/%d", fd);
      const ssize_t k = readlink(link, target, sizeof(target) - 1);
      if (k <= 0) continue;
      target[k] = 0;
      if (p2 == target) lock_fd = fd;
    }
    CHECK(lock_fd >= 0, "lock file descriptor not found");
    const int op = ::open(p2.c_str(), O_PATH | O_CLOEXEC);
    CHECK(op >= 0 && dup2(op, lock_fd) == lock_fd, "dup2 O_PATH");
    ::close(op);
    CHECK(c.error() == 0, "no error before the first lock");
    c.lock_exclusive();
    CHECK(c.error() == EBADF, "flock failure not recorded (%d)", c.error());
    c.unlock_exclusive();
    int counter = 0;
    std::vector<std::thread> ts;
    for (int t = 0; t < 4; ++t)
      ts.emplace_back([&] {
        for (int i = 0; i < 500; ++i) {
          if (i & 1) {
            c.lock_shared();
            c.unlock_shared();
          }
          c.lock_exclusive();
          const int v = counter;
          counter = v + 1;
          c.unlock_exclusive();
        }
      });
    for (auto& t : ts) t.join();
    CHECK(counter == 2000, "in-process exclusion lost after the flock failure: %d", counter);
    unlink(p2.c_str());
    unlink((p2.substr(0, p2.size() - 5) + ".turn").c_str());
  }
  std::string turn = path.substr(0, path.size() - 5) + ".turn";
  unlink(path.c_str());
  unlink(turn.c_str());
  rmdir(dir);
  std::printf("tenancy lock: ok\n");
}

// ------------------------------------------------------------ the small-problem path
// Every shape the small kernels take: n = 1..128, G | n, T = 0 or T | n with its grid tables
// within SMALL_GRID_TAB_MAX (lfm_batch_create's admission, small_grid_T)
static std::vector<SmallShape> small_shape_set(int nmax) {
  std::vector<SmallShape> out;
  for (int n = 1; n <= nmax; ++n)
    for (int G = 1; G <= n; ++G) {
      if (n % G) continue;
      out.push_back({n, G, 0});
      for (int T = 1; T <= n; ++T)
        if (n % T == 0 && tables_doubles(G, T) <= (size_t)SMALL_GRID_TAB_MAX)
          out.push_back({n, G, T});
    }
  return out;
}

// the regions of one map (doubles from the base) with the sizes the kernels use, stated here
// from the layout's description, not from small_map's arithmetic
struct Region {
  const char* name;
  size_t at, len;
};
static std::vector<Region> map_regions(const double* base, const SmallMap& m, const SmallShape& s,
                                       int tabs, int grad, int fit) {
  const size_t n = s.n, G = s.G, T = s.T, W = T ? 2 * T - 1 : 0, nh = 3 * G + 3;
  std::vector<Region> r;
  auto add = [&](const char* name, const void* p, size_t len) {
    if (len) r.push_back({name, (size_t)((const double*)p - base), len});
  };
  add("A", m.A, (n + 1) * (size_t)m.ld);
  add("red", m.red, 16);
  add("hyp", m.hyp, nh);
  add("ktab", m.ktab, tabs ? 3 * G + n + n * G : 0);
  add("colbuf", m.colbuf, n + 1 > 64 ? (grad ? (size_t)SWEEP4_LDS : 512) : 264);
  add("xs", m.xs, 3 * n);
  add("ys", m.ys, n);
  add("gt", m.gt, T ? tables_doubles((int)G, (int)T) : 0);
  add("tms", m.tms, T);
  add("bgs", m.bgs, T ? (n / T + 1) / 2 : 0);  // n / T ints
  if (grad) {
    add("gg", m.gg, 6 * G * W + 8 * G * T);
    add("al", m.al, 128);
    add("wd", m.wd, 128);
    add("wb", m.wb, n + 1 <= 64 ? (n + 1) * (size_t)small_wb_ld((int)n) : 0);
    add("accw", m.accw, 4 * (2 * G + 1));
    add("gout", m.gout, nh);
    add("fcol", m.fcol, n + 1 <= 64 ? 128 : 0);
  }
  if (fit) {
    add("raw", m.raw, nh);
    add("mu", m.mu, nh);
    add("nu", m.nu, nh);
  }
  return r;
}

// regions inside [0, size) and pairwise disjoint; returns false on the first violation
static bool regions_ok(std::vector<Region> r, size_t size, const char** bad) {
  std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.at < b.at; });
  for (size_t i = 0; i < r.size(); ++i) {
    *bad = r[i].name;
    if (r[i].at + r[i].len > size) return false;
    if (i + 1 < r.size() && r[i].at + r[i].len > r[i + 1].at) return false;
  }
  return true;
}

static void check_small_map() {
  const std::vector<SmallShape> set = small_shape_set(SMALL_MAX);
  const int modes[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 1, 1}};
  std::vector<double> lds(64 * 1024);
  for (const SmallShape& s : set) {
    size_t size_grad = 0;
    SmallMap mg{};
    for (const auto& md : modes) {
      SmallMap m{};
      const size_t size = small_map(lds.data(), s.n, s.G, s.T, md[0], md[1], md[2], &m);
      CHECK(size == small_map(nullptr, s.n, s.G, s.T, md[0], md[1], md[2], nullptr),
            "map size with / without a base (%d,%d,%d)", s.n, s.G, s.T);
      CHECK(size <= lds.size(), "map of (%d,%d,%d) is %zu doubles", s.n, s.G, s.T, size);
      const char* bad = "";
      CHECK(regions_ok(map_regions(lds.data(), m, s, md[0], md[1], md[2]), size, &bad),
            "map (%d,%d,%d) mode %d%d%d: region %s overlaps or leaves the map", s.n, s.G, s.T,
            md[0], md[1], md[2], bad);
      CHECK((m.colbuf - lds.data()) % 2 == 0, "colbuf not 16-byte aligned (%d,%d,%d)", s.n, s.G,
            s.T);
      CHECK(m.n == s.n && m.G == s.G && m.ld == ((s.n + 2) | 1),
            "map header (%d,%d,%d)", s.n, s.G, s.T);
      if (md[1] && !md[2]) {
        size_grad = size;
        mg = m;
      }
      if (md[2]) {
        // the fit map = the gradient map + raw, mu, nu: small_value_grad_step's rebuild (fit = 1)
        // sees small_grad_one's offsets (fit = 0)
        const size_t nh = 3 * (size_t)s.G + 3;
        SmallMap e = mg;
        e.raw = lds.data() + size_grad;
        e.mu = e.raw + nh;
        e.nu = e.mu + nh;
        CHECK(size == size_grad + 3 * nh && std::memcmp(&e, &m, sizeof(SmallMap)) == 0,
              "fit map is not the gradient map + 3 trailing regions (%d,%d,%d)", s.n, s.G, s.T);
      }
    }
    CHECK(small_grid_extra(s.n, s.G, s.T) ==
              (s.T ? tables_doubles(s.G, s.T) + s.T + ((size_t)s.n / s.T + 1) / 2 + 1 : 0),
          "small_grid_extra(%d,%d,%d)", s.n, s.G, s.T);
    // the times [T] and the block genes (n / T ints) fit the staging area's grid slots
    CHECK(s.T == 0 || s.T + (s.n / s.T + 1) / 2 <= small_grid_doubles(s.n),
          "small_grid_doubles(%d) below the grid part at T = %d", s.n, s.T);
  }
  std::printf("small map: %zu shapes x 4 modes disjoint, aligned, fit = gradient + 3\n",
              set.size());
}

// plan_small_mll of a batch's SmallDims holds each member's own map, within the limit. Pairs:
// every shape with n in kN x every shape with n in kN (the extremes 1 and 128 included).
static void check_small_bound() {
  const std::set<int> kN = {1, 2, 7, 28, 31, 32, 33, 62, 63, 64, 65, 96, 120, 126, 127, 128};
  std::vector<SmallShape> sub;
  for (const SmallShape& s : small_shape_set(SMALL_MAX))
    if (kN.count(s.n)) sub.push_back(s);
  size_t pairs = 0, worst = 0;
  for (const SmallShape& a : sub)
    for (const SmallShape& b : sub) {
      const SmallMllPlan pl = plan_small_mll(small_dims({a, b}));
      for (const SmallShape& s : {a, b})
        CHECK(pl.lds_bytes >= 8 * small_map(nullptr, s.n, s.G, s.T, pl.tabs, 0, 0, nullptr),
              "plan_small_mll of (%d,%d,%d)+(%d,%d,%d) below a member's map", a.n, a.G, a.T, b.n,
              b.G, b.T);
      CHECK(pl.tabs == (std::max(a.n, b.n) + 1 <= 64), "tabs");
      CHECK(pl.lds_bytes <= SMALL_LDS_BYTES, "admitted pair (%d,%d,%d)+(%d,%d,%d): %zu bytes",
            a.n, a.G, a.T, b.n, b.G, b.T, pl.lds_bytes);
      worst = std::max(worst, pl.lds_bytes);
      ++pairs;
    }
  // the plan grows with each of maxn, maxg and gridtab, so the extreme of the whole shape set
  // bounds every batch: n = G = 128 beside the largest grid part of any shape
  size_t gmax = 0;
  for (const SmallShape& s : small_shape_set(SMALL_MAX))
    gmax = std::max(gmax, small_grid_extra(s.n, s.G, s.T));
  const size_t top = plan_small_mll(SmallDims{SMALL_MAX, SMALL_MAX, (int)gmax}).lds_bytes;
  CHECK(top <= SMALL_LDS_BYTES, "the extreme batch (grid part %zu doubles) takes %zu bytes", gmax,
        top);
  worst = std::max(worst, top);
  // golden: the parent's small_lds / tabs, small_grad_lds
  const int g[5][5] = {{28, 5, 0, 11936, 1}, {63, 9, 0, 43040, 1}, {64, 8, 0, 41328, 0},
                       {128, 16, 0, 143920, 0}, {28, 4, 214, 13376, 1}};
  for (const auto& c : g) {
    const SmallMllPlan pl = plan_small_mll(SmallDims{c[0], c[1], c[2]});
    CHECK((int)pl.lds_bytes == c[3] && pl.tabs == c[4], "plan_small_mll(%d,%d,%d) = %zu / %d",
          c[0], c[1], c[2], pl.lds_bytes, pl.tabs);
  }
  CHECK(small_grid_extra(28, 4, 7) == 214 && small_dims({{28, 4, 7}}).gridtab == 214, "gridtab");
  // (one-wave problems: 1024 bytes more than before the value's factor got its column buffer)
  const int gl[4][5] = {{28, 4, 7, 28800, 29160}, {63, 9, 7, 94024, 94744},
                        {64, 8, 8, 69200, 69848}, {127, 1, 0, 151024, 151168}};
  for (const auto& c : gl)
    CHECK((int)small_grad_lds({{c[0], c[1], c[2]}}, 0) == c[3] &&
              (int)small_grad_lds({{c[0], c[1], c[2]}}, 1) == c[4],
          "small_grad_lds(%d,%d,%d)", c[0], c[1], c[2]);
  // 0: n = 128 (two waves hold n + 1 <= 128 rows), or a map past the limit
  CHECK(small_grad_lds({{28, 4, 7}, {128, 16, 0}}, 0) == 0, "small_grad_lds at n = 128");
  for (const SmallShape& s : sub)
    for (int fit = 0; fit < 2; ++fit) {
      const size_t own = 8 * small_map(nullptr, s.n, s.G, s.T, 1, 1, fit, nullptr);
      CHECK(small_grad_lds({s}, fit) == (s.n > SMALL_GRAD_MAX || own > SMALL_LDS_BYTES ? 0 : own),
            "small_grad_lds(%d,%d,%d)", s.n, s.G, s.T);
    }
  std::printf("small bound: %zu pairs, largest launch %zu bytes\n", pairs, worst);
}

// the kernel's tri_index (lfm_small.hip)
static void tri_index(int q, int* i_out, int* c_out) {
  int i = (int)((std::sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > q) --i;
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  *i_out = i;
  *c_out = q - i * (i + 1) / 2;
}

// lfm_batch_posterior_f64's admission as the parent wrote it inline
static PostPlan::Reject post_reject(const std::vector<SmallShape>& sh,
                                    const std::vector<int64_t>& m, bool cov) {
  int64_t sm = 0, sc = 0, ntiles = 0;
  for (size_t p = 0; p < sh.size(); ++p) {
    if (m[p] < 1 || m[p] % sh[p].G != 0 || m[p] > (1 << 20)) return PostPlan::BAD_M;
    if (!small_post_cols(sh[p].n, sh[p].G, sh[p].T)) return PostPlan::NO_FIT;
    const int64_t tb = (m[p] + 15) / 16;
    sm += m[p];
    sc += cov ? m[p] * m[p] : 0;
    ntiles += cov ? tb * (tb + 1) / 2 : 0;
    if (sm > ((int64_t)1 << 28) || sc > ((int64_t)1 << 29) || ntiles > INT_MAX / 2)
      return PostPlan::TOO_LARGE;
  }
  return PostPlan::OK;
}

static void check_post_plan(const std::vector<SmallShape>& sh, const std::vector<int64_t>& m,
                            int64_t nhyp, bool dv, bool cov) {
  const PostPlan P = plan_small_post(sh, nhyp, m.data(), dv, cov);
  CHECK(P.reject == post_reject(sh, m, cov), "posterior plan: reject %d", (int)P.reject);
  if (P.reject) return;
  const size_t np = sh.size();
  int64_t sm = 0, sn = 0, sv = 0, sc = 0, ntiles = 0, wg64 = 0;
  size_t lds = 0;
  for (size_t p = 0; p < np; ++p) {
    const PostProb& q = P.pp[p];
    CHECK(q.t_off == sm && q.v_off == sv && q.cov_off == sc && q.m == m[p] && q.dv_off == sn &&
              q.tile0 == ntiles && q.pad == 0,
          "PostProb %zu", p);
    const int64_t tb = (m[p] + 15) / 16;
    sm += m[p];
    sn += sh[p].n;
    sv += cov ? sh[p].n * m[p] : 0;
    sc += cov ? m[p] * m[p] : 0;
    ntiles += cov ? tb * (tb + 1) / 2 : 0;
    wg64 += (m[p] + 63) / 64;
  }
  CHECK(P.sm == sm && P.sn == sn && P.sv == sv && P.sc == sc && P.ntiles == ntiles, "sums");
  CHECK(P.unit == (wg64 <= 4096 ? 64 : 256) && P.nsplit >= 1 && P.nsplit <= 1024, "unit / nsplit");
  // the call's buffer, in bytes: disjoint, inside, aligned
  struct B {
    size_t at, len;
  };
  const std::vector<B> in = {{0, (size_t)nhyp * 8}, {P.dadd * 8, np * 8},
                             {P.dv * 8, dv ? (size_t)sn * 8 : 0}, {P.t * 8, (size_t)sm * 24},
                             {P.table * 8, np * sizeof(PostProb)}};
  const std::vector<B> out = {{P.mean * 8, (size_t)sm * 8}, {P.var * 8, (size_t)sm * 8},
                              {P.V * 8, (size_t)sv * 8}, {P.cov * 8, (size_t)sc * 8},
                              {P.status * 8, np * sizeof(int)}};
  size_t end = 0;
  for (const B& b : in) {
    CHECK(b.at == end && b.at % 8 == 0, "posterior inputs: not back to back");
    end = b.at + b.len;
  }
  CHECK(end == P.in_bytes, "in_bytes");
  for (const B& b : out) {
    CHECK(b.at >= end && b.at % 8 == 0, "posterior outputs overlap");
    end = std::max(end, b.at + b.len);
  }
  CHECK(end == P.all_bytes, "all_bytes");
  // small_post_kernel's passes: grid (problem, split), j0 = split unit; j0 += nsplit unit
  int64_t passes = 1;  // the most any problem has
  for (size_t p = 0; p < np; ++p) {
    const int cols = small_post_cols(sh[p].n, sh[p].G, sh[p].T);
    const int unit = std::min(P.unit, cols);
    lds = std::max(lds, 8 * (small_post_base(sh[p].n, sh[p].G, sh[p].T) + (size_t)sh[p].n * cols));
    CHECK(8 * (small_post_base(sh[p].n, sh[p].G, sh[p].T) + (size_t)sh[p].n * unit) <= P.lds_bytes,
          "panel of problem %zu past the launch's LDS", p);
    std::vector<unsigned char> seen((size_t)m[p], 0);
    bool once = true;
    for (int split = 0; split < P.nsplit; ++split) {
      if ((int64_t)split * unit >= m[p]) continue;
      for (int64_t j0 = (int64_t)split * unit; j0 < m[p]; j0 += (int64_t)P.nsplit * unit)
        for (int64_t j = j0; j < j0 + unit && j < m[p]; ++j) once = once && seen[j]++ == 0;
    }
    for (unsigned char c : seen) once = once && c == 1;
    CHECK(once, "test columns of problem %zu not covered exactly once", p);
    passes = std::max(passes, (m[p] + unit - 1) / unit);
  }
  CHECK(P.nsplit == std::min<int64_t>(passes, 1024), "nsplit %d, the most passes of a problem %lld",
        P.nsplit, (long long)passes);
  CHECK(P.lds_bytes == lds && lds <= SMALL_LDS_BYTES, "posterior LDS %zu", P.lds_bytes);
  // small_post_cov_kernel: tile -> the last problem whose first tile is not past it
  size_t p_true = 0;
  for (int tile = 0; tile < P.ntiles; ++tile) {
    int lo = 0, hi = (int)np - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (P.pp[mid].tile0 <= tile) lo = mid;
      else hi = mid - 1;
    }
    const int64_t tb = (m[lo] + 15) / 16;
    while (tile >= P.pp[p_true].tile0 + ((m[p_true] + 15) / 16) * ((m[p_true] + 15) / 16 + 1) / 2)
      ++p_true;
    int ti, tj;
    tri_index(tile - P.pp[lo].tile0, &ti, &tj);
    CHECK((size_t)lo == p_true && tj >= 0 && tj <= ti && ti < tb, "tile %d -> problem %d (%d,%d)",
          tile, lo, ti, tj);
  }
}

static void check_small_post() {
  const std::vector<SmallShape> all = small_shape_set(SMALL_GRAD_MAX);
  std::vector<SmallShape> fits;
  const SmallShape* nofit = nullptr;
  for (const SmallShape& s : all) {
    const int c = small_post_cols(s.n, s.G, s.T);
    const size_t base = small_post_base(s.n, s.G, s.T), cap = SMALL_LDS_BYTES / 8;
    CHECK(c == 0 || (c >= 16 && c <= 256 && (c & (c - 1)) == 0), "cols %d", c);
    CHECK(base + (size_t)s.n * c <= cap, "panel of (%d,%d,%d) past the limit", s.n, s.G, s.T);
    CHECK(c == 256 || base + (size_t)s.n * (c ? 2 * c : 16) > cap, "cols of (%d,%d,%d) not maximal",
          s.n, s.G, s.T);
    if (c) fits.push_back(s);
    else if (!nofit) nofit = &s;
  }
  CHECK(small_post_cols(28, 4, 7) == 256 && small_post_cols(120, 8, 15) == 16 &&
            small_post_cols(127, 1, 0) == 16, "golden small_post_cols");
  // golden: the C5 calls (15 problems, n = 28 on the 4 x 7 grid)
  const std::vector<SmallShape> c5(15, SmallShape{28, 4, 7});
  for (int cov = 0; cov < 2; ++cov) {
    const std::vector<int64_t> m(15, cov ? 400 : 100);
    const PostPlan P = plan_small_post(c5, 15 * 15, m.data(), false, cov);
    CHECK(P.reject == PostPlan::OK && P.unit == 64 && P.nsplit == (cov ? 7 : 2) &&
              P.ntiles == (cov ? 4875 : 0) && P.lds_bytes == 70944,
          "golden C5 posterior plan (cov %d): %d %d %d %zu", cov, P.unit, P.nsplit, P.ntiles,
          P.lds_bytes);
  }
  std::mt19937_64 rng(11);
  int plans = 0;
  for (int np = 1; np <= 16; ++np)
    for (int rep = 0; rep < 6; ++rep) {
      std::vector<SmallShape> sh;
      int64_t nhyp = 0;
      for (int p = 0; p < np; ++p) {
        sh.push_back(fits[rng() % fits.size()]);
        nhyp += 3 * sh.back().G + 3;
      }
      // m: G, 16 G - G, the multiples of G around 64 k (k = 1, 2, 5), and (mode 5; with cov it
      // is past the limits and must be rejected so) one giving wg64 > 4096
      for (int mode = 0; mode < 6; ++mode) {
        std::vector<int64_t> m;
        for (int p = 0; p < np; ++p) {
          const int64_t ks[3] = {1, 2, 5};
          const int64_t G = sh[p].G, k64 = 64 * ks[rng() % 3];
          const int64_t near = std::max<int64_t>(k64 / G, 1) * G;
          m.push_back(mode == 0   ? G
                      : mode == 1 ? 15 * G
                      : mode == 2 ? std::max(near - G, G)
                      : mode == 3 ? near + G
                      : mode == 4 ? near
                                  : (4100 * 64 / np + 64) / G * G + G);
        }
        for (int dv = 0; dv < 2; ++dv)
          for (int cov = 0; cov < 2; ++cov) {
            check_post_plan(sh, m, nhyp, dv, cov);
            ++plans;
          }
      }
    }
  // the rejections, in the parent's precedence
  const SmallShape ok = {28, 4, 7};
  auto rej = [&](std::vector<SmallShape> sh, std::vector<int64_t> m, bool cov) {
    return plan_small_post(sh, 15, m.data(), false, cov).reject;
  };
  CHECK(rej({ok}, {30}, false) == PostPlan::BAD_M, "m not a multiple of G");
  CHECK(rej({ok}, {0}, false) == PostPlan::BAD_M, "m < 1");
  CHECK(rej({ok}, {(1 << 20) + 4}, false) == PostPlan::BAD_M, "m > 2^20");
  CHECK(rej({ok}, {1 << 20}, false) == PostPlan::OK, "m = 2^20");
  CHECK(rej({ok}, {1 << 15}, true) == PostPlan::TOO_LARGE, "cov of 2^30 entries");
  CHECK(rej({ok, ok}, {1 << 15, 30}, true) == PostPlan::TOO_LARGE, "sum limit before the next m");
  CHECK(rej(std::vector<SmallShape>(257, ok), std::vector<int64_t>(257, 1 << 20), false) ==
            PostPlan::TOO_LARGE, "sum of m > 2^28");
  CHECK(nofit != nullptr, "no shape with n <= 127 whose posterior map is past the limit");
  if (nofit) {
    const int64_t G = nofit->G;
    CHECK(rej({*nofit}, {G}, false) == PostPlan::NO_FIT, "map past the limit");
    CHECK(rej({*nofit}, {0}, false) == PostPlan::BAD_M, "its own bad m first");
    CHECK(rej({ok, *nofit}, {30, G}, false) == PostPlan::BAD_M, "an earlier bad m first");
    CHECK(rej({*nofit, ok}, {G, 30}, false) == PostPlan::NO_FIT, "an earlier map first");
  }
  std::printf("small posterior: %zu shapes' columns, %d plans\n", all.size(), plans);
}

static void check_small_pack() {
  const std::vector<SmallShape> set = small_shape_set(SMALL_MAX);
  std::mt19937_64 rng(13);
  for (int rep = 0; rep < 400; ++rep)
    for (int inl = 0; inl < 2; ++inl) {
      std::vector<SmallShape> sh;
      for (int p = 0, np = 1 + (int)(rng() % 16); p < np; ++p) sh.push_back(set[rng() % set.size()]);
      const SmallPack P = plan_small_pack(sh, inl);
      size_t end = 0, bound = 0;
      for (size_t p = 0; p < sh.size(); ++p) {
        const size_t n = sh[p].n, G = sh[p].G, T = sh[p].T;
        const SmallPack::Slot& a = P.at[p];
        // x [3n] | y [n] | D S B [3G] | l obs_stddev jitter [3] | times [T], block genes [n / T]
        CHECK(a.x == end && a.y == a.x + 3 * n && a.dsb == a.y + n, "pack: x y of problem %zu", p);
        CHECK(inl ? a.sc == a.dsb + 3 * G && a.grid == a.sc + 3 : a.grid == a.dsb && a.sc == a.dsb,
              "pack: hyperparameters of problem %zu", p);
        end = a.grid + (T ? T + (n / T + 1) / 2 : 0);
        bound += 4 * n + (inl ? 3 * G + 3 : 0) + n + (n + 1) / 2;
      }
      CHECK(P.bound == bound && end <= P.bound, "pack: the problems end at %zu, bound %zu", end,
            P.bound);
    }
  // golden: the parent's pack_small over the 15 C5 problems and over a mixed batch (a grid, one
  // off the grid, two more grids); per problem x, y, dsb, sc, grid
  const std::vector<SmallShape> c5(15, SmallShape{28, 4, 7});
  const SmallPack a = plan_small_pack(c5, true), b = plan_small_pack(c5, false);
  for (size_t q = 0; q < 15; ++q) {
    const SmallPack::Slot &s = a.at[q], &t = b.at[q];
    CHECK(s.x == 136 * q && s.y == s.x + 84 && s.dsb == s.x + 112 && s.sc == s.x + 124 &&
              s.grid == s.x + 127, "golden C5 pack (inline) %zu", q);
    CHECK(t.x == 121 * q && t.y == t.x + 84 && t.grid == t.x + 112, "golden C5 pack %zu", q);
  }
  CHECK(a.at[14].grid + 9 == 2040 && b.at[14].grid + 9 == 1815, "golden C5 pack totals");
  const std::vector<SmallShape> mix = {{28, 4, 7}, {35, 5, 0}, {64, 8, 8}, {120, 8, 15}};
  const size_t gi[4][5] = {{0, 84, 112, 124, 127}, {136, 241, 276, 291, 294},
                           {294, 486, 550, 574, 577}, {589, 949, 1069, 1093, 1096}};
  const size_t gn[4][3] = {{0, 84, 112}, {121, 226, 261}, {261, 453, 517}, {529, 889, 1009}};
  const SmallPack mi = plan_small_pack(mix, true), mn = plan_small_pack(mix, false);
  for (size_t q = 0; q < 4; ++q) {
    const SmallPack::Slot &s = mi.at[q], &t = mn.at[q];
    CHECK(s.x == gi[q][0] && s.y == gi[q][1] && s.dsb == gi[q][2] && s.sc == gi[q][3] &&
              s.grid == gi[q][4], "golden mixed pack (inline) %zu", q);
    CHECK(t.x == gn[q][0] && t.y == gn[q][1] && t.grid == gn[q][2], "golden mixed pack %zu", q);
  }
  CHECK(mi.at[3].grid + 19 == 1115 && mn.at[3].grid + 19 == 1028, "golden mixed pack totals");
  // the pinned buffer and the fit buffer: back to back, the int status words in their own doubles
  const BatchLayout L = batch_layout(225, 15);
  CHECK(L.out == 225 && L.status == 240 && L.grad == 255 && L.bytes == 480 * 8,
        "batch_layout");
  const FitLayout F = fit_layout(225, 15, 20);
  CHECK(F.mu == 225 && F.nu == 450 && F.bias == 675 && F.hist == 715 && F.status == 1015 &&
            F.bytes == 8180,
        "fit_layout");
  std::printf("small pack: 800 batches, golden C5 and mixed offsets, batch / fit layouts\n");
}

int main() {
  check_small_map();
  check_small_bound();
  check_small_post();
  check_small_pack();
  check_tenancy();
  check_enumeration();
  check_helper_clamp();
  check_detect_grid();
  check_plan();
  check_s3_plans();
  check_s3_golden();
  check_s3_keep();
  check_oracle();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("host_check: all passed\n");
  return 0;
}
