// mid_post_plan_check.cpp — plan_mid_post (dis_project_amd/csrc/lfm_host.cpp), the second arena
// and the launch list of lfm_mbatch_posterior_f64 (lfm_mbatch.hip issues exactly what it says),
// under AddressSanitizer + UBSan: built and run by tests/test_mid_predict_host.py with the flags
// of tests/test_mid_host.py. Over n in {1, 63, 64, 127, 128, 129, 192, 193, 1023, 1024}, m in
// {G, 60, 64, 68, 130, 4096}, with and without diag_vec / cov, and mixed batches:
//   every region is inside the arena, disjoint from the others and 16-byte aligned; V is
//   64 ceil(m / 64) x Mp; the packed outputs are the caller's layout; in every launch every unit
//   has exactly one owner, by the kernels' own unit mapping; the launch list has the stated
//   length; the rejections come in the documented order with the limit in the message.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../dis_project_amd/csrc/lfm_host.h"

using namespace lfm;

static int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      if (++failures <= 20) {                         \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

struct Region {
  int64_t lo, hi;  // bytes
  const char* what;
};

static void check_regions(const MidPostPlan& P, const std::vector<MidShape>& shapes,
                          const std::vector<int64_t>& m, bool dv, bool cov) {
  std::vector<Region> rs;
  auto add = [&](int64_t lo_d, int64_t count_d, const char* what) {
    CHECK(lo_d >= 0 && lo_d % 2 == 0, "%s not 16-byte aligned", what);
    rs.push_back({lo_d * 8, (lo_d + count_d) * 8, what});
  };
  int64_t sn = 0, sm = 0, sc = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    sn += shapes[q].n;
    sm += m[q];
    sc += m[q] * m[q];
  }
  CHECK(P.sn == sn && P.sm == sm && P.sc == sc, "sums");
  add(P.dadd, P.nprob, "diag_add");
  CHECK((P.dv >= 0) == dv && (P.cov >= 0) == cov, "optional regions");
  if (dv) add(P.dv, sn, "diag_vec");
  add(P.t, 3 * sm, "t");
  add(P.mean, sm, "mean");
  add(P.var, sm, "var");
  if (cov) add(P.cov, sc, "cov");
  int64_t on = 0, om = 0, oc = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    const MidPostProb& e = P.pp[q];
    const int nb = mid_blocks((int)shapes[q].n), Mp = nb * MID_TILE;
    CHECK(e.m == m[q] && e.mb == (m[q] + 63) / 64, "m / mb of problem %zu", q);
    add(e.V, (int64_t)64 * e.mb * Mp, "V");  // 64 ceil(m / 64) x Mp
    // the packed inputs and outputs, in problem order as the caller holds them
    CHECK(e.dv == (dv ? P.dv + on : -1), "diag_vec offset of problem %zu", q);
    CHECK(e.t == P.t + 3 * om, "t offset of problem %zu", q);
    CHECK(e.mean == P.mean + om && e.var == P.var + om, "output offsets of problem %zu", q);
    CHECK(e.cov == (cov ? P.cov + oc : -1), "cov offset of problem %zu", q);
    on += shapes[q].n;
    om += m[q];
    oc += m[q] * m[q];
  }
  CHECK(P.table % 16 == 0 && (int64_t)P.table >= P.doubles * 8, "table after the doubles");
  rs.push_back({(int64_t)P.table, (int64_t)(P.table + P.nprob * sizeof(MidPostProb)), "table"});
  std::sort(rs.begin(), rs.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < rs.size(); ++i) {
    CHECK(rs[i].lo >= 0 && rs[i].hi <= (int64_t)P.bytes, "%s outside %zu bytes", rs[i].what,
          P.bytes);
    if (i) CHECK(rs[i - 1].hi <= rs[i].lo, "%s overlaps %s", rs[i - 1].what, rs[i].what);
  }
  // the documented bytes per problem bound the arena
  size_t bound = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    const int64_t Mp = (int64_t)mid_blocks((int)shapes[q].n) * MID_TILE, mb = (m[q] + 63) / 64;
    bound += 8 * (size_t)(64 * mb * Mp + 5 * m[q] + shapes[q].n + 1 + (cov ? m[q] * m[q] : 0)) +
             sizeof(MidPostProb);
  }
  CHECK(P.bytes <= bound + 8 * 8, "%zu bytes, documented %zu", P.bytes, bound);
}

// every unit of every problem has exactly one owner in the launch, by the kernels' mapping
static void check_launch(const MidPostPlan& P, const std::vector<MidShape>& shapes,
                         const MidLaunch& l) {
  CHECK(l.gx == (unsigned)P.nprob && l.gx >= 1, "grid.x %u", l.gx);
  CHECK(l.kind >= 0 && l.kind < MID_KINDS, "launch kind %d", l.kind);
  CHECK(l.gy >= 1 && l.gy <= 65535u, "grid.y %u", l.gy);
  for (size_t q = 0; q < shapes.size(); ++q) {
    const int nb = mid_blocks((int)shapes[q].n), mb = P.pp[q].mb;
    std::map<std::pair<int, int>, int> tiles, units;
    for (unsigned u = 0; u < l.gy; ++u) {
      switch (l.kind) {
        case MID_POST_FILL:
          if ((int)u < P.maxtiles) {
            if ((int)u >= mid_tiles(nb)) break;
            int I, J;
            mid_tile_of((int)u, &I, &J);
            ++tiles[{I, J}];
          } else {
            const int unit = (int)u - P.maxtiles;
            if (unit >= mb * nb) break;
            ++units[{unit / nb, unit % nb}];
          }
          break;
        case MID_COLUMN:
          if (l.k + (int)u < nb) ++tiles[{l.k + (int)u, l.k}];
          break;
        case MID_SOLVE:
          if ((int)u < mb) ++units[{(int)u, 0}];
          break;
        case MID_COV: {
          if ((int)u >= mid_tiles(mb)) break;
          int A, B;
          mid_tile_of((int)u, &A, &B);
          CHECK(0 <= B && B <= A && A < mb, "cov tile %u", u);
          ++units[{A, B}];
          break;
        }
        default:
          CHECK(false, "launch kind %d", l.kind);
      }
    }
    for (const auto& kv : tiles) CHECK(kv.second == 1, "a tile with %d owners", kv.second);
    for (const auto& kv : units) CHECK(kv.second == 1, "a unit with %d owners", kv.second);
    size_t want_t = 0, want_u = 0;
    if (l.kind == MID_POST_FILL) want_t = (size_t)mid_tiles(nb), want_u = (size_t)mb * nb;
    if (l.kind == MID_COLUMN) want_t = l.k < nb ? (size_t)(nb - l.k) : 0;
    if (l.kind == MID_SOLVE) want_u = (size_t)mb;
    if (l.kind == MID_COV) want_u = (size_t)mid_tiles(mb);
    CHECK(tiles.size() == want_t && units.size() == want_u,
          "kind %d k %d: %zu of %zu tiles, %zu of %zu units", l.kind, l.k, tiles.size(), want_t,
          units.size(), want_u);
  }
}

static MidPostPlan check_batch(const std::vector<MidShape>& shapes, const std::vector<int64_t>& m,
                               bool dv, bool cov) {
  const MidPostPlan P = plan_mid_post(shapes, m.data(), dv, cov);
  CHECK(P.reject == MidPostPlan::OK, "rejected: %s", P.why.c_str());
  if (P.reject) return P;
  CHECK(P.nprob == (int64_t)shapes.size() && P.pp.size() == shapes.size(), "problem count");
  int maxnb = 0, maxmb = 0, maxn = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    maxnb = std::max(maxnb, mid_blocks((int)shapes[q].n));
    maxn = std::max(maxn, (int)shapes[q].n);
    maxmb = std::max(maxmb, (int)((m[q] + 63) / 64));
  }
  CHECK(P.maxnb == maxnb && P.maxtiles == mid_tiles(maxnb) && P.maxmb == maxmb &&
            P.maxcov == mid_tiles(maxmb),
        "maxima");
  check_regions(P, shapes, m, dv, cov);
  // ceil((n_max + 1) / 64) + 2 launches, one more with the covariance: the fill, the block
  // columns in order (plan_mid's own column launches), the solve, the covariance
  const int want = (maxn + 1 + 63) / 64 + 2 + (cov ? 1 : 0);
  CHECK((int)P.launches.size() == want, "%zu launches, want %d", P.launches.size(), want);
  CHECK(P.launches.front().kind == MID_POST_FILL, "first launch");
  const MidPlan M = plan_mid(shapes);
  for (int k = 0; k < maxnb; ++k) {
    const MidLaunch &a = P.launches[1 + k], &b = M.value[1 + k];
    CHECK(a.kind == MID_COLUMN && a.k == k && b.kind == MID_COLUMN && a.k == b.k && a.gx == b.gx &&
              a.gy == b.gy,
          "column %d", k);
  }
  CHECK(P.launches[1 + maxnb].kind == MID_SOLVE, "solve launch");
  if (cov) CHECK(P.launches.back().kind == MID_COV, "cov launch");
  for (const MidLaunch& l : P.launches) check_launch(P, shapes, l);
  return P;
}

int main() {
  CHECK(MID_MAX_M == 4096, "MID_MAX_M");
  // rejections, in order: m = 0, m % G != 0, m > MID_MAX_M
  {
    const std::vector<MidShape> s = {{28, 4}, {129, 3}};
    auto rej = [&](std::vector<int64_t> m) { return plan_mid_post(s, m.data(), true, true); };
    CHECK(rej({4, 0}).reject == MidPostPlan::NO_ROWS, "m = 0");
    CHECK(rej({4, -3}).reject == MidPostPlan::NO_ROWS, "m < 0");
    CHECK(rej({4, 130}).reject == MidPostPlan::BAD_M, "m %% G");
    CHECK(rej({4, 4097}).reject == MidPostPlan::BAD_M, "m %% G before the cap");
    CHECK(rej({4, 4095}).reject == MidPostPlan::OK, "m = 4095");
    const MidPostPlan P = rej({4, 4098});
    CHECK(P.reject == MidPostPlan::TOO_MANY_ROWS && P.why.find("4096") != std::string::npos &&
              P.why.find("LFM_MID_MAX_M") != std::string::npos &&
              P.why.find("problem 1") != std::string::npos && P.pp.empty() && P.launches.empty(),
          "m past the cap: %s", P.why.c_str());
    CHECK(rej({0, 4099}).reject == MidPostPlan::NO_ROWS, "the first offending problem");
    CHECK(rej({6, 0}).reject == MidPostPlan::BAD_M, "the first offending problem (2)");
    CHECK(rej({4100, 130}).reject == MidPostPlan::TOO_MANY_ROWS, "the first offending problem (3)");
    CHECK(!rej({4, 130}).why.empty() && !rej({4, 0}).why.empty(), "a rejection has a message");
  }
  long plans = 0;
  const int ns[] = {1, 63, 64, 127, 128, 129, 192, 193, 1023, 1024};
  for (int n : ns)
    for (int G : {1, 3})
      if (n % G == 0)
        for (int64_t m0 : {(int64_t)G, (int64_t)60, (int64_t)64, (int64_t)68, (int64_t)130,
                           (int64_t)4096}) {
          const int64_t m = m0 - m0 % G;
          for (int mode = 0; mode < 4; ++mode) {
            check_batch({{n, G}}, {m}, mode & 1, mode & 2);
            ++plans;
          }
        }
  // mixed batches, both orders, every mode
  std::vector<MidShape> mixed = {{28, 4}, {63, 1}, {64, 1}, {128, 2}, {129, 3}, {192, 3},
                                 {193, 1}, {320, 5}, {1024, 4}, {1, 1}};
  std::vector<int64_t> ms = {20, 130, 64, 68, 129, 66, 68, 130, 4096, 1};
  for (int rev = 0; rev < 2; ++rev) {
    for (int mode = 0; mode < 4; ++mode) {
      check_batch(mixed, ms, mode & 1, mode & 2);
      ++plans;
    }
    std::reverse(mixed.begin(), mixed.end());
    std::reverse(ms.begin(), ms.end());
  }
  // the launch count is a function of the largest n alone, whatever the count and the m's
  for (int n : {1, 64, 320, 1024}) {
    const MidPostPlan one = check_batch({{n, 1}}, {1}, true, true);
    const MidPostPlan many = check_batch(std::vector<MidShape>(100, MidShape{n, 1}),
                                         std::vector<int64_t>(100, 130), true, true);
    CHECK(one.launches.size() == many.launches.size(), "launch count of 100 copies of n = %d", n);
    plans += 2;
  }
  if (failures) {
    std::printf("mid_post_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("mid_post_plan_check: all passed (%ld plans)\n", plans);
  return 0;
}
