// mid_draw_plan_check.cpp — plan_mid_draw (dis_project_amd/csrc/lfm_host.cpp), the fourth arena,
// the second problem table and the launch list of lfm_mbatch_predictive_f64 (lfm_mbatch.hip issues
// exactly what it says), under AddressSanitizer + UBSan: built and run by
// tests/test_mid_draw_host.py with the flags of tests/test_sample_host.py. Over n in {1, 64, 129,
// 1024}, m in {G, 63, 64, 65, 128, 129, 130, 320, 1023, 1024}, nsamp in {0, 1, 3, 64, 65, 130,
// 65536}, with and without ystar, and mixed batches:
//   every region is inside the arena, disjoint from the others and 16-byte aligned; the arena is
//   the sum of the documented bytes per problem plus < 64 bytes of rounding; the second table
//   describes the m x m covariance as plan_mid describes an n x n problem; the packed samples are
//   the caller's layout; in every launch every unit has exactly one owner, by the kernels' own
//   unit mapping, and every pair of normals one generating thread; the launch list has the stated
//   length; the rejections come in the documented order with the limit in the message.
#include <algorithm>
#include <climits>
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

static void check_regions(const MidDrawPlan& P, const std::vector<MidShape>& shapes,
                          const std::vector<int64_t>& m, bool ys, int64_t nsamp) {
  std::vector<Region> rs;
  auto add = [&](int64_t lo_d, int64_t count_d, const char* what) {
    CHECK(lo_d >= 0 && lo_d % 2 == 0, "%s not 16-byte aligned", what);
    rs.push_back({lo_d * 8, (lo_d + count_d) * 8, what});
  };
  int64_t sm = 0;
  for (int64_t v : m) sm += v;
  CHECK(P.sm == sm && P.nsamp == nsamp, "sums");
  add(P.cadd, P.nprob, "cov_add");
  add(P.out, P.nprob, "logp");
  CHECK((P.ystar >= 0) == ys && (P.X >= 0) == (nsamp > 0), "optional regions");
  if (ys) add(P.ystar, sm, "ystar");
  if (nsamp > 0) add(P.X, nsamp * sm, "samples");
  const int64_t sb = (nsamp + 63) / 64;
  int64_t om = 0, oc = 0;
  size_t documented = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    const MidProb& e = P.probs[q];
    const MidDrawProb& d = P.dp[q];
    // the covariance as an augmented problem of its own: plan_mid's shape at n = m
    const int nq = mid_blocks((int)m[q]), Mq = nq * MID_TILE;
    CHECK(e.n == m[q] && e.G == shapes[q].G && e.nb == nq && e.Mp == Mq &&
              Mq == 64 * (int)((m[q] + 1 + 63) / 64),
          "table entry of problem %zu", q);
    CHECK(d.m == m[q] && d.cb == (m[q] + 63) / 64 && d.sb == sb, "draw entry of problem %zu", q);
    add(e.S, (int64_t)Mq * Mq, "A");
    add(e.L, (int64_t)Mq * Mq, "L");
    add(e.dinv, (int64_t)nq * 64 * 64, "dinv");
    // the product reads rows [0, 64 cb) of L and columns [0, 64 cb) of Z
    CHECK(64 * d.cb <= Mq, "the factor's rows cover the product's of problem %zu", q);
    CHECK(d.cov == oc && d.mean == om, "posterior offsets of problem %zu", q);
    CHECK(d.ystar == (ys ? P.ystar + om : -1), "ystar offset of problem %zu", q);
    if (nsamp > 0) {
      add(d.Z, (int64_t)64 * sb * 64 * d.cb, "Z");
      CHECK(d.X == P.X + nsamp * om, "samples offset of problem %zu", q);
    } else {
      CHECK(d.Z == -1 && d.X == -1, "no samples: no Z / X");
    }
    om += m[q];
    oc += m[q] * m[q];
    documented += mid_draw_problem_bytes(m[q], ys, nsamp);
    // the formula of the header, written out
    const size_t f = 8 * (size_t)(2 * (int64_t)Mq * Mq + 4096 * nq + 2) + 152 +
                     (ys ? 8 * (size_t)m[q] : 0) +
                     (nsamp > 0 ? 8 * (size_t)(4096 * sb * d.cb + nsamp * m[q]) : 0);
    CHECK(mid_draw_problem_bytes(m[q], ys, nsamp) == f, "byte formula of problem %zu", q);
  }
  CHECK(sizeof(uint64_t) + sizeof(MidProb) + sizeof(MidDrawProb) == 152, "table bytes");
  CHECK(P.seeds % 16 == 0 && (int64_t)P.seeds >= P.doubles * 8, "seeds after the doubles");
  CHECK(P.table % 16 == 0 && P.dtable % 16 == 0, "tables aligned");
  rs.push_back({(int64_t)P.seeds, (int64_t)(P.seeds + P.nprob * 8), "seeds"});
  rs.push_back({(int64_t)P.table, (int64_t)(P.table + P.nprob * sizeof(MidProb)), "table"});
  rs.push_back({(int64_t)P.dtable, (int64_t)(P.dtable + P.nprob * sizeof(MidDrawProb)), "dtable"});
  std::sort(rs.begin(), rs.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < rs.size(); ++i) {
    CHECK(rs[i].lo >= 0 && rs[i].hi <= (int64_t)P.bytes, "%s outside %zu bytes", rs[i].what,
          P.bytes);
    if (i) CHECK(rs[i - 1].hi <= rs[i].lo, "%s overlaps %s", rs[i - 1].what, rs[i].what);
  }
  CHECK(P.bytes >= documented && P.bytes < documented + 64, "%zu bytes, documented %zu", P.bytes,
        documented);
}

// every unit of every problem has exactly one owner in the launch, by the kernels' mapping
static void check_launch(const MidDrawPlan& P, const MidLaunch& l, bool enumerate_pairs) {
  CHECK(l.gx == (unsigned)P.nprob && l.gx >= 1, "grid.x %u", l.gx);
  CHECK(l.kind >= 0 && l.kind < MID_KINDS, "launch kind %d", l.kind);
  CHECK(l.gy >= 1 && l.gy <= 65535u, "grid.y %u", l.gy);
  for (size_t q = 0; q < P.probs.size(); ++q) {
    const int nq = P.probs[q].nb, cb = P.dp[q].cb, sb = P.dp[q].sb;
    std::map<std::pair<int, int>, int> units;
    size_t want = 0;
    switch (l.kind) {
      case MID_DRAW_SCALE:
        for (unsigned u = 0; u < l.gy; ++u) {
          if ((int)u >= mid_tiles(nq)) continue;
          int I, J;
          mid_tile_of((int)u, &I, &J);
          CHECK(0 <= J && J <= I && I < nq, "scale tile %u", u);
          ++units[{I, J}];
        }
        want = (size_t)mid_tiles(nq);
        break;
      case MID_COLUMN:
        for (unsigned u = 0; u < l.gy; ++u)
          if (l.k + (int)u < nq) ++units[{l.k + (int)u, l.k}];
        want = l.k < nq ? (size_t)(nq - l.k) : 0;
        break;
      case MID_VALUE:
        CHECK(l.gy == 1, "value grid");
        ++units[{0, 0}];
        want = 1;
        break;
      case MID_DRAW_RANDN: {
        // thread (u, tid) takes the pairs u 256 + tid + i gy 256: every pair exactly once
        const int64_t pairs = (int64_t)64 * sb * 32 * cb, stride = (int64_t)l.gy * 256;
        // one pass over the largest problem's pairs, up to the grid-stride cap
        CHECK(l.gy == (unsigned)std::min<int64_t>((int64_t)8 * P.maxsb * P.maxcb,
                                                  MID_DRAW_RANDN_GY),
              "randn grid %u", l.gy);
        if (enumerate_pairs) {
          std::vector<unsigned char> seen((size_t)pairs, 0);
          for (int64_t first = 0; first < stride; ++first)
            for (int64_t p = first; p < pairs; p += stride) ++seen[(size_t)p];
          for (int64_t p = 0; p < pairs; ++p) CHECK(seen[(size_t)p] == 1, "pair %lld", (long long)p);
        }
        continue;
      }
      case MID_DRAW_PRODUCT:
        for (unsigned u = 0; u < l.gy; ++u) {
          const int sblk = (int)u / P.maxcb, c = (int)u - sblk * P.maxcb;
          if (c >= cb) continue;
          const int tj = cb - 1 - c;
          CHECK(sblk < sb && tj >= 0 && tj < cb, "product unit %u", u);
          ++units[{sblk, tj}];
        }
        want = (size_t)sb * cb;
        break;
      default:
        CHECK(false, "launch kind %d", l.kind);
    }
    for (const auto& kv : units) CHECK(kv.second == 1, "a unit with %d owners", kv.second);
    CHECK(units.size() == want, "kind %d k %d: %zu of %zu units", l.kind, l.k, units.size(), want);
  }
}

static void check_batch(const std::vector<MidShape>& shapes, const std::vector<int64_t>& m,
                        bool ys, int64_t nsamp, int64_t sample0) {
  const MidDrawPlan P = plan_mid_draw(shapes, m.data(), true, ys, nsamp, sample0);
  CHECK(P.reject == MidDrawPlan::OK, "rejected: %s", P.why.c_str());
  if (P.reject) return;
  CHECK(P.nprob == (int64_t)shapes.size() && P.probs.size() == shapes.size() &&
            P.dp.size() == shapes.size() && P.sample0 == sample0,
        "problem count");
  int maxnq = 0, maxcb = 0, maxm = 0;
  for (int64_t v : m) {
    maxnq = std::max(maxnq, mid_blocks((int)v));
    maxcb = std::max(maxcb, (int)((v + 63) / 64));
    maxm = std::max(maxm, (int)v);
  }
  CHECK(P.maxnq == maxnq && P.maxtiles == mid_tiles(maxnq) && P.maxcb == maxcb &&
            P.maxsb == (nsamp + 63) / 64,
        "maxima");
  check_regions(P, shapes, m, ys, nsamp);
  // 1 + ceil((m_max + 1) / 64) + (ystar ? 1 : 0) + (nsamp ? 2 : 0) launches after the
  // posterior's ceil((n_max + 1) / 64) + 3
  const size_t want = 1 + (size_t)((maxm + 1 + 63) / 64) + (ys ? 1 : 0) + (nsamp > 0 ? 2 : 0);
  CHECK(P.launches.size() == want, "%zu launches, want %zu", P.launches.size(), want);
  size_t at = 0;
  CHECK(P.launches[at++].kind == MID_DRAW_SCALE, "first launch");
  // the column launches are plan_mid's for problems of n = m
  std::vector<MidShape> as_n;
  for (size_t q = 0; q < shapes.size(); ++q) as_n.push_back({m[q], shapes[q].G});
  const MidPlan M = plan_mid(as_n);
  CHECK(M.reject == MidPlan::OK && M.maxnb == maxnq, "plan_mid at n = m");
  for (int k = 0; k < maxnq; ++k, ++at) {
    const MidLaunch &a = P.launches[at], &b = M.value[1 + k];
    CHECK(a.kind == MID_COLUMN && a.k == k && b.kind == MID_COLUMN && b.k == k && a.gx == b.gx &&
              a.gy == b.gy,
          "column %d", k);
  }
  if (ys) CHECK(P.launches[at++].kind == MID_VALUE, "value launch");
  if (nsamp > 0) {
    CHECK(P.launches[at++].kind == MID_DRAW_RANDN, "randn launch");
    CHECK(P.launches[at++].kind == MID_DRAW_PRODUCT, "product launch");
  }
  CHECK(at == P.launches.size(), "launch order");
  for (const MidLaunch& l : P.launches) check_launch(P, l, nsamp <= 130);
  // with the posterior's launches the call's count is the header's
  const std::vector<int64_t> mm(m);
  const MidPostPlan Q = plan_mid_post(shapes, mm.data(), true, true);
  int maxn = 0;
  for (const MidShape& s : shapes) maxn = std::max(maxn, (int)s.n);
  CHECK(Q.reject == MidPostPlan::OK &&
            Q.launches.size() + P.launches.size() ==
                (size_t)((maxn + 1 + 63) / 64 + (maxm + 1 + 63) / 64 + 4 + (ys ? 1 : 0) +
                         (nsamp > 0 ? 2 : 0)),
        "the call's launch count");
}

int main() {
  CHECK(MID_DRAW_MAX_NSAMP == 65536 && MID_MAX_N == 1024, "limits");
  // rejections, in the documented order
  {
    const std::vector<MidShape> s = {{28, 4}, {129, 3}};
    auto rej = [&](std::vector<int64_t> m, bool ca, bool ys, int64_t ns, int64_t s0) {
      return plan_mid_draw(s, m.data(), ca, ys, ns, s0);
    };
    auto has = [](const MidDrawPlan& P, const char* w) {
      return P.why.find(w) != std::string::npos &&
             P.why.find("lfm_mbatch_predictive_f64") != std::string::npos && P.probs.empty() &&
             P.launches.empty();
    };
    MidDrawPlan P = rej({4, 0}, false, false, -1, -1);
    CHECK(P.reject == MidDrawPlan::NO_COV_ADD && has(P, "cov_add"), "cov_add first");
    P = rej({4, 0}, true, false, -1, -1);
    CHECK(P.reject == MidDrawPlan::BAD_NSAMP && has(P, "nsamp"), "nsamp < 0");
    P = rej({4, 0}, true, false, 0, -1);
    CHECK(P.reject == MidDrawPlan::NOTHING && has(P, "nothing"), "nothing asked for");
    P = rej({4, 0}, true, true, 65537, -1);
    CHECK(P.reject == MidDrawPlan::TOO_MANY && has(P, "65536") && has(P, "sample0"), "nsamp cap");
    P = rej({4, 0}, true, true, 65536, -1);
    CHECK(P.reject == MidDrawPlan::BAD_SAMPLE0 && has(P, "sample0"), "sample0 < 0");
    P = rej({4, 0}, true, true, 2, INT64_MAX - 1);
    CHECK(P.reject == MidDrawPlan::RANGE && has(P, "overflows"), "sample0 + nsamp");
    CHECK(rej({4, 3}, true, true, 2, INT64_MAX - 2).reject == MidDrawPlan::OK, "the last sample");
    P = rej({4, 0}, true, true, 0, 0);
    CHECK(P.reject == MidDrawPlan::NO_ROWS && has(P, "problem 1") && has(P, "m >= 1"), "m = 0");
    CHECK(rej({4, -3}, true, true, 0, 0).reject == MidDrawPlan::NO_ROWS, "m < 0");
    P = rej({4, 130}, true, false, 1, 0);
    CHECK(P.reject == MidDrawPlan::BAD_M && has(P, "multiple"), "m %% G");
    CHECK(rej({4, 1025}, true, true, 0, 0).reject == MidDrawPlan::BAD_M, "m %% G before the cap");
    CHECK(rej({4, 1023}, true, true, 0, 0).reject == MidDrawPlan::OK, "m = 1023");
    P = rej({4, 1026}, true, true, 0, 0);
    CHECK(P.reject == MidDrawPlan::TOO_MANY_ROWS && has(P, "1024") && has(P, "LFM_MID_MAX_N") &&
              has(P, "problem 1") && has(P, "lfm_post_"),
          "m past the cap: %s", P.why.c_str());
    CHECK(rej({0, 1026}, true, true, 0, 0).reject == MidDrawPlan::NO_ROWS, "the first offender");
    CHECK(rej({6, 0}, true, true, 0, 0).reject == MidDrawPlan::BAD_M, "the first offender (2)");
    CHECK(rej({1028, 130}, true, true, 0, 0).reject == MidDrawPlan::TOO_MANY_ROWS,
          "the first offender (3)");
  }
  long plans = 0;
  const int ns[] = {1, 64, 129, 1024};
  const int ms[] = {0, 63, 64, 65, 128, 129, 130, 320, 1023, 1024};  // 0: m = G
  const int64_t nsamps[] = {0, 1, 3, 64, 65, 130, 65536};
  for (int n : ns)
    for (int mi : ms)
      for (int64_t nsamp : nsamps)
        for (int ys = 0; ys < 2; ++ys) {
          if (!ys && nsamp == 0) continue;
          const int64_t G = 1, m = mi ? mi : G;
          check_batch({{n, G}}, {m}, ys != 0, nsamp, nsamp % 2 ? 2 : 0);
          ++plans;
        }
  // mixed batches: the grids follow the largest m, every problem's units have one owner
  {
    const std::vector<MidShape> s = {{28, 4}, {63, 1}, {64, 1}, {64, 1}, {128, 2}, {129, 3},
                                     {320, 5}, {320, 5}, {1024, 4}};
    const std::vector<int64_t> m = {20, 63, 64, 65, 128, 129, 130, 320, 1024};
    for (int64_t nsamp : {0, 1, 65, 130, 1024})
      for (int ys = 0; ys < 2; ++ys) {
        if (!ys && nsamp == 0) continue;
        check_batch(s, m, ys != 0, nsamp, 7);
        std::vector<MidShape> r(s.rbegin(), s.rend());
        std::vector<int64_t> rm(m.rbegin(), m.rend());
        check_batch(r, rm, ys != 0, nsamp, 7);
        plans += 2;
      }
    // a problem's regions' sizes do not depend on its neighbours
    const MidDrawPlan A = plan_mid_draw(s, m.data(), true, true, 65, 0);
    const MidDrawPlan B = plan_mid_draw({s[5]}, &m[5], true, true, 65, 0);
    CHECK(A.probs[5].L - A.probs[5].S == B.probs[0].L - B.probs[0].S &&
              A.dp[5].Z - A.probs[5].S == B.dp[0].Z - B.probs[0].S && A.dp[5].sb == B.dp[0].sb,
          "a problem's layout alone and in a batch");
  }
  std::printf("mid_draw_plan_check: %ld plans, %d failures\n", plans, failures);
  if (failures == 0) std::printf("mid_draw_plan_check: all passed\n");
  return failures ? 1 : 0;
}
