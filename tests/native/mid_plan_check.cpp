// mid_plan_check.cpp — plan_mid (dis_project_amd/csrc/lfm_host.cpp), the arena layout and launch
// plan of the mid-size resident batch (lfm_mbatch.hip issues exactly what it says), under
// AddressSanitizer + UBSan: built and run by tests/test_mid_host.py with the flags of
// tests/native/Makefile. Over an empty batch, n = 1, 63 / 64 / 65, 1024, every n in a sweep and
// mixed batches:
//   every problem's regions are disjoint, aligned and inside the reported bytes (the call
//   buffers, the status words and the table included); in every launch every lower tile the
//   launch's kind covers has exactly one owner, by the kernels' own unit -> tile mapping; the
//   launch count is a function of the largest n alone; grids are within HIP's limits; the
//   rejections come in the documented order with the limit in the message.
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

static void check_regions(const MidPlan& P) {
  std::vector<Region> rs;
  auto add = [&](int64_t lo_d, int64_t count_d, const char* what) {
    CHECK(lo_d % 2 == 0, "%s not 16-byte aligned", what);
    rs.push_back({lo_d * 8, (lo_d + count_d) * 8, what});
  };
  add(P.hyp, P.nhyp, "hyp");
  add(P.out, P.nprob, "out");
  add(P.grad, P.nhyp, "grad");
  int64_t hv = 0, hs = P.nhyp - 3 * P.nprob;
  for (const MidProb& m : P.probs) {
    CHECK(m.nb == (m.n + 1 + 63) / 64 && m.Mp == 64 * m.nb && m.Mp >= m.n + 1, "padding of n %d",
          m.n);
    CHECK(m.hv == hv && m.hs == hs, "packed offsets of n %d", m.n);
    hv += 3 * m.G;
    hs += 3;
    const int64_t mat = (int64_t)m.Mp * m.Mp;
    add(m.x, 3 * (int64_t)m.n, "x");
    add(m.y, m.n, "y");
    add(m.S, mat, "S");
    add(m.L, mat, "L");
    add(m.W, mat, "W");
    add(m.dinv, (int64_t)m.nb * 64 * 64, "dinv");
    add(m.part, (int64_t)mid_tiles(m.nb) * MID_PART, "part");
    CHECK(m.y == m.x + (3 * (int64_t)m.n + 1) / 2 * 2 && m.S == m.y + ((int64_t)m.n + 1) / 2 * 2,
          "x, y and S adjacent (one upload)");
    CHECK(m.part + (int64_t)mid_tiles(m.nb) * MID_PART - m.x <= mid_problem_doubles(m.n),
          "mid_problem_doubles(%d)", m.n);
  }
  CHECK(hv == P.nhyp - 3 * P.nprob && hs == P.nhyp, "nhyp");
  CHECK(P.status % 16 == 0 && P.table % 16 == 0, "status / table alignment");
  rs.push_back({(int64_t)P.status, (int64_t)(P.status + P.nprob * sizeof(int)), "status"});
  rs.push_back({(int64_t)P.table, (int64_t)(P.table + P.nprob * sizeof(MidProb)), "table"});
  std::sort(rs.begin(), rs.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < rs.size(); ++i) {
    CHECK(rs[i].lo >= 0 && rs[i].hi <= (int64_t)P.bytes, "%s outside %zu bytes", rs[i].what,
          P.bytes);
    if (i) CHECK(rs[i - 1].hi <= rs[i].lo, "%s overlaps %s", rs[i - 1].what, rs[i].what);
  }
  CHECK((int64_t)P.status >= P.doubles * 8, "status inside the doubles");
}

// owners[(I, J)] of problem m in launch l, by the kernels' unit -> tile mapping
static void check_launch(const MidPlan& P, const MidLaunch& l) {
  CHECK(l.gx == (unsigned)P.nprob && l.gx >= 1 && l.gx <= 2147483647u, "grid.x %u", l.gx);
  CHECK(l.kind >= 0 && l.kind < MID_KINDS, "launch kind %d", l.kind);
  CHECK(l.gy >= 1 && l.gy <= 65535u, "grid.y %u", l.gy);
  CHECK((uint64_t)l.gx * 256 < ((uint64_t)1 << 32), "threads along x");
  for (const MidProb& m : P.probs) {
    std::map<std::pair<int, int>, int> owners;
    int singles = 0;
    for (unsigned u = 0; u < l.gy; ++u) {
      switch (l.kind) {
        case MID_FILL:
        case MID_SINV:
        case MID_PAIRS: {
          if ((int)u >= mid_tiles(m.nb)) break;
          int I, J;
          mid_tile_of((int)u, &I, &J);
          CHECK(0 <= J && J <= I && I < m.nb && mid_tile_index(I, J) == (int)u, "tile %u", u);
          ++owners[{I, J}];
          break;
        }
        case MID_COLUMN:
          if (l.k + (int)u < m.nb) ++owners[{l.k + (int)u, l.k}];
          break;
        case MID_INVERT:
          for (int i = (int)u; i < m.nb; ++i) ++owners[{i, (int)u}];
          break;
        default:
          if (u == 0) ++singles;
      }
    }
    for (const auto& kv : owners) CHECK(kv.second == 1, "a tile with %d owners", kv.second);
    size_t want = 0;
    if (l.kind == MID_FILL || l.kind == MID_SINV || l.kind == MID_PAIRS || l.kind == MID_INVERT)
      want = (size_t)mid_tiles(m.nb);
    else if (l.kind == MID_COLUMN)
      want = l.k < m.nb ? (size_t)(m.nb - l.k) : 0;
    CHECK(owners.size() == want, "kind %d k %d: %zu of %zu tiles owned (nb %d)", l.kind, l.k,
          owners.size(), want, m.nb);
    if (l.kind == MID_VALUE || l.kind == MID_GRAD) CHECK(singles == 1, "finish launch");
  }
}

static MidPlan check_batch(const std::vector<MidShape>& shapes) {
  const MidPlan P = plan_mid(shapes);
  CHECK(P.reject == MidPlan::OK, "rejected: %s", P.why.c_str());
  if (P.reject) return P;
  CHECK(P.nprob == (int64_t)shapes.size() && P.probs.size() == shapes.size(), "problem count");
  int maxnb = 0;
  for (size_t q = 0; q < shapes.size(); ++q) {
    CHECK(P.probs[q].n == shapes[q].n && P.probs[q].G == shapes[q].G, "shape %zu", q);
    maxnb = std::max(maxnb, P.probs[q].nb);
  }
  CHECK(P.maxnb == maxnb && P.maxtiles == mid_tiles(maxnb), "maxnb");
  check_regions(P);
  // the launches: fill, one per block column in order, value; the gradient call continues them
  CHECK((int)P.value.size() == maxnb + 2 && (int)P.value_grad.size() == maxnb + 6, "launch count");
  CHECK(P.value.front().kind == MID_FILL && P.value.back().kind == MID_VALUE, "value ends");
  for (int k = 0; k < maxnb; ++k)
    CHECK(P.value[1 + k].kind == MID_COLUMN && P.value[1 + k].k == k, "column %d", k);
  for (size_t i = 0; i < P.value.size(); ++i)
    CHECK(P.value[i].kind == P.value_grad[i].kind && P.value[i].k == P.value_grad[i].k &&
              P.value[i].gx == P.value_grad[i].gx && P.value[i].gy == P.value_grad[i].gy,
          "the gradient call starts with the value call's launches");
  const int tail[4] = {MID_INVERT, MID_SINV, MID_PAIRS, MID_GRAD};
  for (int i = 0; i < 4; ++i)
    CHECK(P.value_grad[P.value.size() + i].kind == tail[i], "gradient launch %d", i);
  for (const MidLaunch& l : P.value_grad) check_launch(P, l);
  return P;
}

int main() {
  // the tile enumeration
  for (int t = 0, I = 0, J = 0; t < mid_tiles(17); ++t) {
    int i, j;
    mid_tile_of(t, &i, &j);
    CHECK(i == I && j == J, "tile %d -> (%d, %d), want (%d, %d)", t, i, j, I, J);
    if (++J > I) {
      ++I;
      J = 0;
    }
  }
  // rejections, in order
  CHECK(plan_mid({}).reject == MidPlan::EMPTY && plan_mid({}).value.empty(), "empty batch");
  CHECK(plan_mid({{0, 1}}).reject == MidPlan::BAD_N, "n = 0");
  {
    const MidPlan P = plan_mid({{28, 4}, {1025, 1}});
    CHECK(P.reject == MidPlan::BAD_N && P.why.find("1024") != std::string::npos &&
              P.why.find("1025") != std::string::npos && P.probs.empty() && P.value.empty(),
          "n = 1025: %s", P.why.c_str());
  }
  CHECK(plan_mid({{1025, 7}}).reject == MidPlan::BAD_N, "bad n before bad G");
  CHECK(plan_mid({{129, 2}}).reject == MidPlan::BAD_G, "n %% G");
  CHECK(plan_mid({{12, 0}}).reject == MidPlan::BAD_G, "G = 0");
  CHECK(plan_mid({{12, 24}}).reject == MidPlan::BAD_G, "G > n");
  CHECK(!plan_mid({{129, 2}}).why.empty(), "a rejection has a message");
  CHECK(plan_mid(std::vector<MidShape>((size_t)MID_MAX_PROBS + 1, MidShape{1, 1})).reject ==
            MidPlan::TOO_MANY,
        "too many problems");
  // single problems at the edges and over a sweep
  long plans = 0;
  for (int n : {1, 2, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1023, 1024}) {
    check_batch({{n, 1}});
    ++plans;
  }
  for (int n = 1; n <= 1024; n += 13)
    for (int G : {1, 2, 3, 5})
      if (n % G == 0) {
        check_batch({{n, G}});
        ++plans;
      }
  // mixed batches, both orders
  std::vector<MidShape> mixed = {{28, 4}, {63, 1}, {128, 2}, {129, 3}, {192, 3},
                                 {193, 1}, {256, 4}, {257, 1}, {320, 5}, {1024, 8}, {1, 1}};
  check_batch(mixed);
  std::reverse(mixed.begin(), mixed.end());
  check_batch(mixed);
  plans += 2;
  // the launch count is a function of the largest n alone: 1 and 1000 copies, and company
  for (int n : {1, 64, 320, 1024}) {
    const MidPlan one = check_batch({{n, 1}});
    const MidPlan many = check_batch(std::vector<MidShape>(1000, MidShape{n, 1}));
    std::vector<MidShape> with_small(10, MidShape{7, 7});
    with_small.push_back({n, 1});
    const MidPlan mix = check_batch(with_small);
    CHECK(one.value.size() == many.value.size() && one.value_grad.size() == many.value_grad.size(),
          "launch count of 1000 copies of n = %d", n);
    if (n >= 7)
      CHECK(one.value.size() == mix.value.size() && one.value_grad.size() == mix.value_grad.size(),
            "launch count beside smaller problems, n = %d", n);
    CHECK(many.bytes >= 1000 * (size_t)mid_problem_doubles(n) * 8, "bytes of 1000 copies");
    plans += 3;
  }
  if (failures) {
    std::printf("mid_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("mid_plan_check: all passed (%ld plans)\n", plans);
  return 0;
}
