// post_plan_check.cpp — plan_post (dis_project_amd/csrc/lfm_host.cpp), the launch plan of the
// resident posterior's predicts (lfm_post_api.hip issues exactly what it says), under
// AddressSanitizer + UBSan: built and run by tests/test_post_host.py with the flags of
// tests/native/Makefile. Over n in {1 .. 1400 step 37, 16384}, three gene counts, a range of m,
// chunk in {128, 256, default} and the covariance on / off:
//   the chunks cover every test row exactly once, in order; the super-panels cover [0, Np)
//   exactly once; every update grid equals the tile count by enumeration; the workspace sizes
//   bound every offset the launches use; the rejections come in the documented order.
#include <cstdio>
#include <cstdlib>
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

static int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

static void check_plan(int64_t n, int64_t G, int64_t m, int64_t chunk, bool cov) {
  const ResidentPlan P = plan_post(n, G, m, chunk, cov);
  const int64_t Np = up(n, 128);
  const int64_t eff = chunk ? chunk : post_default_chunk(Np);
  if (cov && m > eff) {
    CHECK(P.reject == ResidentPlan::COV_CHUNK && !P.why.empty() &&
              P.why.find(std::to_string(eff)) != std::string::npos,
          "cov above the chunk: n %ld m %ld chunk %ld -> %d", (long)n, (long)m, (long)chunk,
          P.reject);
    CHECK(P.chunks.empty() && P.panels.empty(), "a rejected plan lists launches");
    return;
  }
  CHECK(P.reject == ResidentPlan::OK, "n %ld m %ld chunk %ld cov %d rejected: %d", (long)n,
        (long)m, (long)chunk, (int)cov, P.reject);
  if (P.reject) return;
  CHECK(P.n == n && P.Np == Np && P.m == m && P.chunk == eff, "header");
  // the chunks: every test row exactly once, in order
  int64_t next = 0, max_pad = 0;
  for (const PostChunk& c : P.chunks) {
    CHECK(c.q0 == next && c.rows >= 1 && c.rows <= eff, "chunk at %ld rows %ld", (long)c.q0,
          (long)c.rows);
    CHECK(c.pad_rows == up(c.rows, 128) && c.tiles * 128 == c.pad_rows, "chunk padding");
    CHECK((int64_t)c.panel_grid * 64 >= c.rows && (int64_t)c.panel_grid * 64 < c.rows + 64 &&
              (int64_t)c.panel_grid * 64 <= c.pad_rows,
          "panel grid %d for %ld rows", c.panel_grid, (long)c.rows);
    next += c.rows;
    max_pad = max_pad > c.pad_rows ? max_pad : c.pad_rows;
  }
  CHECK(next == m, "chunks cover %ld of %ld rows", (long)next, (long)m);
  CHECK(P.vt_rows == max_pad, "vt_rows");
  if (cov) CHECK(P.chunks.size() == 1, "the covariance needs one chunk");
  // the super-panels: [0, Np) exactly once
  int64_t col = 0;
  for (const PostPanel& s : P.panels) {
    CHECK(s.K0 == col && s.w >= 1 && s.w <= POST_W && s.K1 == s.K0 + 128 * (int64_t)s.w,
          "super-panel at %ld", (long)s.K0);
    CHECK(s.tj0 == s.K1 / 128 && s.ntj == (Np - s.K1) / 128 && s.ntj >= 0, "update columns");
    col = s.K1;
  }
  CHECK(col == Np, "super-panels cover %ld of %ld columns", (long)col, (long)Np);
  // every update grid = the tiles to the right of the super-panel, by enumeration; and the
  // largest offsets the launches reach
  const size_t vt_doubles = P.vt_bytes / sizeof(double), acc_doubles = P.acc_bytes / sizeof(double);
  CHECK(vt_doubles == (size_t)P.vt_rows * Np && acc_doubles == 2 * (size_t)P.vt_rows, "sizes");
  for (const PostChunk& c : P.chunks) {
    for (const PostPanel& s : P.panels) {
      int64_t tiles = 0;
      size_t reach = 0;
      for (int64_t ti = 0; ti * 128 < c.rows; ++ti)
        for (int64_t tj = 0; tj * 128 < Np; ++tj) {
          if (tj * 128 < s.K1) continue;
          ++tiles;
          const size_t last = (size_t)(ti * 128 + 127) * Np + (size_t)tj * 128 + 127;
          reach = reach > last ? reach : last;
        }
      CHECK(tiles == (int64_t)c.tiles * s.ntj, "update grid %d x %d, %ld tiles", c.tiles, s.ntj,
            (long)tiles);
      CHECK(tiles == 0 || reach < vt_doubles, "update reaches %zu of %zu", reach, vt_doubles);
      // the panel launch: rows [0, 64 panel_grid), columns [K0, K1); its accumulator slots
      const size_t prow = (size_t)c.panel_grid * 64 - 1;
      CHECK(prow * Np + (size_t)s.K1 - 1 < vt_doubles, "panel reaches past Vt");
      CHECK(prow < (size_t)P.vt_rows && (size_t)P.vt_rows + prow < acc_doubles, "accumulators");
    }
    CHECK((size_t)(c.q0 + c.rows) * 3 * sizeof(double) <= P.t_bytes, "test inputs");
    CHECK((size_t)(m + c.q0 + c.rows) * sizeof(double) <= P.out_bytes, "mean / var");
  }
  if (cov) {
    CHECK(P.cov_bytes == (size_t)m * m * sizeof(double), "cov bytes");
    CHECK((int64_t)P.cov_tiles * 128 >= m && (int64_t)P.cov_tiles * 128 < m + 128, "cov tiles");
    CHECK((int64_t)P.cov_tiles * 128 <= P.vt_rows, "the covariance reads Vt rows past its end");
  } else {
    CHECK(P.cov_bytes == 0 && P.cov_tiles == 0, "nothing m x m without the covariance");
  }
}

static void check_rejections() {
  auto code = [](int64_t n, int64_t G, int64_t m, int64_t chunk, bool cov) {
    return plan_post(n, G, m, chunk, cov).reject;
  };
  // bad m first, whatever else is wrong
  CHECK(code(129, 3, 0, 100, true) == ResidentPlan::BAD_M, "m = 0");
  CHECK(code(129, 3, -3, 0, false) == ResidentPlan::BAD_M, "m < 0");
  CHECK(code(129, 3, 128, 100, true) == ResidentPlan::BAD_M, "m % G");
  // then the covariance above the chunk, before the chunk's own shape
  CHECK(code(129, 3, 129, 100, true) == ResidentPlan::COV_CHUNK, "cov above a bad chunk");
  CHECK(code(129, 3, 129, 128, true) == ResidentPlan::COV_CHUNK, "cov above the chunk");
  CHECK(code(129, 3, 129, 256, true) == ResidentPlan::OK, "cov within the chunk");
  // then the chunk
  CHECK(code(129, 3, 99, 100, true) == ResidentPlan::BAD_CHUNK, "chunk 100 with cov");
  CHECK(code(129, 3, 129, 100, false) == ResidentPlan::BAD_CHUNK, "chunk 100");
  CHECK(code(129, 3, 129, -128, false) == ResidentPlan::BAD_CHUNK, "chunk < 0");
  CHECK(!plan_post(129, 3, 129, 100, false).why.empty(), "a rejection has a message");
}

int main() {
  for (int64_t Np = 128; Np <= 262144; Np *= 2) {
    const int64_t c = post_default_chunk(Np);
    CHECK(c >= 128 && c % 128 == 0 && c <= POST_CHUNK_MAX, "default chunk %ld", (long)c);
    CHECK(c == 128 || (size_t)c * Np * sizeof(double) <= POST_VT_BUDGET, "default over budget");
    CHECK(c == POST_CHUNK_MAX || (size_t)(c + 128) * Np * sizeof(double) > POST_VT_BUDGET,
          "default chunk not maximal");
  }
  std::vector<int64_t> ns;
  for (int64_t n = 1; n <= 1400; n += 37) ns.push_back(n);
  ns.push_back(16384);
  long plans = 0;
  for (int64_t n : ns)
    for (int64_t G : {1, 3, 4})
      for (int64_t k : {1, 2, 32, 43, 64, 100, 129, 1367, 21846})
        for (int64_t chunk : {128, 256, 0})
          for (bool cov : {false, true}) {
            check_plan(n, G, k * G, chunk, cov);
            ++plans;
          }
  check_rejections();
  if (failures) {
    std::printf("post_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("post_plan_check: all passed (%ld plans)\n", plans);
  return 0;
}
