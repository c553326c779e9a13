// post_logp_plan_check.cpp — plan_post_logp (dis_project_amd/csrc/lfm_host.cpp), the plan of
// lfm_post_log_prob_f64 (lfm_post_api.hip issues exactly what it says), under AddressSanitizer +
// UBSan: built and run by tests/test_post_logp_host.py with the flags of tests/native/Makefile.
//   the rejections come in the documented order with their messages; Mp' and Np' at the 128-edges
//   of m; the sweep over the covariance's factor has no update launch up to Np' = 512 and one from
//   640; the passes cover every held-out row once, in order, at the 64- and 128-row edges of k;
//   every byte count is include/lfm.h's formula and bounds every offset the launches reach; the
//   residual rows stay within POST_VT_BUDGET at m = 16384, k = 2^24; and plan_post / plan_sample
//   give what they gave before this plan was built from them.
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
static bool has(const std::string& s, const char* word) {
  return s.find(word) != std::string::npos;
}

static void check_plan(int64_t n, int64_t G, int64_t m, int64_t k, int64_t chunk) {
  const PostLogpPlan P = plan_post_logp(n, G, m, k, chunk);
  CHECK(P.reject == PostLogpPlan::OK, "n %ld m %ld k %ld chunk %ld rejected: %d", (long)n, (long)m,
        (long)k, (long)chunk, P.reject);
  if (P.reject) return;
  const int64_t Np = up(m, 128), Mp = up(m + 1, 128), NpS = up(n, 128);
  CHECK(P.m == m && P.k == k && P.Np == Np && P.Mp == Mp, "header");
  // the pass: the handle's chunk, capped by the budget's chunk for Np' columns
  const int64_t eff = chunk ? chunk : post_default_chunk(NpS);
  const int64_t pass = eff < post_default_chunk(Np) ? eff : post_default_chunk(Np);
  CHECK(P.pass == pass && pass >= 128 && pass % 128 == 0, "pass %ld", (long)P.pass);
  CHECK((size_t)pass * Np * 8 <= POST_VT_BUDGET, "a pass of %ld rows x %ld over the budget",
        (long)pass, (long)Np);
  // the predict is plan_post's with the covariance, unchanged
  const ResidentPlan R = plan_post(n, G, m, chunk, true);
  CHECK(P.pred.reject == 0 && P.pred.chunks.size() == 1 && P.pred.vt_bytes == R.vt_bytes &&
            P.pred.acc_bytes == R.acc_bytes && P.pred.cov_bytes == (size_t)m * m * 8 &&
            P.pred.panels.size() == R.panels.size() && P.pred.Np == NpS,
        "the predict's plan");
  // the passes: every held-out row exactly once, in order
  int64_t next = 0, P128 = 0;
  for (const PostChunk& c : P.rows.chunks) {
    CHECK(c.q0 == next && c.rows >= 1 && c.rows <= pass, "pass at %ld rows %ld", (long)c.q0,
          (long)c.rows);
    CHECK(c.q0 % 128 == 0, "a pass starts inside a 128-row tile");
    CHECK(c.pad_rows == up(c.rows, 128) && (int64_t)c.tiles * 128 == c.pad_rows, "pass padding");
    CHECK(c.panel_grid == (int)((c.rows + 63) / 64) && (int64_t)c.panel_grid * 64 <= c.pad_rows,
          "panel grid %d for %ld rows", c.panel_grid, (long)c.rows);
    next += c.rows;
    P128 = P128 > c.pad_rows ? P128 : c.pad_rows;
  }
  CHECK(next == k, "passes cover %ld of %ld rows", (long)next, (long)k);
  CHECK((int64_t)P.rows.chunks.size() == (k + pass - 1) / pass, "pass count");
  CHECK(P.rows.vt_rows == P128 && P128 == up(k < pass ? k : pass, 128), "rows of R");
  // the sweep: plan_post's panel list for a factor of Np' columns
  int64_t col = 0;
  int updates = 0;
  for (const PostPanel& s : P.rows.panels) {
    CHECK(s.K0 == col && s.w >= 1 && s.w <= POST_W && s.K1 == s.K0 + 128 * (int64_t)s.w,
          "super-panel at %ld", (long)s.K0);
    CHECK(s.tj0 == s.K1 / 128 && s.ntj == (Np - s.K1) / 128 && s.ntj >= 0, "update columns");
    updates += s.ntj > 0;
    col = s.K1;
  }
  CHECK(col == Np && P.rows.Np == Np, "super-panels cover %ld of %ld columns", (long)col, (long)Np);
  CHECK(updates == (int)((Np / 128 - 1) / POST_W), "update launches %d at Np' %ld", updates,
        (long)Np);
  // the byte counts: include/lfm.h's formula
  const size_t V = (size_t)up(m, 128) * NpS, A = 2 * (size_t)up(m, 128);
  const size_t rv = (size_t)P128 * Np, ra = 2 * (size_t)P128;
  CHECK(P.pred.vt_bytes == V * 8 && P.pred.acc_bytes == A * 8, "the predict's V and A");
  CHECK(P.mat_bytes == (size_t)Mp * Mp * 8, "matrix bytes");
  CHECK(P.dinv_bytes + P.zero_bytes == 17 * (size_t)Np * 8 && P.zero_bytes == (size_t)Np * 8,
        "inverses and z");
  CHECK(P.vt_bytes == 8 * (V + (rv > V ? rv - V : 0)), "vt bytes");
  CHECK(P.acc_bytes == 8 * (A + (ra > A ? ra - A : 0)), "acc bytes");
  CHECK(P.logp_bytes == (size_t)P128 * 8, "logp bytes");
  // what the launches reach
  const size_t vt = P.vt_bytes / 8, acc = P.acc_bytes / 8, mat = P.mat_bytes / 8;
  for (const PostChunk& c : P.rows.chunks) {
    // the upload and the residual kernel: rows [0, pad_rows) x columns [0, Np)
    CHECK((size_t)(c.pad_rows - 1) * Np + Np - 1 < vt, "R reaches past the workspace");
    CHECK((int64_t)P.resid_grid * 512 >= Np && ((int64_t)P.resid_grid - 1) * 512 < Np,
          "residual grid %d", P.resid_grid);
    // panel rows and their accumulators (s2 at 0, sz at rows.vt_rows); update tiles
    const size_t prow = (size_t)c.panel_grid * 64 - 1;
    CHECK(prow < (size_t)P.rows.vt_rows && (size_t)P.rows.vt_rows + prow < acc, "accumulators");
    CHECK((size_t)(c.tiles * 128 - 1) * Np + Np - 1 < vt, "update tiles reach past R");
    CHECK((size_t)c.rows <= P.logp_bytes / 8, "one pass's results");
  }
  // the factor as the sweep reads it: rows and columns [0, Np) of the Mp-stride matrix; row m
  CHECK((size_t)(Np - 1) * Mp + Np - 1 < mat && (size_t)m * Mp + m < mat, "factor reach");
  CHECK((int64_t)P.dinv_grid * 128 == Np && (int64_t)P.z_grid * 256 >= Np, "dinv / z grids");
  CHECK((size_t)P.dinv_grid * 8 * 256 * 8 == P.dinv_bytes, "one 8 x 16 x 16 per 128-block");
}

static void check_rejections() {
  auto plan = [](int64_t n, int64_t G, int64_t m, int64_t k, int64_t chunk) {
    return plan_post_logp(n, G, m, k, chunk);
  };
  // the m rules first, in plan_post's order, whatever k is
  CHECK(plan(129, 3, 0, 0, 100).reject == PostLogpPlan::BAD_M, "m = 0 first");
  CHECK(plan(129, 3, 128, -1, 128).reject == PostLogpPlan::BAD_M, "m % G before k");
  CHECK(has(plan(129, 3, 128, 1, 128).why, "num_genes"), "the message names num_genes");
  CHECK(plan(129, 3, 129, 0, 128).reject == PostLogpPlan::COV_CHUNK, "m above the chunk before k");
  CHECK(has(plan(129, 3, 129, 1, 128).why, "128"), "the message names the limit");
  CHECK(plan(129, 3, 99, 0, 100).reject == PostLogpPlan::BAD_CHUNK, "a bad chunk before k");
  CHECK((int)PostLogpPlan::BAD_M == (int)ResidentPlan::BAD_M &&
            (int)PostLogpPlan::COV_CHUNK == (int)ResidentPlan::COV_CHUNK &&
            (int)PostLogpPlan::BAD_CHUNK == (int)ResidentPlan::BAD_CHUNK,
        "the m codes are plan_post's");
  // then k
  CHECK(plan(129, 3, 129, 0, 256).reject == PostLogpPlan::BAD_K, "k = 0");
  CHECK(plan(129, 3, 129, -5, 0).reject == PostLogpPlan::BAD_K, "k < 0");
  CHECK(has(plan(129, 3, 129, 0, 0).why, "k must be"), "the message names k");
  const PostLogpPlan T = plan(129, 3, 129, LOGP_MAX_K + 1, 0);
  CHECK(T.reject == PostLogpPlan::TOO_MANY && has(T.why, "split") &&
            has(T.why, std::to_string(LOGP_MAX_K).c_str()),
        "k above the limit: %s", T.why.c_str());
  CHECK(plan(129, 3, 129, LOGP_MAX_K, 0).reject == PostLogpPlan::OK, "the most a call");
  CHECK(LOGP_MAX_K == (int64_t)1 << 24, "2^24");
  // a rejected plan lists nothing
  CHECK(T.rows.chunks.empty() && T.rows.panels.empty() && T.pred.chunks.empty() &&
            T.mat_bytes == 0 && T.vt_bytes == 0,
        "a rejected plan lists launches");
}

static void check_edges() {
  // Mp' / Np' at the 128-edges of m
  const struct { int64_t m, Np, Mp; } e[] = {{127, 128, 128}, {128, 128, 256}, {129, 256, 256},
                                             {512, 512, 640}, {513, 640, 640}};
  for (const auto& c : e) {
    const PostLogpPlan P = plan_post_logp(1000, 1, c.m, 3, 0);
    CHECK(P.reject == 0 && P.Np == c.Np && P.Mp == c.Mp, "m %ld: Np' %ld Mp' %ld", (long)c.m,
          (long)P.Np, (long)P.Mp);
  }
  // the sweep's launches: no update up to Np' = 512, one from 640 (a panel of 4, then one of 1)
  for (int64_t m : {1, 128, 384, 512}) {
    const PostLogpPlan P = plan_post_logp(300, 1, m, 5, 0);
    CHECK(P.rows.panels.size() == 1 && P.rows.panels[0].ntj == 0, "m %ld: an update launch",
          (long)m);
  }
  {
    const PostLogpPlan P = plan_post_logp(300, 5, 520, 130, 0);
    CHECK(P.Np == 640 && P.rows.panels.size() == 2 && P.rows.panels[0].w == 4 &&
              P.rows.panels[0].ntj == 1 && P.rows.panels[0].tj0 == 4 && P.rows.panels[1].w == 1 &&
              P.rows.panels[1].ntj == 0,
          "Np' = 640: panel, update, panel");
    CHECK(P.rows.chunks.size() == 1 && P.rows.chunks[0].panel_grid == 3 &&
              P.rows.chunks[0].tiles == 2,
          "k = 130: three 64-row slabs, two 128-row tiles");
  }
  // k at the 64- and 128-row edges
  const struct { int64_t k; int grid, tiles; } ke[] = {{1, 1, 1},   {63, 1, 1},  {64, 1, 1},
                                                       {65, 2, 1},  {127, 2, 1}, {128, 2, 1},
                                                       {129, 3, 2}, {130, 3, 2}, {256, 4, 2}};
  for (const auto& c : ke) {
    const PostLogpPlan P = plan_post_logp(105, 5, 100, c.k, 0);
    CHECK(P.reject == 0 && P.rows.chunks.size() == 1 && P.rows.chunks[0].panel_grid == c.grid &&
              P.rows.chunks[0].tiles == c.tiles,
          "k %ld", (long)c.k);
  }
  // lfm_post_set_chunk(128): passes of 128 rows
  {
    const PostLogpPlan P = plan_post_logp(105, 5, 100, 130, 128);
    CHECK(P.pass == 128 && P.rows.chunks.size() == 2 && P.rows.chunks[1].q0 == 128 &&
              P.rows.chunks[1].rows == 2 && P.rows.vt_rows == 128,
          "chunk 128: two passes");
  }
  // the budget at the largest shape: m = 16384 (a chunk the caller sets: the default at
  // n = 16384 is 8192 rows), k = 2^24
  {
    const PostLogpPlan P = plan_post_logp(16384, 1, 16384, LOGP_MAX_K, 16384);
    CHECK(P.reject == 0 && P.pass == 8192 && P.rows.chunks.size() == 2048, "passes at 2^24");
    CHECK((size_t)P.rows.vt_rows * P.Np * 8 <= POST_VT_BUDGET && P.rows.vt_bytes <= POST_VT_BUDGET,
          "R over the budget");
    CHECK(P.vt_bytes == P.pred.vt_bytes, "the predict's workspace is the larger one here");
    if (!P.rows.chunks.empty())
      CHECK(P.rows.chunks.back().q0 + P.rows.chunks.back().rows == LOGP_MAX_K, "the last pass");
    CHECK(plan_post_logp(16384, 1, 16384, 1, 0).reject == PostLogpPlan::COV_CHUNK,
          "m = 16384 above the default chunk");
  }
}

// plan_post and plan_sample at shapes of post_plan_check.cpp and sample_plan_check.cpp: the
// figures they gave before plan_post_logp was built from them
static void check_unchanged() {
  const ResidentPlan a = plan_post(16384, 4, 4 * 1367, 0, true);
  CHECK(a.reject == 0 && a.Np == 16384 && a.chunk == 8192 && a.chunks.size() == 1 &&
            a.vt_rows == 5504 && a.vt_bytes == (size_t)5504 * 16384 * 8 &&
            a.acc_bytes == 2 * 5504 * 8 && a.panels.size() == 32 && a.panels[31].ntj == 0 &&
            a.panels[0].ntj == 124 && a.cov_tiles == 43 && a.cov_bytes == (size_t)5468 * 5468 * 8,
        "plan_post(16384, 4, 5468, 0, cov)");
  const ResidentPlan b = plan_post(1333, 3, 3 * 129, 128, false);
  CHECK(b.reject == 0 && b.Np == 1408 && b.chunks.size() == 4 && b.chunks[3].rows == 3 &&
            b.chunks[3].q0 == 384 && b.vt_rows == 128 && b.panels.size() == 3 &&
            b.panels[2].w == 3 && b.panels[1].ntj == 3 && b.cov_bytes == 0 &&
            b.t_bytes == 387 * 3 * 8 && b.out_bytes == 2 * 387 * 8,
        "plan_post(1333, 3, 387, 128, no cov)");
  CHECK(plan_post(129, 3, 129, 128, true).reject == ResidentPlan::COV_CHUNK, "plan_post rejects");
  const SamplePlan s = plan_sample(16384, 1024, 0);
  CHECK(s.reject == 0 && s.Np == 16384 && s.Mp == 16512 && s.zrows == 1024 && s.ldz == 16384 &&
            s.mat_bytes == (size_t)16512 * 16512 * 8 && s.z_bytes == (size_t)1024 * 16384 * 8 &&
            s.x_bytes == (size_t)1024 * 16384 * 8 && s.tiles_i == 8 && s.tiles_j == 128 &&
            s.pairs == (int64_t)1024 * 8192 && s.randn_grid == 32768,
        "plan_sample(16384, 1024, 0)");
  const SamplePlan u = plan_sample(129, 127, 5);
  CHECK(u.reject == 0 && u.Np == 256 && u.Mp == 256 && u.zrows == 128 && u.tiles_i == 1 &&
            u.tiles_j == 2 && u.x_bytes == 127 * 129 * 8 && u.sample0 == 5,
        "plan_sample(129, 127, 5)");
  CHECK(plan_sample(5, 0, 0).reject == SamplePlan::BAD_NSAMP, "plan_sample rejects");
}

int main() {
  long plans = 0;
  for (int64_t n : {1, 105, 300, 1400, 16384})
    for (int64_t G : {1, 3, 5})
      for (int64_t q : {1, 20, 42, 43, 128, 129, 171, 1367})
        for (int64_t k : {1, 63, 64, 65, 127, 128, 129, 130, 1000, 20000})
          for (int64_t chunk : {0, 128, 256, 8192}) {
            const int64_t m = q * G;
            const int64_t eff = chunk ? chunk : post_default_chunk(up(n, 128));
            if (m > eff) continue;  // the covariance needs m within one chunk: check_rejections
            check_plan(n, G, m, k, chunk);
            ++plans;
          }
  check_plan(16384, 1, 16384, LOGP_MAX_K, 16384);
  check_rejections();
  check_edges();
  check_unchanged();
  if (failures) {
    std::printf("post_logp_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("post_logp_plan_check: all passed (%ld plans)\n", plans);
  return 0;
}
