// loo_plan_check.cpp — plan_loo (dis_project_amd/csrc/lfm_host.cpp), the plan of lfm_loocv_f64 /
// lfm_loocv_grad_f64 (lfm_loo.hip and lfm_api.hip only read it), under AddressSanitizer + UBSan:
// built and run by tests/test_loo_host.py with the flags of tests/native/Makefile.
//   n = 1, 2, 127, 128, 129, 1024, 16384: Bs, W_loo, Bt and the row a lie inside the 2Mp x 2Mp
//   matrix and no two of them share an element (checked as rectangles at stride ld); the scratch
//   vectors are disjoint and inside vec; the product's grid counts the lower 128-tiles and
//   loo_tile walks them once each, in order; the scale kernel's tiles cover Np x Np; the strips of
//   loo_u_kernel cover the rows; the byte counts are the formulas. n = 0, -1, 2^30 + 1 are
//   rejected with a message; n = 2^30 is rejected (its matrix does not fit a size_t of bytes) and
//   no field of a rejected plan holds a size.
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

// rows [r0, r1) x columns [c0, c1) of the matrix
struct Rect {
  const char* name;
  int64_t r0, r1, c0, c1;
};
static Rect rect_at(const char* name, int64_t off, int64_t ld, int64_t rows, int64_t cols) {
  return {name, off / ld, off / ld + rows, off % ld, off % ld + cols};
}
static bool overlap(const Rect& a, const Rect& b) {
  return a.r0 < b.r1 && b.r0 < a.r1 && a.c0 < b.c1 && b.c0 < a.c1;
}

static void check_plan(int64_t n) {
  const LooPlan P = plan_loo(n);
  CHECK(P.reject == LooPlan::OK && P.why.empty(), "n %ld rejected: %d", (long)n, P.reject);
  if (P.reject) return;
  const int64_t Np = up(n, 128), Mp = up(n + 1, 128), ld = 2 * Mp;
  CHECK(P.n == n && P.Np == Np && P.Mp == Mp && P.ld == ld && Np <= Mp, "header of n %ld", (long)n);
  CHECK(P.mat_bytes == (size_t)ld * ld * 8, "mat_bytes");
  // where the bordered factorisation leaves its results (lfm_grad.hip)
  CHECK(P.bt == Mp * ld + Mp && P.a == P.bt + n * ld, "Bt / a");
  const Rect bt = rect_at("Bt", P.bt, ld, n, n), a = rect_at("a", P.a, ld, 1, n);
  const Rect bs = rect_at("Bs", P.bs, ld, Np, Np), w = rect_at("W", P.w, ld, n, n);
  const Rect all[4] = {bt, a, bs, w};
  for (const Rect& r : all) {
    CHECK(r.r0 >= 0 && r.c0 >= 0 && r.r1 <= ld && r.c1 <= ld, "%s leaves the matrix at n %ld",
          r.name, (long)n);
    for (const Rect& q : all)
      if (&r != &q) CHECK(!overlap(r, q), "%s overlaps %s at n %ld", r.name, q.name, (long)n);
  }
  // Bs is the top-left block (the factor's), W the top-right one (never written)
  CHECK(bs.r1 <= Mp && bs.c1 <= Mp && w.r1 <= Mp && w.c0 >= Mp, "blocks at n %ld", (long)n);
  // every 16-byte access of the product's staging is aligned: even offsets, even stride
  CHECK(P.bs % 2 == 0 && ld % 2 == 0 && Np % 16 == 0, "alignment");
  // scratch: five vectors of Np doubles, then the value and a^T b
  const int64_t v[6] = {P.mu, P.var, P.sc, P.b, P.u, P.val};
  for (int i = 0; i < 6; ++i) {
    const int64_t len = i < 5 ? Np : 2;
    CHECK(v[i] >= 0 && v[i] + len <= P.vec, "vector %d outside the scratch", i);
    for (int j = 0; j < i; ++j) {
      const int64_t lj = j < 5 ? Np : 2;
      CHECK(v[i] >= v[j] + lj || v[j] >= v[i] + len, "vectors %d and %d overlap", i, j);
    }
  }
  CHECK(P.vec == 5 * Np + 2 && P.vec_bytes == (size_t)P.vec * 8, "vec");
  // grids
  const int64_t T = Np / 128;
  CHECK(P.tiles == T && P.product_grid == T * (T + 1) / 2, "product grid");
  CHECK(P.scale_tiles * 64 == Np && P.scale_tiles <= 65535, "scale grid");
  CHECK(P.u_grid * 64 >= n && (P.u_grid - 1) * 64 < n, "u grid");
  if (T <= 128) {
    int64_t b = 0;
    for (int64_t ti = 0; ti < T; ++ti)
      for (int64_t tj = 0; tj <= ti; ++tj, ++b) {
        int64_t gi = -1, gj = -1;
        loo_tile(b, &gi, &gj);
        CHECK(gi == ti && gj == tj, "tile %ld of n %ld: (%ld, %ld)", (long)b, (long)n, (long)gi,
              (long)gj);
        // the tile's rows and columns of Bs and of W stay inside their blocks
        CHECK((ti + 1) * 128 <= Np && (tj + 1) * 128 <= Np, "tile outside Bs");
      }
    CHECK(b == P.product_grid, "tiles walked");
  }
}

static void check_tiles_far() {
  // the decode at tile counts no matrix here reaches: exact around the 2^31 - 1 limit
  const int64_t T = 65535, last = T * (T + 1) / 2 - 1;
  int64_t ti, tj;
  loo_tile(last, &ti, &tj);
  CHECK(ti == T - 1 && tj == T - 1, "last tile");
  loo_tile(last - (T - 1), &ti, &tj);
  CHECK(ti == T - 1 && tj == 0, "first tile of the last row");
  loo_tile(last - T, &ti, &tj);
  CHECK(ti == T - 2 && tj == T - 2, "last tile of the row before");
}

static void check_rejected(int64_t n, int code) {
  const LooPlan P = plan_loo(n);
  CHECK(P.reject == code && !P.why.empty(), "n %ld: reject %d, expected %d", (long)n, P.reject,
        code);
  CHECK(P.mat_bytes == 0 && P.vec_bytes == 0 && P.product_grid == 0 && P.scale_tiles == 0 &&
            P.u_grid == 0 && P.ld == 0,
        "a rejected plan holds sizes (n %ld)", (long)n);
}

int main() {
  for (int64_t n : {1, 2, 127, 128, 129, 1024, 16384}) check_plan(n);
  // a few more edges of the 64- and 128-steps
  for (int64_t n : {63, 64, 65, 255, 256, 257, 4096}) check_plan(n);
  check_tiles_far();
  check_rejected(0, LooPlan::BAD_N);
  check_rejected(-1, LooPlan::BAD_N);
  check_rejected(((int64_t)1 << 30) + 1, LooPlan::BAD_N);
  check_rejected((int64_t)1 << 30, LooPlan::TOO_LARGE);
  // the largest n whose scale grid fits a launch, and the first one past it
  check_plan((int64_t)32767 * 128);
  check_rejected((int64_t)32767 * 128 + 1, LooPlan::TOO_LARGE);
  if (failures) {
    std::printf("loo_plan_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("loo_plan_check: all passed\n");
  return 0;
}
