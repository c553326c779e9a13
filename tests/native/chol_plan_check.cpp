// chol_plan_check.cpp — the step plans of the exact-factor cases (tests/chol_cases.py): plan_steps
// and plan_s3 (dis_project_amd/csrc/lfm_host.cpp) as chol_factor_solve calls them, under
// AddressSanitizer + UBSan: built and run by tests/test_chol_cases_host.py with the flags of
// tests/native/Makefile.
//   stdin, one case per line:
//     name n s3 wbulk w4min w2min w0 helper helper_tc helper_min cus side_cus
//   (helper, helper_tc, helper_min and side_cus may be "-": S3Params' own default)
//   stdout, one line per case:
//     name n=.. Mp=.. nblk=.. widths=1,4,5 steps=T:wn:R:hu ...
//   one field per step: T the trailing 128-tiles past the super-panel, wn the next super-panel's
//   width, R the rest region's enumeration (B bands, S the supertiled triangle, - no update) and
//   hu the side-CU helper's units (schedule 1: no plan_s3, hu is 0).
//   Checked on the way: the steps tile [0, nblk) in order; every helper share is a tail of at most
//   half the rest units, lies in a supertiled region and holds no lead tile; the launch grids
//   cover their units.
#include <algorithm>
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

int main() {
  char name[128], helper[32], tc[32], hmin[32], side[32];
  long n, w4min, w2min;
  int s3, wbulk, w0, cus;
  int cases = 0;
  while (std::scanf("%127s %ld %d %d %ld %ld %d %31s %31s %31s %d %31s", name, &n, &s3, &wbulk,
                    &w4min, &w2min, &w0, helper, tc, hmin, &cus, side) == 12) {
    ++cases;
    // "-": S3Params' own default
    auto given = [](const char* t) { return !(t[0] == '-' && t[1] == 0); };
    const int NB = 128;
    const int64_t Mp = (n + 1 + NB - 1) / NB * NB, nblk = (n + NB - 1) / NB;
    const auto steps = plan_steps(nblk, Mp, NB, false, s3 != 0, wbulk, w4min, w2min, w0);
    const int S = (int)steps.size();
    int64_t k = 0;
    for (const auto& st : steps) {
      CHECK(st.first == k && st.second >= 1, "%s: step at %ld, expected %ld", name, (long)st.first,
            (long)k);
      k += st.second;
    }
    CHECK(k == nblk, "%s: the steps end at %ld of %ld", name, (long)k, (long)nblk);
    std::printf("%s n=%ld Mp=%ld nblk=%ld widths=", name, n, (long)Mp, (long)nblk);
    for (int s = 0; s < S; ++s) std::printf("%s%d", s ? "," : "", steps[s].second);
    std::printf(" steps=");
    S3Plan P;
    S3Params pp;
    if (s3) {
      pp.n = n;
      pp.Mp = Mp;
      pp.cus = cus;
      if (given(side)) pp.side_cus = std::atoi(side);
      if (given(helper)) pp.helper = std::atoi(helper);
      if (given(tc)) pp.helper_tc = std::atof(tc);
      if (given(hmin)) pp.helper_min = std::atof(hmin);
      CHECK(pp.nb == NB && pp.st == NB, "%s: tile constants", name);
      P = plan_s3(steps, pp);
      CHECK(P.S == S && (int)P.steps.size() == S, "%s: plan of %d steps", name, P.S);
    }
    for (int s = 0; s < S; ++s) {
      const int64_t K1 = (steps[s].first + steps[s].second) * NB;
      const int T = (int)((Mp - K1) / NB), wn = s + 1 < S ? steps[s + 1].second : 0;
      int64_t hu = 0;
      if (s3) {
        const S3Step& q = P.steps[s];
        hu = q.hu;
        CHECK(q.T == T && q.wn == wn && q.K1 == K1 && q.kd == NB * steps[s].second,
              "%s step %d: T %d wn %d", name, s, q.T, q.wn);
        CHECK(q.nr == (T - wn) * (T - wn + 1) && q.na == 2 * wn * (T - wn), "%s step %d: units",
              name, s);
        CHECK(hu >= 0 && hu <= q.nr / 2 && q.nr_main == q.nr - hu, "%s step %d: hu %ld of %d",
              name, s, (long)hu, q.nr);
        if (hu > 0) {
          CHECK(T - wn > kBandMaxCols && s >= 1 && s + 2 < S, "%s step %d: a helper here", name, s);
          CHECK(q.hgrid >= hu && q.hgrid % 8 == 0, "%s step %d: helper grid", name, s);
          for (int64_t b = q.nr - hu; b < q.nr; ++b) {
            int ti, tj;
            rest_unit_tile(b, T, wn, pp.supertile, &ti, &tj);
            CHECK(tj >= wn && tj < T && ti / 2 >= tj && ti / 2 < T, "%s step %d unit %ld: (%d, %d)",
                  name, s, (long)b, ti, tj);
            CHECK(!(ti / 2 < wn + q.lead && tj < wn + q.lead), "%s step %d: lead tile in the tail",
                  name, s);
          }
        }
        if (s + 1 < S)
          CHECK(q.grid >= q.na + q.nr_main + P.steps[s + 1].nt, "%s step %d: grid", name, s);
      }
      const char* R = s + 1 == S ? "-" : T - wn <= kBandMaxCols ? "B" : "S";
      std::printf("%s%d:%d:%s:%ld", s ? " " : "", T, wn, R, (long)hu);
    }
    std::printf("\n");
  }
  CHECK(cases > 0, "no case on stdin");
  if (failures) {
    std::printf("chol_plan_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("chol_plan_check: all passed (%d cases)\n", cases);
  return 0;
}
