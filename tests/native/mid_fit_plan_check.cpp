// mid_fit_plan_check.cpp — plan_mid_fit (dis_project_amd/csrc/lfm_host.cpp), the third arena and
// the launch list of lfm_mbatch_fit_f64 (lfm_mbatch.hip issues exactly what it says), under
// AddressSanitizer + UBSan: built and run by tests/test_mid_fit_host.py with the flags of
// tests/native/Makefile. Over single problems at the tile edges, mixed batches and
// nsteps = 1 .. 12, 150 and the cap:
//   raw, mu, nu, the bias table, the history and the first-bad-step words are disjoint, 16-byte
//   aligned and inside the reported bytes, and the bytes are the header's formula; the launch
//   list is the constrain, then per step plan_mid's value-and-gradient launches unchanged and
//   one update launch carrying the step, 1 + nsteps (len(value_grad) + 1) in all; every index
//   the update kernel forms (packed slots, history, bias) stays inside its region; the
//   rejections come in the documented order with the limit in the message.
// And adam_bias, the bias table of both on-device fits, against the host's pow entry for entry.
#include <algorithm>
#include <cmath>
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

struct Region {
  int64_t lo, hi;  // bytes
  const char* what;
};

static int64_t even(int64_t d) { return (d + 1) / 2 * 2; }

static void check_fit(const std::vector<MidShape>& shapes, int64_t nsteps) {
  const MidPlan P = plan_mid(shapes);
  const MidFitPlan F = plan_mid_fit(shapes, nsteps);
  CHECK(P.reject == MidPlan::OK && F.reject == MidFitPlan::OK, "rejected: %s", F.why.c_str());
  if (P.reject || F.reject) return;
  CHECK(F.nprob == P.nprob && F.nhyp == P.nhyp && F.nsteps == nsteps, "counts");
  // the regions
  std::vector<Region> rs;
  auto add = [&](int64_t lo_d, int64_t count_d, const char* what) {
    CHECK(lo_d % 2 == 0, "%s not 16-byte aligned", what);
    rs.push_back({lo_d * 8, (lo_d + count_d) * 8, what});
  };
  add(F.raw, F.nhyp, "raw");
  add(F.mu, F.nhyp, "mu");
  add(F.nu, F.nhyp, "nu");
  add(F.bias, 2 * nsteps, "bias");
  add(F.hist, nsteps * F.nprob, "history");
  CHECK(F.first_bad % 16 == 0 && (int64_t)F.first_bad >= F.doubles * 8, "first-bad words");
  rs.push_back({(int64_t)F.first_bad, (int64_t)(F.first_bad + F.nprob * sizeof(int)), "first_bad"});
  std::sort(rs.begin(), rs.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < rs.size(); ++i) {
    CHECK(rs[i].lo >= 0 && rs[i].hi <= (int64_t)F.bytes, "%s outside %zu bytes", rs[i].what,
          F.bytes);
    if (i) CHECK(rs[i - 1].hi <= rs[i].lo, "%s overlaps %s", rs[i - 1].what, rs[i].what);
  }
  // one upload covers raw | mu | nu | bias, one download raw | mu | nu
  CHECK(F.raw == 0 && F.mu == even(F.nhyp) && F.nu == 2 * even(F.nhyp) &&
            F.bias == 3 * even(F.nhyp) && F.hist == F.bias + 2 * nsteps,
        "raw, mu, nu, bias and history adjacent");
  const size_t want = 8 * (size_t)(3 * even(F.nhyp) + 2 * nsteps + even(nsteps * F.nprob)) +
                      16 * (size_t)((F.nprob + 3) / 4);
  CHECK(F.bytes == want, "bytes %zu, the header's formula gives %zu", F.bytes, want);
  // every index the update kernel forms: problem p's slots hv + i (i < 3 G) and hs + j (j < 3)
  // within [0, nhyp), each exactly once; history s nprob + p; bias 2 s, 2 s + 1
  std::vector<int> seen((size_t)F.nhyp, 0);
  for (const MidProb& m : P.probs) {
    for (int i = 0; i < 3 * m.G + 3; ++i) {
      const int64_t gi = i < 3 * m.G ? m.hv + i : m.hs + (i - 3 * m.G);
      CHECK(gi >= 0 && gi < F.nhyp, "slot %lld of n %d", (long long)gi, m.n);
      if (gi >= 0 && gi < F.nhyp) ++seen[(size_t)gi];
    }
  }
  for (int64_t i = 0; i < F.nhyp; ++i) CHECK(seen[(size_t)i] == 1, "slot %lld owners", (long long)i);
  CHECK((nsteps - 1) * F.nprob + F.nprob - 1 < nsteps * F.nprob, "history index");
  // the launches
  const size_t per = P.value_grad.size() + 1;
  CHECK(F.per_step == per, "per_step");
  CHECK(F.launches.size() == 1 + (size_t)nsteps * per, "launch count %zu", F.launches.size());
  if (F.launches.size() != 1 + (size_t)nsteps * per) return;
  for (const MidLaunch& l : F.launches) CHECK(l.kind >= 0 && l.kind < MID_KINDS, "launch kind %d", l.kind);
  const MidLaunch& c = F.launches[0];
  CHECK(c.kind == MID_CONSTRAIN && c.gx == (unsigned)F.nprob && c.gy == 1u, "the constrain");
  for (int64_t s = 0; s < nsteps; ++s) {
    const MidLaunch* l = &F.launches[1 + (size_t)s * per];
    for (size_t i = 0; i + 1 < per; ++i)
      CHECK(l[i].kind == P.value_grad[i].kind && l[i].k == P.value_grad[i].k &&
                l[i].gx == P.value_grad[i].gx && l[i].gy == P.value_grad[i].gy,
            "step %lld launch %zu is not the value-and-gradient call's", (long long)s, i);
    const MidLaunch& u = l[per - 1];
    CHECK(u.kind == MID_ADAM && u.k == (int)s && u.gx == (unsigned)F.nprob && u.gy == 1u,
          "step %lld's update", (long long)s);
    CHECK(u.k >= 0 && u.k < nsteps, "the update's step inside the history and the bias table");
  }
}

int main() {
  // rejections, in order
  CHECK(plan_mid_fit({}, 10).reject == MidFitPlan::BAD_BATCH, "empty batch");
  {
    const MidFitPlan F = plan_mid_fit({{28, 4}, {1025, 1}}, 0);
    CHECK(F.reject == MidFitPlan::BAD_BATCH && F.why.find("1025") != std::string::npos &&
              F.launches.empty() && F.bytes == 0,
          "a bad batch before bad steps: %s", F.why.c_str());
  }
  CHECK(plan_mid_fit({{129, 2}}, 10).reject == MidFitPlan::BAD_BATCH, "n %% G");
  CHECK(plan_mid_fit({{28, 4}}, 0).reject == MidFitPlan::NO_STEPS, "nsteps = 0");
  CHECK(plan_mid_fit({{28, 4}}, -1).reject == MidFitPlan::NO_STEPS, "nsteps = -1");
  CHECK(plan_mid_fit({{28, 4}}, INT64_MIN).reject == MidFitPlan::NO_STEPS, "nsteps = INT64_MIN");
  {
    const MidFitPlan F = plan_mid_fit({{28, 4}}, MID_FIT_MAX_STEPS + 1);
    CHECK(F.reject == MidFitPlan::TOO_MANY_STEPS &&
              F.why.find(std::to_string(MID_FIT_MAX_STEPS)) != std::string::npos &&
              F.launches.empty(),
          "past the cap: %s", F.why.c_str());
  }
  CHECK(plan_mid_fit({{28, 4}}, INT64_MAX).reject == MidFitPlan::TOO_MANY_STEPS, "INT64_MAX");
  CHECK(!plan_mid_fit({{28, 4}}, 0).why.empty(), "a rejection has a message");
  // single problems at the edges, every nsteps up to 12
  long plans = 0;
  for (int n : {1, 2, 63, 64, 65, 127, 128, 129, 192, 320, 1023, 1024})
    for (int64_t ns = 1; ns <= 12; ++ns) {
      check_fit({{n, 1}}, ns);
      ++plans;
    }
  // G up to n: more trainable parameters than one pass of 256 threads
  for (int64_t ns : {1, 3, 150}) {
    check_fit({{256, 128}}, ns);
    check_fit({{1024, 1024}}, ns);
    plans += 2;
  }
  // mixed batches, both orders; odd and even problem counts (the regions' padding)
  std::vector<MidShape> mixed = {{28, 4}, {63, 1}, {128, 2}, {129, 3}, {192, 3}, {320, 5}};
  for (int64_t ns : {1, 2, 3, 4, 5, 10, 149, 150}) {
    check_fit(mixed, ns);
    std::vector<MidShape> rev(mixed.rbegin(), mixed.rend());
    check_fit(rev, ns);
    rev.pop_back();
    check_fit(rev, ns);
    check_fit(std::vector<MidShape>(15, MidShape{320, 5}), ns);
    plans += 4;
  }
  check_fit({{7, 7}}, MID_FIT_MAX_STEPS);  // the cap itself is taken
  ++plans;
  // the bias table both fit entry points upload (adam_bias): the host's pow, entry for entry
  const lfm_adam opt{0.01, 0.9, 0.999, 1e-8, 0.0, 2, 1};
  for (int64_t step0 : {0, 7}) {
    std::vector<double> bias(2 * 3);
    adam_bias(&opt, step0, 3, bias.data());
    for (int64_t s = 0; s < 3; ++s) {
      const double count = (double)(step0 + s + 1);
      CHECK(bias[2 * s] == 1.0 - std::pow(opt.b1, count) &&
                bias[2 * s + 1] == 1.0 - std::pow(opt.b2, count),
            "bias of step %lld after %lld", (long long)s, (long long)step0);
    }
  }
  if (failures) {
    std::printf("mid_fit_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("mid_fit_plan_check: all passed (%ld plans)\n", plans);
  return 0;
}
