// mid_shapes_check.cpp — plan_mid and plan_mid_post (dis_project_amd/csrc/lfm_host.cpp) on the
// shapes given on the command line, one "n G m" triple per problem (m = 0: no posterior call):
// what the planners themselves say of a batch, for tests/test_exact_mid_host.py, which feeds them
// the shapes of the extended-precision fixtures that tests/test_gpu_exact_mid.py runs on the mid
// path. Prints the limits, then per problem "n G m nb mb", then the two planners' rejections
// (0: accepted) and the launch counts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dis_project_amd/csrc/lfm_host.h"

using namespace lfm;

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::printf("usage: mid_shapes_check n G m [n G m ...]\n");
    return 2;
  }
  std::vector<MidShape> shapes;
  std::vector<int64_t> m;
  for (int i = 1; i + 2 < argc; i += 3) {
    shapes.push_back(MidShape{std::atoll(argv[i]), std::atoll(argv[i + 1])});
    m.push_back(std::atoll(argv[i + 2]));
  }
  std::printf("limits MID_MAX_N %d MID_MAX_M %d MID_TILE %d\n", MID_MAX_N, MID_MAX_M, MID_TILE);
  const MidPlan P = plan_mid(shapes);
  std::printf("plan_mid reject %d %s\n", P.reject, P.why.c_str());
  if (P.reject != MidPlan::OK) return 1;
  bool post = true;
  for (int64_t v : m) post = post && v != 0;
  MidPostPlan Q;
  if (post) {
    Q = plan_mid_post(shapes, m.data(), true, true);
    std::printf("plan_mid_post reject %d %s\n", Q.reject, Q.why.c_str());
    if (Q.reject != MidPostPlan::OK) return 1;
  }
  for (size_t p = 0; p < shapes.size(); ++p)
    std::printf("problem %lld %lld %lld nb %d mb %d\n", (long long)shapes[p].n,
                (long long)shapes[p].G, (long long)m[p], P.probs[p].nb, post ? Q.pp[p].mb : 0);
  std::printf("launches value %zu value_grad %zu posterior %zu\n", P.value.size(),
              P.value_grad.size(), post ? Q.launches.size() : (size_t)0);
  return 0;
}
