// small_shapes_check.cpp — the small-problem path's planners (dis_project_amd/csrc/
// lfm_small_plan.h, lfm_host.cpp) on the shapes given on the command line, one "n G T" triple per
// problem (T: timepoints per block of a dataset_3d grid layout, 0 for a layout off the grid):
// what the planners themselves say of a batch, for tests/test_exact_small_host.py, which feeds
// them the shapes of tests/small_exact_inputs.py. Prints the limits, per problem the T the plans
// use (0 when the grid tables are past SMALL_GRID_TAB_MAX), the doubles of its value, gradient
// and fit maps, the LDS bytes of a gradient and a fit launch of it alone (0: refused) and the
// posterior's panel columns (0: refused); then the batch's value launch (KxxTab or not, LDS
// bytes) and its gradient and fit launches.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dis_project_amd/csrc/lfm_host.h"

using namespace lfm;

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::printf("usage: small_shapes_check n G T [n G T ...]\n");
    return 2;
  }
  std::vector<SmallShape> shapes;
  for (int i = 1; i + 2 < argc; i += 3) {
    const int n = std::atoi(argv[i]), G = std::atoi(argv[i + 1]);
    GridLayout lay;
    lay.T = std::atoi(argv[i + 2]);
    lay.ok = lay.T > 0;
    shapes.push_back(SmallShape{n, G, small_grid_T(lay, G)});
  }
  std::printf("limits SMALL_MAX %d SMALL_GRAD_MAX %d SMALL_GRID_TAB_MAX %d SMALL_LDS_BYTES %zu\n",
              SMALL_MAX, SMALL_GRAD_MAX, SMALL_GRID_TAB_MAX, SMALL_LDS_BYTES);
  for (const SmallShape& s : shapes) {
    const std::vector<SmallShape> one{s};
    std::printf("problem %d %d T %d value %zu grad %zu fit %zu grad_lds %zu fit_lds %zu "
                "post_cols %d\n",
                s.n, s.G, s.T, small_map(nullptr, s.n, s.G, s.T, s.n + 1 <= 64, 0, 0, nullptr),
                small_map(nullptr, s.n, s.G, s.T, 1, 1, 0, nullptr),
                small_map(nullptr, s.n, s.G, s.T, 1, 1, 1, nullptr), small_grad_lds(one, 0),
                small_grad_lds(one, 1), s.n <= SMALL_GRAD_MAX ? small_post_cols(s.n, s.G, s.T) : 0);
  }
  const SmallMllPlan mll = plan_small_mll(small_dims(shapes));
  std::printf("batch value tabs %d lds %zu grad_lds %zu fit_lds %zu\n", mll.tabs, mll.lds_bytes,
              small_grad_lds(shapes, 0), small_grad_lds(shapes, 1));
  return mll.lds_bytes <= SMALL_LDS_BYTES ? 0 : 1;
}
