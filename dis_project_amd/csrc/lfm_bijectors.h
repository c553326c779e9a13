// lfm_bijectors.h — the forward maps of the model's bijectors (model.py:66-121) as the on-device
// fits evaluate them: small_fit_kernel (lfm_small.hip) and mid_adam_kernel (lfm_mid.hip) share
// these two functions, so both constrain and differentiate with the same bits.
//   true_d, true_s, true_b, obs_stddev: tfb.Softplus; its derivative is sigmoid
//   l: tfb.Sigmoid(0.5, 3.5) = 0.5 + 3 sigmoid
#pragma once
#include "lfm_internal.h"

namespace lfm {

__device__ __forceinline__ double softplus_d(double x) {
  // np.logaddexp(0, x): x + log1p(exp(-x)) for x >= 0, log1p(exp(x)) below
  return x >= 0.0 ? x + log1p(exp(-x)) : log1p(exp(x));
}
__device__ __forceinline__ double sigmoid_d(double x) {
  const double e = exp(-fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

}  // namespace lfm
