// lfm_bijectors.h — the forward maps of the model's bijectors (model.py:66-121) and one
// parameter's training step as the on-device fits evaluate them: small_fit_kernel (lfm_small.hip)
// and mid_adam_kernel (lfm_mid.hip) share these functions, so both constrain, differentiate and
// update with the same bits. A kernel loads and stores; what is here knows no kernel.
//   true_d, true_s, true_b, obs_stddev: tfb.Softplus; its derivative is sigmoid
//   l: tfb.Sigmoid(0.5, 3.5) = 0.5 + 3 sigmoid
// A problem's packed slots i: D [0, G), S [G, 2 G), B [2 G, 3 G), l 3 G, obs_stddev 3 G + 1 and
// the jitter 3 G + 2 (a static field: never updated).
// fit_constrain and fit_update carry `#pragma clang fp contract(off)` themselves: an inlined
// function keeps its own contraction setting whatever its caller's is, and a fused multiply-add
// here changes the bits.
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

// model.constrain() (trainer.py:103) of slot i: D, S, B, obs_stddev = softplus, l = 0.5 + 3
// sigmoid; the jitter slot holds the static jitter itself
__device__ __forceinline__ double fit_constrain(int i, int G, double x) {
  #pragma clang fp contract(off)
  return i == 3 * G ? 0.5 + 3.0 * sigmoid_d(x) : i == 3 * G + 2 ? x : softplus_d(x);
}

// Step s of a call (step o.step0 + s of the fit) on trainable slot i < 3 G + 2, as
// JaxTrainer.step's tail (trainer.py:105-132) and after_epoch (trainer.py:133-160, 205-210): from
// the unconstrained x, the gradient g with respect to the constrained value, Adam's moments and
// the host's bias corrections c1 = 1 - b1^count, c2 = 1 - b2^count
//   chain rule: g_raw = g softplus'(x) = g sigmoid(x); l: g 3 sigmoid (1 - sigmoid)
//   optax.adam: mu = b1 mu + (1 - b1) g_raw, nu = b2 nu + (1 - b2) g_raw^2, and the bias-
//               corrected update times -lr, in optax's order (below)
//   after_epoch: every o.spe steps (step 0 included), if o.fix, raw true_s[3] = 1.0 and raw
//     true_d[3] = 0.8 (the unconstrained leaves: the reference's quirk; no-op for G <= 3, as JAX
//     drops out-of-bounds updates)
// The new x, mu, nu.
struct FitSlot {
  double x, mu, nu;
};
__device__ __forceinline__ FitSlot fit_update(const AdamOpt& o, int i, int G, int64_t s, double x,
                                              double g, double mu0, double nu0, double c1,
                                              double c2) {
  #pragma clang fp contract(off)
  const double sg = sigmoid_d(x);
  const double gr = i == 3 * G ? g * 3.0 * sg * (1.0 - sg) : g * sg;
  const double mu = o.b1 * mu0 + (1.0 - o.b1) * gr;
  const double nu = o.b2 * nu0 + (1.0 - o.b2) * (gr * gr);
  // optax's order: scale_by_adam's mu_hat / (sqrt(nu_hat + eps_root) + eps), then
  // scale(-learning_rate)
  const double u = (mu / c1) / (sqrt(nu / c2 + o.eps_root) + o.eps);
  const double upd = -o.lr * u;
  double xn = x + upd;
  if (o.fix && (o.step0 + s) % o.spe == 0 && G > 3) {
    if (i == G + 3) xn = 1.0;  // true_s[3]
    if (i == 3) xn = 0.8;      // true_d[3]
  }
  return {xn, mu, nu};
}

}  // namespace lfm
