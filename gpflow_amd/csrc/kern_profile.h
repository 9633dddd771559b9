// The radial profiles of the stationary families on the SCALED squared distance r2 -- k, -2 dk/dr2 and the RationalQuadratic's
// dk/dalpha -- as the epilogues of rbf.hip (64 x 64 VALU tile, d <= GPK_MAX_D) and wide/wide_stationary.hip (MFMA tile, d <= 1024)
// evaluate them: one text, so an element has the same bits from either builder given the same r2.
#pragma once
#include "gpk_internal.h"

namespace {

template <int family>
__device__ __forceinline__ double kern_eval(double r2, double variance, double alpha) {
  if (family == GPK_KERN_SE) return variance * exp(-0.5 * r2);
  if (family == GPK_KERN_RQ) return variance * exp(-alpha * log1p(r2 / (2.0 * alpha)));   // (1 + r2 / (2 alpha))^-alpha, on r2: no clamp
  const double r = sqrt(r2 < 1e-36 ? 1e-36 : r2);   // (not fmax: a NaN r2 has to come out as NaN, as tf.maximum gives)
  if (family == GPK_KERN_MATERN12) return variance * exp(-r);
  if (family == GPK_KERN_EXPONENTIAL) return variance * exp(-0.5 * r);
  if (family == GPK_KERN_MATERN32) {
    const double sqrt3 = 1.7320508075688772;
    return variance * (1.0 + sqrt3 * r) * exp(-sqrt3 * r);
  }
  const double sqrt5 = 2.23606797749979;
  return variance * (1.0 + sqrt5 * r + 5.0 / 3.0 * (r * r)) * exp(-sqrt5 * r);
}

// -2 dk/dr2 at the SCALED squared distance: the factor every lengthscale / input gradient of a stationary kernel starts
// from (for the SquaredExponential it is k itself).  r = sqrt(max(r2, 1e-36)) has derivative 0 where the clamp is
// active (stationaries.py:103-116 under TF autodiff: tf.maximum passes nothing to the clamped argument).
template <int family>
__device__ __forceinline__ double kern_dr2(double r2, double variance, double alpha) {
  if (family == GPK_KERN_SE) return variance * exp(-0.5 * r2);
  if (family == GPK_KERN_RQ) return variance * exp(-(alpha + 1.0) * log1p(r2 / (2.0 * alpha)));
  if (r2 <= 1e-36) return 0.0;   // (a NaN r2 is not clamped: it reaches sqrt and comes out as NaN)
  const double r = sqrt(r2);
  if (family == GPK_KERN_MATERN12) return variance * exp(-r) / r;
  if (family == GPK_KERN_EXPONENTIAL) return variance * exp(-0.5 * r) / (2.0 * r);
  if (family == GPK_KERN_MATERN32) {
    const double sqrt3 = 1.7320508075688772;
    return 3.0 * variance * exp(-sqrt3 * r);
  }
  const double sqrt5 = 2.23606797749979;
  return (5.0 / 3.0) * variance * (1.0 + sqrt5 * r) * exp(-sqrt5 * r);
}

// dk/dalpha of the RationalQuadratic: with u = r2 / (2 alpha) and k = variance exp(-alpha log1p(u)), du/dalpha = -u / alpha gives
// k (u / (1 + u) - log1p(u)); the logarithm is the one k itself needs.
__device__ __forceinline__ double kern_dalpha_rq(double r2, double variance, double alpha) {
  const double u = r2 / (2.0 * alpha), l = log1p(u);
  return variance * exp(-alpha * l) * (u / (1.0 + u) - l);
}

}  // namespace
