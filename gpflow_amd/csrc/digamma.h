// psi(x) = d/dx log Gamma(x) for x > 0, fp64, host and device: the device math library has none.  Used by the Gamma and Beta
// likelihood codes of varexp.hip (the host evaluates psi(shape) and psi(scale) with the same routine).
#pragma once
#include <math.h>

#ifndef __host__
#define __host__
#define __device__
#endif

// The recurrence psi(x) = psi(x + 1) - 1 / x lifts x to X = x + n >= GPK_DIGAMMA_XMIN, n = ceil(XMIN - x) <= 10 steps; there the
// asymptotic series  log X - 1 / (2 X) - sum_{k = 1 .. 7} B_2k / (2 k X^2k)  is summed (Horner in 1 / X^2).
//
// ABSOLUTE error bound, u = 2^-53.  (A relative bound is meaningless: psi has a root at 1.4616...)
//   * recurrence: each x_i = x + i is ONE rounded addition from the original x (relative u), each quotient 1 / x_i is correctly
//     rounded (relative u): 2 u / x_i per term.  The n additions of the running sum round to u times a partial sum <= S =
//     sum_i 1 / x_i each.  Together (2 + n) u S <= 12 u S,  and  S <= 1 / x + (1 + 1/2 + ... + 1/9) < 1 / x + 2.83:
//         12 u / x + 34 u
//   * truncation: the series is enveloping, so the remainder is below the first dropped term |B_16| / (16 X^16) = 0.4433 / X^16
//     <= 4.5e-17 < 0.41 u at X >= 10.
//   * log X: the library's stated limit is 3 ulp (OpenCL fp64), X carries one rounding (u in the logarithm): (4 |log X| + 1) u.
//   * 1 / (2 X) and the Horner sum are below 0.051 in magnitude; their ten operations add less than u.
//   * the three final subtractions: the first two round to u (|log X| + 0.06) each, the last to u |psi(x)| <= u (1 / x + |log X| +
//     0.06):  u / x + 3 |log X| u + 0.2 u.
//   Sum:  u (13 / x + 7 log X + 34 + 0.41 + 1 + 1 + 0.2)  <=  u (GPK_DIGAMMA_BOUND_RECIP / x + GPK_DIGAMMA_BOUND_LOG log(x + 10)
//   + GPK_DIGAMMA_BOUND_CONST), using log X <= log(x + 10).  For x >= XMIN there is no recurrence and the same expression holds
//   with room.  The tests read the three constants from this file.
#define GPK_DIGAMMA_XMIN 10.0
#define GPK_DIGAMMA_BOUND_RECIP 13.0
#define GPK_DIGAMMA_BOUND_LOG 8.0
#define GPK_DIGAMMA_BOUND_CONST 40.0

__host__ __device__ inline double gpk_digamma(double x) {
  double s = 0.0;
  int n = 0;
  for (; x + (double)n < GPK_DIGAMMA_XMIN; ++n) s += 1.0 / (x + (double)n);
  const double X = x + (double)n;
  const double r = 1.0 / X, t = r * r;
  // B_2k / (2 k), k = 1 .. 7:  1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
  const double h = t * (1.0 / 12 - t * (1.0 / 120 - t * (1.0 / 252 - t * (1.0 / 240 - t * (1.0 / 132 - t * (691.0 / 32760 - t * (1.0 / 12)))))));
  return (log(X) - 0.5 * r - h) - s;
}

// the bound derived above, for a caller that wants it next to a value
__host__ __device__ inline double gpk_digamma_abs_bound(double x) {
  return 1.1102230246251565e-16 * (GPK_DIGAMMA_BOUND_RECIP / x + GPK_DIGAMMA_BOUND_LOG * log(x + 10.0) + GPK_DIGAMMA_BOUND_CONST);
}
