// The Periodic kernel's input warp  Phi(x) = (cos a_1, sin a_1, ..., cos a_d, sin a_d),  a_j = 2 pi x_j / p_j,  and its adjoint.
//   || Phi_j(x) - Phi_j(x') ||^2 = 4 sin^2(pi (x_j - x'_j) / p_j):  a stationary kernel on Phi(X) [n, 2 d] with the lengthscales doubled is
// the Periodic kernel over that base, so the covariance builder, the fused drivers and the stationary adjoint run unchanged at width
// 2 d.  The warp costs (rows) * d sincospi; a sin per pair inside the builder would cost n1 * n2 * d.
#include "gpk_internal.h"
#include <cmath>

namespace {
constexpr int PERIODIC_MAX_D = GPK_MAX_D / 2;

struct Periods {
  double p[PERIODIC_MAX_D];
};

// (cos, sin)(2 pi x / p): the quotient carries the one rounding in front of sincospi; no product with pi is formed, and x = k p gives
// exactly (1, 0).  The warp and the moment rows share this function: their entries are bit-identical.
__device__ __forceinline__ void warp_pair(double x, double p, double& c, double& s) { sincospi(2.0 * x / p, &s, &c); }

__global__ __launch_bounds__(256) void periodic_warp_kernel(const double* __restrict__ X, long ldx, int n, int d, Periods per,
                                                            double* __restrict__ Phi, long ldphi) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;   // one (row, dimension) entry of X
  if (e >= (long)n * d) return;
  const long i = e / d;
  const int j = (int)(e - i * d);
  double c, s;
  warp_pair(X[i * ldx + j], per.p[j], c, s);
  Phi[i * ldphi + 2 * j] = c;
  Phi[i * ldphi + 2 * j + 1] = s;
}

// rows of Vt [1 + 6 d, n2]:  1 | Phi(B)^T (2 d) | (Phi(B)^2)^T (2 d) | (b cos)^T, (b sin)^T interleaved as Phi is (2 d)
__global__ __launch_bounds__(256) void periodic_moment_rows_kernel(const double* __restrict__ B, long ldb, int n2, int d, Periods per,
                                                                   double* __restrict__ Vt, long ldv) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2) return;
  Vt[j] = 1.0;
  for (int q = 0; q < d; ++q) {
    const double b = B[(long)j * ldb + q];
    double c, s;
    warp_pair(b, per.p[q], c, s);
    Vt[(long)(1 + 2 * q) * ldv + j] = c;
    Vt[(long)(2 + 2 * q) * ldv + j] = s;
    Vt[(long)(1 + 2 * d + 2 * q) * ldv + j] = c * c;
    Vt[(long)(2 + 2 * d + 2 * q) * ldv + j] = s * s;
    Vt[(long)(1 + 4 * d + 2 * q) * ldv + j] = b * c;
    Vt[(long)(2 + 4 * d + 2 * q) * ldv + j] = b * s;
  }
}

constexpr int PT_THREADS = 1024;
// one workgroup, as adjoint_tail_kernel (train_glue.hip): thread t owns input dimension t % d and walks the rows t / d, t / d + rpp, ...;
// every partial sum has a fixed set of terms in a fixed order and the partials meet in LDS in thread order -- deterministic, no atomics
__global__ __launch_bounds__(PT_THREADS) void periodic_adjoint_tail_kernel(const double* __restrict__ X, long ldx, const double* __restrict__ Phi,
                                                                           long ldphi, const double* __restrict__ Phibar, long ldpb,
                                                                           const double* __restrict__ R, long ldr, int n1, int d,
                                                                           const double* __restrict__ ls, Periods per, int ard_period,
                                                                           double* __restrict__ Xbar, long ldxb, double* __restrict__ dperiod,
                                                                           int accumulate) {
  __shared__ double sh[PT_THREADS];
  __shared__ double sh_dim[PERIODIC_MAX_D];
  const int t = threadIdx.x;
  const int rpp = PT_THREADS / d;
  const int c = t % d, r0 = t / d;
  double acc = 0.0;
  if (r0 < rpp) {
    const double w = 2.0 * M_PI / per.p[c];
    for (int i = r0; i < n1; i += rpp) {
      const double x = X[(long)i * ldx + c];
      const double cs = Phi[(long)i * ldphi + 2 * c], sn = Phi[(long)i * ldphi + 2 * c + 1];
      const double bc = Phibar[(long)i * ldpb + 2 * c], bs = Phibar[(long)i * ldpb + 2 * c + 1];
      const double* Ri = R + (long)i * ldr;
      const double gc = Ri[1 + 2 * c], gs = Ri[2 + 2 * c], gbc = Ri[1 + 4 * d + 2 * c], gbs = Ri[2 + 4 * d + 2 * c];
      const double xb = w * (cs * bs - sn * bc);
      double* o = Xbar + (long)i * ldxb + c;
      *o = accumulate ? *o + xb : xb;
      acc += x * (sn * gc - cs * gs) + (cs * gbs - sn * gbc);
    }
  }
  sh[t] = acc;
  __syncthreads();
  if (t < d) {   // (r0 == 0: this thread's own dimension)
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh[q * d + t];
    const double p = per.p[t], l = ls[t];
    const double r = s * (M_PI / (2.0 * p * p * l * l));
    if (ard_period)
      dperiod[t] = accumulate ? dperiod[t] + r : r;
    else
      sh_dim[t] = r;
  }
  if (!ard_period) {   // one period for every dimension: the sum over them, in index order
    __syncthreads();
    if (t == 0) {
      double r = 0.0;
      for (int q = 0; q < d; ++q) r += sh_dim[q];
      dperiod[0] = accumulate ? dperiod[0] + r : r;
    }
  }
}

// the periods of the C-ABI (d entries if ard_period, else one) spread over the d dimensions; GPK_E_ARG for one that is not positive and finite
int read_periods(Periods& per, const double* period_host, int ard_period, int d) {
  if (!period_host) return GPK_E_ARG;
  for (int j = 0; j < d; ++j) {
    const double p = period_host[ard_period ? j : 0];
    if (!(p > 0.0) || !std::isfinite(p)) return GPK_E_ARG;
    per.p[j] = p;
  }
  for (int j = d; j < PERIODIC_MAX_D; ++j) per.p[j] = 1.0;
  return 0;
}
}  // namespace

extern "C" int gpk_periodic_warp(void* stream, const double* X, long ldx, int n, int d, const double* period_host, int ard_period,
                                 double* Phi, long ldphi) {
  if (n < 0 || d <= 0 || d > PERIODIC_MAX_D || ldx < d || ldphi < 2 * d) return GPK_E_ARG;
  Periods per;
  GPK_TRY(read_periods(per, period_host, ard_period, d));
  if (n == 0) return 0;
  if (!X || !Phi) return GPK_E_ARG;
  const long blocks = ((long)n * d + 255) / 256;   // (d <= 32: below 2^28)
  hipLaunchKernelGGL(periodic_warp_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X, ldx, n, d, per, Phi, ldphi);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_periodic_moment_rows(void* stream, const double* B, long ldb, int n2, int d, const double* period_host, int ard_period,
                                        double* Vt, long ldv) {
  if (n2 < 0 || d <= 0 || d > PERIODIC_MAX_D || ldb < d || ldv < n2) return GPK_E_ARG;
  Periods per;
  GPK_TRY(read_periods(per, period_host, ard_period, d));
  if (n2 == 0) return 0;
  if (!B || !Vt) return GPK_E_ARG;
  hipLaunchKernelGGL(periodic_moment_rows_kernel, dim3((unsigned)gpk_cdiv(n2, 256)), dim3(256), 0, (hipStream_t)stream, B, ldb, n2, d, per,
                     Vt, ldv);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_periodic_adjoint_tail(void* stream, const double* X, long ldx, const double* Phi, long ldphi, const double* Phibar,
                                         long ldpb, const double* R, long ldr, int n1, int d, const double* ls_dev,
                                         const double* period_host, int ard_period, double* Xbar, long ldxb, double* dperiod,
                                         int accumulate) {
  if (n1 < 0 || d <= 0 || d > PERIODIC_MAX_D || ldx < d || ldphi < 2 * d || ldpb < 2 * d || ldr < 1 + 6 * d || ldxb < d) return GPK_E_ARG;
  Periods per;
  GPK_TRY(read_periods(per, period_host, ard_period, d));
  if (!ls_dev || !dperiod || (n1 > 0 && (!X || !Phi || !Phibar || !R || !Xbar))) return GPK_E_ARG;
  hipLaunchKernelGGL(periodic_adjoint_tail_kernel, dim3(1), dim3(PT_THREADS), 0, (hipStream_t)stream, X, ldx, Phi, ldphi, Phibar, ldpb, R, ldr,
                     n1, d, ls_dev, per, ard_period, Xbar, ldxb, dperiod, accumulate);
  GPK_LAUNCH_CHECK();
  return 0;
}
