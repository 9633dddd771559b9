// Covariance-matrix builder for stationary kernels (SquaredExponential, Matern family, Exponential, RationalQuadratic) and the
// static ones (White, Constant), gfx950.
//
// Replaces, in ONE pass over the output (the reference materialises >= 6 full N x N2 tensors):
//   Stationary.scale            gpflow/kernels/stationaries.py:77-79      X / lengthscales
//   square_distance             gpflow/utilities/ops.py:105-122           ||x||^2 + ||y||^2 - 2 x.y
//   K_r2 / K_r                  stationaries.py:111-116, 209-210, 254-313  sigma^2 k(r)
//   add_noise_cov / Kuu jitter  utilities/model_utils.py:33-38, covariances/kuus.py:33
//
// HBM-write-bound: 64 x 64 output tile per 256-thread workgroup, the two 64 x D input slabs are
// scaled once, transposed into LDS ([D][64]: each thread then reads its 4 rows / 4 cols with
// ds_read_b128 pairs, conflict free) together with their squared norms; each thread produces a
// 4 x 4 patch and stores 32 contiguous bytes per row (16 threads -> 512 B contiguous per row).
// The expansion formula and the association (-2 x.y) + (|x|^2 + |y|^2) of the reference are kept
// so rounding has the same structure (the diagonal is exp(-0.5 * ~1e-16), not exactly sigma^2).
#include "pair_tile.h"
#include <algorithm>
#include <cmath>

namespace {

struct RbfArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double variance, diag_add;
  int family, sym, lower_only, ard;
  double ls[GPK_MAX_D];
  const double* G; long ldg;  // COMB instantiations only: the output is G .* k(X1, X2) (1) or G + k(X1, X2) (2)
  int comb_diag;              // COMB: X2 is X1 and diag_add goes onto the diagonal of the combined result
  double alpha;               // GPK_KERN_RQ only: the trailing entry of ls_host (gpk.h)
};

using namespace pair_tile;
constexpr int NORMS = 2 * T;   // doubles of LDS behind the slabs: the squared norms of the tile's rows and columns

// Static families (statics.py): no distance -- White is variance on the diagonal of K(X, X) (X2 == NULL) and 0 elsewhere, whatever the
// values of X2; Constant is variance everywhere.  Their tiles never stage or read X.
template <int family>
constexpr bool kern_static = (family == GPK_KERN_WHITE || family == GPK_KERN_CONSTANT);

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

// MIRROR (symmetric full build): only tiles on or below the diagonal are computed; each is also written
// transposed to its mirror position (K(X,X) from the expansion formula is bitwise symmetric: products and the
// two-term sums commute), which halves the fp64 exp/FMA work of what is otherwise a store-bound kernel.
// COMB = 0: plain build.  COMB = 1 / 2: out = G .* k / G + k, the other factor / term G read from memory (may alias
// the output: every element is read and written by the same thread) -- kernel products and sums (kernels/base.py:216-
// 329) and the elementwise factor of the kernel backward, without materialising the second matrix.
// COMB = 3: out = G .* (-2 dk/dr2); with comb_diag (X2 is X1) the diagonal is written as exact zeros: r2_ii = 0 for
// every parameter value, so it carries no gradient (autodiff of the expansion formula gets rounding noise there,
// amplified by 1/r for Matern12).  COMB = 4 (GPK_KERN_RQ only): out = G .* dk/dalpha, diagonal as for COMB = 3.
template <int FAMILY, int COMB = 0>
__global__ __launch_bounds__(256) void rbf_kernel(RbfArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int d = p.d;
  double* x1t = sm;                 // [d][T]
  double* x2t = sm + (size_t)d * T; // [d][T]
  double* nr1 = x2t + (size_t)d * T;  // [T]
  double* nr2 = nr1 + T;              // [T]

  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const bool mirror = p.sym && !p.lower_only;
  if (p.sym && c0 > r0 + T - 1) return;  // strictly upper tile: skipped (lower_only) or written by its mirror
  const int tid = threadIdx.x;

  double dot[4][4];
  const int tx = tid & 15, ty = tid >> 4;
  if constexpr (!kern_static<FAMILY>) {
    // stage + scale (true division, as the reference) -- thread t handles (row t>>2, dims (t&3)::4)
    for (int e = tid; e < T * d; e += 256) {
      const int row = e / d, dd = e - row * d;
      const double l = p.ard ? p.ls[dd] : p.ls[0];
      const int g1 = r0 + row, g2 = c0 + row;
      x1t[dd * T + row] = (g1 < p.n1) ? p.X1[(long)g1 * p.ldx1 + dd] / l : 0.0;
      x2t[dd * T + row] = (g2 < p.n2) ? p.X2[(long)g2 * p.ldx2 + dd] / l : 0.0;
    }
    __syncthreads();
    if (tid < 2 * T) {
      const double* src = (tid < T) ? x1t : x2t;
      const int row = tid & (T - 1);
      double s = 0.0;
      for (int dd = 0; dd < d; ++dd) {
        const double v = src[dd * T + row];
        s += v * v;
      }
      ((tid < T) ? nr1 : nr2)[row] = s;
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dot[i][j] = 0.0;
    for (int dd = 0; dd < d; ++dd) {
      const d2* a2 = reinterpret_cast<const d2*>(&x1t[dd * T + ty * 4]);
      const d2* b2 = reinterpret_cast<const d2*>(&x2t[dd * T + tx * 4]);
      const d2 a01 = a2[0], a23 = a2[1], b01 = b2[0], b23 = b2[1];
      const double a[4] = {a01.x, a01.y, a23.x, a23.y};
      const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dot[i][j] = fma(a[i], b[j], dot[i][j]);
    }
  }  // !kern_static
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && ((p.ldk & 1) == 0) &&
                    ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    double ni = 0.0;
    if constexpr (!kern_static<FAMILY>) ni = nr1[ty * 4 + i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      double k;
      if constexpr (kern_static<FAMILY>) {
        k = (COMB >= 3) ? 0.0
            : (FAMILY == GPK_KERN_CONSTANT || ((p.sym || p.comb_diag) && gr == gc)) ? p.variance : 0.0;
      } else {
        const double r2 = (-2.0 * dot[i][j]) + (ni + nr2[tx * 4 + j]);
        k = (COMB == 4)   ? kern_dalpha_rq(r2, p.variance, p.alpha)
            : (COMB == 3) ? kern_dr2<FAMILY>(r2, p.variance, p.alpha)
                          : kern_eval<FAMILY>(r2, p.variance, p.alpha);
      }
      if (p.sym && gr == gc) k += p.diag_add;
      if constexpr (COMB != 0) {
        const double g = (gr < p.n1 && gc < p.n2) ? p.G[(long)gr * p.ldg + gc] : 0.0;
        k = (COMB == 2) ? k + g : k * g;
        if (p.comb_diag && gr == gc) k = (COMB >= 3) ? 0.0 : k + p.diag_add;
      }
      v[i][j] = k;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    if (full) {
      d2* out = reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + c0 + tx * 4);
      out[0] = (d2){v[i][0], v[i][1]};
      out[1] = (d2){v[i][2], v[i][3]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gc = c0 + tx * 4 + j;
        if (gc < p.n2) p.K[(long)gr * p.ldk + gc] = v[i][j];
      }
    }
  }
  // (full 16384^2 build: mirror tile through LDS 0.479 ms, this register layout 0.422; nt stores 0.455 / 0.429 -- profiles/r02_ab_kernel_builder.log)
  if (mirror && r0 != c0) {  // transposed copy: rows c0 + tx*4 + j, columns r0 + ty*4 + i
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gr = c0 + tx * 4 + j;
      if (full) {
        d2* out = reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + r0 + ty * 4);
        out[0] = (d2){v[0][j], v[1][j]};
        out[1] = (d2){v[2][j], v[3][j]};
      } else if (gr < p.n1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gc = r0 + ty * 4 + i;
          if (gc < p.n2) p.K[(long)gr * p.ldk + gc] = v[i][j];
        }
      }
    }
  }
}

template <int FAMILY, int COMB>
int launch_family(hipStream_t st, const RbfArgs& a, size_t lds) {
  GPK_HIP((allow_tile_lds<rbf_kernel<FAMILY, COMB>, NORMS>()));
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((rbf_kernel<FAMILY, COMB>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

template <int COMB>
int launch_combine(hipStream_t st, int family, const RbfArgs& a, size_t lds) {
  switch (family) {
    case GPK_KERN_SE: return launch_family<GPK_KERN_SE, COMB>(st, a, lds);
    case GPK_KERN_MATERN12: return launch_family<GPK_KERN_MATERN12, COMB>(st, a, lds);
    case GPK_KERN_MATERN32: return launch_family<GPK_KERN_MATERN32, COMB>(st, a, lds);
    case GPK_KERN_MATERN52: return launch_family<GPK_KERN_MATERN52, COMB>(st, a, lds);
    case GPK_KERN_EXPONENTIAL: return launch_family<GPK_KERN_EXPONENTIAL, COMB>(st, a, lds);
    case GPK_KERN_RQ: return launch_family<GPK_KERN_RQ, COMB>(st, a, lds);
    case GPK_KERN_WHITE: return launch_family<GPK_KERN_WHITE, COMB>(st, a, lds);
    case GPK_KERN_CONSTANT: return launch_family<GPK_KERN_CONSTANT, COMB>(st, a, lds);
  }
  return GPK_E_UNSUPPORTED;
}

// the lengthscales and, for GPK_KERN_RQ, the trailing alpha of ls_host (gpk.h) into the kernel's arguments
int read_hypers(RbfArgs& a, int family, const double* ls_host, int ard, int d) {
  const int nls = ard ? d : 1;
  for (int i = 0; i < nls; ++i) a.ls[i] = ls_host[i];
  a.alpha = 1.0;
  if (family == GPK_KERN_RQ) {
    a.alpha = ls_host[nls];
    if (!(a.alpha > 0.0) || !std::isfinite(a.alpha)) return GPK_E_ARG;
  }
  return 0;
}
}  // namespace

extern "C" int gpk_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1,
                                 const double* X2, int n2, long ldx2, int d, const double* ls_host,
                                 int ard, double variance, double diag_add, int lower_only,
                                 double* K, long ldk) {
  // (gpk.h: an operand without elements may be NULL)
  if (!ls_host || n1 < 0 || (X2 && n2 < 0) || d <= 0 || d > GPK_MAX_D) return GPK_E_ARG;
  if (family < GPK_KERN_SE || family > GPK_KERN_CONSTANT) return GPK_E_UNSUPPORTED;
  if (n1 == 0 || (X2 && n2 == 0)) return 0;
  if (!X1 || !K) return GPK_E_ARG;
  RbfArgs a{};
  const size_t lds = set_operands<NORMS>(a, X1, n1, ldx1, X2, n2, ldx2, d, K, ldk, nullptr, 0);
  a.sym = (X2 == nullptr);
  a.variance = variance; a.diag_add = diag_add;
  a.family = family; a.lower_only = lower_only; a.ard = ard;
  if (const int rc = read_hypers(a, family, ls_host, ard, d)) return rc;
  if (a.n1 == 0 || a.n2 == 0) return 0;
  return launch_combine<0>((hipStream_t)stream, family, a, lds);
}

// out = G .* k(X1, X2) (op 1) or G + k(X1, X2) (op 2), k recomputed from the inputs, not read: one read of G and one
// write.  Used for (a) the elementwise factor every kernel-parameter gradient starts from (dF/dtheta = sum_ij Kbar_ij
// dK_ij/dtheta and dK/dtheta = K .* (...) for the stationary families) and (b) Product / Sum kernels
// (gpflow/kernels/base.py:216-220, 283-329): the second factor / term is folded into the first matrix in place.
// X2 == NULL means K(X1, X1); diag_add is then added to the diagonal of the COMBINED result.  No symmetric shortcut.

extern "C" int gpk_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1,
                                         const double* X2, int n2, long ldx2, int d, const double* ls_host, int ard,
                                         double variance, double diag_add, const double* G, long ldg, double* out,
                                         long ldo) {
  if (!ls_host || n1 < 0 || (X2 && n2 < 0) || d <= 0 || d > GPK_MAX_D) return GPK_E_ARG;
  if (family < GPK_KERN_SE || family > GPK_KERN_CONSTANT) return GPK_E_UNSUPPORTED;
  if (op < 1 || op > 4) return GPK_E_ARG;
  if (op == 4 && family != GPK_KERN_RQ) return GPK_E_UNSUPPORTED;
  if (n1 == 0 || (X2 && n2 == 0)) return 0;
  if (!X1 || !G || !out) return GPK_E_ARG;
  RbfArgs a{};
  const size_t lds = set_operands<NORMS>(a, X1, n1, ldx1, X2, n2, ldx2, d, out, ldo, G, ldg);
  a.comb_diag = (X2 == nullptr);
  a.variance = variance; a.diag_add = a.comb_diag ? diag_add : 0.0;
  a.family = family; a.ard = ard;
  if (const int rc = read_hypers(a, family, ls_host, ard, d)) return rc;
  if (a.n1 == 0 || a.n2 == 0) return 0;
  // White against a second set of points is zero: G + 0 in place is G
  if (family == GPK_KERN_WHITE && op == 2 && X2 && out == G && ldo == ldg) return 0;
  if (op == 4) return launch_family<GPK_KERN_RQ, 4>((hipStream_t)stream, a, lds);
  if (op == 3) return launch_combine<3>((hipStream_t)stream, family, a, lds);
  return op == 1 ? launch_combine<1>((hipStream_t)stream, family, a, lds)
                 : launch_combine<2>((hipStream_t)stream, family, a, lds);
}

extern "C" int gpk_kernel_matrix_hadamard(void* stream, int family, const double* X1, int n1, long ldx1,
                                          const double* X2, int n2, long ldx2, int d, const double* ls_host,
                                          int ard, double variance, const double* G, long ldg, double* out,
                                          long ldo) {
  if (n1 < 0 || n2 < 0) return GPK_E_ARG;
  if (n1 == 0 || n2 == 0) return 0;
  if (!X2) return GPK_E_ARG;
  return gpk_kernel_matrix_combine(stream, family, 1, X1, n1, ldx1, X2, n2, ldx2, d, ls_host, ard, variance, 0.0, G, ldg,
                                   out, ldo);
}
