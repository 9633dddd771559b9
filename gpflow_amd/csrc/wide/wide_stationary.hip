// Covariance builder of the stationary families for WIDE inputs, 1 <= d <= GPK_WIDE_MAX_D columns (gpk_wide_kernel_matrix,
// gpk_wide_kernel_matrix_combine: include/gpk.h), gfx950.  rbf.hip stages both whole d-column slabs of a 64 x 64 tile in LDS and
// does its d products per element on the VALU: right for d ~ 1 .. 16, where the build is bound by its stores, and impossible past
// d = 64.  At d = 65 .. 1024 the build is a GEMM with a transcendental epilogue (2 d flops per element against 8 bytes written):
// this file puts the dot products on the fp64 matrix pipe and walks the columns in slabs.
//
// The tile -- work split, K loop, LDS layout, norms, symmetric build -- is wide_tile.h's; this file brings the value arithmetic of the
// stationary families and the two entry points.
//
// Staging.  Each value is divided by its lengthscale -- TRUE division, as rbf.hip and the reference, so r2 keeps the rounding
// structure of X / ls; a column past d has a divisor of 1.0.  The squared norms are accumulated from the SCALED values.
//
// Epilogue, in the accumulator registers: r2 = (-2 dot) + (n_i + n_j) (rbf.hip's association), the profiles of kern_profile.h,
// diag_add / the COMB ops / the by-index zero diagonal / the NaN rule exactly as rbf_kernel has them.
#include "wide_tile.h"
#include "../kern_profile.h"
#include <cmath>

namespace {

using namespace wide_tile;

struct WideArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double variance, diag_add, alpha;
  int sym, lower_only, ard;
  const double* ls;           // DEVICE: d entries if ard, else one
  const double* G; long ldg;  // COMB instantiations only
  int comb_diag;              // COMB: X2 is X1 and diag_add goes onto the diagonal of the combined result
};

// what the tile of wide_tile.h does to values here: x / l (true division), both operands scaled, |x / l|^2 summed as it is
#define WIDE_STAGE(x, l) ((x) / (l))
#define WIDE_SECOND(staged, raw) (staged)
#define WIDE_NORM_TERM(staged, raw, acc) fma(staged, staged, acc)
#define WIDE_NORM_FINISH(sum) nrm[tid] = (sum)
#define WIDE_SYM p.sym
#define WIDE_SCALES p.ls
#define WIDE_FIRST_PHASE (tid % TPR)
#define WIDE_PARTIAL_OF(e) 0

// COMB as rbf_kernel: 0 plain build; 1 / 2: out = G .* k / G + k; 3: G .* (-2 dk/dr2); 4 (GPK_KERN_RQ): G .* dk/dalpha.
template <int T, int FAMILY, int COMB>
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(256) void wide_kernel(const WideArgs p) {
  constexpr int NPH = Geo<T>::TPR;   // ONE norm partial per staging thread: TPR phases of EPT columns (2 x 8 at T = 128, 4 x 4 at T = 64)
  constexpr double PAD = 1.0;
  constexpr bool BUILD = COMB == 0;
#include "wide_tile_front.inc"
  double nj[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) nj[j] = nrm[T + tc0 + j];
  bool gvec = false;   // (wide_tile_gread.inc)
  if constexpr (!BUILD) gvec = full && ((p.ldg & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.G) & 15) == 0);

  // one row of this lane's block: the NB values of global row r0 + tr, accumulator row g of block row i
  auto row_values = [&](int i, int g, int tr, double* out) {
    const int gr = r0 + tr;
    const double ni = nrm[tr];
#include "wide_tile_gread.inc"
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int gc = c0 + tc0 + j;
      const double r2 = (-2.0 * acc[i][j][g]) + (ni + nj[j]);
      double k = (COMB == 4)   ? kern_dalpha_rq(r2, p.variance, p.alpha)
                 : (COMB == 3) ? kern_dr2<FAMILY>(r2, p.variance, p.alpha)
                               : kern_eval<FAMILY>(r2, p.variance, p.alpha);
      if (p.sym && gr == gc) k += p.diag_add;
      if constexpr (COMB != 0) {
        k = (COMB == 2) ? k + gv[j] : k * gv[j];
        if (p.comb_diag && gr == gc) k = (COMB >= 3) ? 0.0 : k + p.diag_add;
      }
      out[j] = k;
    }
  };
#include "wide_tile_rows.inc"
}

template <int FAMILY, int COMB>
int launch_family(hipStream_t st, const WideArgs& a) {
  int cus = 0;
  GPK_TRY(compute_units(&cus));
  return tile_size(a.n1, a.n2, a.sym != 0, cus) == 128 ? launch_tile<wide_kernel<128, FAMILY, COMB>, 128>(st, a)
                                                      : launch_tile<wide_kernel<64, FAMILY, COMB>, 64>(st, a);
}

template <int COMB>
int launch_combine(hipStream_t st, int family, const WideArgs& a) {
  switch (family) {
    case GPK_KERN_SE: return launch_family<GPK_KERN_SE, COMB>(st, a);
    case GPK_KERN_MATERN12: return launch_family<GPK_KERN_MATERN12, COMB>(st, a);
    case GPK_KERN_MATERN32: return launch_family<GPK_KERN_MATERN32, COMB>(st, a);
    case GPK_KERN_MATERN52: return launch_family<GPK_KERN_MATERN52, COMB>(st, a);
    case GPK_KERN_EXPONENTIAL: return launch_family<GPK_KERN_EXPONENTIAL, COMB>(st, a);
    case GPK_KERN_RQ: return launch_family<GPK_KERN_RQ, COMB>(st, a);
  }
  return GPK_E_UNSUPPORTED;
}

// what both entry points answer before they look at op, G or K: 0 to go on, 1 for "nothing to do", or the refusal
int check_operands(WideArgs& a, int family, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d,
                   const double* ls_dev, int ard, double alpha, double variance) {
  if (!ls_dev || n1 < 0 || (X2 && n2 < 0) || d <= 0 || d > GPK_WIDE_MAX_D) return GPK_E_ARG;
  if (family < GPK_KERN_SE || family > GPK_KERN_RQ) return GPK_E_UNSUPPORTED;   // (White, Constant: gpk_kernel_matrix, they never read X)
  if (family == GPK_KERN_RQ && (!(alpha > 0.0) || !std::isfinite(alpha))) return GPK_E_ARG;
  if (n1 == 0 || (X2 && n2 == 0)) return 1;
  if (!X1 || (n1 > 1 && ldx1 < d) || (X2 && n2 > 1 && ldx2 < d)) return GPK_E_ARG;
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d);
  a.ls = ls_dev; a.ard = ard;
  a.alpha = (family == GPK_KERN_RQ) ? alpha : 1.0;
  a.variance = variance;
  return 0;
}

}  // namespace

extern "C" int gpk_wide_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                      long ldx2, int d, const double* ls_dev, int ard, double alpha, double variance,
                                      double diag_add, int lower_only, double* K, long ldk) {
  WideArgs a{};
  const int rc = check_operands(a, family, X1, n1, ldx1, X2, n2, ldx2, d, ls_dev, ard, alpha, variance);
  if (rc) return rc < 0 ? rc : 0;
  if (!K || (a.n1 > 1 && ldk < a.n2)) return GPK_E_ARG;
  a.K = K; a.ldk = ldk;
  a.sym = (X2 == nullptr);
  a.diag_add = diag_add; a.lower_only = lower_only;
  return launch_combine<0>((hipStream_t)stream, family, a);
}

extern "C" int gpk_wide_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1,
                                              const double* X2, int n2, long ldx2, int d, const double* ls_dev, int ard,
                                              double alpha, double variance, double diag_add, const double* G, long ldg,
                                              double* out, long ldo) {
  WideArgs a{};
  const int rc = check_operands(a, family, X1, n1, ldx1, X2, n2, ldx2, d, ls_dev, ard, alpha, variance);
  if (rc < 0) return rc;
  if (op < 1 || op > 4) return GPK_E_ARG;
  if (op == 4 && family != GPK_KERN_RQ) return GPK_E_UNSUPPORTED;
  if (rc) return 0;
  if (!G || !out || (a.n1 > 1 && (ldg < a.n2 || ldo < a.n2))) return GPK_E_ARG;
  a.K = out; a.ldk = ldo; a.G = G; a.ldg = ldg;
  a.comb_diag = (X2 == nullptr);
  a.diag_add = a.comb_diag ? diag_add : 0.0;
  hipStream_t st = (hipStream_t)stream;
  if (op == 4) return launch_family<GPK_KERN_RQ, 4>(st, a);
  if (op == 3) return launch_combine<3>(st, family, a);
  return op == 1 ? launch_combine<1>(st, family, a) : launch_combine<2>(st, family, a);
}
