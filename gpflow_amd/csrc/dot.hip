// Covariance-matrix builder for the dot-product kernels (gpflow/kernels/linears.py: Linear, Polynomial), gfx950.
//
//   Linear      K = (X1 * w) X2^T            w: one weight, or one per input column (ARD);   K_diag_i = sum_j w_j x_ij^2
//   Polynomial  K = (Linear.K + offset)^degree                                                K_diag_i = (Linear.K_diag_i + offset)^degree
//
// With s = sum_j (x_j w_j) y_j and base = s + offset.  The same 64 x 64 tile per 256-thread workgroup as rbf_kernel (rbf.hip), restated
// here with the differences of a dot product: the X1 slab is multiplied by its weight while it is staged (X * variance of the
// reference: one rounding), the X2 slab is staged as it is, no squared norms; the fma chain runs over the input columns ascending.
// The power is a product, base * base * ... left to right (degree in [1, GPK_DOT_MAX_DEGREE], no pow): a negative base comes out as
// the reference's integer power gives it, and the rounding is (degree - 1) u |k| on top of the error of base.
//
// (x_i w) . x_j and (x_j w) . x_i differ in the last bit, so K(X, X) computed element by element is not symmetric.  The symmetric build
// (X2 == NULL) computes the elements on or below the diagonal only and writes each of them to its mirror position as well: its
// output is exactly symmetric, and the lower triangle of a lower_only build is bit for bit that of the full one.  A build with X2
// given promises no symmetry, whatever X2 holds (as the reference's matmul does not).
#include "pair_tile.h"
#include <cmath>

namespace {

struct DotArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double offset, diag_add;
  int degree, sym, lower_only;
  const double* G; long ldg;  // COMB instantiations only: out = G .* k (1), G + k (2), G .* dk/ds (3)
  int comb_diag;              // COMB: X2 is X1 and diag_add goes onto the diagonal of the combined result (ops 1, 2)
  double w[GPK_MAX_D];        // one weight per input column (a single one repeated)
};

using namespace pair_tile;

// base^degree as base * base * ... * base, left to right
__device__ __forceinline__ double dot_power(double base, int degree) {
  double p = base;
  for (int q = 1; q < degree; ++q) p *= base;
  return p;
}

template <int FAMILY>
__device__ __forceinline__ double dot_eval(double s, double offset, int degree) {
  if (FAMILY == GPK_DOT_LINEAR) return s;
  return dot_power(s + offset, degree);
}

// dk/ds (= dk/doffset):  1 (Linear),  degree * base^(degree - 1) (Polynomial; degree 1: exactly 1)
template <int FAMILY>
__device__ __forceinline__ double dot_ds(double s, double offset, int degree) {
  if (FAMILY == GPK_DOT_LINEAR || degree == 1) return 1.0;
  return (double)degree * dot_power(s + offset, degree - 1);
}

// COMB = 0: plain build.  COMB = 1 / 2 / 3: out = G .* k / G + k / G .* dk/ds, G read from memory (may alias the output: every
// element is read and written by the same thread; these never take the symmetric shortcut).  Unlike the stationary op 3 the
// diagonal is NOT zeroed: s_ii = sum_j w_j x_ij^2 depends on the parameters.
template <int FAMILY, int COMB = 0>
__global__ __launch_bounds__(256) void dot_kernel(DotArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int d = p.d;
  double* x1t = sm;                 // [d][T], times the weights
  double* x2t = sm + (size_t)d * T; // [d][T]

  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  if (p.sym && c0 > r0 + T - 1) return;  // strictly upper tile: skipped (lower_only) or written by its mirror
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;

  // stage: padding rows are 0.0; thread t handles (row t / d, column t % d) and on by 256
  for (int e = tid; e < T * d; e += 256) {
    const int row = e / d, dd = e - row * d;
    const int g1 = r0 + row, g2 = c0 + row;
    x1t[dd * T + row] = (g1 < p.n1) ? p.X1[(long)g1 * p.ldx1 + dd] * p.w[dd] : 0.0;
    x2t[dd * T + row] = (g2 < p.n2) ? p.X2[(long)g2 * p.ldx2 + dd] : 0.0;
  }
  __syncthreads();

  double dot[4][4];
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

  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && ((p.ldk & 1) == 0) &&
                    ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      double k = (COMB == 3) ? dot_ds<FAMILY>(dot[i][j], p.offset, p.degree) : dot_eval<FAMILY>(dot[i][j], p.offset, p.degree);
      if (p.sym && gr == gc) k += p.diag_add;
      if constexpr (COMB != 0) {
        const double g = (gr < p.n1 && gc < p.n2) ? p.G[(long)gr * p.ldg + gc] : 0.0;
        k = (COMB == 2) ? k + g : k * g;
        if (COMB != 3 && p.comb_diag && gr == gc) k += p.diag_add;
      }
      v[i][j] = k;
    }
  }
  // The symmetric build keeps the elements on or below the diagonal.  In a diagonal tile: a patch above the diagonal (tx > ty) is
  // written by the mirror of the patch below it, a patch on it (tx == ty) takes its upper entries from its lower ones.
  const bool diag_tile = p.sym && r0 == c0;
  if (diag_tile && tx == ty) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) v[i][j] = v[j][i];
  }
  if (!(diag_tile && tx > ty)) {
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
  }
  const bool mirror = p.sym && (diag_tile ? tx < ty : !p.lower_only);
  if (mirror) {  // transposed copy: rows c0 + tx*4 + j, columns r0 + ty*4 + i   (sym: n1 == n2)
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

// The row diagonal kd_i = k(x_i, x_i): 64 rows per workgroup, staged into LDS as [d][64] with lanes along the contiguous dimension of X;
// thread r < 64 then sums row r over the columns ascending with the builder's own chain fma(x w, x, .), so kd is the diagonal of the
// built K(X, X) bit for bit (diag_add aside).  op 0: out = kd; 1: g .* kd; 2: g + kd; 3: g .* dkd/ds.
struct DotDiagArgs {
  const double* X; long ldx; int n, d;
  double offset; int degree, op;
  const double* g; double* out;
  double w[GPK_MAX_D];
};

template <int FAMILY>
__global__ __launch_bounds__(256) void dot_diag_kernel(DotDiagArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [d][T]
  row_diag(p, sm, [&](double s) { return (p.op == 3) ? dot_ds<FAMILY>(s, p.offset, p.degree) : dot_eval<FAMILY>(s, p.offset, p.degree); });
}

constexpr int DT_THREADS = 1024;
// one workgroup, as adjoint_tail_kernel (train_glue.hip): thread t owns input column t % d and walks the rows t / d, t / d + rpp, ...;
// every partial sum has a fixed set of terms in a fixed order and the partials meet in LDS in thread order -- deterministic, no atomics
__global__ __launch_bounds__(DT_THREADS) void dot_adjoint_tail_kernel(const double* __restrict__ R, long ldr, const double* __restrict__ A,
                                                                      long lda, int n1, int d, const double* __restrict__ w, int ard,
                                                                      int symmetric, double* __restrict__ dsmall,
                                                                      double* __restrict__ Abar, long ldab) {
  __shared__ double sh[DT_THREADS];
  __shared__ double sh_rs[DT_THREADS];
  __shared__ double sh_dim[GPK_MAX_D];
  const int t = threadIdx.x;
  const int rpp = DT_THREADS / d;
  const int c = t % d, r0 = t / d;
  double acc = 0.0, acc_rs = 0.0;
  if (r0 < rpp) {
    const double wc = (symmetric ? 2.0 : 1.0) * w[ard ? c : 0];   // (the factor 2 is exact)
    for (int i = r0; i < n1; i += rpp) {
      const double* Ri = R + (long)i * ldr;
      const double gb = Ri[1 + c];
      acc += A[(long)i * lda + c] * gb;
      Abar[(long)i * ldab + c] = wc * gb;
      if (c == 0) acc_rs += Ri[0];
    }
  }
  sh[t] = acc;
  sh_rs[t] = acc_rs;
  __syncthreads();
  if (t < d) {   // (r0 == 0: this thread's own column)
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh[q * d + t];
    if (ard)
      dsmall[t] = s;
    else
      sh_dim[t] = s;
  }
  if (!ard) __syncthreads();   // (uniform: ard is a kernel argument)
  if (t == 0) {
    if (!ard) {   // one weight for every column: the sum over them, in index order
      double s = 0.0;
      for (int q = 0; q < d; ++q) s += sh_dim[q];
      dsmall[0] = s;
    }
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh_rs[q * d];
    dsmall[ard ? d : 1] = s;
  }
}

template <int FAMILY, int COMB>
int launch_dot(hipStream_t st, const DotArgs& a, size_t lds) {
  GPK_HIP((allow_tile_lds<dot_kernel<FAMILY, COMB>>()));
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((dot_kernel<FAMILY, COMB>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

template <int COMB>
int launch_dot_family(hipStream_t st, int family, const DotArgs& a, size_t lds) {
  return family == GPK_DOT_LINEAR ? launch_dot<GPK_DOT_LINEAR, COMB>(st, a, lds) : launch_dot<GPK_DOT_POLYNOMIAL, COMB>(st, a, lds);
}

// what every entry point checks of a leaf before it looks at the operands; the weights spread over the d columns into `w`
int read_dot_leaf(double* w, int family, int d, const double* w_host, int ard, double offset, int degree) {
  if (d <= 0 || d > GPK_MAX_D || !w_host) return GPK_E_ARG;
  if (family != GPK_DOT_LINEAR && family != GPK_DOT_POLYNOMIAL) return GPK_E_UNSUPPORTED;
  if (!std::isfinite(offset)) return GPK_E_ARG;
  if (family == GPK_DOT_POLYNOMIAL && (degree < 1 || degree > GPK_DOT_MAX_DEGREE)) return GPK_E_ARG;
  return spread_weights(w, d, w_host, ard, /*allow_negative=*/true);
}
}  // namespace

extern "C" int gpk_dot_kernel_matrix(void* stream, int family, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2,
                                     int d, const double* w_host, int ard, double offset, int degree, double diag_add, int lower_only,
                                     double* K, long ldk) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  DotArgs a{};
  GPK_TRY(read_dot_leaf(a.w, family, d, w_host, ard, offset, degree));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldk < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;   // (gpk.h: an operand without elements may be NULL)
  if (!X1 || !K) return GPK_E_ARG;
  const size_t lds = set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, K, ldk, nullptr, 0);
  a.sym = (X2 == nullptr);
  a.offset = offset; a.degree = degree; a.diag_add = diag_add; a.lower_only = lower_only;
  return launch_dot_family<0>((hipStream_t)stream, family, a, lds);
}

extern "C" int gpk_dot_kernel_matrix_combine(void* stream, int family, int op, const double* X1, int n1, long ldx1, const double* X2,
                                             int n2, long ldx2, int d, const double* w_host, int ard, double offset, int degree,
                                             double diag_add, const double* G, long ldg, double* out, long ldo) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  DotArgs a{};
  GPK_TRY(read_dot_leaf(a.w, family, d, w_host, ard, offset, degree));
  if (op < 1 || op > 3) return GPK_E_ARG;
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldg < m2 || ldo < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !G || !out) return GPK_E_ARG;
  const size_t lds = set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, out, ldo, G, ldg);
  a.comb_diag = (X2 == nullptr);
  a.offset = offset; a.degree = degree; a.diag_add = a.comb_diag ? diag_add : 0.0;
  const hipStream_t st = (hipStream_t)stream;
  return op == 1 ? launch_dot_family<1>(st, family, a, lds)
         : op == 2 ? launch_dot_family<2>(st, family, a, lds)
                   : launch_dot_family<3>(st, family, a, lds);
}

extern "C" int gpk_dot_kernel_diag(void* stream, int family, int op, const double* X, int n, long ldx, int d, const double* w_host, int ard,
                                   double offset, int degree, const double* g, double* out) {
  if (n < 0) return GPK_E_ARG;
  DotDiagArgs a{};
  GPK_TRY(read_dot_leaf(a.w, family, d, w_host, ard, offset, degree));
  if (op < 0 || op > 3 || ldx < d) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!X || !out || (op != 0 && !g)) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.offset = offset; a.degree = degree; a.op = op; a.g = g; a.out = out;
  const size_t lds = (size_t)d * T * sizeof(double);   // at most 32 KB
  const dim3 grid((unsigned)gpk_cdiv(n, T));
  if (family == GPK_DOT_LINEAR)
    hipLaunchKernelGGL(dot_diag_kernel<GPK_DOT_LINEAR>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(dot_diag_kernel<GPK_DOT_POLYNOMIAL>, grid, dim3(256), lds, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_dot_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, int d, const double* w_dev,
                                    int ard, int symmetric, double* dsmall, double* Abar, long ldab) {
  if (n1 < 0 || d <= 0 || d > GPK_MAX_D || ldr < 1 + d || lda < d || ldab < d) return GPK_E_ARG;
  if (!w_dev || !dsmall || (n1 > 0 && (!R || !A || !Abar))) return GPK_E_ARG;
  hipLaunchKernelGGL(dot_adjoint_tail_kernel, dim3(1), dim3(DT_THREADS), 0, (hipStream_t)stream, R, ldr, A, lda, n1, d, w_dev, ard, symmetric,
                     dsmall, Abar, ldab);
  GPK_LAUNCH_CHECK();
  return 0;
}
