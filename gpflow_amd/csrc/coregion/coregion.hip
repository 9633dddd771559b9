// The Coregion kernel (gpflow/kernels/misc.py `Coregion`: intrinsic coregionalisation over one column of task labels), gfx950.
//
//   B = W W^T + diag(kappa)  [P, P]          K(x, y) = B[l(x), l(y)]          K_diag(x) = B[l(x), l(x)]
//
// Contract (restated in include/gpk.h):
//  1. LABELS.  l is the row's one column converted as tf.cast(., int32) converts it: truncation toward zero (2.7 -> 2, -0.5 -> 0).  A
//     label is valid when the DOUBLE satisfies -1 < x < P -- tested on the double, before any conversion to an integer (`label_of`).
//     Anything else (NaN, +-Inf, x <= -1, x >= P) is an invalid label and never forms an address.
//  2. THE NaN RULE of the library -- a NaN in row i of X1 makes row i of K NaN and nothing else -- holds for an invalid label: it makes
//     row i of K NaN (in the symmetric build, and for X2, the column as well), kd_i NaN and column i of E NaN, and touches nothing else.
//  3. EXACT ELEMENTS.  K[i, k] has the bits of B[l_i, l_k]; B is exactly symmetric (its products commute and its chains have the same
//     order), so the symmetric build is exactly symmetric WITHOUT a mirror pass, lower_only is bit for bit the lower triangle of the
//     full build, and the row diagonal, read from B, is bit for bit the diagonal of K(X, X).
//
// The tile.  One 64 x 64 tile per 256-thread workgroup, a 4 x 4 patch per thread, the stores of dot_kernel (dot.hip).  The workgroup
// stages B ([P][P], 32 KB at P = 64) and the labels of its 64 rows and 64 columns in LDS; an element is one LDS gather and one global
// store.  No atomics, no environment reads, vector or plain C++ stores only.
#include "../pair_tile.h"
#include "../label.h"   // label_of
#include <cmath>

namespace {

using namespace pair_tile;
constexpr int MAXP = GPK_COREGION_MAX_OUTPUTS;
constexpr int MAXR = GPK_COREGION_MAX_RANK;

struct CoArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;                        // 1: the label column (pair_tile.h's set_operands fills it)
  double* K; long ldk;
  const double* G; long ldg;    // MODE 1 / 2: the other factor / summand
  const double* B; long ldb; int P;
  double diag_add;
  int sym, lower_only;          // MODE 0 with X2 == NULL: diag_add on the diagonal; lower_only: nothing above it is written
  int comb_diag;                // MODE 1 / 2 with X2 == NULL: diag_add goes onto the diagonal of the combined result
};

// MODE 0: the build.  1 / 2: out = G .* k / G + k (out may alias G: an element is read and written by the same thread).
template <int MODE>
__global__ __launch_bounds__(256) void coregion_kernel(CoArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sB[];   // [P][P]
  __shared__ int s_l1[T], s_l2[T];
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const bool low = MODE == 0 && p.lower_only;
  if (low && c0 > r0 + T - 1) return;   // strictly upper tile of a lower_only build
  const int tid = threadIdx.x, P = p.P;
  const int tx = tid & 15, ty = tid >> 4;

  for (int e = tid; e < P * P; e += 256) {
    const int a = e / P, b = e - a * P;
    sB[e] = p.B[(long)a * p.ldb + b];
  }
  if (tid < 2 * T) {   // the labels of the 64 rows (threads 0 .. 63) and of the 64 columns (64 .. 127); padding rows take label 0
    const int r = tid & (T - 1);
    const bool first = tid < T;
    const int g = (first ? r0 : c0) + r;
    const double x = first ? (g < p.n1 ? p.X1[(long)g * p.ldx1] : 0.0) : (g < p.n2 ? p.X2[(long)g * p.ldx2] : 0.0);
    (first ? s_l1 : s_l2)[r] = label_of(x, P);
  }
  __syncthreads();

  int li[4], lk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    li[i] = s_l1[ty * 4 + i];
    lk[i] = s_l2[tx * 4 + i];
  }
  const bool diag_tile = r0 == c0;
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && ((p.ldk & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0) &&
                    !(low && diag_tile);
  const double nan = __builtin_nan("");
  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    const int a = li[i] < 0 ? 0 : li[i];   // (an invalid label reads element 0 of its row / column and is replaced below)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      const int b = lk[j] < 0 ? 0 : lk[j];
      const double g = sB[a * P + b];
      double k = ((li[i] | lk[j]) >= 0) ? g : nan;
      if constexpr (MODE == 0) {
        if (p.sym && gr == gc) k += p.diag_add;
      } else {
        const double gv = (gr < p.n1 && gc < p.n2) ? p.G[(long)gr * p.ldg + gc] : 0.0;
        k = (MODE == 2) ? gv + k : gv * k;
        if (p.comb_diag && gr == gc) k += p.diag_add;
      }
      v[i][j] = k;
    }
  }
  // (the whole patch first, then its stores: with the sixteen elements of G in flight together the fold is 8 % faster than row by row)
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
        if (gc < p.n2 && !(low && gc > gr)) p.K[(long)gr * p.ldk + gc] = v[i][j];
      }
    }
  }
}

// The row diagonal kd_i = B[l_i, l_i], read from B in global memory (one element per row: nothing to stage).
// op 0: out = kd; 1: g .* kd; 2: g + kd.
struct CoDiagArgs {
  const double* X; long ldx; int n;
  const double* B; long ldb; int P;
  int op; const double* g; double* out;
};

__global__ __launch_bounds__(256) void coregion_diag_kernel(CoDiagArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const int l = label_of(p.X[(long)i * p.ldx], p.P);
  const double k = l >= 0 ? p.B[(long)l * p.ldb + l] : __builtin_nan("");
  p.out[i] = (p.op == 0) ? k : (p.op == 2) ? p.g[i] + k : p.g[i] * k;
}

// E[a, i] = (l_i == a), column i NaN for an invalid label; row a is blockIdx.y
struct CoHotArgs {
  const double* X; long ldx; int n, P;
  double* E; long lde;
};

__global__ __launch_bounds__(256) void coregion_onehot_kernel(CoHotArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
  if (i >= p.n) return;
  const int l = label_of(p.X[(long)i * p.ldx], p.P);
  p.E[(long)a * p.lde + i] = l < 0 ? __builtin_nan("") : (l == a ? 1.0 : 0.0);
}

// B = W W^T + diag(kappa): one workgroup, element (a, b) by one thread, an fma chain over r ascending from 0.0.  fma(x, y, acc) and
// fma(y, x, acc) have the same bits, so B[a, b] and B[b, a] do.
struct CoCovArgs {
  const double* W; long ldw; const double* kappa; int P, R;
  double* B; long ldb;
};

__global__ __launch_bounds__(256) void coregion_cov_kernel(CoCovArgs p) {
  for (int e = threadIdx.x; e < p.P * p.P; e += 256) {
    const int a = e / p.P, b = e - a * p.P;
    const double* wa = p.W + (long)a * p.ldw;
    const double* wb = p.W + (long)b * p.ldw;
    double acc = 0.0;
    for (int r = 0; r < p.R; ++r) acc = fma(wa[r], wb[r], acc);
    if (a == b) acc += p.kappa[a];
    p.B[(long)a * p.ldb + b] = acc;
  }
}

// The adjoint tail: one workgroup.  S = Bbar + Bbar^T meets in LDS; dW[a, r] is an fma chain over b ascending of S[a, b] W[b, r], by one
// thread; dkappa = diag(Bbar).  Fixed order, no atomics.
struct CoTailArgs {
  const double* Bbar; long ldbb; const double* W; long ldw; int P, R;
  double* dW; long lddw; double* dkappa;
};

__global__ __launch_bounds__(256) void coregion_adjoint_tail_kernel(CoTailArgs p) {
  __shared__ double S[MAXP * MAXP];
  const int P = p.P, R = p.R;
  for (int e = threadIdx.x; e < P * P; e += 256) {
    const int a = e / P, b = e - a * P;
    S[e] = p.Bbar[(long)a * p.ldbb + b] + p.Bbar[(long)b * p.ldbb + a];
  }
  if (threadIdx.x < P) p.dkappa[threadIdx.x] = p.Bbar[(long)threadIdx.x * p.ldbb + threadIdx.x];
  __syncthreads();
  for (int e = threadIdx.x; e < P * R; e += 256) {
    const int a = e / R, r = e - a * R;
    double acc = 0.0;
    for (int b = 0; b < P; ++b) acc = fma(S[a * P + b], p.W[(long)b * p.ldw + r], acc);
    p.dW[(long)a * p.lddw + r] = acc;
  }
}

template <int MODE>
int launch_coregion(hipStream_t st, const CoArgs& a) {
  GPK_HIP((allow_tile_lds<coregion_kernel<MODE>>()));
  const size_t lds = (size_t)a.P * a.P * sizeof(double);   // at most 32 KB
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((coregion_kernel<MODE>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

int check_outputs(int P) { return (P <= 0 || P > MAXP) ? GPK_E_ARG : 0; }
int check_rank(int R) { return (R <= 0 || R > MAXR) ? GPK_E_ARG : 0; }
}  // namespace

extern "C" int gpk_coregion_output_covariance(void* stream, const double* W, long ldw, const double* kappa, int P, int R, double* B,
                                              long ldb) {
  GPK_TRY(check_outputs(P));
  GPK_TRY(check_rank(R));
  if (ldw < R || ldb < P || !W || !kappa || !B) return GPK_E_ARG;
  CoCovArgs a{W, ldw, kappa, P, R, B, ldb};
  hipLaunchKernelGGL(coregion_cov_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_coregion_kernel_matrix(void* stream, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2,
                                          const double* B, long ldb, int P, double diag_add, int lower_only, double* K, long ldk) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  GPK_TRY(check_outputs(P));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < 1 || (X2 && ldx2 < 1) || ldb < P || ldk < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;   // (gpk.h: an operand without elements may be NULL)
  if (!X1 || !K || !B) return GPK_E_ARG;
  CoArgs a{};
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, 1, K, ldk, nullptr, 0);
  a.B = B; a.ldb = ldb; a.P = P;
  a.sym = (X2 == nullptr);
  a.lower_only = a.sym && lower_only;
  a.diag_add = diag_add;
  return launch_coregion<0>((hipStream_t)stream, a);
}

extern "C" int gpk_coregion_kernel_matrix_combine(void* stream, int op, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                                  long ldx2, const double* B, long ldb, int P, double diag_add, const double* G, long ldg,
                                                  double* out, long ldo) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  GPK_TRY(check_outputs(P));
  if (op < 1 || op > 2) return GPK_E_ARG;
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < 1 || (X2 && ldx2 < 1) || ldb < P || ldg < m2 || ldo < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !G || !out || !B) return GPK_E_ARG;
  CoArgs a{};
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, 1, out, ldo, G, ldg);
  a.B = B; a.ldb = ldb; a.P = P;
  a.comb_diag = (X2 == nullptr);
  a.diag_add = a.comb_diag ? diag_add : 0.0;
  const hipStream_t st = (hipStream_t)stream;
  return op == 1 ? launch_coregion<1>(st, a) : launch_coregion<2>(st, a);
}

extern "C" int gpk_coregion_kernel_diag(void* stream, int op, const double* X, int n, long ldx, const double* B, long ldb, int P,
                                        const double* g, double* out) {
  if (n < 0) return GPK_E_ARG;
  GPK_TRY(check_outputs(P));
  if (op < 0 || op > 2 || ldx < 1 || ldb < P) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!X || !B || !out || (op != 0 && !g)) return GPK_E_ARG;
  CoDiagArgs a{X, ldx, n, B, ldb, P, op, g, out};
  const dim3 grid((unsigned)gpk_cdiv(n, 256));
  hipLaunchKernelGGL(coregion_diag_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_coregion_onehot_rows(void* stream, const double* X, int n, long ldx, int P, double* E, long lde) {
  if (n < 0) return GPK_E_ARG;
  GPK_TRY(check_outputs(P));
  if (ldx < 1 || lde < n) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!X || !E) return GPK_E_ARG;
  CoHotArgs a{X, ldx, n, P, E, lde};
  const dim3 grid((unsigned)gpk_cdiv(n, 256), (unsigned)P);
  hipLaunchKernelGGL(coregion_onehot_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_coregion_adjoint_tail(void* stream, const double* Bbar, long ldbb, const double* W, long ldw, int P, int R, double* dW,
                                         long lddw, double* dkappa) {
  GPK_TRY(check_outputs(P));
  GPK_TRY(check_rank(R));
  if (ldbb < P || ldw < R || lddw < R || !Bbar || !W || !dW || !dkappa) return GPK_E_ARG;
  CoTailArgs a{Bbar, ldbb, W, ldw, P, R, dW, lddw, dkappa};
  hipLaunchKernelGGL(coregion_adjoint_tail_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
