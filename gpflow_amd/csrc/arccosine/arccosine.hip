// The ArcCosine kernel (gpflow/kernels/misc.py: the neural-network covariance of Cho & Saul), gfx950.
//
//   s(x, y) = sum_j (x_j w_j) y_j + b          p(x) = s(x, x)            (w: weight_variances, one or one per column; b: bias_variance)
//   c  = s / (sqrt p(x) sqrt p(y))             theta = acos(clamp(eps + (1 - 2 eps) c)),   eps = 1e-15
//   J_0 = pi - theta    J_1 = sin theta + (pi - theta) cos theta    J_2 = 3 sin theta cos theta + (pi - theta)(1 + 2 cos^2 theta)
//   K(x, y)   = (v / pi) J_order(theta) p(x)^(order/2) p(y)^(order/2)
//   K_diag(x) = v (J_order(0) / pi) p(x)^order                           (J(0) / pi = 1, 1, 3)
//
// Contract (restated in include/gpk.h):
//  1. DIAGONAL BY INDEX.  Where X2 is NULL the element (i, i) takes c = 1 because its row index equals its column index, never
//     because two values compare equal: the acos argument there is the double 1.0 - 1e-15, its value is
//     (v / pi) J(acos(1 - eps)) p_i^order, and in the adjoint stage its angular derivative is zero -- only p_i^order differentiates.
//     (Evaluated from the data, acos sits at 1 - eps plus rounding noise: theta ~ 4.5e-8 +- 15 %, with d theta / dc = 2.2e7.)
//     K_diag stays the closed form above and is NOT the diagonal of K(X, X) bit for bit (1.4e-8 apart, relatively, at order 0).
//  2. RANGE.  Rounding in s can push |c| past 1 by more than eps: the argument is clamped to [-1, 1] by two comparisons, which are
//     false for a NaN, so a NaN or Inf in a row of X1 / X2 makes exactly that row / column of K NaN.
//  3. NO SINGULAR FORMS.  With cos theta = the clamped argument and sin theta = sqrt((1 - cos)(1 + cos)) the kernel needs acos and sqrt
//     only.  (dJ/dtheta)(dtheta/d arg) = 1 / sin theta (order 0), pi - theta (order 1), 4 J_1(theta) (order 2).  Order 0 is singular
//     where the argument is +-1 (two proportional rows in different positions): the reference's gradient is infinite there as well.
//
// Arithmetic.  The same 64 x 64 tile per 256-thread workgroup as dot_kernel (dot.hip).  Both slabs are staged RAW, [d][64] each (64 KB at
// d = GPK_MAX_D); x_j w_j is formed in registers (one rounding, as X * w of the reference), the sum over j is an fma chain over ascending
// columns from 0.0, and b is added last.  p of the tile's 64 rows and of its 64 columns comes from the staged slabs with the same chain
// fma(x_j w_j, x_j, .): no second pass over X, no norm vectors in global memory, and p of row i as a row equals p of row i as a column
// bit for bit.  The symmetric build computes the elements on or below the diagonal and mirrors them (exactly symmetric; lower_only is bit
// for bit the lower triangle of the full build).
#include "../pair_tile.h"
#include <cmath>

namespace {

using namespace pair_tile;
static_assert(T == GPK_ARC_TILE, "include/gpk.h states the tile of the adjoint stage's partials");
constexpr double ARC_EPS = 1e-15;
constexpr double ARC_SCALE = 1.0 - 2.0 * ARC_EPS;
constexpr double ARC_CT_DIAG = 1.0 - ARC_EPS;   // the acos argument of a diagonal element taken by index
constexpr double ARC_PI = 3.14159265358979323846;
constexpr double ARC_INV_PI = 1.0 / ARC_PI;

struct ArcArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double vpi, bias, diag_add;   // vpi = variance / pi
  int sym, lower_only;          // the mirrored build (MODE 0 with X2 == NULL)
  int same;                     // X2 is X1: the diagonal takes c = 1 by index
  const double* G; long ldg;    // MODE 1 / 2: the other factor / summand; MODE 3: Kbar
  int comb_diag;                // MODE 1 / 2 with X2 == NULL: diag_add goes onto the diagonal of the combined result
  double* parts; int tr, tc;    // MODE 3: the partials and the tile counts that lay them out
  double w[GPK_MAX_D];
};

// J_ORDER at cos theta = ct, and D = dJ / d(acos argument)
template <int ORDER, bool WANT_D>
__device__ __forceinline__ void arc_eval(double ct, double& J, double& D) {
  const double pt = ARC_PI - acos(ct);
  if (ORDER == 0) {
    J = pt;
    if (WANT_D) D = 1.0 / sqrt((1.0 - ct) * (1.0 + ct));
    return;
  }
  const double sn = sqrt((1.0 - ct) * (1.0 + ct));
  const double J1 = sn + pt * ct;
  if (ORDER == 1) {
    J = J1;
    D = pt;
  } else {
    J = 3.0 * sn * ct + pt * (1.0 + 2.0 * ct * ct);
    D = 4.0 * J1;
  }
}

// MODE 0: the build.  1 / 2: out = G .* k / G + k (out may alias G: an element is read and written by the same thread).
// 3: the adjoint stage -- out = Kbar .* dk/ds and the tile's partial sums of Kbar .* dk/dp (by row), Kbar .* dk/dq (by column) and
// Kbar .* k / v.  Modes 1 - 3 never mirror.
template <int ORDER, int MODE>
__global__ __launch_bounds__(256) void arccos_kernel(ArcArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double s_p[T], s_q[T], s_rp[T], s_rq[T];
  const int d = p.d;
  double* x1t = sm;                 // [d][T]
  double* x2t = sm + (size_t)d * T; // [d][T]

  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  if (MODE == 0 && p.sym && c0 > r0 + T - 1) return;  // strictly upper tile: skipped (lower_only) or written by its mirror
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;

  for (int e = tid; e < T * d; e += 256) {   // padding rows are 0.0: p = b there
    const int row = e / d, dd = e - row * d;
    const int g1 = r0 + row, g2 = c0 + row;
    x1t[dd * T + row] = (g1 < p.n1) ? p.X1[(long)g1 * p.ldx1 + dd] : 0.0;
    x2t[dd * T + row] = (g2 < p.n2) ? p.X2[(long)g2 * p.ldx2 + dd] : 0.0;
  }
  __syncthreads();

  if (tid < 2 * T) {   // p of the 64 rows (threads 0 .. 63) and of the 64 columns (64 .. 127), with the builder's chain
    const int r = tid & (T - 1);
    const double* xs = tid < T ? x1t : x2t;
    double acc = 0.0;
    for (int dd = 0; dd < d; ++dd) {
      const double x = xs[dd * T + r];
      acc = fma(x * p.w[dd], x, acc);
    }
    const double pv = acc + p.bias;
    (tid < T ? s_p : s_q)[r] = pv;
    (tid < T ? s_rp : s_rq)[r] = sqrt(pv);
  }

  double dot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dot[i][j] = 0.0;
  for (int dd = 0; dd < d; ++dd) {
    const d2* a2 = reinterpret_cast<const d2*>(&x1t[dd * T + ty * 4]);
    const d2* b2 = reinterpret_cast<const d2*>(&x2t[dd * T + tx * 4]);
    const d2 a01 = a2[0], a23 = a2[1], b01 = b2[0], b23 = b2[1];
    const double wd = p.w[dd];
    const double a[4] = {a01.x * wd, a01.y * wd, a23.x * wd, a23.y * wd};
    const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dot[i][j] = fma(a[i], b[j], dot[i][j]);
  }
  __syncthreads();   // s_p .. s_rq

  double pr[4], rpr[4], qc[4], rqc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pr[i] = s_p[ty * 4 + i];
    rpr[i] = s_rp[ty * 4 + i];
    qc[i] = s_q[tx * 4 + i];
    rqc[i] = s_rq[tx * 4 + i];
  }

  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && ((p.ldk & 1) == 0) &&
                    ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  double v[4][4];
  double rs[4] = {0.0, 0.0, 0.0, 0.0}, cs[4] = {0.0, 0.0, 0.0, 0.0}, ks[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      const bool ondiag = p.same && gr == gc;
      const double rr = rpr[i] * rqc[j];
      const double c = (dot[i][j] + p.bias) / rr;
      const double arg = fma(ARC_SCALE, c, ARC_EPS);
      double ct = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);   // (both comparisons are false for a NaN: it passes)
      if (ondiag) ct = fma(rr, 0.0, ARC_CT_DIAG);   // the constant, or the NaN of a row that holds a NaN or an Inf
      double J, D = 0.0;
      arc_eval<ORDER, MODE == 3>(ct, J, D);
      const double m = ORDER == 0 ? 1.0 : ORDER == 1 ? rr : pr[i] * qc[j];
      const double jm = J * m;
      double k = p.vpi * jm;
      if constexpr (MODE == 0) {
        if (p.sym && gr == gc) k += p.diag_add;
      } else if constexpr (MODE == 1 || MODE == 2) {
        const double g = (gr < p.n1 && gc < p.n2) ? p.G[(long)gr * p.ldg + gc] : 0.0;
        k = (MODE == 2) ? k + g : k * g;
        if (p.comb_diag && gr == gc) k += p.diag_add;
      } else {
        const bool in = gr < p.n1 && gc < p.n2;
        const double g = in ? p.G[(long)gr * p.ldg + gc] : 0.0;
        if (ondiag) D = 0.0;                                   // by index: no angular derivative
        const double sd = ARC_SCALE * D;
        const double h = 0.5 * p.vpi * ((double)ORDER * J - sd * (ondiag ? 1.0 : c));
        const double dks = ORDER == 0 ? p.vpi * sd / rr : ORDER == 1 ? p.vpi * sd : p.vpi * sd * rr;
        const double dkp = ORDER == 0 ? h / pr[i] : ORDER == 1 ? h * rqc[j] / rpr[i] : h * qc[j];
        const double dkq = ORDER == 0 ? h / qc[j] : ORDER == 1 ? h * rpr[i] / rqc[j] : h * pr[i];
        k = g * dks;
        rs[i] += in ? g * dkp : 0.0;     // (a padding element never enters a sum: its derivative may be infinite)
        cs[j] += in ? g * dkq : 0.0;
        ks[i] += in ? g * jm : 0.0;
      }
      v[i][j] = k;
    }
  }
  // The symmetric build keeps the elements on or below the diagonal.  In a diagonal tile: a patch above the diagonal (tx > ty) is
  // written by the mirror of the patch below it, a patch on it (tx == ty) takes its upper entries from its lower ones.
  const bool sym = MODE == 0 && p.sym;
  const bool diag_tile = sym && r0 == c0;
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
  const bool mirror = sym && (diag_tile ? tx < ty : !p.lower_only);
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

  if constexpr (MODE == 3) {
    // The tile's partial sums, each by ONE thread in a fixed order: a thread's four elements left to right (above), then the sixteen
    // threads of a row (column) in ascending tx (ty); the tile's sum of Kbar .* k / v adds its 64 row sums in row order.  Slots:
    //   parts[bx * n1 + i]                       row i's sum over the columns of column tile bx    (rho)
    //   parts[tc * n1 + by * n2 + k]             column k's sum over the rows of row tile by       (gamma)
    //   parts[tc * n1 + tr * n2 + by * tc + bx]  the tile's sum of Kbar .* J m                     (d/dvariance, times 1 / pi in the tail)
    __shared__ double red_r[T * 16], red_c[T * 16], red_k[T * 16], s_k[T];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red_r[(ty * 4 + i) * 16 + tx] = rs[i];
      red_k[(ty * 4 + i) * 16 + tx] = ks[i];
      red_c[(tx * 4 + i) * 16 + ty] = cs[i];
    }
    __syncthreads();
    const int r = tid & (T - 1);
    if (tid < 3 * T) {
      const double* src = tid < T ? red_r : tid < 2 * T ? red_c : red_k;
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc += src[r * 16 + q];
      if (tid < T) {
        if (r0 + r < p.n1) p.parts[(long)blockIdx.x * p.n1 + r0 + r] = acc;
      } else if (tid < 2 * T) {
        if (c0 + r < p.n2) p.parts[(long)p.tc * p.n1 + (long)blockIdx.y * p.n2 + c0 + r] = acc;
      } else {
        s_k[r] = acc;
      }
    }
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int q = 0; q < T; ++q) acc += s_k[q];
      p.parts[(long)p.tc * p.n1 + (long)p.tr * p.n2 + (long)blockIdx.y * p.tc + blockIdx.x] = acc;
    }
  }
}

// The row diagonal, the closed form: kd_i = v jf p_i^order with jf = J_order(0) / pi = 1, 1, 3; pair_tile.h's row_diag, p_i by the
// builder's chain.  op 0: out = kd; 1: g .* kd; 2: g + kd; 3: g .* dkd/dp.  Order 0 does not depend on p:
// p enters as fma(p, 0, 1), so a NaN or Inf in the row still reaches kd.
struct ArcDiagArgs {
  const double* X; long ldx; int n, d;
  double variance, bias; int op;
  const double* g; double* out;
  double w[GPK_MAX_D];
};

template <int ORDER>
__global__ __launch_bounds__(256) void arccos_diag_kernel(ArcDiagArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [d][T]
  row_diag(p, sm, [&](double acc) {
    const double pv = acc + p.bias;
    if (p.op == 3) return ORDER == 0 ? 0.0 * pv : ORDER == 1 ? fma(pv, 0.0, p.variance) : 6.0 * p.variance * pv;
    return ORDER == 0 ? p.variance * fma(pv, 0.0, 1.0) : ORDER == 1 ? p.variance * pv : 3.0 * p.variance * pv * pv;
  });
}

// The adjoint tail: one workgroup, as dot_adjoint_tail_kernel.  Phase 1 sums the stage's partials in slot order into rg:
// rg[i] = rho_i (symmetric: rho_i + gamma_i, both arguments collected), rg[n1 + k] = gamma_k.  Phase 2: thread t owns input column
// t % d and walks the rows t / d, t / d + rpp, ...; every partial sum has a fixed set of terms in a fixed order and the partials meet in
// LDS in thread order -- deterministic, no atomics.
constexpr int AT_THREADS = 1024;
struct ArcTailArgs {
  const double* R; long ldr;
  const double* A; long lda; int n1;
  const double* B; long ldb; int n2;   // symmetric: B == nullptr, n2 == n1
  int d, ard, symmetric, tr, tc;
  const double* parts; double* rg;
  double* dsmall; double* Abar; long ldab;
  double w[GPK_MAX_D];
};

__global__ __launch_bounds__(AT_THREADS) void arccos_adjoint_tail_kernel(ArcTailArgs p) {
  __shared__ double sh[AT_THREADS];
  __shared__ double sh_b[AT_THREADS];
  __shared__ double sh_v[AT_THREADS];
  __shared__ double sh_dim[GPK_MAX_D];
  const int t = threadIdx.x, d = p.d, n1 = p.n1, n2 = p.n2;
  const double* gam = p.parts + (long)p.tc * n1;
  for (int i = t; i < n1; i += AT_THREADS) {
    double acc = 0.0;
    for (int q = 0; q < p.tc; ++q) acc += p.parts[(long)q * n1 + i];
    if (p.symmetric) {
      double g = 0.0;
      for (int q = 0; q < p.tr; ++q) g += gam[(long)q * n2 + i];
      acc += g;
    }
    p.rg[i] = acc;
  }
  if (!p.symmetric) {
    for (int k = t; k < n2; k += AT_THREADS) {
      double acc = 0.0;
      for (int q = 0; q < p.tr; ++q) acc += gam[(long)q * n2 + k];
      p.rg[n1 + k] = acc;
    }
  }
  double acc_v = 0.0;
  {
    const double* sums = gam + (long)p.tr * n2;
    const int nt = p.tr * p.tc;
    for (int q = t; q < nt; q += AT_THREADS) acc_v += sums[q];
  }
  __syncthreads();   // rg, written above by this workgroup, is read below

  const int rpp = AT_THREADS / d;
  const int c = t % d, r0 = t / d;
  double acc = 0.0, acc_b = 0.0;
  if (r0 < rpp) {
    const double wj = p.w[c];
    const double wc = (p.symmetric ? 2.0 : 1.0) * wj;   // (the factor 2 is exact)
    for (int i = r0; i < n1; i += rpp) {
      const double* Ri = p.R + (long)i * p.ldr;
      const double gb = Ri[1 + c], a = p.A[(long)i * p.lda + c], rho = p.rg[i];
      acc += a * (gb + rho * a);
      p.Abar[(long)i * p.ldab + c] = wc * gb + 2.0 * wj * a * rho;
      if (c == 0) acc_b += Ri[0] + rho;
    }
    if (!p.symmetric) {
      for (int k = r0; k < n2; k += rpp) {
        const double bk = p.B[(long)k * p.ldb + c], g = p.rg[n1 + k];
        acc += g * bk * bk;
        if (c == 0) acc_b += g;
      }
    }
  }
  sh[t] = acc;
  sh_b[t] = acc_b;
  sh_v[t] = acc_v;
  __syncthreads();
  if (t < d) {   // (r0 == 0: this thread's own column)
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh[q * d + t];
    if (p.ard)
      p.dsmall[1 + t] = s;
    else
      sh_dim[t] = s;
  }
  if (t >= 64 && t < 96) {   // d/dvariance: 32 threads add 32 partials each, thread 64 adds theirs
    const int u = t - 64;
    double s = 0.0;
    for (int q = 0; q < 32; ++q) s += sh_v[u * 32 + q];
    sh_v[u * 32] = s;
  }
  __syncthreads();
  if (t == 0) {
    if (!p.ard) {   // one weight for every column: the sum over them, in index order
      double s = 0.0;
      for (int q = 0; q < d; ++q) s += sh_dim[q];
      p.dsmall[1] = s;
    }
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh_b[q * d];
    p.dsmall[p.ard ? 1 + d : 2] = s;
  }
  if (t == 64) {
    double s = 0.0;
    for (int q = 0; q < 32; ++q) s += sh_v[q * 32];
    p.dsmall[0] = s * ARC_INV_PI;
  }
}

template <int ORDER, int MODE>
int launch_arc(hipStream_t st, const ArcArgs& a, size_t lds) {
  GPK_HIP((allow_tile_lds<arccos_kernel<ORDER, MODE>>()));
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((arccos_kernel<ORDER, MODE>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
int launch_arc_order(hipStream_t st, int order, const ArcArgs& a, size_t lds) {
  return order == 0 ? launch_arc<0, MODE>(st, a, lds) : order == 1 ? launch_arc<1, MODE>(st, a, lds) : launch_arc<2, MODE>(st, a, lds);
}

// what every entry point checks of a leaf before it looks at the operands; the weights spread over the d columns into `w`
int read_arc_weights(double* w, int d, const double* w_host, int ard) {
  if (d <= 0 || d > GPK_MAX_D || !w_host) return GPK_E_ARG;
  return spread_weights(w, d, w_host, ard, /*allow_negative=*/false);
}

int read_arc_leaf(double* w, int order, int d, const double* w_host, int ard, double variance, double bias) {
  GPK_TRY(read_arc_weights(w, d, w_host, ard));
  if (order < 0 || order > 2) return GPK_E_UNSUPPORTED;
  if (!std::isfinite(variance) || !std::isfinite(bias) || !(bias > 0.0)) return GPK_E_ARG;
  return 0;
}
}  // namespace

extern "C" int gpk_arccos_kernel_matrix(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2,
                                        int d, const double* w_host, int ard, double variance, double bias, double diag_add,
                                        int lower_only, double* K, long ldk) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  ArcArgs a{};
  GPK_TRY(read_arc_leaf(a.w, order, d, w_host, ard, variance, bias));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldk < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;   // (gpk.h: an operand without elements may be NULL)
  if (!X1 || !K) return GPK_E_ARG;
  const size_t lds = set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, K, ldk, nullptr, 0);
  a.sym = a.same = (X2 == nullptr);
  a.vpi = variance * ARC_INV_PI; a.bias = bias; a.diag_add = diag_add; a.lower_only = lower_only;
  return launch_arc_order<0>((hipStream_t)stream, order, a, lds);
}

extern "C" int gpk_arccos_kernel_matrix_combine(void* stream, int order, int op, const double* X1, int n1, long ldx1, const double* X2,
                                                int n2, long ldx2, int d, const double* w_host, int ard, double variance, double bias,
                                                double diag_add, const double* G, long ldg, double* out, long ldo) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  ArcArgs a{};
  GPK_TRY(read_arc_leaf(a.w, order, d, w_host, ard, variance, bias));
  if (op < 1 || op > 2) return GPK_E_ARG;
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldg < m2 || ldo < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !G || !out) return GPK_E_ARG;
  const size_t lds = set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, out, ldo, G, ldg);
  a.comb_diag = a.same = (X2 == nullptr);
  a.vpi = variance * ARC_INV_PI; a.bias = bias; a.diag_add = a.comb_diag ? diag_add : 0.0;
  const hipStream_t st = (hipStream_t)stream;
  return op == 1 ? launch_arc_order<1>(st, order, a, lds) : launch_arc_order<2>(st, order, a, lds);
}

extern "C" int gpk_arccos_kernel_diag(void* stream, int order, int op, const double* X, int n, long ldx, int d, const double* w_host, int ard,
                                      double variance, double bias, const double* g, double* out) {
  if (n < 0) return GPK_E_ARG;
  ArcDiagArgs a{};
  GPK_TRY(read_arc_leaf(a.w, order, d, w_host, ard, variance, bias));
  if (op < 0 || op > 3 || ldx < d) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!X || !out || (op != 0 && !g)) return GPK_E_ARG;
  a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.variance = variance; a.bias = bias; a.op = op; a.g = g; a.out = out;
  const size_t lds = (size_t)d * T * sizeof(double);   // at most 32 KB
  const dim3 grid((unsigned)gpk_cdiv(n, T));
  const hipStream_t st = (hipStream_t)stream;
  if (order == 0)
    hipLaunchKernelGGL(arccos_diag_kernel<0>, grid, dim3(256), lds, st, a);
  else if (order == 1)
    hipLaunchKernelGGL(arccos_diag_kernel<1>, grid, dim3(256), lds, st, a);
  else
    hipLaunchKernelGGL(arccos_diag_kernel<2>, grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_arccos_adjoint_stage(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2,
                                        int d, const double* w_host, int ard, double variance, double bias, const double* Kbar,
                                        long ldkb, double* G, long ldg, double* parts) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  ArcArgs a{};
  GPK_TRY(read_arc_leaf(a.w, order, d, w_host, ard, variance, bias));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldkb < m2 || ldg < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !Kbar || !G || !parts) return GPK_E_ARG;
  const size_t lds = set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, G, ldg, Kbar, ldkb);
  a.same = (X2 == nullptr);
  a.vpi = variance * ARC_INV_PI; a.bias = bias;
  a.parts = parts; a.tr = gpk_cdiv(a.n1, T); a.tc = gpk_cdiv(a.n2, T);
  return launch_arc_order<3>((hipStream_t)stream, order, a, lds);
}

extern "C" int gpk_arccos_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, const double* B, long ldb,
                                       int n2, int d, const double* w_host, int ard, const double* parts, double* rg, double* dsmall,
                                       double* Abar, long ldab) {
  ArcTailArgs a{};
  GPK_TRY(read_arc_weights(a.w, d, w_host, ard));
  if (n1 < 0 || (B && n2 < 0) || ldr < 1 + d || lda < d || (B && ldb < d) || ldab < d) return GPK_E_ARG;
  a.symmetric = (B == nullptr);
  a.n1 = n1; a.n2 = a.symmetric ? n1 : n2;
  if (!dsmall || (a.n1 > 0 && a.n2 > 0 && (!R || !A || !Abar || !parts || !rg))) return GPK_E_ARG;
  if (a.n1 == 0 || a.n2 == 0) a.n1 = a.n2 = 0;   // no element of K: every sum is empty, dsmall is zeros and Abar is not written
  a.R = R; a.ldr = ldr; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
  a.d = d; a.ard = ard ? 1 : 0; a.tr = gpk_cdiv(a.n1, T); a.tc = gpk_cdiv(a.n2, T);
  a.parts = parts; a.rg = rg; a.dsmall = dsmall; a.Abar = Abar; a.ldab = ldab;
  hipLaunchKernelGGL(arccos_adjoint_tail_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
