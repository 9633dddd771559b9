// What the 64 x 64 pair-tile builders (rbf.hip, dot.hip, arccosine/arccosine.hip) share WITHOUT changing their tile kernels' code:
// the host side of a launch and the row-diagonal skeleton.  The tile's device pieces (staging, 4 x 4 chain, `full`, the two stores)
// stay restated in rbf_kernel, dot_kernel and arccos_kernel: as __forceinline__ helpers they compute the same bits, but a helper is
// simplified before it is inlined and the kernels came out with other register counts -- profiles/pair_tile_refactor.txt.
#pragma once
#include "gpk_internal.h"
#include <cmath>

namespace pair_tile {

constexpr int T = 64;

// one term of s(x, x) = sum_j (x_j w_j) x_j, the builders' chain: x w rounded once, then one fma
__device__ __forceinline__ double weighted_square(double x, double w, double acc) { return fma(x * w, x, acc); }

// The row diagonal kd_i = k(x_i, x_i) from s_i = sum_j (x_ij w_j) x_ij: T rows per workgroup staged as [d][T] with lanes along the
// contiguous dimension of X (padding rows 0.0), thread r < T sums row r with the builders' chain (so s_i is the diagonal of the built
// s bit for bit), k = eval(s_i), and the op tail -- 0: out = k; 2: g + k; else g .* k (the caller's eval picks k or its derivative).
// P: X, ldx, n, d, w, op, g, out.  One workgroup of 256 threads per T rows along blockIdx.x.  It is the WHOLE body of its kernel:
// the `return` below leaves this helper only, so nothing may follow the call.
template <class P, class EVAL>
__device__ __forceinline__ void row_diag(const P& p, double* sm, EVAL eval) {
  const int d = p.d, r0 = blockIdx.x * T, tid = threadIdx.x;
  for (int e = tid; e < T * d; e += 256) {
    const int row = e / d, dd = e - row * d;
    const int gi = r0 + row;
    sm[dd * T + row] = (gi < p.n) ? p.X[(long)gi * p.ldx + dd] : 0.0;
  }
  __syncthreads();
  const int gi = r0 + tid;
  if (tid >= T || gi >= p.n) return;
  double s = 0.0;
  for (int dd = 0; dd < d; ++dd) s = weighted_square(sm[dd * T + tid], p.w[dd], s);
  const double k = eval(s);
  p.out[gi] = (p.op == 0) ? k : (p.op == 2) ? p.g[gi] + k : p.g[gi] * k;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a tile launch: the two [d][T] slabs and EXTRA doubles behind them
template <int EXTRA>
constexpr size_t tile_lds(int d) { return ((size_t)2 * d * T + EXTRA) * sizeof(double); }

// The operand fields of an args struct (X1, ldx1, n1, X2, ldx2, n2, d, K, ldk, G, ldg).  X2 == NULL: the second slab is the first
// (the caller sets sym / comb_diag / same from that, after its own checks -- this checks nothing).  The grid -- one T x T tile per
// workgroup -- stays next to each launch, where tests/test_launch_geometry.py pins its text.  Returns the launch's LDS bytes.
template <int EXTRA = 0, class A>
size_t set_operands(A& a, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d, double* out, long ldo,
                    const double* G, long ldg) {
  a.X1 = X1; a.ldx1 = ldx1; a.n1 = n1;
  a.X2 = X2 ? X2 : X1; a.ldx2 = X2 ? ldx2 : ldx1; a.n2 = X2 ? n2 : n1;
  a.d = d; a.K = out; a.ldk = ldo; a.G = G; a.ldg = ldg;
  return tile_lds<EXTRA>(d);
}

// once per (KERNEL, EXTRA): dynamic LDS up to d = GPK_MAX_D (64 KB of slabs).  The launch itself follows in the caller's file.
template <auto KERNEL, int EXTRA = 0>
hipError_t allow_tile_lds() {
  static const hipError_t at = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)tile_lds<EXTRA>(GPK_MAX_D));
  return at;
}

// one weight, or one per column (ard), spread over the d columns of w [GPK_MAX_D], the rest 0.0; GPK_E_ARG for one that is not finite
// (or negative, unless allowed).  The caller has checked d and w_host.
inline int spread_weights(double* w, int d, const double* w_host, int ard, bool allow_negative) {
  for (int j = 0; j < d; ++j) {
    const double v = w_host[ard ? j : 0];
    if (!std::isfinite(v) || (!allow_negative && v < 0.0)) return GPK_E_ARG;
    w[j] = v;
  }
  for (int j = d; j < GPK_MAX_D; ++j) w[j] = 0.0;
  return 0;
}

}  // namespace pair_tile
