// The 64 x 64 pair tile of the narrow builders (d <= GPK_MAX_D columns): one tile per 256-thread workgroup, thread (tx, ty) = (tid & 15,
// tid >> 4) owns the 4 x 4 patch at rows r0 + ty * 4, columns c0 + tx * 4.  Written here once: the host side of a launch, the
// row-diagonal skeleton, and the tile's device pieces as textual fragments, pair_tile_*.inc, each a run of statements included inside
// a file's own kernel.  Fragments and not __forceinline__ helpers: a helper is simplified before it is inlined and the kernels came out
// with other register counts (profiles/pair_tile_refactor.txt); as text a fragment is the kernel's own tokens, and every kernel of the
// seven files is instruction for instruction what it was when it restated them (profiles/pair_tile_fragments.txt).
//
// A tile kernel `__global__ __launch_bounds__(256)` over an args struct `p` with n1, n2 #defines the macros of the fragments it uses
// ahead of its template line and includes pair_tile_end.inc, which #undefs them all, behind its closing brace.  Every fragment expects
// T (below), r0, c0, tx, ty.  In the order of a kernel's body:
//   pair_tile_stage.inc         expects tid, d, x1t, x2t and p.X1 ldx1 X2 ldx2; fills the two [d][T] slabs (padding rows 0.0), one barrier
//       PAIR_STAGE_LOCALS           a statement per staged (row, dd), or empty: what the two transforms share (rbf.hip: the lengthscale)
//       PAIR_STAGE_FIRST(x)         the staged value of an element x of X1;  PAIR_STAGE_SECOND(x): of X2
//   pair_tile_chain.inc         expects d, x1t, x2t and `double dot[4][4]`; leaves dot[i][j]: two d2 reads per slab and column, 16 fmas
//       PAIR_FIRST(x)               the first factor from the staged x (arccosine.hip: x * p.w[dd], formed in registers)
//   pair_tile_full.inc          leaves `const bool full`: the tile is whole, PAIR_LDO even and PAIR_OUT 16-byte aligned
//       PAIR_OUT, PAIR_LDO          the output and its leading dimension (p.K, p.ldk; changepoints.hip: p.out, p.ldo)
//   the file's epilogue         `double v[4][4]` from dot: what is particular to each file, with the predicates of its symmetric build
//   pair_tile_diag_patch.inc    expects `diag_tile`, v; a patch on the diagonal of a diagonal tile takes its upper entries from its lower
//   pair_tile_store_rows.inc    expects full, v; PAIR_OUT, PAIR_LDO; two 16-byte stores per row where full, else guarded scalar stores
//       PAIR_WRITTEN(gr, gc)        the scalar store's condition on the column: gc < p.n2 (coregion.hip: and not above the diagonal of
//                                   a lower_only build)
//   pair_tile_store_mirror.inc  expects full, v; PAIR_OUT, PAIR_LDO; the transposed copy.  WHEN it runs stays in each file: that is the
//                               file's contract (rbf.hip: whole tiles off the diagonal; dot.hip, arccosine.hip: also inside a diagonal tile)
// Users: rbf.hip, dot.hip, arccosine/arccosine.hip all of it (rbf.hip no diag_patch); changepoints/, coregion/ the row stores;
// multiscale/ `full` (ms_kfu_kernel) and diag_patch (ms_kuu_kernel) -- its store_row helper and ms_kuu_kernel's `full` over M stay:
// with the fragments in their place its five builders came out with other code (profiles/pair_tile_fragments.txt, section 1).
// An edit to the tile -- a staged vector more, another store -- is made in one fragment and proved equal once per file
// (tools/kernel_code_diff.py).
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
