// The 128 x 128 / 64 x 64 MFMA pair tile of the WIDE builders, 1 <= d <= GPK_WIDE_MAX_D columns (wide_stationary.hip,
// wide_arccosine.hip), gfx950: out[i][j] = f(<a_i, b_j>, norm(a_i), norm(b_j)) with the dot products on the fp64 matrix pipe and the
// columns walked in slabs.  The tile is written here once: its geometry and LDS layout, its body (the wide_tile_*.inc fragments, which
// own every index) and the host side of its launch.  A file brings what is done to VALUES -- the list is at the fragments below.
//
// Work split.  One T x T output tile per 256-thread workgroup, T = 128 or 64; the four waves (2 x 2) own a square quarter each,
// WT = T / 2, as NB x NB blocks of v_mfma_f64_16x16x4_f64 (NB = WT / 16; A frag: row = lane & 15, k = lane >> 4, the B^T frag the
// same; D: col = lane & 15, row = (lane >> 4) + 4 reg -- gemm.hip).  T = 128 is the primary tile: 16 accumulators per wave and half
// the LDS traffic per MFMA of T = 64.  T = 64 is launched when the 128-tile grid would have fewer workgroups than the device has
// compute units (tile_size below: a function of n1, n2 and the symmetric flag alone).
//
// K loop.  A slab is BK = 16 columns of both operands.  Thread t stages EPT = T / 16 consecutive columns of tile row t / TPR of each
// operand (TPR = 16 / EPT threads per row; 16-byte loads where the operand allows them), applies the file's per-column scale and
// writes the staged values to LDS in the layout the MFMA fragments are read from.  Two LDS buffers: the global loads of slab s + 1 are
// issued before the MFMAs of slab s and written to the other buffer after them, one barrier per slab.  Columns past d are zero-filled
// with the file's padding scale, rows past n1 / n2 are zero-filled.
//
// LDS layout.  Both slabs are [T][16] with rows LD = 18 doubles apart (+ 2 doubles per 16-row group: lds_off), so the 32-lane groups
// of a fragment's ds_read_b64 hit distinct banks.  The ROWS are permuted at staging so that a lane's accumulators are neighbours in
// memory: tile row 16 i + 4 a + b of X1 sits in LDS row 16 i + a + 4 b (the D rows (lane >> 4) + 4 reg of a lane are then the four
// consecutive tile rows 16 i + 4 (lane >> 4) + reg), and column (lane & 15) NB + j of a wave's WT columns sits in LDS row 16 j +
// (lane & 15) of X2's slab (a lane's NB blocks are NB consecutive columns).  Direct and mirrored stores are then 16-byte stores.
//
// Norms.  The norm of every tile row and column is accumulated from the values as they are staged: a staging thread keeps one
// register partial per COLUMN PHASE it touches across the slabs -- the file sets the number of phases NPH, a phase is BK / NPH
// consecutive columns of every slab -- the partials meet in LDS after the last slab and are added in phase order.  The order depends
// on the column alone: a row's norm has the same bits as a row and as a column, in every tile, and a rerun is bit-identical.  No
// atomics.  NPH is part of the bits and differs between the files on purpose (each says why where it sets NPH).
//
// Symmetric build (WIDE_SYM: X2 == NULL, plain build): only tiles on or below the diagonal run.  An off-diagonal tile
// is also written transposed unless lower_only; a diagonal tile writes its lower half and mirrors it inside the tile, so K == K^T
// holds by construction and does not rest on dot[i][j] and dot[j][i] leaving the matrix pipe with the same bits.
#pragma once
#include "../gpk_internal.h"

namespace wide_tile {

constexpr int BK = 16;   // columns per slab
constexpr int LD = 18;   // doubles between LDS rows of a slab

template <int T>
struct Geo {
  static constexpr int WT = T / 2, NB = WT / 16, EPT = T / 16, TPR = BK / EPT;
  static constexpr int SLAB = T * LD + 2 * (T / 16);    // doubles of one operand's slab (lds_off of the last row + its 16 columns)
  static constexpr size_t LDS = (size_t)4 * SLAB * sizeof(double);   // two operands, two buffers
};

__device__ __forceinline__ int lds_off(int lrow) { return lrow * LD + 2 * (lrow >> 4); }
// tile row of X1 -> LDS row: 16 i + 4 a + b -> 16 i + a + 4 b
__device__ __forceinline__ int lds_row_a(int r) { return (r & ~15) | ((r >> 2) & 3) | ((r & 3) << 2); }
// tile column (row of X2's slab) -> LDS row: wave half wc, c = l NB + j -> wc WT + 16 j + l
template <int T>
__device__ __forceinline__ int lds_row_b(int c) {
  constexpr int WT = Geo<T>::WT, NB = Geo<T>::NB;
  const int wc = c / WT, cc = c % WT;
  return wc * WT + (cc % NB) * 16 + cc / NB;
}

// ---- the tile body: three textual fragments -------------------------------------------------------
// A tile kernel is `template <int T, ...> __attribute__((amdgpu_waves_per_eu(2, 2))) __global__ __launch_bounds__(256)` (two
// workgroups per CU: one's staging and epilogue under the other's MFMAs) over an args struct `p` with X1 ldx1 n1 X2 ldx2 n2 d K ldk
// lower_only ard (and G ldg unless BUILD).  Its body is, in this order:
//
//   the file's names     constexpr int NPH         column phases of the norms: a phase is BK / NPH consecutive columns of a slab
//                        constexpr double PAD      the scale of a column past d
//                        constexpr bool BUILD      the plain build: no G is read, and the symmetric build exists
//   #include "wide_tile_front.inc"   staging slots, gload / lstore, accumulators and fragments, the K loop, the meeting of the norm
//                        partials, the edge predicates.  It takes from the file, as macros (text, so that each kernel keeps the
//                        expressions it was written with):
//                          WIDE_SYM                          only tiles on or below the diagonal run (a condition on p)
//                          WIDE_SCALES                       DEVICE: the per-column scales, d entries if p.ard, else one
//                          WIDE_STAGE(x, s)                  the staged value of x under scale s
//                          WIDE_SECOND(staged, raw)          what of the SECOND operand goes to the slab
//                          WIDE_NORM_TERM(staged, raw, acc)  one term of a norm's chain
//                          WIDE_PARTIAL_OF(e)                which of this thread's EPT / (BK / NPH) partials column e of its EPT adds to
//                          WIDE_FIRST_PHASE                  the phase of this thread's first column
//                          WIDE_NORM_FINISH(sum)             a statement, run by thread tid < 2 T for tile row (tid < T) or column
//                                                            tid - T: nrm[tid] (and what else the file keeps per row) from the sum
//                        and leaves r0 c0 tid lane w wr wc l15 lq tc0, sm nrm, acc[NB][NB], full mirror diag_mirror.
//   the file's column values (nrm[T + tc0 + j]); `gvec`, whether G is read in 16-byte loads (it follows the column values in both
//                        files: ahead of them it costs every kernel that reads G an instruction); and the file's lambda
//                        row_values(i, g, tr, out): the NB values of global row gr = r0 + tr from accumulator row g of block row i, with
//   #include "wide_tile_gread.inc"   inside it: gv[NB], the row's values of G
//   #include "wide_tile_rows.inc"    store_row and the block-row loop that calls row_values, with both mirror paths
//   what the file does at the tile's end (the adjoint stage's slot writes).
//
// Fragments and not a kernel template over a policy class: as text they are the hand-written kernels' tokens -- wide_arc_kernel's
// instructions are unchanged one for one, wide_kernel's are the same in another order -- where the template kept the bits but moved
// every tile kernel's code and registers (profiles/wide_tile_refactor.txt).  A third caller is a third kernel of this shape.

// ---- host ---------------------------------------------------------------------------------------
// The tile: 128, unless the 128-tile grid would run fewer workgroups than the device has compute units.  A function of (n1, n2, sym)
// alone -- nothing else selects a kernel.
inline int tile_size(int n1, int n2, bool sym, int cus) {
  const long nb1 = gpk_cdiv(n1, 128), nb2 = gpk_cdiv(n2, 128);
  const long tiles = sym ? nb1 * (nb1 + 1) / 2 : nb1 * nb2;
  return tiles < cus ? 64 : 128;
}

// (asked per call: the count belongs to the device that is current now, and the lookup is a cached attribute of the runtime)
inline int compute_units(int* cus) {
  int dev = 0, n = 0;
  GPK_HIP(hipGetDevice(&dev));
  GPK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  *cus = n > 0 ? n : 1;
  return 0;
}

// one launch of KERNEL, an instantiation on the T-tile, over the n1 x n2 rectangle of `a`
template <auto KERNEL, int T, class A>
int launch_tile(hipStream_t st, const A& a) {
  if (gpk_cdiv(a.n1, T) > 65535) return GPK_E_ARG;   // (grid.y: n1 <= 65535 T rows, include/gpk.h)
  static const hipError_t at = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)Geo<T>::LDS);   // (once per KERNEL)
  GPK_HIP(at);
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), Geo<T>::LDS, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

// The operand fields of an args struct.  X2 == NULL: the second operand is the first (the caller sets sym / comb_diag / same from
// that, after its own checks -- this checks nothing).
template <class A>
void set_operands(A& a, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d) {
  a.X1 = X1; a.ldx1 = ldx1; a.n1 = n1;
  a.X2 = X2 ? X2 : X1; a.ldx2 = X2 ? ldx2 : ldx1; a.n2 = X2 ? n2 : n1;
  a.d = d;
}

}  // namespace wide_tile
