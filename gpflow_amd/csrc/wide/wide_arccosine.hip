// The ArcCosine kernel for WIDE inputs, 1 <= d <= GPK_WIDE_MAX_D columns (gpk_wide_arc_*: include/gpk.h), gfx950.
// arccosine.hip stages both whole d-column slabs of a 64 x 64 tile (64 KB at d = 64), forms every dot product on the VALU and holds
// the weights by value: impossible past d = 64.  At d = 65 .. 1024 the kernel is a GEMM with an expensive fp64 epilogue (acos, two
// sqrt and a division per element against 2 d flops): this file puts the dot products on the fp64 matrix pipe, walks the columns in
// slabs and collects the norms on the way, as wide_stationary.hip does for the stationary families.
//
//   s(x, y) = sum_j (x_j w_j) y_j + b     p(x) = s(x, x)     c = s / (sqrt p(x) sqrt p(y))     theta = acos(clamp(eps + (1 - 2 eps) c))
//   K(x, y) = (v / pi) J_order(theta) p(x)^(order/2) p(y)^(order/2)        (J_order and the three contract items: arccosine.hip)
//
// Work split (that of wide_stationary.hip, restated: sharing device code moves register counts here).  One T x T output tile per
// 256-thread workgroup, T = 128 or 64; the four waves (2 x 2) own a square quarter each, WT = T / 2, as NB x NB blocks of
// v_mfma_f64_16x16x4_f64 (NB = WT / 16; A frag: row = lane & 15, k = lane >> 4, the B^T frag the same; D: col = lane & 15,
// row = (lane >> 4) + 4 reg).  T = 64 is launched when the 128-tile grid would have fewer workgroups than the device has compute
// units (arc_tile below: a function of n1, n2 and the symmetric flag alone).
//
// K loop.  A slab is BK = 16 columns of both operands, two LDS buffers, one barrier per slab: the global loads of slab s + 1 are
// issued before the MFMAs of slab s and written to the other buffer after them.  Thread t stages EPT = T / 16 consecutive columns of
// tile row t / TPR of each operand (16-byte loads where the operand allows them).  The FIRST operand is staged as x_j w_j -- one
// rounding, as X * w of the reference -- and the second raw; w is read from the DEVICE (d entries if ard, else one).  Columns past d
// are zero-filled with a weight of 0.0, rows past n1 / n2 are zero-filled.  LDS rows are LD = 18 doubles apart (+ 2 per 16-row group)
// and permuted (lds_row_a, lds_row_b) so that a lane's accumulators are neighbours in memory.
//
// Norms.  p of the tile's rows and q of its columns are accumulated by the staging threads from the staged values,
// fma(x_j w_j, x_j, .), one register partial per COLUMN PHASE: phase f holds the columns j with (j % 16) / 4 == f, ascending.  The four
// partials of a row meet in LDS after the last slab and are added in phase order, b is added last.  The order depends on the column
// alone and not on the tile: p of row i as a row has the bits of p of row i as a column, at T = 128 and at T = 64, in the adjoint
// stage and in the row diagonal (wide_arc_diag_kernel walks the same four chains), and on a rerun.  No atomics, no norm vectors in
// global memory.
//
// Epilogue, in the accumulator registers: arc_eval and the contract of arccosine.hip (the eps-scaled, clamped argument; the by-index
// diagonal c = 1 - 1e-15 where X2 == NULL; a NaN / Inf row poisons exactly its row / column).  MODE 0: the build (diag_add,
// lower_only); 1 / 2: out = G .* k / G + k (out may be G: an element is read and written by the same lane); 3: the adjoint stage.
//
// Symmetric build (X2 == NULL, MODE 0): only tiles on or below the diagonal run.  An off-diagonal tile is also written transposed
// unless lower_only; a diagonal tile writes its lower half and mirrors it inside the tile: K == K^T holds by construction.
//
// Adjoint stage (MODE 3): out = Kbar .* dk/ds, and the sums of Kbar .* dk/dp by row, Kbar .* dk/dq by column and Kbar .* k / v go
// to `parts` in the layout of gpk_arccos_adjoint_stage -- one slot per 64-wide tile row / column / tile (GPK_ARC_TILE).  A lane adds
// its own elements left to right, the sixteen (four) lanes of a row (column) meet by a butterfly inside the wave, the waves' partials
// go to the LDS the slabs leave free.  The stage runs on the 64-tile ALONE (at T = 128 it spills: DESIGN 6), where the tile is one
// slot: two waves share a row / column slot and four the tile's, added in wave order.  Every slot is written by exactly one thread;
// a second call gives the same bits.
//
// Tail, two launches (the ChangePoints tail is the model).  wide_arc_tail_rows_kernel: one workgroup per 256 rows of A, then (not
// symmetric) per 256 rows of B; it sums the slots of its rows in slot order into rg, writes its rows of A_bar and leaves its partial
// column sums for d/dw_j and d/db in `scratch`.  wide_arc_tail_sum_kernel: one workgroup adds the blocks' partials in block order and
// the tile sums for d/dvariance.
#include "../gpk_internal.h"
#include <cmath>

namespace {

constexpr int BK = 16;    // columns per slab
constexpr int LD = 18;    // doubles between LDS rows of a slab
constexpr int NPH = 4;    // column phases of the norms: four columns of a slab each
constexpr int SLOT = GPK_ARC_TILE;
constexpr double ARC_EPS = 1e-15;
constexpr double ARC_SCALE = 1.0 - 2.0 * ARC_EPS;
constexpr double ARC_CT_DIAG = 1.0 - ARC_EPS;   // the acos argument of a diagonal element taken by index
constexpr double ARC_PI = 3.14159265358979323846;
constexpr double ARC_INV_PI = 1.0 / ARC_PI;

struct WArcArgs {
  const double* X1; long ldx1; int n1;
  const double* X2; long ldx2; int n2;
  int d;
  double* K; long ldk;
  double vpi, bias, diag_add;   // vpi = variance / pi
  int sym, lower_only;          // the mirrored build (MODE 0 with X2 == NULL)
  int same;                     // X2 is X1: the diagonal takes c = 1 by index
  int ard;
  const double* w;              // DEVICE: d entries if ard, else one
  const double* G; long ldg;    // MODE 1 / 2: the other factor / summand; MODE 3: Kbar
  int comb_diag;                // MODE 1 / 2 with X2 == NULL: diag_add goes onto the diagonal of the combined result
  double* parts; int tr, tc;    // MODE 3: the partials and the counts of 64-wide tile rows / columns that lay them out
};

template <int T>
struct Geo {
  static constexpr int WT = T / 2, NB = WT / 16, EPT = T / 16, TPR = BK / EPT, PPT = EPT / 4;   // PPT: norm phases per staging thread
  static constexpr int SLAB = T * LD + 2 * (T / 16);    // doubles of one operand's slab
  static constexpr size_t LDS = (size_t)4 * SLAB * sizeof(double);   // two operands, two buffers
  static constexpr int PART = 0, NRM = 2 * T * NPH, ROOT = NRM + 2 * T, RED = ROOT + 2 * T, END = RED + 4 * T + 4;
  static_assert(END <= 4 * SLAB, "the norm partials, the norms and the stage's partial sums reuse the slabs");
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

// J_ORDER at cos theta = ct, and D = dJ / d(acos argument)   (arccosine.hip, contract item 3: acos and sqrt only)
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

// the sum over the lanes that differ in the bits of MASK, by a butterfly: every lane ends with the same bits
template <int FIRST, int LAST>
__device__ __forceinline__ double lane_sum(double v) {
#pragma unroll
  for (int m = FIRST; m <= LAST; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// (two workgroups per CU: one's staging and epilogue under the other's MFMAs)
template <int T, int ORDER, int MODE>
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(256) void wide_arc_kernel(const WArcArgs p) {
  using G_ = Geo<T>;
  constexpr int WT = G_::WT, NB = G_::NB, EPT = G_::EPT, TPR = G_::TPR, PPT = G_::PPT, SLAB = G_::SLAB;
  static_assert(MODE != 3 || T == SLOT, "the adjoint stage runs on the 64-tile alone: a tile is one slot of `parts`");
  extern __shared__ __attribute__((aligned(16))) double sm[];   // [2 buffers][2 operands][SLAB]

  if (MODE == 0 && p.sym && blockIdx.x > blockIdx.y) return;   // strictly upper tile: skipped (lower_only) or written by its mirror
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  const int d = p.d;

  // ---- staging slots --------------------------------------------------------------------------
  const int srow = tid / TPR, scol = (tid % TPR) * EPT;
  const int g1 = r0 + srow, g2 = c0 + srow;
  const double* __restrict__ x1 = p.X1 + (long)g1 * p.ldx1 + scol;
  const double* __restrict__ x2 = p.X2 + (long)g2 * p.ldx2 + scol;
  const bool in1 = g1 < p.n1, in2 = g2 < p.n2;
  const bool vec1 = in1 && ((p.ldx1 & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.X1) & 15) == 0);
  const bool vec2 = in2 && ((p.ldx2 & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.X2) & 15) == 0);
  const int so1 = lds_off(lds_row_a(srow)) + scol, so2 = SLAB + lds_off(lds_row_b<T>(srow)) + scol;
  const double w0 = p.w[0];

  double ra[EPT], rb[EPT], rw[EPT];
  auto gload = [&](int ks) {
    const bool inside = ks + scol + EPT <= d;   // none of this thread's columns is past d
    if (vec1 && inside) {
#pragma unroll
      for (int e = 0; e < EPT; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(x1 + ks + e);
        ra[e] = v[0]; ra[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) ra[e] = (in1 && ks + scol + e < d) ? x1[ks + e] : 0.0;
    }
    if (vec2 && inside) {
#pragma unroll
      for (int e = 0; e < EPT; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(x2 + ks + e);
        rb[e] = v[0]; rb[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) rb[e] = (in2 && ks + scol + e < d) ? x2[ks + e] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) rw[e] = (ks + scol + e < d) ? (p.ard ? p.w[ks + scol + e] : w0) : 0.0;
  };
  // this thread's share of p of row srow of X1 and of q of row srow of X2: one chain per column phase, over every slab
  double np1[PPT], np2[PPT];
#pragma unroll
  for (int f = 0; f < PPT; ++f) np1[f] = np2[f] = 0.0;
  auto lstore = [&](double* buf) {
#pragma unroll
    for (int e = 0; e < EPT; e += 2) {
      const double a0 = ra[e] * rw[e], a1 = ra[e + 1] * rw[e + 1];   // x_j w_j: one rounding
      const double b0 = rb[e] * rw[e], b1 = rb[e + 1] * rw[e + 1];
      np1[e / 4] = fma(a0, ra[e], np1[e / 4]); np1[e / 4] = fma(a1, ra[e + 1], np1[e / 4]);
      np2[e / 4] = fma(b0, rb[e], np2[e / 4]); np2[e / 4] = fma(b1, rb[e + 1], np2[e / 4]);
      *reinterpret_cast<d2*>(&buf[so1 + e]) = (d2){a0, a1};
      *reinterpret_cast<d2*>(&buf[so2 + e]) = (d2){rb[e], rb[e + 1]};
    }
  };

  d4 acc[NB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // MFMA fragments: block i of the wave's rows is LDS rows wr WT + 16 i .. + 15 of X1's slab, block j LDS rows wc WT + 16 j .. of X2's
  int fa[NB], fb[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    fa[i] = lds_off(wr * WT + i * 16 + l15) + lq;
    fb[i] = SLAB + lds_off(wc * WT + i * 16 + l15) + lq;
  }

  const int nslab = (d + BK - 1) / BK;
  gload(0);
  lstore(sm);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const double* cur = sm + (s & 1) * 2 * SLAB;
    const bool more = s + 1 < nslab;
    if (more) gload((s + 1) * BK);                     // in flight under this slab's arithmetic
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double a[NB], b[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) a[i] = cur[fa[i] + kk * 4];
#pragma unroll
      for (int j = 0; j < NB; ++j) b[j] = cur[fb[j] + kk * 4];
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) lstore(sm + ((s + 1) & 1) * 2 * SLAB);   // (its last readers passed the barrier that ended slab s - 1)
    __syncthreads();
  }

  // ---- norms: the four phase partials of a row in phase order, then b (the slabs are no longer read) -------
  double* part = sm + G_::PART;    // [2][T][NPH]
  double* nrm = sm + G_::NRM;      // [2][T]: p of the rows, then q of the columns, by TILE index
  double* root = sm + G_::ROOT;    // [2][T]: their square roots
#pragma unroll
  for (int f = 0; f < PPT; ++f) {
    part[srow * NPH + scol / 4 + f] = np1[f];
    part[(T + srow) * NPH + scol / 4 + f] = np2[f];
  }
  __syncthreads();
  if (tid < 2 * T) {
    double s = part[tid * NPH];
#pragma unroll
    for (int ph = 1; ph < NPH; ++ph) s += part[tid * NPH + ph];
    const double pv = s + p.bias;
    nrm[tid] = pv;
    root[tid] = sqrt(pv);
  }
  __syncthreads();

  // ---- epilogue ----------------------------------------------------------------------------------
  const bool aligned = ((p.ldk & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
  const bool full = (r0 + T <= p.n1) && (c0 + T <= p.n2) && aligned;
  const bool mirror = MODE == 0 && p.sym && !p.lower_only;
  const bool diag_mirror = mirror && r0 == c0;   // the lower half and, inside the tile, its transpose
  const int tc0 = wc * WT + l15 * NB;            // this lane's NB consecutive tile columns
  double qc[NB], rqc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    qc[j] = nrm[T + tc0 + j];
    rqc[j] = root[T + tc0 + j];
  }
  bool gvec = false;
  if constexpr (MODE != 0) gvec = full && ((p.ldg & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.G) & 15) == 0);
  double cs[NB], ks = 0.0;   // MODE 3: this lane's column sums of Kbar .* dk/dq and its sum of Kbar .* J m
#pragma unroll
  for (int j = 0; j < NB; ++j) cs[j] = 0.0;
  double* red_r = sm + G_::RED;          // [2 = wc][T]  MODE 3: a wave's row sums of Kbar .* dk/dp
  double* red_c = red_r + 2 * T;         // [2 = wr][T]  its column sums
  double* red_k = red_c + 2 * T;         // [4 = w]      its sum of Kbar .* J m

  // one row of this lane's block: the NB values of global row r0 + tr, accumulator row g of block row i
  auto row_values = [&](int i, int g, int tr, double* out) {
    const int gr = r0 + tr;
    const double pr = nrm[tr], rpr = root[tr];
    double gv[NB];
    if constexpr (MODE != 0) {
      if (gvec) {
#pragma unroll
        for (int j = 0; j < NB; j += 2) {
          const d2 t = *reinterpret_cast<const d2*>(p.G + (long)gr * p.ldg + c0 + tc0 + j);
          gv[j] = t[0]; gv[j + 1] = t[1];
        }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) gv[j] = (gr < p.n1 && c0 + tc0 + j < p.n2) ? p.G[(long)gr * p.ldg + c0 + tc0 + j] : 0.0;
      }
    }
    double rs = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int gc = c0 + tc0 + j;
      const bool ondiag = p.same && gr == gc;
      const double rr = rpr * rqc[j];
      const double c = (acc[i][j][g] + p.bias) / rr;
      const double arg = fma(ARC_SCALE, c, ARC_EPS);
      double ct = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);   // (both comparisons are false for a NaN: it passes)
      if (ondiag) ct = fma(rr, 0.0, ARC_CT_DIAG);   // the constant, or the NaN of a row that holds a NaN or an Inf
      double J, D = 0.0;
      arc_eval<ORDER, MODE == 3>(ct, J, D);
      const double m = ORDER == 0 ? 1.0 : ORDER == 1 ? rr : pr * qc[j];
      const double jm = J * m;
      double k = p.vpi * jm;
      if constexpr (MODE == 0) {
        if (p.sym && gr == gc) k += p.diag_add;
      } else if constexpr (MODE == 1 || MODE == 2) {
        k = (MODE == 2) ? k + gv[j] : k * gv[j];
        if (p.comb_diag && gr == gc) k += p.diag_add;
      } else {
        const bool in = gr < p.n1 && gc < p.n2;
        const double gg = gv[j];
        if (ondiag) D = 0.0;                                   // by index: no angular derivative
        const double sd = ARC_SCALE * D;
        const double h = 0.5 * p.vpi * ((double)ORDER * J - sd * (ondiag ? 1.0 : c));
        const double dks = ORDER == 0 ? p.vpi * sd / rr : ORDER == 1 ? p.vpi * sd : p.vpi * sd * rr;
        const double dkp = ORDER == 0 ? h / pr : ORDER == 1 ? h * rqc[j] / rpr : h * qc[j];
        const double dkq = ORDER == 0 ? h / qc[j] : ORDER == 1 ? h * rpr / rqc[j] : h * pr;
        k = gg * dks;
        rs += in ? gg * dkp : 0.0;     // (a padding element never enters a sum: its derivative may be infinite)
        cs[j] += in ? gg * dkq : 0.0;
        ks += in ? gg * jm : 0.0;
      }
      out[j] = k;
    }
    if constexpr (MODE == 3) {   // the row's sum over this wave's WT columns: the sixteen lanes that share lq
      rs = lane_sum<1, 8>(rs);
      if (l15 == 0) red_r[wc * T + tr] = rs;
    }
  };
  auto store_row = [&](int gr, const double* v) {
    if (full) {
#pragma unroll
      for (int j = 0; j < NB; j += 2) *reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + c0 + tc0 + j) = (d2){v[j], v[j + 1]};
    } else if (gr < p.n1) {
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (c0 + tc0 + j < p.n2) p.K[(long)gr * p.ldk + c0 + tc0 + j] = v[j];
    }
  };

#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int tr0 = wr * WT + i * 16 + 4 * lq;   // this lane's four consecutive tile rows of block row i
    if constexpr (MODE != 0) {   // no mirror: a row is stored as soon as it is formed
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double v[NB];
        row_values(i, g, tr0 + g, v);
        store_row(r0 + tr0 + g, v);
      }
    } else {
      double v[4][NB];
#pragma unroll
      for (int g = 0; g < 4; ++g) row_values(i, g, tr0 + g, v[g]);
      if (diag_mirror) {   // element by element: (gr, gc) for gc <= gr, and its transpose
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int gr = r0 + tr0 + g;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const int gc = c0 + tc0 + j;
            if (gr < p.n1 && gc <= gr) {
              p.K[(long)gr * p.ldk + gc] = v[g][j];
              if (gc < gr) p.K[(long)gc * p.ldk + gr] = v[g][j];
            }
          }
        }
        continue;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) store_row(r0 + tr0 + g, v[g]);
      if (mirror && r0 != c0) {   // transposed copy: rows c0 + tc0 + j, columns r0 + tr0 .. + 3   (sym: n1 == n2)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int gr = c0 + tc0 + j;
          if (full) {
            d2* out = reinterpret_cast<d2*>(p.K + (long)gr * p.ldk + r0 + tr0);
            out[0] = (d2){v[0][j], v[1][j]};
            out[1] = (d2){v[2][j], v[3][j]};
          } else if (gr < p.n1) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
              if (r0 + tr0 + g < p.n2) p.K[(long)gr * p.ldk + r0 + tr0 + g] = v[g][j];
          }
        }
      }
    }
  }

  if constexpr (MODE == 3) {
    // a wave's column sums: the four lanes that share l15; its sum of Kbar .* J m: every lane
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double s = lane_sum<16, 32>(cs[j]);
      if (lq == 0) red_c[wr * T + tc0 + j] = s;
    }
    ks = lane_sum<1, 32>(ks);
    if (lane == 0) red_k[w] = ks;
    __syncthreads();
    // Slots (gpk_arccos_adjoint_stage), bx / by counting 64-wide tiles:
    //   parts[bx * n1 + i]                       row i's sum over the columns of column tile bx    (rho)
    //   parts[tc * n1 + by * n2 + k]             column k's sum over the rows of row tile by       (gamma)
    //   parts[tc * n1 + tr * n2 + by * tc + bx]  the tile's sum of Kbar .* J m                     (d/dvariance, times 1 / pi in the tail)
    double* gam = p.parts + (long)p.tc * p.n1;
    double* sums = gam + (long)p.tr * p.n2;
    // (T == SLOT: the tile is one slot) the two waves of a row / column, the four of the tile, in wave order
    const int r = tid & (T - 1);
    if (tid < T) {
      if (r0 + r < p.n1) p.parts[(long)blockIdx.x * p.n1 + r0 + r] = red_r[r] + red_r[T + r];
    } else if (tid < 2 * T) {
      if (c0 + r < p.n2) gam[(long)blockIdx.y * p.n2 + c0 + r] = red_c[r] + red_c[T + r];
    } else if (tid == 2 * T) {
      sums[(long)blockIdx.y * p.tc + blockIdx.x] = ((red_k[0] + red_k[1]) + red_k[2]) + red_k[3];
    }
  }
}

// The row diagonal, the closed form: kd_i = v jf p_i^order with jf = J_order(0) / pi = 1, 1, 3.  Four threads per row, one per column
// phase of the builder's norms; the four chains meet by lane reads in phase order and b is added last: p has the builder's bits.
// op 0: out = kd; 1: g .* kd; 2: g + kd; 3: g .* dkd/dp.  Order 0 does not depend on p: p enters as fma(p, 0, 1), so a NaN or Inf in
// the row still reaches kd.
constexpr int DIAG_ROWS = 256 / NPH;
struct WArcDiagArgs {
  const double* X; long ldx; int n, d;
  double variance, bias; int op, ard;
  const double* w;   // DEVICE
  const double* g; double* out;
};

template <int ORDER>
__global__ __launch_bounds__(256) void wide_arc_diag_kernel(const WArcDiagArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, ph = tid & (NPH - 1);
  const int gi = blockIdx.x * DIAG_ROWS + tid / NPH;
  const bool in = gi < p.n;
  const double* __restrict__ x = p.X + (long)(in ? gi : 0) * p.ldx;
  const double w0 = p.w[0];
  double acc = 0.0;
  if (in) {
    for (int c = ph * 4; c < p.d; c += BK) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e < p.d) {
          const double xv = x[c + e];
          acc = fma(xv * (p.ard ? p.w[c + e] : w0), xv, acc);
        }
      }
    }
  }
  const int l0 = lane & ~(NPH - 1);
  double s = __shfl(acc, l0);
#pragma unroll
  for (int f = 1; f < NPH; ++f) s += __shfl(acc, l0 + f);
  if (!in || ph != 0) return;
  const double pv = s + p.bias;
  const double k = (p.op == 3) ? (ORDER == 0 ? 0.0 * pv : ORDER == 1 ? fma(pv, 0.0, p.variance) : 6.0 * p.variance * pv)
                               : (ORDER == 0 ? p.variance * fma(pv, 0.0, 1.0) : ORDER == 1 ? p.variance * pv : 3.0 * p.variance * pv * pv);
  p.out[gi] = (p.op == 0) ? k : (p.op == 2) ? p.g[gi] + k : p.g[gi] * k;
}

// ---- the adjoint tail ------------------------------------------------------------------------------
// scratch: [nblk][d + 1], nblk = ceil(n1 / 256) + (symmetric ? 0 : ceil(n2 / 256)); block q leaves its partial of d/dw_j at
// [q (d + 1) + j] and of d/db at [q (d + 1) + d].  The first ceil(n1 / 256) blocks walk rows of A, the others rows of B.
constexpr int TAIL_ROWS = GPK_WIDE_ARC_TAIL_ROWS;
constexpr int SUM_THREADS = 1024;
static_assert(GPK_WIDE_MAX_D <= SUM_THREADS, "wide_arc_tail_sum_kernel: one thread per input column");
struct WArcTailArgs {
  const double* R; long ldr;
  const double* A; long lda; int n1;
  const double* B; long ldb; int n2;   // symmetric: B == nullptr, n2 == n1
  int d, ard, symmetric, tr, tc, nb1, nblk;
  const double* w;                     // DEVICE
  const double* parts; double* rg; double* scratch;
  double* dsmall; double* Abar; long ldab;
};

__global__ __launch_bounds__(TAIL_ROWS) void wide_arc_tail_rows_kernel(const WArcTailArgs p) {
  __shared__ double sh_rho[TAIL_ROWS], sh_red[TAIL_ROWS], sh_b[TAIL_ROWS / 64];
  const int t = threadIdx.x, d = p.d, blk = blockIdx.x;
  const bool first = blk < p.nb1;   // rows of A (rho; symmetric: rho + gamma), or rows of B (gamma)
  const int base = (first ? blk : blk - p.nb1) * TAIL_ROWS;
  const int left = (first ? p.n1 : p.n2) - base, rows = left < TAIL_ROWS ? left : TAIL_ROWS;
  const double* gam = p.parts + (long)p.tc * p.n1;

  // phase 1: the slots of this block's rows in slot order
  double rho = 0.0, bterm = 0.0;
  if (t < rows) {
    const int i = base + t;
    if (first) {
      for (int q = 0; q < p.tc; ++q) rho += p.parts[(long)q * p.n1 + i];
      if (p.symmetric) {
        double g = 0.0;
        for (int q = 0; q < p.tr; ++q) g += gam[(long)q * p.n2 + i];
        rho += g;
      }
      p.rg[i] = rho;
      bterm = p.R[(long)i * p.ldr] + rho;
    } else {
      for (int q = 0; q < p.tr; ++q) rho += gam[(long)q * p.n2 + i];
      p.rg[p.n1 + i] = rho;
      bterm = rho;
    }
  }
  sh_rho[t] = rho;
  bterm = lane_sum<1, 32>(bterm);
  if ((t & 63) == 0) sh_b[t >> 6] = bterm;
  __syncthreads();

  // phase 2: thread (rl, c0) owns the input columns c0, c0 + cw, ... and walks the rows rl, rl + rpp, ... of the block
  const int cw = d < TAIL_ROWS ? d : TAIL_ROWS, rpp = TAIL_ROWS / cw;
  const int c0 = t % cw, rl = t / cw;
  double* out = p.scratch + (long)blk * (d + 1);
  if (rl < rpp) {
    for (int c = c0; c < d; c += cw) {
      double acc = 0.0;
      if (first) {
        const double wj = p.ard ? p.w[c] : p.w[0];
        const double wc = (p.symmetric ? 2.0 : 1.0) * wj;   // (the factor 2 is exact)
        for (int r = rl; r < rows; r += rpp) {
          const long i = base + r;
          const double gb = p.R[i * p.ldr + 1 + c], a = p.A[i * p.lda + c], rh = sh_rho[r];
          acc += a * (gb + rh * a);
          p.Abar[i * p.ldab + c] = wc * gb + 2.0 * wj * a * rh;
        }
      } else {
        for (int r = rl; r < rows; r += rpp) {
          const double bk = p.B[(long)(base + r) * p.ldb + c];
          acc += sh_rho[r] * bk * bk;
        }
      }
      if (rpp == 1)
        out[c] = acc;
      else
        sh_red[rl * cw + c0] = acc;   // (d < 256: one column per thread)
    }
  }
  if (rpp > 1) {   // (uniform over the workgroup)
    __syncthreads();
    if (t < d) {
      double s = 0.0;
      for (int q = 0; q < rpp; ++q) s += sh_red[q * cw + t];
      out[t] = s;
    }
  }
  if (t == 0) out[d] = ((sh_b[0] + sh_b[1]) + sh_b[2]) + sh_b[3];
}

// sh[0 .. SUM_THREADS) -> sh[0]: 32 threads from `t0` add 32 neighbours each, thread t0 adds theirs (barriers inside: every thread calls)
__device__ __forceinline__ double sum_1024(double* sh, int t, int t0) {
  __syncthreads();
  if (t >= t0 && t < t0 + 32) {
    const int u = t - t0;
    double s = 0.0;
    for (int q = 0; q < 32; ++q) s += sh[u * 32 + q];
    sh[u * 32] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (t == t0)
    for (int q = 0; q < 32; ++q) s += sh[q * 32];
  return s;
}

__global__ __launch_bounds__(SUM_THREADS) void wide_arc_tail_sum_kernel(const WArcTailArgs p) {
  __shared__ double sh_v[SUM_THREADS], sh_w[SUM_THREADS];
  const int t = threadIdx.x, d = p.d;
  double acc_w = 0.0, acc_v = 0.0;
  if (t < d) {
    for (int q = 0; q < p.nblk; ++q) acc_w += p.scratch[(long)q * (d + 1) + t];   // the blocks in block order
    if (p.ard) p.dsmall[1 + t] = acc_w;
  }
  {
    const double* sums = p.parts + (long)p.tc * p.n1 + (long)p.tr * p.n2;
    const int nt = p.tr * p.tc;
    for (int q = t; q < nt; q += SUM_THREADS) acc_v += sums[q];
  }
  sh_w[t] = acc_w;   // (0.0 past d)
  sh_v[t] = acc_v;
  const double sw = sum_1024(sh_w, t, 0);
  const double sv = sum_1024(sh_v, t, 64);
  if (t == 0) {
    if (!p.ard) p.dsmall[1] = sw;   // one weight for every column: the sum over them
    double s = 0.0;
    for (int q = 0; q < p.nblk; ++q) s += p.scratch[(long)q * (d + 1) + d];
    p.dsmall[p.ard ? 1 + d : 2] = s;
  }
  if (t == 64) p.dsmall[0] = sv * ARC_INV_PI;
}

// ---- host ---------------------------------------------------------------------------------------
// The tile: 128, unless the 128-tile grid would run fewer workgroups than the device has compute units.  A function of (n1, n2, sym)
// alone -- nothing else selects a kernel.
int arc_tile(int n1, int n2, bool sym, int cus) {
  const long nb1 = gpk_cdiv(n1, 128), nb2 = gpk_cdiv(n2, 128);
  const long tiles = sym ? nb1 * (nb1 + 1) / 2 : nb1 * nb2;
  return tiles < cus ? 64 : 128;
}

int compute_units(int* cus) {
  int dev = 0, n = 0;
  GPK_HIP(hipGetDevice(&dev));
  GPK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  *cus = n > 0 ? n : 1;
  return 0;
}

template <int T, int ORDER, int MODE>
int launch_tile(hipStream_t st, const WArcArgs& a) {
  if (gpk_cdiv(a.n1, T) > 65535) return GPK_E_ARG;   // (grid.y: n1 <= 65535 T rows, include/gpk.h)
  static const hipError_t at = hipFuncSetAttribute(reinterpret_cast<const void*>(wide_arc_kernel<T, ORDER, MODE>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)Geo<T>::LDS);
  GPK_HIP(at);
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((wide_arc_kernel<T, ORDER, MODE>), grid, dim3(256), Geo<T>::LDS, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

// (the adjoint stage: the 64-tile at every size -- at T = 128 its 64 accumulators per lane, J, D, h and the partial sums spill)
template <int ORDER, int MODE>
int launch_order(hipStream_t st, const WArcArgs& a) {
  if constexpr (MODE == 3) {
    return launch_tile<64, ORDER, MODE>(st, a);
  } else {
    int cus = 0;
    GPK_TRY(compute_units(&cus));
    return arc_tile(a.n1, a.n2, a.sym != 0, cus) == 128 ? launch_tile<128, ORDER, MODE>(st, a) : launch_tile<64, ORDER, MODE>(st, a);
  }
}

template <int MODE>
int launch_mode(hipStream_t st, int order, const WArcArgs& a) {
  return order == 0 ? launch_order<0, MODE>(st, a) : order == 1 ? launch_order<1, MODE>(st, a) : launch_order<2, MODE>(st, a);
}

// what every entry point checks of a leaf before it looks at the operands (the weights live on the device: not read here)
int check_leaf(int order, int d, const double* w_dev, double variance, double bias) {
  if (d <= 0 || d > GPK_WIDE_MAX_D || !w_dev) return GPK_E_ARG;
  if (order < 0 || order > 2) return GPK_E_UNSUPPORTED;
  if (!std::isfinite(variance) || !std::isfinite(bias) || !(bias > 0.0)) return GPK_E_ARG;
  return 0;
}

void set_operands(WArcArgs& a, const double* X1, int n1, long ldx1, const double* X2, int n2, long ldx2, int d, const double* w_dev,
                  int ard, double variance, double bias, double* out, long ldo, const double* G, long ldg) {
  a.X1 = X1; a.ldx1 = ldx1; a.n1 = n1;
  a.X2 = X2 ? X2 : X1; a.ldx2 = X2 ? ldx2 : ldx1; a.n2 = X2 ? n2 : n1;
  a.d = d; a.w = w_dev; a.ard = ard ? 1 : 0;
  a.vpi = variance * ARC_INV_PI; a.bias = bias;
  a.K = out; a.ldk = ldo; a.G = G; a.ldg = ldg;
  a.same = (X2 == nullptr);
}

long parts_extent(int n1, int n2) {
  const long tr = gpk_cdiv(n1, SLOT), tc = gpk_cdiv(n2, SLOT);
  return tc * n1 + tr * n2 + tr * tc;
}

}  // namespace

extern "C" int gpk_wide_arc_kernel_matrix(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                          long ldx2, int d, const double* w_dev, int ard, double variance, double bias,
                                          double diag_add, int lower_only, double* K, long ldk) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  GPK_TRY(check_leaf(order, d, w_dev, variance, bias));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldk < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;   // (gpk.h: an operand without elements may be NULL)
  if (!X1 || !K) return GPK_E_ARG;
  WArcArgs a{};
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, w_dev, ard, variance, bias, K, ldk, nullptr, 0);
  a.sym = a.same;
  a.diag_add = diag_add; a.lower_only = lower_only;
  return launch_mode<0>((hipStream_t)stream, order, a);
}

extern "C" int gpk_wide_arc_kernel_matrix_combine(void* stream, int order, int op, const double* X1, int n1, long ldx1,
                                                  const double* X2, int n2, long ldx2, int d, const double* w_dev, int ard,
                                                  double variance, double bias, double diag_add, const double* G, long ldg,
                                                  double* out, long ldo) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  GPK_TRY(check_leaf(order, d, w_dev, variance, bias));
  if (op < 1 || op > 2) return GPK_E_ARG;
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldg < m2 || ldo < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !G || !out) return GPK_E_ARG;
  WArcArgs a{};
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, w_dev, ard, variance, bias, out, ldo, G, ldg);
  a.comb_diag = a.same;
  a.diag_add = a.comb_diag ? diag_add : 0.0;
  const hipStream_t st = (hipStream_t)stream;
  return op == 1 ? launch_mode<1>(st, order, a) : launch_mode<2>(st, order, a);
}

extern "C" int gpk_wide_arc_kernel_diag(void* stream, int order, int op, const double* X, int n, long ldx, int d, const double* w_dev,
                                        int ard, double variance, double bias, const double* g, double* out) {
  if (n < 0) return GPK_E_ARG;
  GPK_TRY(check_leaf(order, d, w_dev, variance, bias));
  if (op < 0 || op > 3 || ldx < d) return GPK_E_ARG;
  if (n == 0) return 0;
  if (!X || !out || (op != 0 && !g)) return GPK_E_ARG;
  WArcDiagArgs a{};
  a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.variance = variance; a.bias = bias; a.op = op; a.ard = ard ? 1 : 0; a.w = w_dev;
  a.g = g; a.out = out;
  const dim3 grid((unsigned)gpk_cdiv(n, DIAG_ROWS));
  const hipStream_t st = (hipStream_t)stream;
  if (order == 0)
    hipLaunchKernelGGL(wide_arc_diag_kernel<0>, grid, dim3(256), 0, st, a);
  else if (order == 1)
    hipLaunchKernelGGL(wide_arc_diag_kernel<1>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(wide_arc_diag_kernel<2>, grid, dim3(256), 0, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

extern "C" int gpk_wide_arc_adjoint_stage(void* stream, int order, const double* X1, int n1, long ldx1, const double* X2, int n2,
                                          long ldx2, int d, const double* w_dev, int ard, double variance, double bias,
                                          const double* Kbar, long ldkb, double* G, long ldg, double* parts, long parts_len) {
  if (n1 < 0 || (X2 && n2 < 0)) return GPK_E_ARG;
  GPK_TRY(check_leaf(order, d, w_dev, variance, bias));
  const int m2 = X2 ? n2 : n1;
  if (ldx1 < d || (X2 && ldx2 < d) || ldkb < m2 || ldg < m2) return GPK_E_ARG;
  if (n1 == 0 || m2 == 0) return 0;
  if (!X1 || !Kbar || !G || !parts || parts_len < parts_extent(n1, m2)) return GPK_E_ARG;
  WArcArgs a{};
  set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d, w_dev, ard, variance, bias, G, ldg, Kbar, ldkb);
  a.parts = parts; a.tr = gpk_cdiv(a.n1, SLOT); a.tc = gpk_cdiv(a.n2, SLOT);
  return launch_mode<3>((hipStream_t)stream, order, a);
}

extern "C" int gpk_wide_arc_adjoint_tail(void* stream, const double* R, long ldr, const double* A, long lda, int n1, const double* B,
                                         long ldb, int n2, int d, const double* w_dev, int ard, const double* parts, long parts_len,
                                         double* rg, double* scratch, long scratch_len, double* dsmall, double* Abar, long ldab) {
  if (d <= 0 || d > GPK_WIDE_MAX_D || !w_dev) return GPK_E_ARG;
  if (n1 < 0 || (B && n2 < 0) || ldr < 1 + d || lda < d || (B && ldb < d) || ldab < d || !dsmall) return GPK_E_ARG;
  WArcTailArgs a{};
  a.symmetric = (B == nullptr);
  a.n1 = n1; a.n2 = a.symmetric ? n1 : n2;
  if (a.n1 == 0 || a.n2 == 0) return 0;   // no element of K: nothing is launched (the caller's dsmall and Abar stay as they are)
  a.nb1 = gpk_cdiv(a.n1, TAIL_ROWS);
  a.nblk = a.nb1 + (a.symmetric ? 0 : gpk_cdiv(a.n2, TAIL_ROWS));
  if (!R || !A || !Abar || !parts || !rg || !scratch || parts_len < parts_extent(a.n1, a.n2) || scratch_len < (long)a.nblk * (d + 1))
    return GPK_E_ARG;
  a.R = R; a.ldr = ldr; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
  a.d = d; a.ard = ard ? 1 : 0; a.tr = gpk_cdiv(a.n1, SLOT); a.tc = gpk_cdiv(a.n2, SLOT);
  a.w = w_dev; a.parts = parts; a.rg = rg; a.scratch = scratch; a.dsmall = dsmall; a.Abar = Abar; a.ldab = ldab;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wide_arc_tail_rows_kernel, dim3((unsigned)a.nblk), dim3(TAIL_ROWS), 0, st, a);
  GPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(wide_arc_tail_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
