// The ArcCosine kernel for WIDE inputs, 1 <= d <= GPK_WIDE_MAX_D columns (gpk_wide_arc_*: include/gpk.h), gfx950.
// arccosine.hip stages both whole d-column slabs of a 64 x 64 tile (64 KB at d = 64), forms every dot product on the VALU and holds
// the weights by value: impossible past d = 64.  At d = 65 .. 1024 the kernel is a GEMM with an expensive fp64 epilogue (acos, two
// sqrt and a division per element against 2 d flops): this file puts the dot products on the fp64 matrix pipe, walks the columns in
// slabs and collects the norms on the way, as wide_stationary.hip does for the stationary families.
//
//   s(x, y) = sum_j (x_j w_j) y_j + b     p(x) = s(x, x)     c = s / (sqrt p(x) sqrt p(y))     theta = acos(clamp(eps + (1 - 2 eps) c))
//   K(x, y) = (v / pi) J_order(theta) p(x)^(order/2) p(y)^(order/2)        (J_order and the three contract items: arccosine.hip)
//
// The tile -- work split, K loop, LDS layout, symmetric build -- is wide_tile.h's, shared with wide_stationary.hip; this file brings
// the value arithmetic of the ArcCosine kernel, the row diagonal, the adjoint tail and the entry points.
//
// Staging.  The FIRST operand is staged as x_j w_j -- one rounding, as X * w of the reference -- and the second raw; w is read from
// the DEVICE (d entries if ard, else one).  A column past d has a weight of 0.0.
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
#include "wide_tile.h"
#include <cmath>

namespace {

using namespace wide_tile;

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

// What this file keeps in the LDS that the slabs leave free after the K loop, behind the tile's phase partials and norms
// (wide_tile_front.inc: part [2][T][NPH], nrm [2][T]): the square roots of the norms, and the adjoint stage's partial sums.
template <int T>
struct ArcLds {
  static constexpr int ROOT = 2 * T * NPH + 2 * T, RED = ROOT + 2 * T, END = RED + 4 * T + 4;
  static_assert(END <= 4 * Geo<T>::SLAB, "the norm partials, the norms and the stage's partial sums reuse the slabs");
};

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

// what the tile of wide_tile.h does to values here: the first operand as x w (one rounding), the second raw, fma(x w, x, .) summed
// as it is staged; a norm is finished by + b, and its square root is kept beside it
#define WIDE_STAGE(x, w) ((x) * (w))
#define WIDE_SECOND(staged, raw) (raw)
#define WIDE_NORM_TERM(staged, raw, acc) fma(staged, raw, acc)
#define WIDE_NORM_FINISH(sum)       \
  const double pv = (sum) + p.bias; \
  nrm[tid] = pv;                    \
  sm[ArcLds<T>::ROOT + tid] = sqrt(pv)
#define WIDE_SYM (MODE == 0 && p.sym)   // the mirrored build
#define WIDE_FIRST_PHASE (scol / 4)
#define WIDE_PARTIAL_OF(e) ((e) / 4)
#define WIDE_SCALES p.w

template <int T, int ORDER, int MODE>
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(256) void wide_arc_kernel(const WArcArgs p) {
  static_assert(MODE != 3 || T == SLOT, "the adjoint stage runs on the 64-tile alone: a tile is one slot of `parts`");
  constexpr double PAD = 0.0;
  constexpr bool BUILD = MODE == 0;
  // (NPH, above: four phases of four columns at both tiles, EPT / 4 partials per staging thread)
#include "wide_tile_front.inc"
  double* root = sm + ArcLds<T>::ROOT;   // [2][T]: the square roots of nrm, p of the rows, then q of the columns
  double qc[NB], rqc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    qc[j] = nrm[T + tc0 + j];
    rqc[j] = root[T + tc0 + j];
  }
  bool gvec = false;   // (wide_tile_gread.inc)
  if constexpr (!BUILD) gvec = full && ((p.ldg & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.G) & 15) == 0);
  double cs[NB], ks = 0.0;   // MODE 3: this lane's column sums of Kbar .* dk/dq and its sum of Kbar .* J m
#pragma unroll
  for (int j = 0; j < NB; ++j) cs[j] = 0.0;
  double* red_r = sm + ArcLds<T>::RED;   // [2 = wc][T]  MODE 3: a wave's row sums of Kbar .* dk/dp
  double* red_c = red_r + 2 * T;         // [2 = wr][T]  its column sums
  double* red_k = red_c + 2 * T;         // [4 = w]      its sum of Kbar .* J m

  // one row of this lane's block: the NB values of global row r0 + tr, accumulator row g of block row i
  auto row_values = [&](int i, int g, int tr, double* out) {
    const int gr = r0 + tr;
    const double pr = nrm[tr], rpr = root[tr];
#include "wide_tile_gread.inc"
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
#include "wide_tile_rows.inc"

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
// (the adjoint stage: the 64-tile at every size -- at T = 128 its 64 accumulators per lane, J, D, h and the partial sums spill)
template <int ORDER, int MODE>
int launch_order(hipStream_t st, const WArcArgs& a) {
  if constexpr (MODE == 3) {
    return launch_tile<wide_arc_kernel<64, ORDER, MODE>, 64>(st, a);
  } else {
    int cus = 0;
    GPK_TRY(compute_units(&cus));
    return tile_size(a.n1, a.n2, a.sym != 0, cus) == 128 ? launch_tile<wide_arc_kernel<128, ORDER, MODE>, 128>(st, a)
                                                        : launch_tile<wide_arc_kernel<64, ORDER, MODE>, 64>(st, a);
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
  wide_tile::set_operands(a, X1, n1, ldx1, X2, n2, ldx2, d);
  a.w = w_dev; a.ard = ard ? 1 : 0;
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
