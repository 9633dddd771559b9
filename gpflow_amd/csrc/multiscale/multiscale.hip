// Multiscale inducing variables against the SquaredExponential kernel (gpflow/covariances/kufs.py, kuus.py: Multiscale x
// SquaredExponential), gfx950.  Every inducing point z_m carries a length s_mj >= 0 per column; l_j: the kernel's lengthscale, v: variance.
//
//   Kfu[n, m]  = v prod_j (l_j r_mj) exp(-1/2 sum_j ((x_nj - z_mj) r_mj)^2)                       r_mj = 1 / (l_j + s_mj)
//   Kuu[m, m'] = v sqrt(prod_j l_j^2 q_j) exp(-1/2 sum_j D_j^2 q_j)      D_j = z_mj - z_m'j,  q_j = 1 / ((a_mj + a_m'j) - l_j^2),  a = (l + s)^2
//
// Contract (restated in include/gpk.h):
//  1. NO EXPANSION.  The effective lengthscale differs per output column (Kfu) or per PAIR (Kuu), so |x|^2 + |y|^2 - 2 x.y is not
//     available: each element is the difference form, an fma chain over ascending columns from 0.0 -- no cancellation.
//  2. Kfu stages three slabs [d][64]: the raw X rows, the raw Z columns and r, formed ONCE per tile as it is staged (one division per
//     staged value, none per element); behind them the 64 column prefactors c_m = v prod_j (l_j r_mj), multiplied in column order.
//     An element costs 3 fp64 operations per column (subtract, multiply, fma), then one exp and one multiply.
//  3. Kuu stages (z, a) of the tile's rows and of its columns, four slabs.  q is a true division per element and column; the prefactor is
//     ONE square root per element of the running product of l_j^2 q_j.  a_m + a_m' and D^2 commute, so k(m, m') == k(m', m) bit for bit;
//     the build computes the tiles on or below the diagonal and mirrors them: Kuu is EXACTLY symmetric.
//  4. NaN.  A NaN or Inf in a row of X makes that row of Kfu NaN (sum_j 0 x_nj is added to the row's elements: 0.0, or NaN); a NaN in z_m
//     or s_m makes column m of Kfu and row and column m of Kuu NaN, and nothing else.
//  5. No atomics; every sum has a fixed set of terms in a fixed order: a second call gives the same bits.
#include "../pair_tile.h"
#include <cmath>

namespace {

using namespace pair_tile;
static_assert(T == GPK_MS_TILE, "include/gpk.h states the tile of the adjoint stage's partials");
constexpr int KFU_EXTRA = GPK_MAX_D * T + T;   // the slab of reciprocals and the column prefactors
constexpr int KUU_EXTRA = 2 * GPK_MAX_D * T;   // the two slabs of a
constexpr int TAIL_ROWS = GPK_MS_TAIL_ROWS;

struct MsArgs {
  const double* X1; long ldx1; int n1;   // the tile's rows: X (Kfu), Z (Kuu)
  const double* X2; long ldx2; int n2;   // the tile's columns: Z
  int d;
  double* K; long ldk;
  const double* G; long ldg;             // op 1 / 2: the other factor / summand; the stage: Kbar
  const double* S; long lds;             // scales, laid out as Z
  double variance, diag_add;
  double* parts;
  double ell[GPK_MAX_D], ell2[GPK_MAX_D];   // l_j and l_j^2
};

// one row of a thread's 4 x 4 patch: two 16-byte stores where the tile is whole and aligned, else guarded
__device__ __forceinline__ void store_row(double* K, long ldk, int gr, int gc0, int nr, int nc, bool full, double v0, double v1, double v2,
                                          double v3) {
  if (full) {
    d2* out = reinterpret_cast<d2*>(K + (long)gr * ldk + gc0);
    out[0] = (d2){v0, v1};
    out[1] = (d2){v2, v3};
  } else if (gr < nr) {
    const double v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gc0 + j < nc) K[(long)gr * ldk + gc0 + j] = v[j];
  }
}

// OP 0: the build.  1 / 2: out = G .* Kfu / G + Kfu (out may alias G: an element is read and written by the same thread).
#define PAIR_OUT p.K
#define PAIR_LDO p.ldk
template <int OP>
__global__ __launch_bounds__(256) void ms_kfu_kernel(MsArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double s_px[T];
  const int d = p.d;
  double* xt = sm;                       // [d][T] raw rows of X
  double* zt = sm + (size_t)d * T;       // [d][T] raw rows of Z
  double* rt = sm + (size_t)2 * d * T;   // [d][T] 1 / (l_j + s_mj)
  double* cm = sm + (size_t)3 * d * T;   // [T]    v prod_j l_j r_mj
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  for (int e = tid; e < T * d; e += 256) {   // padding: x = z = s = 0.0, every value finite
    const int row = e / d, dd = e - row * d;
    const int g1 = r0 + row, g2 = c0 + row;
    const bool in2 = g2 < p.n2;
    xt[dd * T + row] = (g1 < p.n1) ? p.X1[(long)g1 * p.ldx1 + dd] : 0.0;
    zt[dd * T + row] = in2 ? p.X2[(long)g2 * p.ldx2 + dd] : 0.0;
    rt[dd * T + row] = 1.0 / (p.ell[dd] + (in2 ? p.S[(long)g2 * p.lds + dd] : 0.0));
  }
  __syncthreads();
  if (tid < T) {
    double c = p.variance;
    for (int dd = 0; dd < d; ++dd) c *= p.ell[dd] * rt[dd * T + tid];
    cm[tid] = c;
  } else if (tid < 2 * T) {   // 0.0 for a finite row of X, NaN for one that holds a NaN or an Inf
    double acc = 0.0;
    for (int dd = 0; dd < d; ++dd) acc = fma(xt[dd * T + tid - T], 0.0, acc);
    s_px[tid - T] = acc;
  }

  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int dd = 0; dd < d; ++dd) {
    const d2* a2 = reinterpret_cast<const d2*>(&xt[dd * T + ty * 4]);
    const d2* b2 = reinterpret_cast<const d2*>(&zt[dd * T + tx * 4]);
    const d2* r2 = reinterpret_cast<const d2*>(&rt[dd * T + tx * 4]);
    const d2 a01 = a2[0], a23 = a2[1], b01 = b2[0], b23 = b2[1], r01 = r2[0], r23 = r2[1];
    const double a[4] = {a01.x, a01.y, a23.x, a23.y};
    const double b[4] = {b01.x, b01.y, b23.x, b23.y};
    const double r[4] = {r01.x, r01.y, r23.x, r23.y};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double t = (a[i] - b[j]) * r[j];
        acc[i][j] = fma(t, t, acc[i][j]);
      }
  }
  __syncthreads();   // cm, s_px

#include "../pair_tile_full.inc"
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
    const double px = s_px[ty * 4 + i];
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      double k = cm[tx * 4 + j] * exp(-0.5 * acc[i][j]) + px;
      if constexpr (OP != 0) {
        const double g = (gr < p.n1 && gc < p.n2) ? p.G[(long)gr * p.ldg + gc] : 0.0;
        k = (OP == 2) ? g + k : g * k;
      }
      v[j] = k;
    }
    store_row(p.K, p.ldk, gr, c0 + tx * 4, p.n1, p.n2, full, v[0], v[1], v[2], v[3]);
  }
}

// MODE 0: the build -- tiles on or below the diagonal, each mirrored; diag_add on the diagonal.  1: out = G .* Kuu over every tile
// (G need not be symmetric; out may alias G).  3: the adjoint stage over the tiles on or below the diagonal (below).
template <int MODE>
__global__ __launch_bounds__(256) void ms_kuu_kernel(MsArgs p) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int d = p.d, M = p.n1;
  double* z1 = sm;                       // [d][T] z of the tile's rows
  double* z2 = sm + (size_t)d * T;       // [d][T] z of its columns
  double* a1 = sm + (size_t)2 * d * T;   // [d][T] (l + s)^2 of its rows
  double* a2 = sm + (size_t)3 * d * T;   // [d][T] and of its columns
  const int r0 = blockIdx.y * T, c0 = blockIdx.x * T;
  if (MODE != 1 && c0 > r0) return;      // a tile above the diagonal: written by its mirror (0), counted through it (3)
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  for (int e = tid; e < T * d; e += 256) {   // padding: z = s = 0.0, so q = 1 / l^2 there: finite
    const int row = e / d, dd = e - row * d;
    const int g1 = r0 + row, g2 = c0 + row;
    const bool in1 = g1 < M, in2 = g2 < M;
    const double t1 = p.ell[dd] + (in1 ? p.S[(long)g1 * p.lds + dd] : 0.0);
    const double t2 = p.ell[dd] + (in2 ? p.S[(long)g2 * p.lds + dd] : 0.0);
    z1[dd * T + row] = in1 ? p.X1[(long)g1 * p.ldx1 + dd] : 0.0;
    z2[dd * T + row] = in2 ? p.X1[(long)g2 * p.ldx1 + dd] : 0.0;
    a1[dd * T + row] = t1 * t1;
    a2[dd * T + row] = t2 * t2;
  }
  __syncthreads();

  double acc[4][4], pr[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i][j] = 0.0;
      pr[i][j] = 1.0;
    }
  for (int dd = 0; dd < d; ++dd) {
    const double l2 = p.ell2[dd];
    double za[4], zb[4], aa[4], ab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      za[i] = z1[dd * T + ty * 4 + i];
      aa[i] = a1[dd * T + ty * 4 + i];
      zb[i] = z2[dd * T + tx * 4 + i];
      ab[i] = a2[dd * T + tx * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double dl = za[i] - zb[j];
        const double q = 1.0 / ((aa[i] + ab[j]) - l2);
        acc[i][j] = fma(dl * dl, q, acc[i][j]);
        pr[i][j] *= l2 * q;
      }
  }

  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = c0 + tx * 4 + j;
      double k = p.variance * sqrt(pr[i][j]) * exp(-0.5 * acc[i][j]);
      if constexpr (MODE == 0) {
        if (gr == gc) k += p.diag_add;
      } else if constexpr (MODE == 1) {
        k *= (gr < M && gc < M) ? p.G[(long)gr * p.ldg + gc] : 0.0;
      } else {
        // g: what the pair {m, m'} carries -- Kbar[m, m'] + Kbar[m', m] off the diagonal, Kbar[m, m] on it; an element above the
        // diagonal or in the padding carries nothing (a select, never a product with 0: its k may be anything)
        const bool in = gr < M && gc <= gr;
        const double kb = !in ? 0.0 : gr == gc ? p.G[(long)gr * p.ldg + gc] : p.G[(long)gr * p.ldg + gc] + p.G[(long)gc * p.ldg + gr];
        k = in ? kb * k : 0.0;
      }
      v[i][j] = k;
    }
  }

  if constexpr (MODE != 3) {
    // (its own line: with pair_tile_full.inc's p.n1 / p.n2 for M the two kernels come out with other code)
    const bool full = (r0 + T <= M) && (c0 + T <= M) && ((p.ldk & 1) == 0) && ((reinterpret_cast<uintptr_t>(p.K) & 15) == 0);
    // In a diagonal tile of the build: a patch above the diagonal (tx > ty) is written by the mirror of the patch below it, a patch
    // on it (tx == ty) takes its upper entries from its lower ones.
    const bool diag_tile = MODE == 0 && r0 == c0;
#include "../pair_tile_diag_patch.inc"
    if (!(diag_tile && tx > ty)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) store_row(p.K, p.ldk, r0 + ty * 4 + i, c0 + tx * 4, M, M, full, v[i][0], v[i][1], v[i][2], v[i][3]);
    }
    if (MODE == 0 && (diag_tile ? tx < ty : true)) {   // the transposed copy: rows c0 + tx*4 + j, columns r0 + ty*4 + i
#pragma unroll
      for (int j = 0; j < 4; ++j) store_row(p.K, p.ldk, c0 + tx * 4 + j, r0 + ty * 4, M, M, full, v[0][j], v[1][j], v[2][j], v[3][j]);
    }
    return;
  } else {
    // The adjoint stage.  With g as above and w_j = D_j^2 q_j^2 - q_j, a counted element (m, m'), m' <= m, gives
    //   to row m  (slot bx of the row's block):      sum g,  sum g D_j q_j,  sum g w_j
    //   to row m' (slot by + 1, through the mirror):    -    -sum g D_j q_j,  sum g w_j        (D changes sign, the diagonal counts in both)
    // parts[(slot M + m) (2 d + 1) + {0, 1 + j, 1 + d + j}]: row m of block b has the slots 0 .. b (tiles (b, slot)) and b + 1 .. tr
    // (tiles (slot - 1, b)); entry 0 of a mirror slot is not written and not read.  Each entry is written by one thread: a thread's
    // four elements left to right, then the sixteen threads of a row by a butterfly over the lanes, the columns by a butterfly over the
    // four patch rows of a wave and then the four waves in order.
    __shared__ double colred[2][4][T][2];
    const long W = 2 * d + 1;
    const int lane = tid & 63, wave = tid >> 6;
    double* prow = p.parts + ((long)blockIdx.x * M + r0) * W;
    double* pcol = p.parts + ((long)(blockIdx.y + 1) * M + c0) * W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s = (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
      if (tx == 0 && r0 + ty * 4 + i < M) prow[(long)(ty * 4 + i) * W] = s;
    }
    for (int dd = 0; dd < d; ++dd) {
      const double l2 = p.ell2[dd];
      double za[4], zb[4], aa[4], ab[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        za[i] = z1[dd * T + ty * 4 + i];
        aa[i] = a1[dd * T + ty * 4 + i];
        zb[i] = z2[dd * T + tx * 4 + i];
        ab[i] = a2[dd * T + tx * 4 + i];
      }
      double rv[4] = {0.0, 0.0, 0.0, 0.0}, rw[4] = {0.0, 0.0, 0.0, 0.0}, cv[4] = {0.0, 0.0, 0.0, 0.0}, cw[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double dl = za[i] - zb[j];
          const double q = 1.0 / ((aa[i] + ab[j]) - l2);
          const double dq = dl * q;
          const double gv = v[i][j] * dq, gw = v[i][j] * (dq * dq - q);
          rv[i] += gv;
          rw[i] += gw;
          cv[j] -= gv;
          cw[j] += gw;
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          rv[i] += __shfl_xor(rv[i], o);
          rw[i] += __shfl_xor(rw[i], o);
        }
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          cv[i] += __shfl_xor(cv[i], o);
          cw[i] += __shfl_xor(cw[i], o);
        }
        if (tx == 0 && r0 + ty * 4 + i < M) {
          prow[(long)(ty * 4 + i) * W + 1 + dd] = rv[i];
          prow[(long)(ty * 4 + i) * W + 1 + d + dd] = rw[i];
        }
        if (lane < 16) {
          colred[dd & 1][wave][tx * 4 + i][0] = cv[i];
          colred[dd & 1][wave][tx * 4 + i][1] = cw[i];
        }
      }
      __syncthreads();   // (one per column: the buffer written here is read below while the next column fills the other one)
      if (tid < 2 * T) {
        const int c = tid & (T - 1), wh = tid >> 6;
        const double s = ((colred[dd & 1][0][c][wh] + colred[dd & 1][1][c][wh]) + colred[dd & 1][2][c][wh]) + colred[dd & 1][3][c][wh];
        if (c0 + c < M) pcol[(long)c * W + 1 + wh * d + dd] = s;
      }
    }
  }
}
#include "../pair_tile_end.inc"

// The tails.  Stage 1, a workgroup per TAIL_ROWS inducing points: thread t owns column t % d and walks the rows t / d, t / d + rpp, ...
// of its block; it finishes dZ and dscales of its (row, column)s and leaves the block's sums in blocks[b (1 + d) + {0, 1 + j}]:
//   symmetric (Kuu), from the stage's parts:  V, Wm = the row's slot sums in slot order,  S0 = those of the slots 0 .. b
//     dZ = -V      dscales = Wm (l + s)      block sums: S0 and Wm (l / 2 + s)
//   else (Kfu), from R [M, 1 + 2 d] = G^T [1, X, X^2] (columns S0, S1_j, S2_j), the moment identities:
//     dZ = r^2 (S1 - z S0)      dscales = r^3 ((S2 - 2 z S1) + z^2 S0) - r S0      block sums: S0 and dscales
// Stage 2, one workgroup, adds the blocks in order:  F = sum S0,  dv = F / v,  dl_j = sum_b blocks[b][1 + j] + F / l_j  (one lengthscale:
// their sum over j in column order).
struct MsTailArgs {
  const double* Z; long ldz; const double* S; long lds;
  int M, d, ard, symmetric, tr, nblk;
  const double* src; long ldsrc;
  double* blocks; double* dZ; long lddz; double* dS; long ldds; double* dsmall;
  double variance;
  double ell[GPK_MAX_D];
};

__global__ __launch_bounds__(TAIL_ROWS) void ms_tail_rows_kernel(MsTailArgs p) {
  __shared__ double sh[TAIL_ROWS], sh0[TAIL_ROWS];
  const int t = threadIdx.x, d = p.d, M = p.M, rpp = TAIL_ROWS / d, c = t % d, q0 = t / d;
  const int m0 = blockIdx.x * TAIL_ROWS, m1 = min(M, m0 + TAIL_ROWS);
  double acc = 0.0, acc0 = 0.0;
  if (q0 < rpp) {
    const double l = p.ell[c];
    for (int m = m0 + q0; m < m1; m += rpp) {
      const double z = p.Z[(long)m * p.ldz + c], s = p.S[(long)m * p.lds + c];
      double s0 = 0.0, dz, ds, lt;
      if (p.symmetric) {
        const long W = 2 * d + 1;
        const int b = m / T;
        double V = 0.0, Wm = 0.0;
        for (int slot = 0; slot <= p.tr; ++slot) {
          const double* e = p.src + ((long)slot * M + m) * W;
          V += e[1 + c];
          Wm += e[1 + d + c];
          if (c == 0 && slot <= b) s0 += e[0];
        }
        dz = -V;
        ds = Wm * (l + s);
        lt = Wm * (0.5 * l + s);
      } else {
        const double* R = p.src + (long)m * p.ldsrc;
        const double S1 = R[1 + c], S2 = R[1 + d + c], r = 1.0 / (l + s);
        s0 = R[0];
        dz = r * r * (S1 - z * s0);
        ds = r * r * r * ((S2 - 2.0 * z * S1) + z * z * s0) - r * s0;
        lt = ds;
      }
      p.dZ[(long)m * p.lddz + c] = dz;
      p.dS[(long)m * p.ldds + c] = ds;
      acc += lt;
      if (c == 0) acc0 += s0;
    }
  }
  sh[t] = acc;
  sh0[t] = acc0;
  __syncthreads();
  double* blk = p.blocks + (long)blockIdx.x * (1 + d);
  if (t < d) {
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh[q * d + t];
    blk[1 + t] = s;
  } else if (t == TAIL_ROWS - 1) {   // (d <= 64: never one of the threads above)
    double s = 0.0;
    for (int q = 0; q < rpp; ++q) s += sh0[q * d];
    blk[0] = s;
  }
}

__global__ __launch_bounds__(128) void ms_tail_blocks_kernel(MsTailArgs p) {
  __shared__ double sh[GPK_MAX_D], shF;
  const int t = threadIdx.x, d = p.d;
  if (t < d) {
    double s = 0.0;
    for (int b = 0; b < p.nblk; ++b) s += p.blocks[(long)b * (1 + d) + 1 + t];
    sh[t] = s;
  } else if (t == 127) {
    double s = 0.0;
    for (int b = 0; b < p.nblk; ++b) s += p.blocks[(long)b * (1 + d)];
    shF = s;
  }
  __syncthreads();
  if (t < d) {
    const double dl = sh[t] + shF / p.ell[t];
    if (p.ard) p.dsmall[1 + t] = dl;
    sh[t] = dl;
  }
  __syncthreads();
  if (t == 0) {
    p.dsmall[0] = shF / p.variance;
    if (!p.ard) {
      double s = 0.0;
      for (int j = 0; j < d; ++j) s += sh[j];
      p.dsmall[1] = s;
    }
  }
}

// what every entry point checks of the kernel before it looks at an operand; l_j spread over the d columns
int read_ms_kernel(double* ell, double* ell2, int d, const double* ls_host, int ard, double variance) {
  if (d <= 0 || d > GPK_MAX_D || !ls_host) return GPK_E_ARG;
  GPK_TRY(spread_weights(ell, d, ls_host, ard, /*allow_negative=*/false));
  for (int j = 0; j < d; ++j) {
    if (!(ell[j] > 0.0)) return GPK_E_ARG;
    if (ell2) ell2[j] = ell[j] * ell[j];
  }
  if (!std::isfinite(variance) || !(variance > 0.0)) return GPK_E_ARG;
  return 0;
}

template <int OP>
int launch_kfu(hipStream_t st, const MsArgs& a) {
  GPK_HIP((allow_tile_lds<ms_kfu_kernel<OP>, KFU_EXTRA>()));
  const size_t lds = ((size_t)3 * a.d * T + T) * sizeof(double);   // 98.5 KB at d = 64
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((ms_kfu_kernel<OP>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
int launch_kuu(hipStream_t st, const MsArgs& a) {
  GPK_HIP((allow_tile_lds<ms_kuu_kernel<MODE>, KUU_EXTRA>()));
  const size_t lds = (size_t)4 * a.d * T * sizeof(double);   // 128 KB at d = 64
  dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));
  hipLaunchKernelGGL((ms_kuu_kernel<MODE>), grid, dim3(256), lds, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" size_t gpk_multiscale_parts_len(int M, int d) {
  if (M <= 0 || d <= 0) return 0;
  return (size_t)(gpk_cdiv(M, T) + 1) * (size_t)M * (size_t)(2 * d + 1);
}

extern "C" int gpk_multiscale_kfu(void* stream, const double* X, int n, long ldx, const double* Z, const double* S, int M, long ldz, long lds,
                                  int d, const double* ls_host, int ard, double variance, int op, const double* G, long ldg, double* out,
                                  long ldo) {
  if (n < 0 || M < 0) return GPK_E_ARG;
  MsArgs a{};
  GPK_TRY(read_ms_kernel(a.ell, nullptr, d, ls_host, ard, variance));
  if (op < 0 || op > 2 || ldx < d || ldz < d || lds < d || ldo < M || (op != 0 && ldg < M)) return GPK_E_ARG;
  if (n == 0 || M == 0) return 0;
  if (!X || !Z || !S || !out || (op != 0 && !G)) return GPK_E_ARG;
  set_operands<KFU_EXTRA>(a, X, n, ldx, Z, M, ldz, d, out, ldo, G, ldg);
  a.S = S; a.lds = lds; a.variance = variance;
  const hipStream_t st = (hipStream_t)stream;
  return op == 0 ? launch_kfu<0>(st, a) : op == 1 ? launch_kfu<1>(st, a) : launch_kfu<2>(st, a);
}

extern "C" int gpk_multiscale_kuu(void* stream, const double* Z, const double* S, int M, long ldz, long lds, int d, const double* ls_host,
                                  int ard, double variance, double diag_add, int op, const double* G, long ldg, double* out, long ldo) {
  if (M < 0) return GPK_E_ARG;
  MsArgs a{};
  GPK_TRY(read_ms_kernel(a.ell, a.ell2, d, ls_host, ard, variance));
  if (op < 0 || op > 1 || ldz < d || lds < d || ldo < M || (op != 0 && ldg < M)) return GPK_E_ARG;
  if (M == 0) return 0;
  if (!Z || !S || !out || (op != 0 && !G)) return GPK_E_ARG;
  set_operands<KUU_EXTRA>(a, Z, M, ldz, nullptr, 0, 0, d, out, ldo, G, ldg);
  a.S = S; a.lds = lds; a.variance = variance; a.diag_add = diag_add;
  const hipStream_t st = (hipStream_t)stream;
  return op == 0 ? launch_kuu<0>(st, a) : launch_kuu<1>(st, a);
}

extern "C" int gpk_multiscale_kuu_adjoint_stage(void* stream, const double* Z, const double* S, int M, long ldz, long lds, int d,
                                                const double* ls_host, int ard, double variance, const double* Kbar, long ldkb,
                                                double* parts, long parts_len) {
  if (M < 0) return GPK_E_ARG;
  MsArgs a{};
  GPK_TRY(read_ms_kernel(a.ell, a.ell2, d, ls_host, ard, variance));
  if (ldz < d || lds < d || ldkb < M || parts_len < 0 || (size_t)parts_len < gpk_multiscale_parts_len(M, d)) return GPK_E_ARG;
  if (M == 0) return 0;
  if (!Z || !S || !Kbar || !parts) return GPK_E_ARG;
  set_operands<KUU_EXTRA>(a, Z, M, ldz, nullptr, 0, 0, d, nullptr, 0, Kbar, ldkb);
  a.S = S; a.lds = lds; a.variance = variance; a.parts = parts;
  return launch_kuu<3>((hipStream_t)stream, a);
}

extern "C" int gpk_multiscale_adjoint_tail(void* stream, int symmetric, const double* Z, const double* S, int M, long ldz, long lds, int d,
                                           const double* ls_host, int ard, double variance, const double* src, long ldsrc, long src_len,
                                           double* blocks, double* dZ, long lddz, double* dS, long ldds, double* dsmall) {
  if (M < 0) return GPK_E_ARG;
  MsTailArgs a{};
  GPK_TRY(read_ms_kernel(a.ell, nullptr, d, ls_host, ard, variance));
  if (ldz < d || lds < d || lddz < d || ldds < d) return GPK_E_ARG;
  if (symmetric ? (src_len < 0 || (size_t)src_len < gpk_multiscale_parts_len(M, d)) : ldsrc < 1 + 2 * d) return GPK_E_ARG;
  if (M == 0) return 0;
  if (!Z || !S || !src || !blocks || !dZ || !dS || !dsmall) return GPK_E_ARG;
  a.Z = Z; a.ldz = ldz; a.S = S; a.lds = lds; a.M = M; a.d = d; a.ard = ard ? 1 : 0; a.symmetric = symmetric ? 1 : 0;
  a.tr = gpk_cdiv(M, T); a.nblk = gpk_cdiv(M, TAIL_ROWS);
  a.src = src; a.ldsrc = ldsrc; a.blocks = blocks; a.dZ = dZ; a.lddz = lddz; a.dS = dS; a.ldds = ldds; a.dsmall = dsmall;
  a.variance = variance;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ms_tail_rows_kernel, dim3((unsigned)a.nblk), dim3(TAIL_ROWS), 0, st, a);
  GPK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_tail_blocks_kernel, dim3(1), dim3(128), 0, st, a);
  GPK_LAUNCH_CHECK();
  return 0;
}
