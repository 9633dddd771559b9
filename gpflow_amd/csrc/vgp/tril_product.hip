// gpk_tril_product (include/gpk.h): P_r = L S_r for lower-triangular L and S_r, with the row sum of squares as the epilogue (the
// product is not stored) or rowscale .* P_r stored below the diagonal -- the hot path of the full variational GP (models/vgp.py).
//
// One 128 x 128 output tile (bi, bj), bj <= bi, per workgroup: 256 threads = 4 waves (2 x 2), wave tile 64 x 64 = 4 x 4 blocks of
// v_mfma_f64_16x16x4_f64 (A frag: row = lane & 15, k = lane >> 4; B frag: k = lane >> 4, col = lane & 15; D: col = lane & 15,
// row = (lane >> 4) + 4 reg).  K runs over the tile-block range only, columns 128 bj .. min(128 (bi + 1), n), in slabs of 16 staged
// global -> VGPR -> LDS; both operands are read row-major (L tile [128][16], rows padded to 18 doubles; S tile [16][128], rows padded
// to 144: the 32-lane ds_read_b64 groups hit 64 distinct banks either way), so there is no transpose pass.
//
// The triangle at 16 x 16 granularity.  For the block (r0, c0) of the output and the slab ks (all multiples of 16):
//     ks < c0 or ks > r0      every term has k < j or k > i: the slab is skipped (a block with r0 < c0 skips every slab);
//     c0 < ks < r0            every term is inside both triangles: MFMA;
//     ks == c0 or ks == r0    the slab crosses a diagonal: VALU, each term under the predicate j <= k <= i.
// A masked entry of L or S is never loaded (its LDS slot holds 0), and a product with it is never FORMED -- 0 x NaN is NaN, so a
// zero-filled MFMA over a diagonal slab would carry a NaN of S[k, .] into the rows i < k of its block.  The diagonal slabs are two of
// the (r0 - c0) / 16 + 1 of a block.
//
// Tiles have K lengths from 1 to nb tile blocks: the grid is one-dimensional and walks the block diagonals from the longest
// (bi - bj = nb - 1) to the main one, the R latents of a tile next to each other, so the last workgroups to start are the shortest.
// ssq: every tile leaves the row sums over its 128 columns in parts[r, bj, i]; tril_rowsum_kernel adds them in the order bj = 0, 1, ..
#include "../gpk_internal.h"

namespace {

constexpr int TT = GPK_TRIL_TILE;   // output tile edge
constexpr int BK = 16;              // K slab
constexpr int LDA = 18;             // doubles per row of the L tile in LDS
constexpr int LDB = 144;            // doubles per row of the S tile in LDS
static_assert(TT == 128, "the wave layout below is 2 x 2 waves of 64 x 64");

struct TrilArgs {
  const double* L; long ldl;
  const double* S; long lds, stride_s;
  int n, R, nb;
  double* parts;                    // [R, nb, n], null: no row sums
  const double* rowscale;           // [R, n] or null
  double* T; long ldt, stride_t;    // null: the product is not stored
};

// (two workgroups per CU -- one's staging barriers under the other's MFMAs: 253 VGPRs, no AGPR copies, no scratch)
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(256) void tril_product_kernel(const TrilArgs a) {
  __shared__ double As[TT * LDA];
  __shared__ double Bs[BK * LDB];
  __shared__ double red[2 * TT];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, l15 = lane & 15, lq = lane >> 4;
  const int r = (int)(blockIdx.x % (unsigned)a.R);
  int t = (int)(blockIdx.x / (unsigned)a.R);
  int d = a.nb - 1;                 // block diagonal bi - bj = d holds nb - d tiles
  while (t >= a.nb - d) { t -= a.nb - d; --d; }
  const int bi = d + t, bj = t;
  const int I0 = bi * TT, J0 = bj * TT, n = a.n;
  const double* __restrict__ L = a.L;
  const double* __restrict__ S = a.S + (long)r * a.stride_s;
  const bool vec_ok = ((a.ldl & 1) == 0) && ((a.lds & 1) == 0) && ((a.stride_s & 1) == 0) &&
                      ((reinterpret_cast<uintptr_t>(a.L) & 15) == 0) && ((reinterpret_cast<uintptr_t>(a.S) & 15) == 0);

  // staging slots: L tile row tid >> 1, k offset 8 (tid & 1); S tile row (k) tid >> 4, column offset 8 (tid & 15)
  const int arow = tid >> 1, ak = (tid & 1) * 8;
  const int bk = tid >> 4, bc = (tid & 15) * 8;
  double ra[8], rb[8];
  auto gload = [&](int ks) {
    const int gi = I0 + arow;
    const double* pa = L + (long)gi * a.ldl + ks + ak;
    if (vec_ok && ks + BK - 1 <= I0 && I0 + TT <= n) {          // (block-uniform) no entry of the slab is masked
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(pa + e);
        ra[e] = v[0]; ra[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) ra[e] = (gi < n && ks + ak + e <= gi) ? pa[e] : 0.0;
    }
    const int gk = ks + bk;
    const double* pb = S + (long)gk * a.lds + J0 + bc;
    if (vec_ok && J0 + TT - 1 <= ks && ks + BK <= n) {
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const d2 v = *reinterpret_cast<const d2*>(pb + e);
        rb[e] = v[0]; rb[e + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) rb[e] = (gk < n && J0 + bc + e <= gk) ? pb[e] : 0.0;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      *reinterpret_cast<d2*>(&As[arow * LDA + ak + e]) = (d2){ra[e], ra[e + 1]};
      *reinterpret_cast<d2*>(&Bs[bk * LDB + bc + e]) = (d2){rb[e], rb[e + 1]};
    }
  };

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  const int R0 = I0 + wr * 64, C0 = J0 + wc * 64;   // this wave's 64 x 64
  const bool wave_live = R0 + 63 >= C0;             // (the upper-right wave of a diagonal tile has nothing below the diagonal)
  const double* as = As + (wr * 64 + l15) * LDA + lq;        // MFMA fragments
  const double* bs = Bs + lq * LDB + wc * 64 + l15;
  const int kend = (I0 + TT < n ? I0 + TT : n);     // K range [J0, kend)
  const int nslab = (kend - J0 + BK - 1) / BK;

  gload(J0);
  for (int s = 0; s < nslab; ++s) {
    const int ks = J0 + s * BK;
    lstore();
    __syncthreads();
    if (s + 1 < nslab) gload(ks + BK);              // in flight under this slab's arithmetic
    if (wave_live) {
      if (ks >= C0 + 64 && ks + BK <= R0) {         // strictly between the diagonals for all 16 blocks of the wave
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
          double fa[4], fb[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) fa[i] = as[i * 16 * LDA + kk * 4];
#pragma unroll
          for (int j = 0; j < 4; ++j) fb[j] = bs[kk * 4 * LDB + j * 16];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r0 = R0 + i * 16, c0 = C0 + j * 16;
            if (ks < c0 || ks > r0) continue;       // (wave-uniform)
            if (ks != c0 && ks != r0) {
#pragma unroll
              for (int kk = 0; kk < BK / 4; ++kk)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i * 16 * LDA + kk * 4], bs[kk * 4 * LDB + j * 16], acc[i][j], 0, 0, 0);
            } else {                                 // a diagonal slab: every term under j <= k <= i
              const int col = c0 + l15;
              const double* av = As + (wr * 64 + i * 16 + lq) * LDA;
              const double* bv = Bs + wc * 64 + j * 16 + l15;
#pragma unroll 4
              for (int kk = 0; kk < BK; ++kk) {
                const int k = ks + kk;
                const double b = bv[kk * LDB];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                  const double p = fma(av[4 * g * LDA + kk], b, acc[i][j][g]);
                  if (k >= col && k <= r0 + lq + 4 * g) acc[i][j][g] = p;
                }
              }
            }
          }
      }
    }
    __syncthreads();
  }

  // ---- epilogue ---------------------------------------------------------------------------------
  const int row_base = R0 + lq, col_base = C0 + l15;
  if (a.T) {
    double* __restrict__ T = a.T + (long)r * a.stride_t;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = row_base + i * 16 + 4 * g;
        if (row >= n) continue;
        const double rs = a.rowscale ? a.rowscale[(long)r * n + row] : 1.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = col_base + j * 16;
          if (col <= row) T[(long)row * a.ldt + col] = rs * acc[i][j][g];
        }
      }
  }
  if (a.parts) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fma(acc[i][j][g], acc[i][j][g], s);   // (a block above the diagonal holds zeros)
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        if (l15 == 0) red[wc * TT + wr * 64 + i * 16 + lq + 4 * g] = s;
      }
    __syncthreads();
    if (tid < TT && I0 + tid < n) a.parts[((long)r * a.nb + bj) * n + I0 + tid] = red[tid] + red[TT + tid];
  }
}

// ssq[r, i] = sum over the tile columns t = 0 .. i / 128 of parts[r, t, i], in that order
__global__ __launch_bounds__(256) void tril_rowsum_kernel(const double* __restrict__ parts, int n, int R, int nb, double* __restrict__ ssq) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)R * n) return;
  const int r = (int)(idx / n), i = (int)(idx % n);
  const double* p = parts + (long)r * nb * n + i;
  double s = 0.0;
  for (int t = 0; t <= i / TT; ++t) s += p[(long)t * n];
  ssq[idx] = s;
}

}  // namespace

extern "C" int gpk_tril_product_tiles(int n) { return n > 0 ? gpk_cdiv(n, TT) : 0; }

extern "C" int gpk_tril_product(void* stream, const double* L, int n, long ldl, const double* S, long lds, long stride_s, int R,
                                double* ssq, double* parts, const double* rowscale, double* T, long ldt, long stride_t) {
  if (n < 0 || R < 0) return GPK_E_ARG;
  if (n == 0 || R == 0) return 0;
  if (!L || !S || ldl < n || lds < n) return GPK_E_ARG;
  if (!ssq && !T) return GPK_E_ARG;
  if (ssq && !parts) return GPK_E_ARG;
  if (T && ldt < n) return GPK_E_ARG;
  if (rowscale && !T) return GPK_E_ARG;
  const int nb = gpk_cdiv(n, TT);
  const long tiles = (long)nb * (nb + 1) / 2 * R;
  if (tiles > 0x7fffffffL) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  TrilArgs a{L, ldl, S, lds, stride_s, n, R, nb, ssq ? parts : nullptr, rowscale, T, ldt, stride_t};
  hipLaunchKernelGGL(tril_product_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
  GPK_LAUNCH_CHECK();
  if (ssq) {
    const long blocks = ((long)R * n + 255) / 256;
    hipLaunchKernelGGL(tril_rowsum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, parts, n, R, nb, ssq);
    GPK_LAUNCH_CHECK();
  }
  return 0;
}
