// fp64 MFMA GEMM for gfx950:  C = alpha * A * B^T + beta * C   (A [m,k], B [n,k], row-major).
//
// Every matmul-shaped piece of the dense-GP path is this one kernel:
//   * Cholesky panel solve  X = A21 * inv(L11)^T          (in place, b_tri = 2)
//   * Cholesky trailing / look-ahead updates  C -= P P^T   (c_lower, alpha=-1, beta=1)
//   * triangular solves against a cached factor            (gpk_trsm)
//   * the projection  A^T [Lq | q_mu]  with a fused row-sum-of-squares epilogue (epi = 1)
//
// Design (CDNA4): 256 threads = 4 waves (2x2), workgroup tile BM x BN, wave tile (BM/2) x (BN/2)
// built from v_mfma_f64_16x16x4_f64 (A frag: row = lane&15, k = lane>>4, one f64 per lane; same for
// the B^T frag; D: col = lane&15, row = (lane>>4) + 4*reg).  K is walked in BK=16 slabs, staged
// global -> VGPR -> LDS with register double-buffering and one barrier per slab.  LDS rows are
// padded to 18 doubles (144 B): the 32-lane ds_read_b64 groups then hit 64 distinct banks.
// 2 workgroups/CU (73.7 KB LDS each) keep one wave per SIMD issuing MFMAs while the other waits.
// Block ids are remapped so that (a) each XCD gets a contiguous range of tiles (private L2s) and
// (b) tiles are swept in 8-wide column groups (A/B panel reuse out of the 4 MiB L2).
#include "gpk_internal.h"
#include <mutex>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

namespace {

constexpr int BK = kGemmBK;
constexpr int LDSS = kGemmLDSS;
constexpr int GROUP_N = kGemmGroupN;

template <int BM, int BN, int WGM, int WGN>
struct TileCfg {
  static constexpr int WM = BM / WGM, WN = BN / WGN;
  static constexpr int TM = WM / 16, TN = WN / 16;
  static constexpr int A_CH = BM * (BK / 2) / 256;
  static constexpr int B_CH = BN * (BK / 2) / 256;
  static constexpr size_t LDS_BYTES = 2 * (size_t)(BM + BN) * LDSS * sizeof(double);
};

// ---- XCD-contiguous + column-grouped tile order -------------------------------------------------
// Tiles are numbered group-of-8-columns major, row-major inside a group; each XCD takes a
// contiguous 1/8 of that sequence.  With c_lower (and square tiles) only the tiles on or below
// the diagonal are numbered, so every XCD gets the same amount of work.
// position nl of the tile sequence -> (tile_m, tile_n)
__device__ __forceinline__ void tile_decode(int nl, int gx, int gy, int compact, int& tile_m, int& tile_n) {
  tile_m = 0; tile_n = 0;
  if (compact) {
    int g = 0;
    for (;; ++g) {
      const int first = g * GROUP_N;
      const int gsz = (gx - first) < GROUP_N ? (gx - first) : GROUP_N;
      const int avail = gy - first;
      const int tr = avail < gsz ? avail : gsz;
      const int cnt = tr * (tr + 1) / 2 + (avail > gsz ? (avail - gsz) * gsz : 0);
      if (nl < cnt) {
        int ro = 0, co = nl;
        const int tri = gsz * (gsz + 1) / 2;
        if (nl < tri) {
          while (co > ro) { co -= ro + 1; ++ro; }
        } else {
          const int w = nl - tri;
          ro = gsz + w / gsz;
          co = w - (w / gsz) * gsz;
        }
        tile_m = first + ro;
        tile_n = first + co;
        break;
      }
      nl -= cnt;
    }
  } else {
    const int gspan = GROUP_N * gy;
    const int group = nl / gspan, within = nl - group * gspan;
    const int first_n = group * GROUP_N;
    const int gsz = (gx - first_n) < GROUP_N ? (gx - first_n) : GROUP_N;
    tile_n = first_n + within % gsz;
    tile_m = within / gsz;
  }
}

__device__ __forceinline__ void tile_order(int lin, int b_tri, int gx, int gy, int total, int compact, int& tile_m,
                                           int& tile_n) {
  const int xcd = lin & 7, local = lin >> 3;
  const int q = total >> 3, r = total & 7;
  int nl = xcd * q + (xcd < r ? xcd : r) + local;
  // triangular-K work (b_tri = 1, many column tiles) is heaviest in the first column groups:
  // keep plain round-robin there so all XCDs walk the groups together, heaviest first
  if (b_tri == 1 && gx > GROUP_N) nl = lin;
  tile_decode(nl, gx, gy, compact, tile_m, tile_n);
}

__device__ __forceinline__ d2 load2(const double* __restrict__ base, long ld, int row, int nrows,
                                    int k, int ke, bool vec_ok) {
  d2 v = {0.0, 0.0};
  if (row < nrows && k < ke) {
    const double* ptr = base + (long)row * ld + k;
    if (vec_ok && k + 1 < ke) {
      v = *reinterpret_cast<const d2*>(ptr);
    } else {
      v.x = ptr[0];
      if (k + 1 < ke) v.y = ptr[1];
    }
  }
  return v;
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(GemmArgs p, int gx, int gy, int total, int compact) {
  using Cfg = TileCfg<BM, BN, WGM, WGN>;
  constexpr int WM = Cfg::WM, WN = Cfg::WN, TM = Cfg::TM, TN = Cfg::TN;
  constexpr int A_CH = Cfg::A_CH, B_CH = Cfg::B_CH;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // entry signal of a stream hand-off without queue packets (GemmArgs::sig_ptr, as in gemm_nt_small): "everything queued before
  // this kernel on its stream has completed"
  if (p.sig_ptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0)
    __hip_atomic_store(p.sig_ptr, p.sig_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int bz = p.k_off_step ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;   // (see fast_tile)

  int tile_m, tile_n;
  if (BM == 64 && BN == 64 && p.tail_first1 > 0) {
    // the last, partial round of a lower-only launch of the 128 x 128 fast tile (launch_fast, "tail split"): positions
    // tail_first + blockIdx.x / 4 of ITS tile sequence (gx, gy in 128-tiles), each as four 64 x 64 quarters
    int tm, tn;
    tile_decode(p.tail_first1 - 1 + ((int)blockIdx.x >> 2), gx, gy, compact, tm, tn);
    tile_m = 2 * tm + (((int)blockIdx.x >> 1) & 1);
    tile_n = 2 * tn + ((int)blockIdx.x & 1);
  } else if (p.tile_snake) {
    // under-filled triangular-K launches (every workgroup resident at once, column tile 0 the heaviest): workgroups x, x + 256,
    // x + 512, ... land on the same compute unit (round-robin placement), so round 0 takes the heaviest 256 tiles in falling
    // order, round 1 the LIGHTEST 256 in rising order, round 2 the next heaviest, ... -- every CU gets the same K total.
    // (A batch of problems with ONE round each alternates the direction from problem to problem instead.)
    const int r = (int)blockIdx.x >> 8, c = (int)blockIdx.x & 255, R = (int)gridDim.x >> 8;
    const int rr = (r & 1) ? R - 1 - (r >> 1) : (r >> 1);
    if (p.tile_snake == 2) {
      // ... and each XCD (workgroup x runs on XCD x % 8) keeps gy / 8 row tiles to itself: A is read by one L2 only
      const int xcd = c & 7, s = c >> 3, rpx = gy >> 3;
      const int q = rr * 32 + (((r ^ bz) & 1) ? 31 - s : s);
      tile_n = q / rpx;
      tile_m = xcd * rpx + (q - tile_n * rpx);
    } else {
      const int nl = rr * 256 + ((r & 1) ? 255 - c : c);
      if (nl >= total) return;
      tile_n = nl / gy;
      tile_m = nl - tile_n * gy;
    }
  } else {
    tile_order(blockIdx.x, p.b_tri, gx, gy, total, compact, tile_m, tile_n);
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (p.c_lower && n0 > m0 + BM - 1) return;
  if (m0 >= p.m || n0 >= p.n) return;

  const double* __restrict__ A = p.A + (long)bz * p.strideA;
  const double* __restrict__ B = p.B + (long)bz * p.strideB;

  int kb = 0, ke = p.k;
  const int koff = bz * p.k_off_step;   // (K-split of a triangular product: this batch entry holds columns koff .. koff + k of the operands)
  if (p.b_tri && (n0 + BN < p.n ? n0 + BN : p.n) <= p.b_tri_rows) {   // (the tile's existing rows; a partial last tile too)
    if (p.b_tri == 1) {
      int f = n0 + p.b_tri_off - koff;
      kb = (f > 0 ? f : 0) & ~(BK - 1);
    } else {
      int l = n0 + BN + p.b_tri_off - koff;
      ke = l < p.k ? l : p.k;
    }
  }
  if (p.a_tri == 1) {         // rows m0.. of an upper-triangular A are zero left of column m0
    int f = m0 - koff;
    f = (f > 0 ? f : 0) & ~(BK - 1);
    kb = kb > f ? kb : f;
  } else if (p.a_tri == 2) {  // rows ..m0+BM-1 of a lower-triangular A are zero right of column m0+BM-1
    int l = ((m0 + BM + BK - 1) & ~(BK - 1)) - koff;
    l = l < p.k ? l : p.k;
    ke = ke < l ? ke : l;
  }
  const bool vec_ok = ((p.lda & 1) == 0) && ((p.ldb & 1) == 0) &&
                      ((reinterpret_cast<uintptr_t>(A) & 15) == 0) &&
                      ((reinterpret_cast<uintptr_t>(B) & 15) == 0);

  constexpr int BUF = (BM + BN) * LDSS;  // doubles per LDS buffer: [A tile | B tile]

  d4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // per-thread staging slots: chunk c = tid + 256 q  ->  tile row c>>3, k offset (c&7)*2.
  // Rows are clamped (then zero-selected) so the fast path is branch-free: all loads of a slab
  // are issued back to back and drain under the MFMAs of the previous slabs.
  // TWO register sets (round 6, late): the loads of slab s+2 go out at the top of slab s, so a slab's data has two slab times to
  // arrive instead of one.  This kernel's slab is short -- 16 MFMAs per wave for a 64 x 64 tile, 0.43 us -- and its K loop ran at the
  // global-load round trip instead (0.97 us per slab: the 64 x 64 remainders of the capped extra-row updates, K = 512, took 62 / 52 /
  // 35 us per SVGP step; the heaviest tile of a few-row projection walks 128 slabs).  Same arithmetic, same order.
  d2 ra0[A_CH], rb0[B_CH], ra1[A_CH], rb1[B_CH];
  const double* pa[A_CH];
  const double* pb[B_CH];
  bool va[A_CH], vb[B_CH];
#pragma unroll
  for (int q = 0; q < A_CH; ++q) {
    const int c = tid + 256 * q;
    const int row = m0 + (c >> 3);
    va[q] = row < p.m;
    pa[q] = A + (long)(va[q] ? row : p.m - 1) * p.lda + (c & 7) * 2;
  }
#pragma unroll
  for (int q = 0; q < B_CH; ++q) {
    const int c = tid + 256 * q;
    const int row = n0 + (c >> 3);
    vb[q] = row < p.n;
    pb[q] = B + (long)(vb[q] ? row : p.n - 1) * p.ldb + (c & 7) * 2;
  }
  const d2 zero2 = {0.0, 0.0};
  auto gload = [&](int k0, d2* __restrict__ ra, d2* __restrict__ rb) {
    if (vec_ok && k0 + BK <= ke) {  // wave-uniform
#pragma unroll
      for (int q = 0; q < A_CH; ++q) {
        ra[q] = *reinterpret_cast<const d2*>(pa[q] + k0);
      }
#pragma unroll
      for (int q = 0; q < B_CH; ++q) {
        rb[q] = *reinterpret_cast<const d2*>(pb[q] + k0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < A_CH; ++q) {
        const int c = tid + 256 * q;
        ra[q] = load2(A, p.lda, m0 + (c >> 3), p.m, k0 + (c & 7) * 2, ke, false);
      }
#pragma unroll
      for (int q = 0; q < B_CH; ++q) {
        const int c = tid + 256 * q;
        rb[q] = load2(B, p.ldb, n0 + (c >> 3), p.n, k0 + (c & 7) * 2, ke, false);
      }
    }
  };
  auto lstore = [&](int buf, const d2* __restrict__ ra, const d2* __restrict__ rb) {
#pragma unroll
    for (int q = 0; q < A_CH; ++q) {
      const int c = tid + 256 * q;
      *reinterpret_cast<d2*>(&smem[buf * BUF + (c >> 3) * LDSS + (c & 7) * 2]) =
          va[q] ? ra[q] : zero2;
    }
#pragma unroll
    for (int q = 0; q < B_CH; ++q) {
      const int c = tid + 256 * q;
      *reinterpret_cast<d2*>(&smem[buf * BUF + (BM + (c >> 3)) * LDSS + (c & 7) * 2]) =
          vb[q] ? rb[q] : zero2;
    }
  };

  const int nkt = ke > kb ? (ke - kb + BK - 1) / BK : 0;
  if (nkt > 0) {
    gload(kb, ra0, rb0);
    lstore(0, ra0, rb0);
    if (nkt > 1) gload(kb + BK, ra1, rb1);
    __syncthreads();
  }
  const int frag_r = lane & 15, frag_k = lane >> 4;
  // slab j travels in register set j & 1: at slab kt its own set is free again (stored to LDS during slab kt - 1) and takes slab
  // kt + 2; the other set holds slab kt + 1, requested a whole slab ago
  auto step = [&](int kt, d2* __restrict__ fa_, d2* __restrict__ fb_, const d2* __restrict__ na_, const d2* __restrict__ nb_) {
    const int cur = kt & 1;
    if (kt + 2 < nkt) gload(kb + (kt + 2) * BK, fa_, fb_);
    __builtin_amdgcn_sched_barrier(0);   // (the loads go out BEFORE anything waits for the other set: without this the zero-select of lstore is hoisted above them)
    const double* as = smem + cur * BUF + (wm * WM + frag_r) * LDSS + frag_k;
    const double* bs = smem + cur * BUF + (BM + wn * WN + frag_r) * LDSS + frag_k;
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = as[i * 16 * LDSS + kk * 4];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = bs[j * 16 * LDSS + kk * 4];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nkt) lstore(cur ^ 1, na_, nb_);
    __syncthreads();
  };
  for (int kt = 0; kt < nkt; kt += 2) {
    step(kt, ra0, rb0, ra1, rb1);
    if (kt + 1 < nkt) step(kt + 1, ra1, rb1, ra0, rb0);
  }

  // ---- epilogue ---------------------------------------------------------------------------------
  const int row_base = m0 + wm * WM + (lane >> 4);
  const int col_base = n0 + wn * WN + (lane & 15);
  if (p.epi == 0) {
    double* __restrict__ C = p.C + (long)bz * p.strideC;
    const double alpha = p.alpha, beta = p.beta;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row_base + i * 16 + 4 * r;
        if (row < p.m) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int col = col_base + j * 16;
            if (col < p.n) {
              double* cp = C + (long)row * p.ldc + col;
              double v = alpha * acc[i][j][r];
              if (beta != 0.0) v += beta * (*cp);
              *cp = v;
            }
          }
        }
      }
  } else {
    double* __restrict__ C2 = p.C2 + (long)bz * p.strideC2;
    double* __restrict__ part = p.part + (long)bz * p.stridePart;
    const double alpha = p.alpha;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row_base + i * 16 + 4 * r;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = col_base + j * 16;
          const double v = alpha * acc[i][j][r];
          if (col < p.sq_cols) {
            s += v * v;
          } else if (row < p.m && col - p.sq_cols < p.c2_cols && col < p.n) {
            C2[(long)row * p.ldc2 + (col - p.sq_cols)] = v;
          }
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        // one partial per 64 columns of the output: tile_n * (BN / 64) + (this wave's 64-column slot within the tile)
        if constexpr (WN >= 64) {
          if ((lane & 15) == 0 && row < p.m) part[(long)(tile_n * (BN / 64) + (wn * WN) / 64) * p.part_ld + row] = s;
        } else {
          // several waves share a 64-column slot: their partial sums meet in LDS (free after the K loop) and are added in wave order
          if ((lane & 15) == 0) smem[wn * BM + (row - m0)] = s;
        }
      }
    if constexpr (WN < 64) {
      constexpr int WPS = 64 / WN;   // waves per slot
      __syncthreads();
      if (wn % WPS == 0 && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = row_base + i * 16 + 4 * r;
            double s = smem[wn * BM + (row - m0)];
#pragma unroll
            for (int u = 1; u < WPS; ++u) s += smem[(wn + u) * BM + (row - m0)];
            if (row < p.m) part[(long)(tile_n * (BN / 64) + (wn * WN) / 64) * p.part_ld + row] = s;
          }
      }
    }
  }
}


// =====================================================================================================
// One-round-trip 64 x 64 tile for SHORT-K updates that run beside bulk work (round 6, late): the rest-update of a single-leaf
// panel of the SVGP step is K = 128, beta = 1, lower tiles only -- 10 to 400 tiles of ~1 MFLOP.  On gemm_nt_kernel<64, 64, 4, 1>
// every 16-wide slab is a dependent global-load round trip (8 of them, then the read-modify-write of C: 10 in a row), and while
// the extra-row stream's capped GEMM keeps the memory pipes of 224 compute units full a round trip takes several microseconds:
// 36 tiles took 60 us (profiles/r06_step_timeline.txt), longer than the chain's own 41-us period, and every strip waits for the
// previous rest-update.  Here a thread issues ALL its loads -- eight slabs of A and B (32 x 16 bytes) and its 16 values of C --
// before the first barrier; the slabs then go through the same two 18-KB LDS buffers with the same fragment layout, slab order
// and epilogue arithmetic as the generic kernel (bit-identical results).  36 KB of LDS: fits beside any other workgroup.
__global__ __launch_bounds__(256, 2) void gemm_nt_pre64(GemmArgs p, int gx, int gy, int total, int compact) {
  constexpr int BM = 64, BN = 64, MAXS = 8;
  constexpr int BUF = (BM + BN) * LDSS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (p.sig_ptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0)
    __hip_atomic_store(p.sig_ptr, p.sig_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;   // wave w: rows 16 w .. 16 w + 15, all 64 columns
  const int bz = blockIdx.y;
  int tile_m, tile_n;
  tile_order(blockIdx.x, 0, gx, gy, total, compact, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (p.c_lower && n0 > m0 + BM - 1) return;
  if (m0 >= p.m || n0 >= p.n) return;
  const double* __restrict__ A = p.A + (long)bz * p.strideA;
  const double* __restrict__ B = p.B + (long)bz * p.strideB;
  double* __restrict__ C = p.C + (long)bz * p.strideC;
  const int nkt = p.k / BK;   // (the launcher: k a multiple of 16, <= 128)

  // staging slots as in gemm_nt_kernel: chunk c = tid + 256 q -> tile row c >> 3, k offset (c & 7) * 2; rows clamped, then zero-selected
  d2 ra[MAXS][2], rb[MAXS][2];
  const double* pa[2];
  const double* pb[2];
  bool va[2], vb[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q;
    const int rowa = m0 + (c >> 3), rowb = n0 + (c >> 3);
    va[q] = rowa < p.m;
    vb[q] = rowb < p.n;
    pa[q] = A + (long)(va[q] ? rowa : p.m - 1) * p.lda + (c & 7) * 2;
    pb[q] = B + (long)(vb[q] ? rowb : p.n - 1) * p.ldb + (c & 7) * 2;
  }
#pragma unroll
  for (int s = 0; s < MAXS; ++s)
    if (s < nkt) {   // (wave-uniform)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        ra[s][q] = *reinterpret_cast<const d2*>(pa[q] + s * BK);
        rb[s][q] = *reinterpret_cast<const d2*>(pb[q] + s * BK);
      }
    }
  // C of this lane's 16 outputs (D layout: col = lane & 15 (+ 16 j), row = (lane >> 4) + 4 r)
  const int row_base = m0 + wave * 16 + (lane >> 4);
  const int col_base = n0 + (lane & 15);
  const double alpha = p.alpha, beta = p.beta;
  double cpre[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = row_base + 4 * r, col = col_base + j * 16;
      cpre[r][j] = (beta != 0.0 && row < p.m && col < p.n) ? C[(long)row * p.ldc + col] : 0.0;
    }

  const d2 zero2 = {0.0, 0.0};
  auto lstore = [&](int buf, const d2 (&xa)[2], const d2 (&xb)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + 256 * q;
      *reinterpret_cast<d2*>(&smem[buf * BUF + (c >> 3) * LDSS + (c & 7) * 2]) = va[q] ? xa[q] : zero2;
      *reinterpret_cast<d2*>(&smem[buf * BUF + (BM + (c >> 3)) * LDSS + (c & 7) * 2]) = vb[q] ? xb[q] : zero2;
    }
  };
  d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
  if (nkt > 0) {
    lstore(0, ra[0], rb[0]);
    __syncthreads();
  }
  const int frag_r = lane & 15, frag_k = lane >> 4;
#pragma unroll
  for (int kt = 0; kt < MAXS; ++kt)
    if (kt < nkt) {
      const int cur = kt & 1;
      const double* as = smem + cur * BUF + (wave * 16 + frag_r) * LDSS + frag_k;
      const double* bs = smem + cur * BUF + (BM + frag_r) * LDSS + frag_k;
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        const double a = as[kk * 4];
        double b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bs[j * 16 * LDSS + kk * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);
      }
      if (kt + 1 < MAXS && kt + 1 < nkt) lstore(cur ^ 1, ra[kt + 1 < MAXS ? kt + 1 : 0], rb[kt + 1 < MAXS ? kt + 1 : 0]);
      __syncthreads();
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row_base + 4 * r;
    if (row < p.m) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = col_base + j * 16;
        if (col < p.n) {
          double v = alpha * acc[j][r];
          if (beta != 0.0) v += beta * cpre[r][j];
          C[(long)row * p.ldc + col] = v;
        }
      }
    }
  }
}


// =====================================================================================================
// Fast path: 128 x 128 x 16 tiles, every K range a multiple of 16, 16-byte aligned rows.
//
// v_mfma_f64_16x16x4_f64 occupies a SIMD's matrix pipe for 64 cycles (measured: 77.4 TFLOP/s chip-wide
// from ONE wave per SIMD, tools/ubench_f64.hip), so a wave has ~16 issue slots per MFMA for everything
// else and the only way to lose throughput is to let the pipe run dry.  The loop is therefore a
// software pipeline in which no MFMA ever waits for data requested in the same phase:
//   * global -> VGPR loads of slab s+1 are issued at the top of slab s (a full slab = 4096 cycles early),
//   * MFMA fragments are double-buffered in registers: the 8 ds_read_b64 of step kk+1 are issued before
//     the 16 MFMAs of step kk,
//   * the VGPR -> LDS stores of slab s+1 are interleaved one-per-MFMA into step kk=2, the workgroup
//     barrier sits between steps 2 and 3, and step 3 (whose fragments were fetched before the barrier)
//     covers the LDS latency of the first fragments of slab s+1.
// With beta != 0 the accumulators start as (beta/alpha) C, loaded in the prologue next to the first
// slab, so the epilogue is store-only.
// rev != 0: the K slabs are walked from the LAST to the first (same slabs, same per-slab arithmetic; the sum over slabs is
// taken in the opposite order).  Used by the paired triangular-K launches: see gemm_nt_fast.
// SP = 1 (EPI 1; GemmArgs::stat_*): row statistics of A from the staging registers.  Between its global load and its LDS store a
// thread holds A[srow + 32 q, 2 (t & 7) + {0, 1}] of a slab -- the 256 threads hold the slab exactly once -- so sum a^2 and
// sum a V[k, p] cost 16 FMAs and two 8-byte loads of V per thread and slab, no pass over A of their own (row_stats_kernel: 134 MB,
// 28 us in front of the headline projection).  Batch entry p is latent p: it takes column p of V, so the registers do not grow
// with P (all latents in one workgroup: 67 spilled registers, the P = 4 projection 12 % slower).  The accumulation is
// unconditional -- a branch inside the slab would cut the basic block the sched_group_barriers arrange -- and only a workgroup
// whose K range is all of [0, k) (column tile 0) reduces the eight lanes of a row and stores.
template <int EPI, int SP = 0>
__device__ __forceinline__ void fast_tile(const GemmArgs& p, int tile_m, int tile_n, double* smem, int rev = 0, int bz_queue = -1) {
  constexpr int BM = 128, BN = 128;
  constexpr int BUF = (BM + BN) * LDSS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // (K-split of a triangular product: the LAST chunks hold the most non-empty tiles -- they are dispatched first)
  const int bz = bz_queue >= 0 ? bz_queue : (p.k_off_step ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if (p.c_lower && n0 > m0 + BM - 1) return;

  const double* __restrict__ A = p.A + (long)bz * p.strideA;
  const double* __restrict__ B = p.B + (long)bz * p.strideB;
  int kb = 0, ke = p.k;
  const int koff = bz * p.k_off_step;   // (see gemm_nt_kernel)
  if (p.b_tri && (n0 + BN < p.n ? n0 + BN : p.n) <= p.b_tri_rows) {   // (the tile's existing rows; a partial last tile too)
    if (p.b_tri == 1) {
      const int f = n0 + p.b_tri_off - koff;
      kb = (f > 0 ? f : 0) & ~(BK - 1);
    } else {
      const int l = n0 + BN + p.b_tri_off - koff;
      ke = l < p.k ? l : p.k;
    }
  }
  if (p.a_tri == 1) {         // (see gemm_nt_kernel)
    int f = m0 - koff;
    f = (f > 0 ? f : 0) & ~(BK - 1);
    kb = kb > f ? kb : f;
  } else if (p.a_tri == 2) {
    int l = ((m0 + BM + BK - 1) & ~(BK - 1)) - koff;
    l = l < p.k ? l : p.k;
    ke = ke < l ? ke : l;
  }
  const int nk = ke > kb ? (ke - kb) / BK : 0;

  // ---- staging: thread t moves 16 B of row (t>>3) + 32 q, k offset 2 (t&7), for A and for B -----
  // addresses = wave-uniform 64-bit base (advanced per slab) + per-thread 32-bit byte offset
  const int srow = tid >> 3, scol = (tid & 7) * 2;
  const int mrows = p.m - m0, nrows = p.n - n0;  // rows of this tile that exist (clamp the rest)
  const char* abase = reinterpret_cast<const char*>(A + (long)m0 * p.lda + kb);
  const char* bbase = reinterpret_cast<const char*>(B + (long)n0 * p.ldb + kb);
  unsigned oa[4], ob[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int ra = srow + 32 * q, rb = srow + 32 * q;
    ra = ra < mrows ? ra : mrows - 1;  // clamped rows only feed outputs that are never stored
    rb = rb < nrows ? rb : nrows - 1;
    oa[q] = (unsigned)(((long)ra * p.lda + scol) * 8);
    ob[q] = (unsigned)(((long)rb * p.ldb + scol) * 8);
  }
  const int woff = srow * LDSS + scol;
  d2 st[8];
  double ssq[4], smv[4], sv[2];
  const char* vbase = nullptr;   // V[kb + scol, bz]
  if constexpr (SP > 0) {
    vbase = reinterpret_cast<const char*>(p.stat_V + (long)(kb + scol) * p.stat_P + bz);
#pragma unroll
    for (int q = 0; q < 4; ++q) { ssq[q] = 0.0; smv[q] = 0.0; }
  }
  auto gload = [&](int s) {
    const long so = rev ? (long)(nk - 1 - s) : (long)s;
    const char* ab = abase + so * (BK * 8);
    const char* bb = bbase + so * (BK * 8);
#pragma unroll
    for (int q = 0; q < 4; ++q) st[q] = *reinterpret_cast<const d2*>(ab + oa[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) st[4 + q] = *reinterpret_cast<const d2*>(bb + ob[q]);
    if constexpr (SP > 0) {
      const char* vb = vbase + so * (BK * 8) * p.stat_P;
      sv[0] = *reinterpret_cast<const double*>(vb);
      sv[1] = *reinterpret_cast<const double*>(vb + p.stat_P * 8);
    }
  };
  // the A half of the staged slab (st[0..3]) into the row statistics; called where that slab goes to LDS
  auto stat_acc = [&]() {
    if constexpr (SP > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ssq[q] = fma(st[q].x, st[q].x, ssq[q]);
        ssq[q] = fma(st[q].y, st[q].y, ssq[q]);
        smv[q] = fma(st[q].x, sv[0], smv[q]);
        smv[q] = fma(st[q].y, sv[1], smv[q]);
      }
    }
  };
  auto lstore1 = [&](int buf, int q) {
    const int row = (q < 4) ? 32 * q : BM + 32 * (q - 4);
    *reinterpret_cast<d2*>(&smem[buf * BUF + row * LDSS + woff]) = st[q];
  };

  d4 acc[4][4];
  // Accumulator layout.  The MFMA's M index (D row = (lane >> 4) + 4 reg) is fed from the B tile and its N index
  // (D column = lane & 15) from the A tile, and the B-tile row that MFMA row x = g + 4 r reads is permuted to
  // 2 g + (r & 1) + 8 (r >> 1).  A lane (c = lane & 15, g = lane >> 4) then owns, of every 16 x 16 block (i, j), row
  // 16 i + c and the COLUMN PAIRS {2 g, 2 g + 1} (registers 0, 1) and {8 + 2 g, 9 + 2 g} (registers 2, 3): the accumulator
  // preload and the store are 16-byte accesses (32 + 32 per thread and tile, the four g lanes of a row covering 64
  // contiguous bytes per instruction) instead of the 64 + 64 8-byte accesses of the plain D layout, which made the
  // prologue / epilogue of the K = 640 trailing updates store-issue-bound (MI355X_MICROARCH.md: 8-byte accesses reach
  // 0.54 - 0.70 of the 16-byte rate).
  const int lane_c = lane & 15, lane_g = lane >> 4;
  const int row_base = m0 + wm * 64 + lane_c;            // + 16 i
  const int col_base = n0 + wn * 64 + 2 * lane_g;        // + 16 j + 8 h (+ 0 / 1)
  // (EPI = 1 with a C operand: the streamed projection's last group squares C + A B^T without storing it)
  const bool load_c = (p.beta != 0.0) && (EPI == 0 || p.C != nullptr);
  if (nk > 0) gload(0);
  // C is addressed as  wave-uniform base + a 32-bit byte offset per accumulator row block (4) + one per column pair (8),
  // both clamped into the matrix
  const int c_r0 = wm * 64 + lane_c, c_c0 = wn * 64 + 2 * lane_g;
  const int c_rmax = p.m - 1 - m0, c_cmax = p.n - 1 - n0;  // last valid row / column of the matrix, relative to the tile
  // (computed where they are used -- prologue and epilogue -- so that no address register lives across the K loop)
  auto c_roff = [&](int i) -> unsigned {
    const int rr = c_r0 + 16 * i;
    return (unsigned)(((long)(rr < c_rmax ? rr : c_rmax) * p.ldc) * 8);
  };
  auto c_coff = [&](int j, int h) -> unsigned {
    const int c = c_c0 + j * 16 + 8 * h;
    return (unsigned)((c < c_cmax ? c : c_cmax) * 8);
  };
  // 16-byte accesses need whole column pairs inside the matrix and 16-byte aligned rows (block-uniform)
  const bool c_vec = (EPI == 0 || p.C != nullptr) && (n0 + BN <= p.n) && !(p.ldc & 1) && !(p.strideC & 1) &&
                     !(reinterpret_cast<uintptr_t>(p.C) & 15);
  if (load_c) {
    const double* __restrict__ C = p.C + (long)bz * p.strideC;
    const double sc = p.beta / p.alpha;
    const char* cb = reinterpret_cast<const char*>(C + (long)m0 * p.ldc + n0);
    if (c_vec) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* rowp = cb + c_roff(i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const d2 lo = *reinterpret_cast<const d2*>(rowp + c_coff(j, 0));
          const d2 hi = *reinterpret_cast<const d2*>(rowp + c_coff(j, 1));
          acc[i][j] = (d4){sc * lo.x, sc * lo.y, sc * hi.x, sc * hi.y};
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* rowp = cb + c_roff(i);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = c_c0 + j * 16 + 8 * (r >> 1) + (r & 1);
            acc[i][j][r] = sc * *reinterpret_cast<const double*>(rowp + (unsigned)((c < c_cmax ? c : c_cmax) * 8));
          }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  }

  // B-tile row read by MFMA row x = lane & 15 (see "Accumulator layout"): a permutation inside each 16-row block, so the
  // 32-lane ds_read_b64 groups still hit 64 distinct banks
  const int bperm = 2 * (lane_c & 3) + ((lane_c >> 2) & 1) + 8 * (lane_c >> 3);
  const double* as = smem + (wm * 64 + lane_c) * LDSS + lane_g;
  const double* bs = smem + (BM + wn * 64 + bperm) * LDSS + lane_g;
  double fa[2][4], fb[2][4];
  auto fload = [&](int buf, int kk, int f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[f][i] = as[buf * BUF + i * 16 * LDSS + kk * 4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[f][j] = bs[buf * BUF + j * 16 * LDSS + kk * 4];
  };
#define GPK_MFMA_ROW(f, i)                                                                         \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] =                                       \
      __builtin_amdgcn_mfma_f64_16x16x4f64(fb[f][j], fa[f][i], acc[i][j], 0, 0, 0)

  if (nk > 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) lstore1(0, q);
    stat_acc();
    __syncthreads();
    fload(0, 0, 0);
  }
  // one K slab; MORE = another slab follows (its loads / LDS stores / first fragments ride along)
  auto slab = [&](int s, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    const int cur = s & 1;
    // ---- kk = 0 ------------------------------------------------------------------------------
    if constexpr (MORE) gload(s + 1);
    fload(cur, 1, 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) { GPK_MFMA_ROW(0, i); }
    if constexpr (MORE) __builtin_amdgcn_sched_group_barrier(0x020, 8 + 2 * SP, 0);  // 8 global loads (+ the V values of the row statistics)
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);                      // 8 fragment reads
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);                     // 16 MFMA
    __builtin_amdgcn_sched_barrier(0);
    // ---- kk = 1 ------------------------------------------------------------------------------
    fload(cur, 2, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { GPK_MFMA_ROW(1, i); }
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    // ---- kk = 2: also park slab s+1 in the other LDS buffer, one store per MFMA -------------------
    fload(cur, 3, 1);
    if constexpr (MORE) {
#pragma unroll
      for (int q = 0; q < 8; ++q) lstore1(cur ^ 1, q);
      stat_acc();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { GPK_MFMA_ROW(0, i); }
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    if constexpr (MORE) {
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // 1 DS write
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    } else {
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MORE) __syncthreads();
    // ---- kk = 3 (fragments fetched before the barrier) hides the first reads of slab s+1 -------------
    if constexpr (MORE) fload(cur ^ 1, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { GPK_MFMA_ROW(1, i); }
    if constexpr (MORE) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  for (int s = 0; s + 1 < nk; ++s) slab(s, std::true_type{});
  if (nk > 0) slab(nk - 1, std::false_type{});
#undef GPK_MFMA_ROW

  // ---- epilogue ---------------------------------------------------------------------------------
  if constexpr (EPI == 0) {
    double* __restrict__ C = p.C + (long)bz * p.strideC;
    const double alpha = p.alpha;
    char* cb = reinterpret_cast<char*>(C + (long)m0 * p.ldc + n0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (c_r0 + 16 * i <= c_rmax) {
        char* rowp = cb + c_roff(i);
        if (c_vec) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<d2*>(rowp + c_coff(j, 0)) = (d2){alpha * acc[i][j][0], alpha * acc[i][j][1]};
            *reinterpret_cast<d2*>(rowp + c_coff(j, 1)) = (d2){alpha * acc[i][j][2], alpha * acc[i][j][3]};
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = c_c0 + j * 16 + 8 * (r >> 1) + (r & 1);
              if (c <= c_cmax) *reinterpret_cast<double*>(rowp + (unsigned)(c * 8)) = alpha * acc[i][j][r];
            }
        }
      }
    }
  } else {
    double* __restrict__ C2 = p.C2 + (long)bz * p.strideC2;
    double* __restrict__ part = p.part + (long)bz * p.stridePart;
    const double alpha = p.alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row_base + i * 16;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = col_base + j * 16 + 8 * (r >> 1) + (r & 1);
          const double v = alpha * acc[i][j][r];
          if (col < p.sq_cols) {
            s += v * v;
          } else if (row < p.m && col - p.sq_cols < p.c2_cols && col < p.n) {
            C2[(long)row * p.ldc2 + (col - p.sq_cols)] = v;
          }
        }
      // the four g lanes of a row hold its 64 columns of this wave
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (lane_g == 0 && row < p.m) part[(long)(tile_n * 2 + wn) * p.part_ld + row] = s;
    }
    if constexpr (SP > 0) {
      if (tile_n == 0) {   // (kb = 0, ke = k there: gpk_gemm_fuses_row_stats)
        // the eight lanes t & 7 of a row hold its 16 columns of every slab; a row lives in one wave
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int o = 1; o < 8; o <<= 1) {
            ssq[q] += __shfl_xor(ssq[q], o);
            smv[q] += __shfl_xor(smv[q], o);
          }
          const int row = m0 + srow + 32 * q;
          if ((tid & 7) == 0 && row < p.m) {
            if (bz == 0) p.stat_sumsq[row] = ssq[q];
            p.stat_mv[(long)row * p.stat_P + bz] = smv[q];
          }
        }
      }
    }
  }
}


// pair = 0: one tile per workgroup, XCD-contiguous / column-grouped order.
// pair = 1 (triangular-K operand, b_tri = 1): the K range of column tile j shrinks with j, so a workgroup
// takes column tiles j and gx-1-j back to back -- every workgroup then carries the same number of K slabs
// and the launch finishes together instead of waiting for the full-K tiles.
// QUEUE (round 6, late): the queue form is its own instantiation -- with the queue loops and the static walk in ONE kernel it carried
// three inlined copies of the tile, 25 000 instructions and 241 spilled registers.
template <int EPI, bool PAIR, bool QUEUE = false, int SP = 0>
__global__ __launch_bounds__(256, 2) void gemm_nt_fast(GemmArgs p, int gx, int gy, int total, int compact) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (p.sig_ptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0)   // entry signal (GemmArgs::sig_ptr)
    __hip_atomic_store(p.sig_ptr, p.sig_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if constexpr (!PAIR) {
    // De-phasing: the two workgroups that share a CU are dispatched together and, with equal tile times, stay in
    // lock-step -- both in their load/store prologue and epilogue at the same moment, when neither feeds the MFMA
    // pipes.  In big launches the second resident set (workgroups 256..511 of the dispatch order) therefore starts
    // half a tile late, once; the offset then persists for the whole kernel.
    if (p.stagger_ticks > 0 && (int)blockIdx.x >= p.stagger_first && (int)blockIdx.x < 2 * p.stagger_first && blockIdx.y == 0) {
      const long long t0 = wall_clock64();
      while (wall_clock64() - t0 < p.stagger_ticks) __builtin_amdgcn_s_sleep(32);
    }
    // (ONE call site of the tile in ONE kernel -- a single loop that either fetches from the queue or walks statically -- was 84 spilled
    //  registers and 2 % SLOWER on every workload: Cm 1.79 - 1.81 against 1.75 - 1.77 ms, GPR C2 30.9 - 31.0 against 30.3 - 30.6 ms, same
    //  box, profiles/r06_ab_single_call_site.log.)
    if constexpr (QUEUE) {
      // Tile QUEUE (round 6): persistent workgroups take (batch entry, tile) pairs from a device counter, last batch entry first.  For
      // launches whose tiles differ widely in K -- the K chunks of a triangular x triangular product: 480 of 1024 pairs non-empty, 8 to
      // 32 slabs each -- a static assignment leaves the launch as long as its most loaded compute unit.  Every pair is computed by exactly
      // one workgroup and written to its own output tile: results do not depend on who took what.
      // (One queue per XCD -- a contiguous eighth of the tile sequence per L2, workgroups helping the other queues once theirs is empty --
      //  was measured and removed: FETCH_SIZE of the first N = 16384 trailing update is 50 % higher with the single queue, but C2 30.85 /
      //  30.99 against 30.72 / 30.73 ms, profiles/r06_ab_gpr_tile_queue.log.)
      volatile int* s_next = reinterpret_cast<volatile int*>(&smem[BK]);   // (the padding of LDS row 0: no tile access touches it)
      const int nbatch = p.batch > 0 ? p.batch : 1;
      const int all = total * nbatch;
      for (;;) {
        if (threadIdx.x == 0) *s_next = (int)((unsigned)atomicAdd(p.queue, 1) - (unsigned)p.queue_base);
        __syncthreads();
        const int t = *s_next;
        __syncthreads();   // (s_next is rewritten, and both LDS buffers refilled, only after everybody has read / finished)
        if (t >= all || t < 0) break;
        const int zq = t / total, tq = t - zq * total;
        int tile_m, tile_n;
        tile_order(tq, p.b_tri, gx, gy, total, compact, tile_m, tile_n);
        fast_tile<EPI>(p, tile_m, tile_n, smem, 0, nbatch - 1 - zq);
      }
      return;
    }
    // gridDim.x < total: persistent workgroups, each walks the tile list with stride gridDim.x
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
      int tile_m, tile_n;
      if (EPI == 1 && p.tile_snake) {
        // a triangular-K projection whose PAIRS would not fill the chip twice (launch_fast): one tile per workgroup, workgroups x and
        // x + total / 2 -- the same compute unit under round-robin placement -- take column tiles j and gx-1-j of one row tile
        const int q = t / gy, half = gx >> 1;
        tile_m = t - q * gy;
        tile_n = q < half ? q : gx - 1 - (q - half);
      } else if (p.k_off_step) {
        // K-split of a triangular product: the chunks of one output tile must not meet on one compute unit (workgroup x of every
        // batch entry lands on about the same CU, and the tiles near the origin are non-empty in EVERY chunk: the launch would last
        // as long as unsplit) -- each chunk walks the tile list from its own offset
        int tt = t + (int)blockIdx.y * (total / (int)gridDim.y);
        if (tt >= total) tt -= total;
        tile_order(tt, p.b_tri, gx, gy, total, compact, tile_m, tile_n);
      } else {
        tile_order(t, p.b_tri, gx, gy, total, compact, tile_m, tile_n);
      }
      fast_tile<EPI, SP>(p, tile_m, tile_n, smem);
      if (t + (int)gridDim.x < total) __syncthreads();  // both LDS buffers are about to be refilled
    }
  } else {
    // The workgroups of one row tile (block ids tile_m + j gy: the same XCD, all resident together) read the same rows of A.
    // Column tile j only needs K >= 128 j, so started at their own first slab they would sit at eight different K offsets
    // and every one of them would pull its rows of A through an L2 that cannot hold them (8 row tiles x 2 MB per XCD):
    // FETCH_SIZE of the projection was 6.8 x its algorithmic bytes.  Time-aligned instead: the first tile of every pair walks
    // K DOWN from the common end (all eight start at the same slab), the second, short one walks UP to it (all eight
    // finish at the same slab), so a slab of A is fetched once per XCD and hit by the other seven.  (b_tri = 1 only.)
    const int align = (EPI == 1 && p.b_tri == 1) ? p.pair_k_align : 0;
    const int tile_m = blockIdx.x % gy, j = blockIdx.x / gy;
    fast_tile<EPI, SP>(p, tile_m, j, smem, align);
    if (gx - 1 - j != j) {
      __syncthreads();  // both LDS buffers are about to be refilled
      fast_tile<EPI>(p, tile_m, gx - 1 - j, smem, 0);
    }
  }
}

// counters of the tile-queue launches: a ring of device words per device, never reset -- a launch of `fetches` fetches (one per tile
// and one failing fetch per workgroup) on a word leaves it at a value the host knows, which is the base of the next launch on that
// word (two launches would have to be 1024 launches apart AND in flight together to meet on a word).  No memset, no packet.
int queue_slot(unsigned fetches, int** out, unsigned* base) {
  constexpr int kRing = 1024, kMaxDev = 16;
  static std::mutex mu;
  static int* ring[kMaxDev] = {};
  static unsigned* value[kMaxDev] = {};
  static unsigned next[kMaxDev] = {};
  int dev = 0;
  GPK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDev) return GPK_E_UNSUPPORTED;
  std::lock_guard<std::mutex> lock(mu);
  if (!ring[dev]) {
    GPK_HIP(hipMalloc((void**)&ring[dev], sizeof(int) * kRing));
    GPK_HIP(hipMemset(ring[dev], 0, sizeof(int) * kRing));
    value[dev] = (unsigned*)calloc(kRing, sizeof(unsigned));
    if (!value[dev]) return GPK_E_ARG;
  }
  const unsigned slot = next[dev]++ % kRing;
  *out = ring[dev] + slot;
  *base = value[dev][slot];
  value[dev][slot] += fetches;
  return 0;
}


// =====================================================================================================
// Latency path for the short GEMMs on the critical path of the factorisation (panel solve  A21 inv(L11)^T,
// inner updates: K <= 128, a few thousand rows).  There the K loop of the tiled kernels is pure latency
// (every 16-wide slab waits a full global-load round trip), so this kernel stages EVERYTHING at once:
// one workgroup = 16 rows x 128 columns, its A rows and the whole B tile go global -> LDS by LDS-DMA
// (global_load_lds_dwordx4: one 1 KiB row per wave instruction, no VGPR staging, padded row stride),
// one barrier, then each of the 8 waves runs its 16x16 output tile over the full K with two
// independent accumulators.  One column tile covers n <= 128, so the in-place solve (C aliases A)
// only overwrites rows the workgroup alone has read.
constexpr int SM_BM = kGemmSmallBM, SM_BN = kGemmSmallBN, SM_THREADS = kGemmSmallThreads;

__global__ __launch_bounds__(SM_THREADS) void gemm_nt_small(GemmArgs p, int ldk) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bz = blockIdx.z;
  const int n0 = blockIdx.x * SM_BN;
  const double* __restrict__ A = p.A + (long)bz * p.strideA;
  const double* __restrict__ B = p.B + (long)bz * p.strideB;
  int kb = 0, ke = p.k;
  if (p.b_tri && (n0 + SM_BN < p.n ? n0 + SM_BN : p.n) <= p.b_tri_rows) {   // (the tile's existing rows; a partial last tile too)
    if (p.b_tri == 1) {
      const int f = n0 + p.b_tri_off;
      kb = (f > 0 ? f : 0) & ~(BK - 1);
    } else {
      const int l = n0 + SM_BN + p.b_tri_off;
      ke = l < p.k ? l : p.k;
    }
  }
  const int kc = ke > kb ? ke - kb : 0;  // multiple of 16
  double* As = smem;                  // [16][ldk]
  double* Bs = smem + SM_BM * ldk;    // [128][ldk]
  const int r = lane & 15, g = lane >> 4;
  const int col = n0 + wave * 16 + r;
  double* __restrict__ C = p.C + (long)bz * p.strideC;
  // stream hand-offs without queue packets (GemmArgs::sig_ptr / wait_ptr)
  if (p.sig_ptr && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
    __hip_atomic_store(p.sig_ptr, p.sig_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (p.wait_ptr) {
    if (tid == 0) {
      const long long t0 = wall_clock64();   // (100 MHz; bounded: a lost hand-off must never hang the device -- 0.5 s, then on)
      bool timed_out = false;
      while ((int)(__hip_atomic_load(p.wait_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - p.wait_val) < 0) {
        if (wall_clock64() - t0 >= 50000000LL) { timed_out = true; break; }
        __builtin_amdgcn_s_sleep(2);
      }
      // a hand-off that never arrived is an internal error: the factorisation status becomes INT_MAX (gpk.h, "info")
      if (timed_out && p.wait_info) atomicMax(p.wait_info, 0x7fffffff);
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the producer's tiles were released by ITS kernel end; drop stale lines
  }
  // gridDim.y < number of 16-row blocks: the workgroup walks the row blocks with stride gridDim.y and keeps its B tile
  // (used when the chain is confined to the reserved compute units: ONE round of workgroups, B staged once per CU)
  const int nmb = (p.m + SM_BM - 1) / SM_BM;
  bool first = true;
  for (int mb = blockIdx.y; mb < nmb; mb += gridDim.y) {
    const int m0 = mb * SM_BM;
    if (p.c_lower && n0 > m0 + SM_BM - 1) continue;  // (workgroup-uniform)
    // ---- this wave's 16x16 output tile: columns n0 + 16 wave .. ------------------------------------------
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    if (p.beta != 0.0) {
      const double sc = p.beta / p.alpha;
      const int cc = col < p.n ? col : p.n - 1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int row = m0 + g + 4 * e;
        row = row < p.m ? row : p.m - 1;
        acc0[e] = sc * C[(long)row * p.ldc + cc];
      }
    }
    // ---- stage: row q of the 144 (16 A rows; 128 B rows: first pass only), one LDS-DMA instruction each ----------------
    if (2 * lane < kc) {
      for (int q = wave; q < (first ? SM_BM + SM_BN : SM_BM); q += SM_THREADS / 64) {
        const double* src;
        if (q < SM_BM) {
          int rr = m0 + q;
          rr = rr < p.m ? rr : p.m - 1;
          src = A + (long)rr * p.lda + kb;
        } else {
          int rr = n0 + q - SM_BM;
          rr = rr < p.n ? rr : p.n - 1;
          src = B + (long)rr * p.ldb + kb;
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 2 * lane),
                                         (__attribute__((address_space(3))) void*)(smem + q * ldk), 16, 0, 0);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0): the LDS-DMA rows of this wave have landed (and the C preload)
    __syncthreads();
    const double* ap = As + r * ldk + g;
    const double* bp = Bs + (wave * 16 + r) * ldk + g;
    const int nkk = kc >> 2;
#pragma unroll 4
    for (int kk = 0; kk < nkk; kk += 2) {
      const double a0 = ap[kk * 4], b0 = bp[kk * 4];
      const double a1 = ap[kk * 4 + 4], b1 = bp[kk * 4 + 4];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
    first = false;
    if (col < p.n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m0 + g + 4 * e;
        if (row < p.m) C[(long)row * p.ldc + col] = p.alpha * (acc0[e] + acc1[e]);
      }
    }
    if (mb + (int)gridDim.y < nmb) __syncthreads();  // the A rows in LDS are about to be replaced
  }
}

// one launch of a tiled kernel (trailing arguments gx, gy, total, compact); its LDS limit is raised once (function-local static:
// initialised once, thread-safe; MAX_LDS = 0: the default limit does)
template <auto KERNEL, int MAX_LDS>
int launch_tiled(hipStream_t s, dim3 grid, size_t lds_bytes, const GemmArgs& a, const GemmPlan& p, int total) {
  if constexpr (MAX_LDS > 0) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS);
    GPK_HIP(attr);
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds_bytes, s, a, p.gx, p.gy, total, p.compact);
  GPK_LAUNCH_CHECK();
  return 0;
}
template <int BM, int BN, int WGM, int WGN>
int launch_generic(hipStream_t s, dim3 grid, const GemmArgs& a, const GemmPlan& p, int total) {
  constexpr size_t LDS = TileCfg<BM, BN, WGM, WGN>::LDS_BYTES;
  static_assert(LDS == gemm_tile_lds(BM, BN), "the plan's LDS bytes are the kernel's");
  return launch_tiled<gemm_nt_kernel<BM, BN, WGM, WGN>, (int)LDS>(s, grid, LDS, a, p, total);
}

// Carries out what make_gemm_plan decided (gemm_plan.h): no decision is taken here.
int launch_plan(hipStream_t s, const GemmArgs& a, const GemmPlan& p) {
  if (p.kernel == GemmKernel::none) return 0;
  if (p.kernel == GemmKernel::unsupported) return GPK_E_UNSUPPORTED;
  GemmArgs b = a;
  b.tile_snake = p.tile_snake; b.stagger_first = p.stagger_first; b.stagger_ticks = p.stagger_ticks; b.pair_k_align = p.pair_k_align;
  const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
  switch (p.kernel) {
    case GemmKernel::small: {
      static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_small),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         (int)((SM_BM + SM_BN) * 130 * sizeof(double)));
      GPK_HIP(attr);
      hipLaunchKernelGGL(gemm_nt_small, grid, dim3(p.threads), p.lds_bytes, s, b, p.ldk);
      GPK_LAUNCH_CHECK();
      return 0;
    }
    case GemmKernel::pre64: return launch_tiled<gemm_nt_pre64, 0>(s, grid, p.lds_bytes, b, p, p.total);
    case GemmKernel::generic:
      switch (p.tile) {
        case GemmTile::t128x128: return launch_generic<128, 128, 2, 2>(s, grid, b, p, p.total);
        case GemmTile::t128x64: return launch_generic<128, 64, 2, 2>(s, grid, b, p, p.total);
        case GemmTile::t64x128_1x4: return launch_generic<64, 128, 1, 4>(s, grid, b, p, p.total);
        case GemmTile::t64x128_2x2: return launch_generic<64, 128, 2, 2>(s, grid, b, p, p.total);
        case GemmTile::t64x64: return launch_generic<64, 64, 4, 1>(s, grid, b, p, p.total);
        case GemmTile::t32x64: return launch_generic<32, 64, 2, 2>(s, grid, b, p, p.total);
      }
      return GPK_E_UNSUPPORTED;
    default: break;   // fast
  }
  // (unpaired capped launches ask for more LDS than the tile needs: the limit of the unpaired walk is the whole 160 KB)
  constexpr int FAST = (int)kGemmFastLds, WHOLE = 160 * 1024;
  if (p.queue) {
    unsigned qbase = 0;
    GPK_TRY(queue_slot(p.queue_fetches, &b.queue, &qbase));
    b.queue_base = (int)qbase;
    return launch_tiled<gemm_nt_fast<0, false, true>, FAST>(s, grid, p.lds_bytes, b, p, p.total);
  }
  int rc = GPK_E_UNSUPPORTED;
  switch (4 * p.epi + 2 * p.pair + p.sp) {
    case 0: rc = launch_tiled<gemm_nt_fast<0, false, false, 0>, WHOLE>(s, grid, p.lds_bytes, b, p, p.total); break;
    case 2: rc = launch_tiled<gemm_nt_fast<0, true, false, 0>, FAST>(s, grid, p.lds_bytes, b, p, p.total); break;
    case 4: rc = launch_tiled<gemm_nt_fast<1, false, false, 0>, WHOLE>(s, grid, p.lds_bytes, b, p, p.total); break;
    case 5: rc = launch_tiled<gemm_nt_fast<1, false, false, 1>, WHOLE>(s, grid, p.lds_bytes, b, p, p.total); break;
    case 6: rc = launch_tiled<gemm_nt_fast<1, true, false, 0>, FAST>(s, grid, p.lds_bytes, b, p, p.total); break;
    case 7: rc = launch_tiled<gemm_nt_fast<1, true, false, 1>, FAST>(s, grid, p.lds_bytes, b, p, p.total); break;
  }
  if (rc || p.tail_tiles == 0) return rc;
  GemmArgs t = a;   // (the caller's args: the quarters of the last, partial round)
  t.tail_first1 = p.tail_first1;
  return launch_generic<64, 64, 4, 1>(s, dim3(p.tail_grid_x, 1, 1), t, p, (int)p.tail_grid_x);
}

}  // namespace

int gpk_gemm_tiles_n(int n) { return gpk_cdiv(n, 128); }
bool gpk_gemm_takes_latency_kernel(const GemmArgs& a) { return make_gemm_plan(a).kernel == GemmKernel::small; }
bool gpk_gemm_fuses_row_stats(const GemmArgs& a) {
  const GemmPlan p = make_gemm_plan(a);
  return p.kernel == GemmKernel::fast && p.sp;
}

// ---- optional per-launch timing (bench.py roofline leg): HIP events around every GEMM launch, on the
// stream the kernel is launched on.  Off by default; adds two event records per launch when on. -------
namespace {
struct ProfRec { hipEvent_t e0, e1; double flops; int kind; };
bool g_prof_on = false;
ProfRec* g_prof = nullptr;
int g_prof_n = 0, g_prof_cap = 0;

double algorithmic_flops(const GemmArgs& a) {
  // useful multiply-adds only: lower-trapezoid outputs for c_lower, the non-zero K range for b_tri
  const double m = a.m, n = a.n, k = a.k;
  double outs = m * n;
  if (a.c_lower) outs = (m >= n) ? n * (n + 1) / 2 + (m - n) * n : m * (m + 1) / 2;
  double kk = k;
  if (a.b_tri) {
    const double nn = (a.b_tri_rows < a.n ? a.b_tri_rows : a.n);
    const double tri = (nn <= k) ? nn * (nn + 1) / 2 + nn * (k - nn) : k * (k + 1) / 2;
    return 2.0 * m * (tri + (n - nn) * k) * (a.batch > 0 ? a.batch : 1);
  }
  return 2.0 * outs * kk * (a.batch > 0 ? a.batch : 1);
}

// total_ms / launches / flops of the recorded launches with at least min_flops (any_kind, or those of kernel `kind`); synchronises the device
int prof_collect(bool any_kind, int kind, double min_flops, double* total_ms, long* launches, double* flops) {
  GPK_HIP(hipDeviceSynchronize());
  double ms = 0.0, fl = 0.0;
  long cnt = 0;
  for (int i = 0; i < g_prof_n; ++i) {
    if ((!any_kind && g_prof[i].kind != kind) || g_prof[i].flops < min_flops) continue;
    float t = 0.f;
    GPK_HIP(hipEventElapsedTime(&t, g_prof[i].e0, g_prof[i].e1));
    ms += t;
    fl += g_prof[i].flops;
    ++cnt;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = cnt;
  if (flops) *flops = fl;
  return 0;
}
}  // namespace

int gpk_profile_gemm_is_on() { return g_prof_on ? 1 : 0; }

extern "C" void gpk_profile_gemm_enable(int on) {
  g_prof_on = on != 0;
  g_prof_n = 0;
}

// total_ms / launches / flops of the GEMM launches recorded since enable(1) whose ALGORITHMIC flop count is at
// least min_flops (0 = all); synchronises the device.  keep != 0 leaves the records in place for another query.
extern "C" int gpk_profile_gemm_collect_min(double min_flops, int keep, double* total_ms, long* launches,
                                            double* flops) {
  GPK_TRY(prof_collect(true, 0, min_flops, total_ms, launches, flops));
  if (!keep) g_prof_n = 0;
  return 0;
}
// The phase spanned by the launches with >= min_flops (first such launch's start .. last such launch's end, by HIP
// events) and the algorithmic flops of EVERY recorded launch issued in between, whatever its stream: the chip-wide
// rate of e.g. the trailing-update phase of a factorisation, where the bulk stream's big GEMMs and the look-ahead
// panel's smaller ones share the machine.  Records are kept.
extern "C" int gpk_profile_gemm_window(double min_flops, double* window_ms, double* flops_all, double* flops_matching,
                                       long* launches_all) {
  GPK_HIP(hipDeviceSynchronize());
  int first = -1, last = -1;
  for (int i = 0; i < g_prof_n; ++i)
    if (g_prof[i].flops >= min_flops) { if (first < 0) first = i; last = i; }
  double fa = 0.0, fm = 0.0;
  float t = 0.f;
  long cnt = 0;
  if (first >= 0) {
    GPK_HIP(hipEventElapsedTime(&t, g_prof[first].e0, g_prof[last].e1));
    for (int i = first; i <= last; ++i) {
      fa += g_prof[i].flops;
      if (g_prof[i].flops >= min_flops) fm += g_prof[i].flops;
      ++cnt;
    }
  }
  if (window_ms) *window_ms = t;
  if (flops_all) *flops_all = fa;
  if (flops_matching) *flops_matching = fm;
  if (launches_all) *launches_all = cnt;
  return 0;
}
// the same, restricted to launches of ONE kernel (kind: 1 gemm_nt_small, 2 gemm_nt_fast<0,false>, 3 <0,true>, 4 <1,false>,
// 5 <1,true>, 6 gemm_nt_kernel) -- directly comparable with rocprofv3's per-kernel average.  Records are kept.
extern "C" int gpk_profile_gemm_collect_kind(int kind, double min_flops, double* total_ms, long* launches, double* flops) {
  return prof_collect(false, kind, min_flops, total_ms, launches, flops);
}
extern "C" int gpk_profile_gemm_collect(double* total_ms, long* launches, double* flops) {
  return gpk_profile_gemm_collect_min(0.0, 0, total_ms, launches, flops);
}

// grow the record table of the profiling facility.  The table pointer is published right after realloc (the old block may
// have moved) and the capacity only ever covers records whose two events exist: a failed hipEventCreate leaves a shorter,
// consistent table instead of a dangling pointer (advisor, round 4).
static int prof_grow() {
  const int cap = g_prof_cap ? 2 * g_prof_cap : 1024;
  ProfRec* p = (ProfRec*)realloc(g_prof, sizeof(ProfRec) * cap);
  if (!p) return GPK_E_ARG;
  g_prof = p;
  for (int i = g_prof_cap; i < cap; ++i) {
    if (hipEventCreate(&p[i].e0) != hipSuccess) return i > g_prof_n ? 0 : GPK_E_ARG;
    if (hipEventCreate(&p[i].e1) != hipSuccess) {
      (void)hipEventDestroy(p[i].e0);
      return i > g_prof_n ? 0 : GPK_E_ARG;
    }
    g_prof_cap = i + 1;
  }
  return 0;
}

int gpk_launch_gemm(hipStream_t s, const GemmArgs& a) {
  const GemmPlan plan = make_gemm_plan(a);
  if (!g_prof_on || plan.kernel == GemmKernel::none) return launch_plan(s, a, plan);
  if (g_prof_n == g_prof_cap) {
    const int rcg = prof_grow();
    if (rcg) return rcg;
    if (g_prof_n == g_prof_cap) return GPK_E_ARG;
  }
  ProfRec& r = g_prof[g_prof_n++];
  r.flops = algorithmic_flops(a);
  r.kind = plan.kind;
  GPK_HIP(hipEventRecord(r.e0, s));
  const int rc = launch_plan(s, a, plan);
  GPK_HIP(hipEventRecord(r.e1, s));
  return rc;
}



namespace {
// K = 0: C = beta C (exact zeros for beta = 0, C not read), on the tiles a 128 x 128 launch would write
__global__ __launch_bounds__(256) void gemm_nt_empty_k_kernel(double* __restrict__ C, int row0, int n, long ldc, long strideC,
                                                              double beta, int c_lower) {
  double* Cz = C + (long)blockIdx.z * strideC;
  const int i = row0 + (int)blockIdx.y;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    if (c_lower && (j & ~127) > (i & ~127)) continue;
    double* c = Cz + (long)i * ldc + j;
    *c = beta != 0.0 ? beta * *c : 0.0;
  }
}
}  // namespace

extern "C" int gpk_gemm_nt(void* stream, int m, int n, int k, double alpha, const double* A,
                           long lda, const double* B, long ldb, double beta, double* C, long ldc,
                           int b_tri, int c_lower, int batch, long strideA, long strideB,
                           long strideC) {
  // (gpk.h: an operand without elements may be NULL -- A / B when m, n or k is 0, C when m or n is 0)
  if (m < 0 || n < 0 || k < 0 || batch < 0) return GPK_E_ARG;
  if ((b_tri & ~0x133) || (b_tri & 3) == 3 || ((b_tri >> 4) & 3) == 3 || ((b_tri & 0x100) && (k & 15))) return GPK_E_ARG;
  if (m == 0 || n == 0) return 0;
  if (!C) return GPK_E_ARG;
  if (k == 0) {
    // no product: C = beta C (BLAS), on the tiles the K > 0 launches write (c_lower: 128-wide tiles on or below the diagonal)
    const int nbatch = batch > 0 ? batch : 1;
    if (nbatch > 65535) return GPK_E_ARG;
    for (int i0 = 0; i0 < m; i0 += 65535) {
      dim3 grid((unsigned)std::min(gpk_cdiv(n, 256), 64), (unsigned)std::min(m - i0, 65535), (unsigned)nbatch);
      hipLaunchKernelGGL(gemm_nt_empty_k_kernel, grid, dim3(256), 0, (hipStream_t)stream, C, i0, n, ldc,
                         nbatch > 1 ? strideC : 0L, beta, c_lower);
      GPK_LAUNCH_CHECK();
    }
    return 0;
  }
  if (!A || !B) return GPK_E_ARG;
  GemmArgs g{};
  g.A = A; g.lda = lda; g.strideA = strideA;
  g.B = B; g.ldb = ldb; g.strideB = strideB;
  g.C = C; g.ldc = ldc; g.strideC = strideC;
  g.m = m; g.n = n; g.k = k; g.alpha = alpha; g.beta = beta;
  g.c_lower = c_lower; g.b_tri = b_tri & 3; g.b_tri_off = 0; g.b_tri_rows = n;
  // bit 8: the batch is a K-SPLIT of one triangular product -- entry z holds columns z k .. (z + 1) k of both operands (strided views),
  // and the triangular statements are about the UNSPLIT column index.  The caller sums the `batch` partial products.
  const int ksplit = (b_tri >> 8) & 1;
  g.a_tri = (m <= k * (ksplit ? (batch > 0 ? batch : 1) : 1)) ? ((b_tri >> 4) & 3) : 0;  // (a hint: ignoring it is always correct)
  g.k_off_step = ksplit ? k : 0;
  g.epi = 0; g.batch = batch > 0 ? batch : 1;
  if (kGpkExp) g.max_wgs = GPK_TUNE(GEMM_NT_MAX_WGS, 0);   // (A/B build only: tools/capped_gemm_probe.py)
  return gpk_launch_gemm((hipStream_t)stream, g);
}
