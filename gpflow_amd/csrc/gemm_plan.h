// Which kernel a GEMM call gets and how it is launched (gemm.hip, gpk_launch_gemm) as DATA: everything the launcher decides from one
// GemmArgs before a single HIP call is made.  Plain C++17 and no HIP header, so the plan can be printed and tested on a machine
// without a GPU (tests/test_gemm_plan.py, tests/gemm_plan_dump.cpp).  gemm.hip's launch_plan carries out what the plan says; a change
// of the SELECTION -- kernel, tile shape, pairing, caps, tail split, LDS request, stagger, tile queue -- is a change to this file,
// with its A/B record next to the threshold and a pin in the test.
//
// The operand-dependent facts (16-byte alignment of A / B, parity of lda / ldb / stride*, lda <= 2^21) are read from the GemmArgs.
// What is NOT here: the tile queue's counter (queue_slot, taken at launch time) and the device code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gpk_tune.h"

// ---- GEMM (gemm.hip):  C = alpha * A * B^T + beta * C ----------------------------------------
struct GemmArgs {
  const double* A; long lda; long strideA;   // [m,k]
  const double* B; long ldb; long strideB;   // [n,k]
  double* C; long ldc; long strideC;         // [m,n]
  int m, n, k;
  double alpha, beta;
  int c_lower;      // skip tiles strictly above the diagonal (row r / col c of C: skip if c0 > r_last)
  int b_tri;        // 0 dense, 1 B[j,kk]==0 for kk<j, 2 B[j,kk]==0 for kk>j (+ b_tri_off on kk)
  int a_tri;        // structure of A, a hint that only shortens the K range of a tile: 1 A[i,kk]==0 for kk<i (upper), 2 for kk>i (lower)
  int b_tri_off;    // the triangular structure is B[j,kk] vs kk - b_tri_off
  int b_tri_rows;   // structure applies to rows j < b_tri_rows of B only (rows beyond are dense)
  int k_off_step;   // batch entry z is the K chunk [z k_off_step, z k_off_step + k) of ONE product: a_tri / b_tri refer to the unsplit column index
  // epilogue 1 ("project"): columns < sq_cols are squared and row-summed into part[(tile_n*2+wn), row];
  // columns >= sq_cols (the q_mu rows of the operand) are stored to C2[row, col - sq_cols]; C unused.
  int epi;
  int sq_cols;
  double* part; long part_ld; long stridePart;   // [2*tiles_n, m]
  double* C2; long ldc2; long strideC2; int c2_cols;
  // epilogue 1 on gemm_nt_fast only (ask gpk_gemm_fuses_row_stats): the row statistics of A ride along.  The workgroup of column
  // tile 0 walks all of [0, k) with its A slabs staged in registers; it also forms  stat_sumsq[r] = sum_k A[r,k]^2  and
  // stat_mv[r, p] = sum_k A[r,k] stat_V[k, p]  (stat_V [k, stat_P] row-major, stat_P = batch <= 4) and writes them itself: one wave per
  // row, fixed order, no atomics.  The batch shares A (strideA = 0): entry p forms column p of stat_mv, entry 0 stat_sumsq as well.
  double* stat_sumsq; double* stat_mv; const double* stat_V; int stat_P;
  int batch;
  int stagger_first;  // fast path only: number of CUs the launch stream may use (first workgroup of the 2nd resident set), 0 = 256
  int stagger_ticks;  // fast path only: start delay (100 MHz ticks) of the second resident workgroup set, 0 = none
  int no_small;     // never take the one-shot LDS-DMA latency kernel (150 KB of LDS per workgroup: needs a CU free of GEMM workgroups)
  int small_loop;   // K <= 128 launches with MORE than 512 row slivers may still take the one-shot latency kernel: its workgroups
                    // then walk the row blocks with their B tile staged once (the in-group updates of the extra rows)
  int max_wgs;      // fast path only: cap on the number of (persistent) workgroups per batch entry, 0 = one per tile
  int pair_k_align; // set by the launcher for paired triangular-K launches: time-aligned K traversal (gemm_nt_fast)
  // In-kernel stream hand-offs of the factorisation's latency chain (one-shot latency kernel only; potrf.hip, round 5).  An
  // event record / wait between two kernels of one stream costs 4.6 / 6.3 us on MI355X, back-to-back kernels 0.3 us:
  //   sig_ptr:  workgroup (0,0,0) stores sig_val there on entry -- "everything queued before this kernel on its stream has
  //             completed" (in-order queue: the previous kernel's end-of-kernel release is done), read by
  //             hipStreamWaitValue32 on other streams or by another kernel's wait_ptr (every GEMM kernel honours sig_ptr);
  //   wait_ptr: every workgroup spins (bounded) until (int)(*wait_ptr - wait_val) >= 0, then acquires at agent scope: the
  //             word is written by hipStreamWriteValue32 behind the producing kernel on ITS stream.
  int* sig_ptr; int sig_val;
  const int* wait_ptr; int wait_val;
  int* wait_info;   // device int that receives INT_MAX if the bounded wait expires (the factorisation's status word)
  int tile_queue;   // fast path, epi 0: persistent workgroups that take their tiles from a device counter (launches with more than 512 tiles)
  int* queue; int queue_base;   // set by the launcher only: that counter and its value before this launch
  int tile64;       // epi 0 only (flag): take the generic kernel's 64 x 64 tiles (36 KB of LDS per workgroup: fits beside any other workgroup on a CU)
  int tile_snake;   // set by the launcher only (generic kernel, under-filled triangular-K projections): heavy / light tiles alternate per CU
  int tail_first1;  // set by the launcher only (generic 64 x 64 kernel; the fast path's "tail split"): 1 + first position, 0 = off
};
static inline GemmArgs gemm_base(int m, int n, int k, double alpha, const double* A, long lda,
                                 const double* B, long ldb, double beta, double* C, long ldc, int batch,
                                 long sA, long sB, long sC) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.strideA = sA;
  g.B = B; g.ldb = ldb; g.strideB = sB;
  g.C = C; g.ldc = ldc; g.strideC = sC;
  g.m = m; g.n = n; g.k = k; g.alpha = alpha; g.beta = beta;
  g.b_tri_rows = n; g.batch = batch > 0 ? batch : 1;
  return g;
}

// ---- the plan ------------------------------------------------------------------------------------
constexpr int kGemmBK = 16;              // K slab of the tiled kernels
constexpr int kGemmLDSS = kGemmBK + 2;   // their padded LDS row, in doubles
constexpr int kGemmGroupN = 8;           // column tiles per group of the tile order (gemm.hip, tile_decode)
constexpr int kGemmSmallBM = 16, kGemmSmallBN = 128, kGemmSmallThreads = 512;   // the one-shot latency kernel's tile
constexpr size_t kGemmFastLds = 2 * (size_t)256 * kGemmLDSS * sizeof(double);   // two buffers of a 128 + 128 row slab

enum class GemmKernel : unsigned char {
  none,         // m or n is 0: nothing to launch
  small,        // gemm_nt_small, the one-shot latency kernel
  pre64,        // gemm_nt_pre64
  generic,      // gemm_nt_kernel<tile>
  fast,         // gemm_nt_fast<epi, pair, queue, sp>
  unsupported   // the call is refused with GPK_E_UNSUPPORTED
};
// the <BM, BN, WGM, WGN> instantiations of gemm_nt_kernel in use
enum class GemmTile : unsigned char { t128x128, t128x64, t64x128_1x4, t64x128_2x2, t64x64, t32x64 };
struct GemmTileShape { int bm, bn, wgm, wgn; };
constexpr GemmTileShape gemm_tile_shape(GemmTile t) {
  switch (t) {
    case GemmTile::t128x128: return {128, 128, 2, 2};
    case GemmTile::t128x64: return {128, 64, 2, 2};
    case GemmTile::t64x128_1x4: return {64, 128, 1, 4};
    case GemmTile::t64x128_2x2: return {64, 128, 2, 2};
    case GemmTile::t64x64: return {64, 64, 4, 1};
    default: return {32, 64, 2, 2};
  }
}
constexpr size_t gemm_tile_lds(int bm, int bn) { return 2 * (size_t)(bm + bn) * kGemmLDSS * sizeof(double); }

struct GemmPlan {
  GemmKernel kernel = GemmKernel::none;
  GemmTile tile = GemmTile::t128x128;        // generic only
  int epi = 0, pair = 0, queue = 0, sp = 0;  // fast only: the template arguments (sp: the row statistics ride along)
  int kind = 0;   // the bench's profiling facility (gpk_profile_gemm_collect_kind): 1 gemm_nt_small, 2 + 2 EPI + PAIR gemm_nt_fast<EPI, PAIR>,
                  // 6 gemm_nt_kernel and gemm_nt_pre64
  // geometry: the kernel's trailing arguments and its launch
  int gx = 0, gy = 0, total = 0, compact = 0;
  int ldk = 0;    // small only: its one trailing argument, the LDS row stride
  unsigned grid_x = 0, grid_y = 0, grid_z = 0;
  unsigned threads = 0;
  size_t lds_bytes = 0;
  // the GemmArgs fields "set by the launcher only", as the kernel's copy of the args gets them (tail_first1: the TAIL launch's copy)
  int tile_snake = 0, stagger_first = 0, stagger_ticks = 0, pair_k_align = 0, tail_first1 = 0;
  // tail split: the last tail_tiles positions of the 128 x 128 tile sequence run as gemm_nt_kernel<64, 64, 4, 1> quarters in a second
  // launch of grid (tail_grid_x, 1, 1) on the caller's args; 0 = none
  int tail_tiles = 0;
  unsigned tail_grid_x = 0;
  // tile queue (fast, queue = 1): persistent workgroups and the fetches they make (one per tile and one failing fetch each)
  unsigned queue_wgs = 0, queue_fetches = 0;
};

static inline int gemm_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int gemm_nbatch(const GemmArgs& a) { return a.batch > 0 ? a.batch : 1; }

// Tiles on or below the diagonal of a gy x gx tile grid, counted as the device numbers them (gemm.hip, tile_decode): column groups
// of kGemmGroupN, inside a group the triangle on the diagonal, then the full rows below it.
static inline int gemm_lower_tiles(int gx, int gy) {
  int total = 0;
  for (int first = 0; first < gx; first += kGemmGroupN) {
    const int gsz = (gx - first) < kGemmGroupN ? (gx - first) : kGemmGroupN;
    const int avail = gy - first;
    if (avail <= 0) break;
    const int tr = avail < gsz ? avail : gsz;
    total += tr * (tr + 1) / 2 + (avail > gsz ? (avail - gsz) * gsz : 0);
  }
  return total;
}

static inline bool gemm_rows_16b(const GemmArgs& a) {   // 16-byte aligned rows of both operands, every batch entry
  if ((a.lda & 1) || (a.ldb & 1) || (a.strideA & 1) || (a.strideB & 1)) return false;
  return !((reinterpret_cast<uintptr_t>(a.A) & 15) || (reinterpret_cast<uintptr_t>(a.B) & 15));
}

static inline bool gemm_pre64_ok(const GemmArgs& a) {
  if (a.epi != 0 || a.k <= 0 || a.k > 128 || (a.k & 15) || a.b_tri || a.a_tri || a.k_off_step || a.tile_snake || a.tail_first1) return false;
  return gemm_rows_16b(a);
}

// 16-byte aligned rows and K ranges that are multiples of 16 everywhere (per-tile b_tri ranges too)
static inline bool gemm_fast_ok(const GemmArgs& a) {
  if (GPK_TUNE(GEMM_NO_FAST, 0)) return false;
  if (a.k <= 0 || (a.k & 15) || (a.b_tri && (a.b_tri_off & 15))) return false;
  if (!gemm_rows_16b(a)) return false;
  if (a.epi == 0 && a.beta != 0.0 && a.alpha == 0.0) return false;
  if (a.lda > (1L << 21) || a.ldb > (1L << 21)) return false;  // 32-bit byte offsets inside a tile
  return true;
}

// small-K latency path: K <= 128 in whole 16-slabs, 16-byte aligned rows, modest row count
static inline bool gemm_small_ok(const GemmArgs& a) {
  if (GPK_TUNE(GEMM_NO_SMALL, 0) || a.epi != 0) return false;
  if (a.k <= 0 || a.k > 128 || (a.k & 15) || (a.b_tri && (a.b_tri_off & 15)) || a.k_off_step) return false;
  if (!gemm_rows_16b(a)) return false;
  if (a.beta != 0.0 && a.alpha == 0.0) return false;
  const long max_wgs = GPK_TUNE(SMALL_MAX_WGS, 512);
  if (a.small_loop && a.batch <= 1) return true;
  return (long)gemm_cdiv(a.m, kGemmSmallBM) * gemm_cdiv(a.n, kGemmSmallBN) * gemm_nbatch(a) <= max_wgs && a.batch < 65536;
}

// column-tile PAIRS of a triangular-K projection on the 128 x 128 tile, all batch entries
static inline long gemm_proj_pairs(const GemmArgs& a) {
  return (long)((gemm_cdiv(a.n, 128) + 1) / 2) * gemm_cdiv(a.m, 128) * gemm_nbatch(a);
}
// under-filled projections leave gemm_nt_fast for the generic kernel's small tiles
static inline bool gemm_proj_small_tiles(const GemmArgs& a) {
  if (!(a.epi == 1 && a.b_tri == 1 && !(a.beta != 0.0 && a.C) && a.m > 64)) return false;
  return gemm_proj_pairs(a) < GPK_TUNE(PROJ_SMALL_TILE_BELOW, 200);
}

// Row statistics ride along (GemmArgs::stat_*) where the selection ends in gemm_nt_fast<1> AND the workgroup of column tile 0 walks
// the whole K range: no K split, no structure in A, B dense or upper-triangular from column 0.
static inline bool gemm_row_stats_fusable(const GemmArgs& a) {
  if (a.epi != 1 || !a.stat_sumsq || !a.stat_mv || !a.stat_V || a.stat_P < 1 || a.stat_P > 4) return false;
  if (a.m <= 0 || a.n <= 0 || a.k_off_step || a.a_tri || a.b_tri == 2 || (a.b_tri == 1 && a.b_tri_off != 0)) return false;
  if ((a.beta != 0.0 && a.C) || a.batch != a.stat_P || (a.batch > 1 && a.strideA != 0)) return false;   // (batch entry p = latent p of one shared A)
  return !gemm_proj_small_tiles(a) && gemm_fast_ok(a);
}

static inline void gemm_plan_small(const GemmArgs& a, GemmPlan& p) {
  p.kernel = GemmKernel::small;
  p.kind = 1;
  p.ldk = a.k + 2;
  p.lds_bytes = (size_t)(kGemmSmallBM + kGemmSmallBN) * p.ldk * sizeof(double);
  unsigned gy = (unsigned)gemm_cdiv(a.m, kGemmSmallBM);
  const unsigned gxs = (unsigned)gemm_cdiv(a.n, kGemmSmallBN);
  if (a.max_wgs > 0 && gy * gxs > (unsigned)a.max_wgs) gy = ((unsigned)a.max_wgs + gxs - 1) / gxs;  // row blocks walked in-kernel
  else if (a.small_loop && a.max_wgs <= 0 && gy * gxs > 512u) gy = (512u + gxs - 1) / gxs;
  p.grid_x = gxs; p.grid_y = gy; p.grid_z = (unsigned)gemm_nbatch(a);
  p.threads = kGemmSmallThreads;
}

static inline void gemm_plan_pre64(const GemmArgs& a, GemmPlan& p) {
  p.kernel = GemmKernel::pre64;
  p.kind = 6;
  p.gx = gemm_cdiv(a.n, 64); p.gy = gemm_cdiv(a.m, 64);
  p.total = p.gx * p.gy;
  if (a.c_lower) {
    p.compact = 1;
    p.total = gemm_lower_tiles(p.gx, p.gy);
  }
  // (A/B, level: few tiles asking for 80 KB of LDS so that they cannot share a compute unit with a capped bulk workgroup and run on the CUs
  //  the cap leaves free -- Cm 1.734 - 1.745 against 1.741 - 1.758 ms, profiles/r06_ab_rest_pre64.log; s_setprio 1 / 3 likewise)
  p.lds_bytes = gemm_tile_lds(64, 64);
  p.grid_x = (unsigned)p.total; p.grid_y = (unsigned)gemm_nbatch(a); p.grid_z = 1;
  p.threads = 256;
}

static inline void gemm_plan_generic(const GemmArgs& a, GemmPlan& p, GemmTile tile) {
  const GemmTileShape t = gemm_tile_shape(tile);
  p.kernel = GemmKernel::generic;
  p.tile = tile;
  p.kind = 6;
  p.gx = gemm_cdiv(a.n, t.bn); p.gy = gemm_cdiv(a.m, t.bm);
  p.total = p.gx * p.gy;
  if (a.c_lower && t.bm == t.bn && a.epi == 0) {
    p.compact = 1;
    p.total = gemm_lower_tiles(p.gx, p.gy);
  }
  p.grid_x = (unsigned)p.total;
  if (p.tile_snake) {   // (see the kernel: needs whole rounds of 256 workgroups per batch entry, or a single problem)
    const int nbatch = gemm_nbatch(a);
    if (a.b_tri != 1 || p.compact || p.total < 256 || (p.total == 256 && nbatch < 2)) p.tile_snake = 0;
    else if ((p.gy & 7) == 0 && (p.total & 255) == 0) p.tile_snake = 2;
    else if (nbatch == 1) { p.tile_snake = 1; p.grid_x = (unsigned)((p.total + 255) & ~255); }
    else p.tile_snake = 0;
  }
  p.grid_y = (unsigned)gemm_nbatch(a); p.grid_z = 1;
  p.threads = 256;
  p.lds_bytes = gemm_tile_lds(t.bm, t.bn);
}

// the fast path: 128 x 128 x 16 tiles (gemm_fast_ok holds)
static inline void gemm_plan_fast(const GemmArgs& a, GemmPlan& p) {
  const int EPI = a.epi == 1 ? 1 : 0;
  p.kernel = GemmKernel::fast;
  p.epi = EPI;
  p.sp = (EPI == 1 && a.stat_sumsq) ? 1 : 0;
  p.threads = 256;
  p.lds_bytes = kGemmFastLds;
  p.gx = gemm_cdiv(a.n, 128); p.gy = gemm_cdiv(a.m, 128);
  p.total = p.gx * p.gy;
  if (a.c_lower && EPI == 0) {
    p.compact = 1;
    p.total = gemm_lower_tiles(p.gx, p.gy);
  }
  const unsigned nb = (unsigned)gemm_nbatch(a);
  p.grid_y = nb; p.grid_z = 1;
  // triangular-K operands (K range shrinking with the column tile for b_tri 1, growing for b_tri 2): paired column
  // tiles.  EPI 0 too (the tri-K GEMMs of the reverse pass, gradients.py: 45 -> 60 TFLOP/s class) unless the launch
  // is lower-only or capped.
  {
    const int gx = p.gx, gy = p.gy;
    const bool pair_ok = (EPI == 1) ? (a.b_tri == 1)
                                    : ((a.b_tri == 1 || a.b_tri == 2) && !a.c_lower && a.max_wgs == 0 && a.b_tri_off == 0 && a.k_off_step == 0);
    // (round 6) pairs that fill the chip at most once -- C3's projection: 4 x 64 = 256 workgroups, one per CU, whose K loop runs at
    // 79 % alone -- run unpaired instead, heavy and light tile of a pair as TWO workgroups of one CU (88 % together)
    if (EPI == 1 && pair_ok && gx >= 4 && !(gx & 1) && a.b_tri_rows >= a.n && a.max_wgs == 0 &&
        (long)(gx / 2) * gy * nb <= GPK_TUNE(PROJ_UNPAIR_UPTO, 256)) {
      p.tile_snake = 1;
      p.stagger_first = 256;
      p.stagger_ticks = 0;
      p.kind = 2 + 2 * EPI;
      p.grid_x = (unsigned)p.total;
      return;
    }
    if (pair_ok && gx >= 4 && a.b_tri_rows >= a.n) {
      p.total = ((gx + 1) / 2) * gy;
      p.kind = 2 + 2 * EPI + 1;
      p.pair = 1;
      p.pair_k_align = GPK_TUNE(PAIR_K_ALIGN, 1);
      p.grid_x = (unsigned)p.total;
      return;
    }
  }
  int tail_tiles = 0;
  // Tail split of the capped launches of the extra-row stream (round 5): 224 persistent workgroups walk 768 / 512 /
  // 256 tiles in 4 / 3 / 2 rounds of ~78 us where 3.43 / 2.29 / 1.14 would do -- a few rounds, no drift, and that stream is the
  // critical path of the SVGP step.  The whole rounds stay on the persistent workgroups; the remainder runs as 64 x 64 quarters
  // on every compute unit, for about a third of a round.
  if (EPI == 0 && !a.c_lower && a.max_wgs > 0 && a.max_wgs < p.total && nb == 1 && !a.b_tri && !a.a_tri &&
      GPK_TUNE(TAIL_SPLIT_CAPPED, 1)) {
    const int r = p.total % a.max_wgs;
    if (r > 0 && r * 100 <= a.max_wgs * GPK_TUNE(TAIL_SPLIT_CAPPED_PCT, 60)) tail_tiles = r;
  }
  const int total_all = p.total;
  p.total -= tail_tiles;
  const int total = p.total;
  unsigned nwg = (unsigned)total;
  if (a.max_wgs > 0 && (unsigned)a.max_wgs < nwg) nwg = (unsigned)a.max_wgs;
  p.kind = 2 + 2 * EPI;
  {
    // half a tile in 100 MHz ticks: a 128x128x16 slab costs ~1.7 us per workgroup when two share a CU
    // (A/B, 16384^2 x 512, beta = 1: 60.7 -> 63.0 TFLOP/s; lower-only 55.8 -> 58.8; percent of a half tile, 0 = off)
    const int stagger_on = GPK_TUNE(GEMM_STAGGER, 100);
    if (p.stagger_first <= 0) p.stagger_first = 256;
    p.stagger_ticks = (stagger_on && EPI == 0 && !a.b_tri && total >= 1024 && (nwg == (unsigned)total || nwg >= 2u * (unsigned)p.stagger_first))
                          ? (int)((a.k / 16) * 170 * stagger_on / 200)
                          : 0;
  }
  // A CAPPED launch (persistent workgroups, fewer than compute units x 2) asks for more than half of a CU's LDS, so that no two
  // of its workgroups can share a compute unit.  Without that the dispatcher doubles them up on whatever CUs are free at launch
  // time -- the chain's strip holds 80 - 120 CUs for ~10 us -- and, the tile walk being static, the doubled-up pairs run at half
  // speed for the WHOLE kernel: the first extra-row update of an SVGP step took 318 or 483 us depending on what it was launched
  // beside (profiles/r05_step_timeline_before_extra_row_work.txt, round 5).
  if (EPI == 0 && a.max_wgs > 0 && nwg < (unsigned)total && nb == 1) {
    const int kb = GPK_TUNE(CAP_EXCL_LDS_KB, 84);
    if (kb > 0 && kb <= 160 && (size_t)kb * 1024 > kGemmFastLds) p.lds_bytes = (size_t)kb * 1024;
  }
  if (EPI == 0 && tail_tiles == 0 && a.max_wgs == 0 &&
      ((a.k_off_step && GPK_TUNE(KSPLIT_QUEUE, 1)) || (a.tile_queue && (long)total * nb > 512))) {
    p.queue = 1;
    p.stagger_ticks = 0;
    const long all = (long)total * nb;
    const long qw = a.stagger_first > 0 ? 2L * a.stagger_first : GPK_TUNE(QUEUE_WGS, 512);   // (two per compute unit of the launch stream)
    p.queue_wgs = (unsigned)(all < qw ? all : qw);
    p.queue_fetches = (unsigned)all + p.queue_wgs;
    p.lds_bytes = kGemmFastLds;
    p.grid_x = p.queue_wgs; p.grid_y = 1;
    return;
  }
  p.grid_x = nwg;
  if (tail_tiles > 0) {
    p.tail_tiles = tail_tiles;
    p.tail_first1 = total_all - tail_tiles + 1;
    p.tail_grid_x = (unsigned)(4 * tail_tiles);
  }
}

// Everything gpk_launch_gemm decides for one call.  gpk_gemm_fuses_row_stats(a) is "kernel == fast with sp";
// gpk_gemm_takes_latency_kernel(a) is "kernel == small" -- the selection's own answer, tile64 (tested first) and the stat_* refusal
// included, where the predicate of old only asked  !no_small && small_ok  (its callers, the strip and the split rest-update of
// potrf.hip, set neither tile64 nor stat_*, so the two definitions agree for them).
static inline GemmPlan make_gemm_plan(const GemmArgs& a) {
  GemmPlan p;
  p.tile_snake = a.tile_snake; p.stagger_first = a.stagger_first; p.stagger_ticks = a.stagger_ticks;
  p.pair_k_align = a.pair_k_align;
  if (a.m <= 0 || a.n <= 0) return p;
  const auto unsupported = [&p]() { p.kernel = GemmKernel::unsupported; return p; };
  if (a.stat_sumsq && !gemm_row_stats_fusable(a)) return unsupported();   // (the caller asks first: drivers.hip, project_parts)
  const long tiles = (long)gemm_cdiv(a.m, 128) * gemm_cdiv(a.n, 128) * gemm_nbatch(a);
  if (a.tile64 && a.epi == 0) {
    if (GPK_TUNE(REST_PRE64, 1) && gemm_pre64_ok(a)) gemm_plan_pre64(a, p);
    else gemm_plan_generic(a, p, GemmTile::t64x64);
    return p;
  }
  if (!a.no_small && gemm_small_ok(a)) {   // K <= 128, <= 512 workgroups: the latency path
    gemm_plan_small(a, p);
    return p;
  }
  if (a.epi == 1 && a.beta != 0.0 && a.C && !gemm_fast_ok(a)) return unsupported();  // only the fast tile preloads C for epi 1
  GemmTile tile = GemmTile::t128x128;
  if (a.epi == 0 && a.k >= GPK_TUNE(HALF_TILE_KMIN, 1024) && a.m > 64 && a.n > 64 && (a.max_wgs == 0 || a.max_wgs >= tiles) &&
      (a.c_lower ? tiles / 2 : tiles) < GPK_TUNE(HALF_TILE_BELOW, 300)) {
    // under-filled long-K launches (the M^3 triangular products of the reverse pass: 256 tiles of 128 x 128 = ONE
    // workgroup per CU, so the launch lasts as long as its longest tile, 283 us at M = 2048) go to 64 x 128 tiles:
    // twice the workgroups, half the longest tile.  Training step 7.15 -> 6.90 ms (same box, 300; 600: 7.00).
    tile = GemmTile::t64x128_1x4;
  } else if (gemm_proj_small_tiles(a)) {
    // under-filled projections (a rank's 1024-row shard of a strong-scaled step: 8 row tiles x 8 column pairs = 64
    // workgroups, ONE of them per four CUs, 296 us for 4.3 GFLOP; a CU cannot finish a 128 x 128 x 16 slab in less than
    // 1.7 us however many workgroups it holds): 64 x 64 tiles, unpaired -- sixteen times the workgroups.
    // tools/proj_small_probe.py (profiles/r03_projection_few_rows.txt), paired 128-row tiles / 64 x 128 / 64 x 64:
    // 1024 x 2048: 296 / 194 / 155 us, 300 x 1024 (P = 2): 162 / 98 / 62 us, 2048 x 2048: 306 / 268 / 221 us; from 256 pairs
    // on the paired 128-row tiles win (4096 x 2048: 327 us against 483 us on 64 x 128).
    p.tile_snake = GPK_TUNE(PROJ_SNAKE, 1);
    // (every 64-column partial slot the reduction reads must be written: 64-wide tiles only if they cover the same
    // slots as the 128-wide ones, else 64 x 128 tiles)
    if (gemm_cdiv(a.n, 64) != 2 * gemm_cdiv(a.n, 128)) tile = GemmTile::t64x128_2x2;
    else tile = gemm_proj_pairs(a) < GPK_TUNE(PROJ_TILE32_BELOW, 100) ? GemmTile::t32x64 : GemmTile::t64x64;
  } else if (gemm_fast_ok(a) && (a.epi == 1 || (a.n > 64 && (tiles >= 24 || a.m <= 64)))) {
    gemm_plan_fast(a, p);
    return p;
  } else if (a.epi == 1) {
    tile = GemmTile::t128x128;
  } else if (a.n <= 64) {
    tile = GemmTile::t128x64;
  } else if (tiles < 192 && a.m > 64) {
    // narrow / small problems: 64-row tiles double the number of workgroups (256 CUs to fill)
    tile = GemmTile::t64x128_1x4;
  }
  gemm_plan_generic(a, p, tile);
  return p;
}
