// Fused in-group solves of the trapezoidal Cholesky (potrf.hip): right-hand-side rows against a column group of the factor, two
// kernels (staged 16-row slivers, pipelined 32-row slivers) and the choice between them.  fp64 MFMA, gfx950.
#include "gpk_internal.h"
#include <algorithm>

namespace {


// =====================================================================================================
// Fused in-group solve of right-hand-side ROWS against a column group of the factor (nb <= 4 leaf blocks):
//     for j = 0 .. nb-1:   S_j = E_j X_j^T                       (X_j = L_jj^-1, the leaf's block inverse)
//                          E_j' -= S_j L_j'j^T   for j' > j       (the rest of the group)
// i.e. exactly the 2 nb - 1 launches of the latency kernel (gemm.hip, gemm_nt_small) that the right-looking row solve issues per group
// (4 solves + 3 updates at nb = 4), with the SAME arithmetic per element (two alternating accumulators over K = 128,
// the update accumulated onto -C and negated) -- so the results are bit-identical -- but as ONE launch: a workgroup owns
// 16 rows, keeps their nb x (16 x 128) panel in accumulator registers for the whole group (8 waves x one 16 x 16 tile
// per block), and only the 10 operand tiles X_j / L_j'j stream through LDS.  The extra-row stream of an SVGP step spent
// ~150 us per group in those seven dependent launches (mostly launch ramp and drain on a 256-CU chip); this is one.
struct GroupSolveArgs {
  const double* E; long lde;     // rows to solve, columns of the group start at E (in/out unless Eo differs)
  double* Eo; long ldeo;         // solved rows out (may alias E)
  const double* L; long ldl;     // L[c0, c0]: top-left element of the group's diagonal block
  const double* X;               // block inverses of the group, consecutive [nb][128][128]
  int rows, nb;
  long strideE, strideEo, strideL, strideX;   // batched form (blockIdx.y = problem): element offsets between problems
  int j0, j1;                                 // group_solve2_kernel: leaf blocks [j0, j1) are solved by THIS launch (the blocks before j0 by
                                              // earlier ones); the updated, still unsolved blocks >= j1 go back to E (E == Eo then)
};

__global__ __launch_bounds__(512) void group_solve_kernel(GroupSolveArgs p) {
  constexpr int LDK = 130, NBK = 128;
  {
    const long b = blockIdx.y;
    p.E += b * p.strideE; p.Eo += b * p.strideEo; p.L += b * p.strideL; p.X += b * p.strideX;
  }
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  double* As = smem;               // [16][LDK]
  double* Bs = smem + 16 * LDK;    // [128][LDK]
  // (gridDim.x < number of 16-row slivers: the workgroup walks the slivers with stride gridDim.x -- a cap on the resident
  //  workgroups keeps compute units free for the factorisation's chain, GROUP_SOLVE_MAX_WGS in potrf.hip)
  for (int m0 = blockIdx.x * 16; m0 < p.rows; m0 += gridDim.x * 16) {
  if (m0 != (int)blockIdx.x * 16) __syncthreads();   // the previous sliver's last operand tile is no longer read
  int rowi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int rr = m0 + g + 4 * e;
    rowi[e] = rr < p.rows ? rr : p.rows - 1;
  }
  const int colw = wave * 16 + r;  // this lane's column inside a 128-block
  d4 c[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    if (jb < p.nb) {
#pragma unroll
      for (int e = 0; e < 4; ++e) c[jb][e] = p.E[(long)rowi[e] * p.lde + jb * NBK + colw];
    }
  }
  const double* ap = As + r * LDK + g;
  const double* bp = Bs + (wave * 16 + r) * LDK + g;
  auto stage_b = [&](const double* src, long ld) {  // 128 rows of 128 doubles, one LDS-DMA instruction each
    for (int q = wave; q < NBK; q += 8)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long)q * ld + 2 * lane),
                                       (__attribute__((address_space(3))) void*)(Bs + q * LDK), 16, 0, 0);
  };
  auto put_a = [&](const d4& v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) As[(g + 4 * e) * LDK + colw] = v[e];
  };
  auto product = [&](d4& acc0, d4& acc1) {
#pragma unroll 4
    for (int kk = 0; kk < 32; kk += 2) {
      const double a0 = ap[kk * 4], b0 = bp[kk * 4];
      const double a1 = ap[kk * 4 + 4], b1 = bp[kk * 4 + 4];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
  };
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= p.nb) break;
    // ---- S_j = E_j X_j^T ------------------------------------------------------------------------------------------
    if (j > 0) __syncthreads();  // previous readers of As / Bs are done
    put_a(c[j]);
    stage_b(p.X + (long)j * NBK * NBK, NBK);
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0): this wave's LDS-DMA rows have landed
    __syncthreads();
    d4 s0 = {0.0, 0.0, 0.0, 0.0}, s1 = {0.0, 0.0, 0.0, 0.0};
    product(s0, s1);
    d4 sj;
#pragma unroll
    for (int e = 0; e < 4; ++e) sj[e] = 1.0 * (s0[e] + s1[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rr = m0 + g + 4 * e;
      if (rr < p.rows) p.Eo[(long)rr * p.ldeo + j * NBK + colw] = sj[e];
    }
    if (j + 1 >= p.nb) break;
    __syncthreads();  // everyone has read E_j / X_j
    put_a(sj);
    // ---- E_j' -= S_j L_j'j^T ----------------------------------------------------------------------------------------
#pragma unroll
    for (int jp = 1; jp < 4; ++jp) {
      if (jp <= j || jp >= p.nb) continue;
      if (jp > j + 1) __syncthreads();  // the previous operand tile is no longer read
      stage_b(p.L + (long)jp * NBK * p.ldl + (long)j * NBK, p.ldl);
      __builtin_amdgcn_s_waitcnt(0x0070);
      __syncthreads();
      d4 u0, u1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int e = 0; e < 4; ++e) u0[e] = -1.0 * c[jp][e];  // (beta / alpha) C with alpha = -1, beta = 1
      product(u0, u1);
#pragma unroll
      for (int e = 0; e < 4; ++e) c[jp][e] = -1.0 * (u0[e] + u1[e]);
    }
  }
  }  // sliver loop
}


// Round 5: the same in-group solve with 32 rows per workgroup and the operand tiles PIPELINED through LDS.
// The kernel above stages each 128 x 128 operand tile whole (133 KB, nothing else fits) and waits for it: 10 exposed L2 round trips
// per 16-row sliver, 512 workgroups at one per compute unit = two rounds, ~111 us per 8192 x 512 group on the extra-row stream --
// which is the critical path of the SVGP step from the fourth panel on (profiles/r05_step_timeline_before_extra_row_work.txt).  Here
//   * a workgroup owns TWO 16-row tiles: every B fragment read from LDS feeds two MFMAs, 256 workgroups = one round at 8192 rows;
//   * the operand tiles of all products of the group form ONE stream of K-quarters (128 rows x 32 K = 32 KB, up to 40 of them)
//     that runs two quarters ahead of the MFMAs through a ring of three LDS buffers, across product boundaries -- their addresses
//     do not depend on any result;
//   * the quarters are unpadded; the 16-byte chunk c of tile row r sits in slot c ^ (r & 15) (the permutation is applied on the
//     GLOBAL address of the LDS-DMA lane), so the 32 lanes of a ds_read_b64 group still hit 64 distinct banks.
// Per element the arithmetic is unchanged (K ascending, two alternating accumulators, the update accumulated onto -C and negated).
constexpr int GS2_LDK = 130;                     // A rows: 128 + 2 doubles
// GS2_QK = K columns per pipeline stage: 40 stages of 16 MFMAs per wave, 132 KB of LDS (a compute unit of its own).  GS2_RING = stage
// buffers; the operand stream runs GS2_RING - 1 stages ahead of the MFMAs.  (Stage width 16 and a ring of 5: DESIGN 6, "Closed
// experiments whose code was removed".)
constexpr int GS2_QK = 32, GS2_RING = 3;
constexpr size_t GS2_LDS = (size_t)(32 * GS2_LDK + GS2_RING * 128 * GS2_QK) * sizeof(double);

// s_waitcnt vmcnt(n * DPW) for a wave-uniform n in 0 .. NMAX (the instruction takes an immediate)
template <int DPW, int NMAX>
__device__ __forceinline__ void gs2_wait_vm(int n) {
  if constexpr (NMAX > 0) {
    if (n >= NMAX) {
      constexpr int c = NMAX * DPW;
      static_assert(c < 64, "vmcnt");
      __builtin_amdgcn_s_waitcnt(0x0F70 | (c & 15) | ((c >> 4) << 14));
      return;
    }
    gs2_wait_vm<DPW, NMAX - 1>(n);
  } else {
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }
}

__global__ __launch_bounds__(512) void group_solve2_kernel(GroupSolveArgs p) {
  constexpr int LDK = GS2_LDK, NBK = 128, QK = GS2_QK, RING = GS2_RING;
  constexpr int AHEAD = RING - 1;
  constexpr int NQ = NBK / QK;            // stages per product
  constexpr int QELEMS = 128 * QK;        // doubles per stage buffer
  constexpr int CH = QK / 2;              // 16-byte chunks per row of a stage
  constexpr int DROWS = 64 / CH;          // rows per LDS-DMA instruction
  constexpr int DPW = (128 / DROWS) / 8;  // LDS-DMA instructions per wave and stage
  static_assert(QK == 32, "stage width: the chunk swizzle below");
  {
    const long b = blockIdx.y;
    p.E += b * p.strideE; p.Eo += b * p.strideEo; p.L += b * p.strideL; p.X += b * p.strideX;
  }
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  double* As = smem;                 // [32][LDK]
  double* Bq = smem + 32 * LDK;      // [RING][128][QK], chunk-swizzled
  const int nb = p.nb, j0 = p.j0, j1 = p.j1;
  int nprod = 0;
  for (int j = j0; j < j1; ++j) nprod += nb - j;
  const int nstages = NQ * nprod;
  // swizzle of a tile row's 16 chunks
  auto swz = [](int row) -> int { return row & 15; };
  // LDS-DMA of one stage: 64 lanes x 16 bytes = DROWS rows x CH chunks per instruction.  The operand tiles come in issue order
  // (j = j0: X_j0, L_(j0+1)j0, ...; then j0 + 1: ...), tracked by (pj, pjp, pq): block column, block row (pjp == pj: the block
  // inverse X_pj), stage inside the tile.  Per lane only a 32-bit element offset inside the tile, for either row stride.
  const int drow = lane / CH, dslot = lane % CH;
  const int drow0 = wave * DPW * DROWS + drow;   // this lane's row in the wave's first copy; copy i adds i * DROWS
  int issue = 0, pj = j0, pjp = j0, pq = 0;
  auto issue_stage = [&]() {
    if (issue < nstages) {
      const bool isx = pjp == pj;
      const double* src = (isx ? p.X + (long)pj * NBK * NBK : p.L + (long)pjp * NBK * p.ldl + (long)pj * NBK) + pq * QK;
      const unsigned ld = isx ? (unsigned)NBK : (unsigned)p.ldl;   // (rows < 128, ld < 2^21: 32-bit element offsets)
      double* dst = Bq + (issue % RING) * QELEMS;
#pragma unroll
      for (int i = 0; i < DPW; ++i) {
        const int rb = wave * DPW + i;
        const int row = drow0 + i * DROWS;
        const double* gsrc = src + ((unsigned)row * ld + (unsigned)((dslot ^ swz(row)) << 1));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                         (__attribute__((address_space(3))) void*)(dst + rb * 128), 16, 0, 0);
      }
      if (++pq == NQ) {
        pq = 0;
        if (pjp + 1 < nb) ++pjp;
        else { ++pj; pjp = pj; }
      }
    }
    ++issue;
  };
  // fragment addresses: B[row 16 w + r][k = 4 kk + g] of a stage -> chunk 2 kk + (g >> 1), half g & 1
  const int brow = (wave * 16 + r) * QK + (g & 1);
  const int bsw = swz(r), bgh = g >> 1;
  const double* ap = As + r * LDK + g;
  for (int m0 = blockIdx.x * 32; m0 < p.rows; m0 += gridDim.x * 32) {
    if (m0 != (int)blockIdx.x * 32) __syncthreads();   // the previous sliver's buffers are no longer read
    issue = 0; pj = j0; pjp = j0; pq = 0;
    int cs = 0;
#pragma unroll
    for (int a = 0; a < AHEAD; ++a) issue_stage();
    const int colw = wave * 16 + r;
    int rowi[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = m0 + 16 * t + g + 4 * e;
        rowi[t][e] = rr < p.rows ? rr : p.rows - 1;
      }
    d4 c[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        if (jb >= j0 && jb < nb) {
#pragma unroll
          for (int e = 0; e < 4; ++e) c[t][jb][e] = p.E[(long)rowi[t][e] * p.lde + jb * NBK + colw];
        }
      }
    auto put_a = [&](const d4& v0, const d4& v1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[(g + 4 * e) * LDK + colw] = v0[e];
        As[(16 + g + 4 * e) * LDK + colw] = v1[e];
      }
    };
    // one stage of the current product: acc[t][0] takes the even K groups of four, acc[t][1] the odd ones
    // The B rows a wave reads (tile rows 16 w .. 16 w + 15 = its output columns) are the rows IT copies: the operand stream needs
    // no workgroup barrier at all, only the wave's own vmcnt -- the eight waves drift apart and fill each other's LDS waits.  The
    // A rows are shared: one barrier after each put_a (first stage of a product whose A operand changed).
    auto stage = [&](int q, d4 (&acc)[2][2], bool a_changed) {
      // stage cs has landed when at most the stages behind it are in flight: min(AHEAD - 1, stages left) x DPW of this wave's copies
      {
        const int behind = nstages - 1 - cs < AHEAD - 1 ? nstages - 1 - cs : AHEAD - 1;
        gs2_wait_vm<DPW, AHEAD - 1>(behind);
      }
      asm volatile("" ::: "memory");
      if (a_changed) {
        __builtin_amdgcn_s_waitcnt(0xC07F);                      // lgkmcnt(0): this wave's A rows are in LDS
        __builtin_amdgcn_s_barrier();
      }
      issue_stage();   // stage cs + AHEAD replaces stage cs - 1 of this wave's rows, whose fragments it has consumed
      // fragments double-buffered in registers, the three LDS reads of step kk + 1 between the two MFMAs of step kk.  (Measured
      // and not kept: the same pipeline hand-issued three steps deep with counted lgkmcnt waits -- 64.3 against 62.3 us per launch,
      // and rings of 5 / 7 stage buffers -- 72 - 84 us: neither the LDS round trip nor the L2 one is what a sliver waits for; the
      // seven barrier pairs around the changes of the shared A rows and the 20-odd us of launch, load and store are.)
      const double* bq = Bq + (cs % RING) * QELEMS + brow;
      double fb[2], fa0[2], fa1[2];
      auto frag = [&](int kk, int f) {
        fb[f] = bq[((2 * kk + bgh) ^ bsw) << 1];
        fa0[f] = ap[q * QK + kk * 4];
        fa1[f] = ap[16 * LDK + q * QK + kk * 4];
      };
      frag(0, 0);
#pragma unroll
      for (int kk = 0; kk < QK / 4; ++kk) {
        if (kk + 1 < QK / 4) frag(kk + 1, (kk + 1) & 1);
        acc[0][kk & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0[kk & 1], fb[kk & 1], acc[0][kk & 1], 0, 0, 0);
        acc[1][kk & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1[kk & 1], fb[kk & 1], acc[1][kk & 1], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // 1 MFMA
        if (kk + 1 < QK / 4) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);   // 3 DS reads
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // 1 MFMA
      }
      ++cs;
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < j0) continue;
      if (j >= j1) break;
      // ---- S_j = E_j X_j^T --------------------------------------------------------------------------------------------
      if (j > j0) __syncthreads();   // every wave has finished reading the previous A rows
      put_a(c[0][j], c[1][j]);
      d4 acc[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t) { acc[t][0] = (d4){0.0, 0.0, 0.0, 0.0}; acc[t][1] = (d4){0.0, 0.0, 0.0, 0.0}; }
#pragma unroll
      for (int q = 0; q < NQ; ++q) stage(q, acc, q == 0);
      d4 sj[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sj[t][e] = 1.0 * (acc[t][0][e] + acc[t][1][e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rr = m0 + 16 * t + g + 4 * e;
          if (rr < p.rows) p.Eo[(long)rr * p.ldeo + j * NBK + colw] = sj[t][e];
        }
      }
      if (j + 1 >= nb) break;
      __syncthreads();   // everyone has read E_j
      put_a(sj[0], sj[1]);
      // ---- E_j' -= S_j L_j'j^T ----------------------------------------------------------------------------------------
#pragma unroll
      for (int jp = 1; jp < 4; ++jp) {
        if (jp <= j || jp >= nb) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][0][e] = -1.0 * c[t][jp][e];  // (beta / alpha) C with alpha = -1, beta = 1
          acc[t][1] = (d4){0.0, 0.0, 0.0, 0.0};
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) stage(q, acc, q == 0 && jp == j + 1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) c[t][jp][e] = -1.0 * (acc[t][0][e] + acc[t][1][e]);
      }
    }
    // a partial launch hands the updated, unsolved blocks back (in place)
#pragma unroll
    for (int jp = 1; jp < 4; ++jp) {
      if (jp < j1 || jp >= nb) continue;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rr = m0 + 16 * t + g + 4 * e;
          if (rr < p.rows) p.Eo[(long)rr * p.ldeo + jp * NBK + colw] = c[t][jp][e];
        }
    }
  }  // sliver loop
}

// Which kernel, and how many workgroups per problem.  The pipelined one (32 rows per workgroup) runs its 10 block products in ~63 us
// whatever the row count; the staged one (16 rows) needs ~45 us per ROUND of 256 workgroups (one per CU).
// tools/group_solve_probe.py, 512 columns, us:
//   rows 1024: 41 / 62   2048: 47 / 64   4096: 54 / 66   8192: 101 / 74   (staged / pipelined)
// so the pipelined kernel takes over where the staged one would need a second round.  (The first version of this switch sent
// everything to the pipelined kernel: the 1024- / 2048- / 4096-row rank shards of the strong-scaling workload lost 5 / 9 / 5 %.)
// Only the pipelined kernel solves blocks [j0, j1) of a group and hands the later blocks back updated (`partial`).
struct GroupSolveChoice { bool pipelined; unsigned wgs; };
GroupSolveChoice group_solve_choice(int rows, int batch, int max_wgs, bool partial) {
  const long slivers16 = (long)gpk_cdiv(rows, 16) * batch;
  GroupSolveChoice c;
  c.pipelined = GPK_TUNE(GROUP_SOLVE_V2, 1) && (partial || slivers16 > GPK_TUNE(GROUP_SOLVE_V2_MIN_SLIVERS, 256));
  c.wgs = (unsigned)gpk_cdiv(rows, c.pipelined ? 32 : 16);
  if (max_wgs > 0 && c.wgs * (unsigned)batch > (unsigned)max_wgs) c.wgs = (unsigned)std::max(1, max_wgs / batch);
  return c;
}

}  // namespace

// (a partial solve is one the choice sends to the pipelined kernel whatever its size)
bool gpk_group_solve_takes_parts() { return group_solve_choice(1, 1, 0, true).pipelined; }

int gpk_launch_group_solve(hipStream_t s, const double* E, long lde, double* Eo, long ldeo, int rows, const double* Lgg, long ldl,
                           const double* X, int nb, int batch, long strideE, long strideEo, long strideL, long strideX, int max_wgs,
                           int j0, int j1) {
  if (rows <= 0) return 0;
  if (j1 < 0) j1 = nb;
  if (j0 < 0 || j0 >= j1 || j1 > nb) return GPK_E_ARG;
  const bool partial = j0 > 0 || j1 < nb;
  if (partial && (E != Eo || lde != ldeo || strideE != strideEo || !gpk_group_solve_takes_parts())) return GPK_E_UNSUPPORTED;
  if (batch < 1) batch = 1;
  if (!E || !Eo || !Lgg || !X || nb < 1 || nb > 4) return GPK_E_ARG;
  if ((ldl & 1) || (reinterpret_cast<uintptr_t>(Lgg) & 15) || (reinterpret_cast<uintptr_t>(X) & 15)) return GPK_E_UNSUPPORTED;
  if (batch > 1 && ((strideL & 1) || (strideX & 1))) return GPK_E_UNSUPPORTED;   // (16-byte LDS-DMA of every problem's tiles)
  constexpr size_t LDS = (size_t)(16 + 128) * 130 * sizeof(double);
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(group_solve_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
  GPK_HIP(attr);
  GroupSolveArgs a{};
  a.E = E; a.lde = lde; a.Eo = Eo; a.ldeo = ldeo; a.L = Lgg; a.ldl = ldl; a.X = X; a.rows = rows; a.nb = nb;
  a.strideE = strideE; a.strideEo = strideEo; a.strideL = strideL; a.strideX = strideX;
  a.j0 = j0; a.j1 = j1;
  const GroupSolveChoice c = group_solve_choice(rows, batch, max_wgs, partial);
  const dim3 grid(c.wgs, (unsigned)batch);
  if (c.pipelined) {
    static const hipError_t attr2 = hipFuncSetAttribute(reinterpret_cast<const void*>(group_solve2_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)GS2_LDS);
    GPK_HIP(attr2);
    hipLaunchKernelGGL(group_solve2_kernel, grid, dim3(512), GS2_LDS, s, a);
  } else {
    hipLaunchKernelGGL(group_solve_kernel, grid, dim3(512), LDS, s, a);
  }
  GPK_LAUNCH_CHECK();
  return 0;
}
