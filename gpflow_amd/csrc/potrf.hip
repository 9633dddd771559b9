// Host-side orchestration (no device code here): the trapezoidal blocked Cholesky on its per-device stream set and the
// triangular solves against a cached factor.  (What merely CALLS the factorisation -- the projection onto q_sqrt and the
// fused model drivers -- is drivers.hip, through gpk_potrf_core.)
//
// Trapezoidal Cholesky.  A is [(n + extra) x n]: the top square block is factored, the `extra` rows
// below ride along through every panel solve and trailing update and come out as  B L^-T  -- the
// tf.linalg.triangular_solve of the reference fused into the factorisation.  Two-level right-looking:
//   outer panels of 640 columns (n >= 4096) -> trailing update is a K = 640 MFMA GEMM,
//   inner blocks of NB = 128 columns        -> leaf kernel (L11 and L11^-1), in-place panel solve
//                                              A21 <- A21 * L11^-T as a GEMM, update of the rest of the panel.
// For n < 4096 (the SVGP sizes) the outer panel IS one 128-column block: the factorisation is a latency chain
// leaf -> panel solve -> strip, and everything that is not on that chain (the solve of the minibatch rows) runs beside it
// as bulk work on a stream of its own.
//
// How the scheduler is laid out (gpk_potrf_core is an outline over these):
//   potrf_plan.h   WHAT to do: make_potrf_plan() turns (n, extra, batch, tri) and two device facts into the schedule as data -- panel
//                  cuts, wide / narrow panels, ride or extra-row stream, group ends, tail zone, progressive first group, the regime of
//                  each rest-update, which hand-off may be a flag word, streams by role.  No HIP header; every threshold and the A/B
//                  measurement behind it is there; tested without a device (tests/test_potrf_plan.py).
//   ChainSync      HOW streams hand over: flag word (written on a kernel's entry or by a set-flag kernel), gate kernel or stream wait,
//                  event recorded only on demand.
//   PotrfRun       the enqueue calls: enqueue_chain / enqueue_rest_update / enqueue_extra_rows per panel.  The three predicates that
//                  depend on the operands are applied there (and once in gpk_potrf_core, for the progressive group), ANDed with the
//                  plan's *_candidate fields.
#include "gpk_internal.h"
#include "potrf_plan.h"
#include <algorithm>
#include <mutex>
#include <vector>

namespace {
constexpr int NB = kPotrfNB;
constexpr int NBO = kPotrfNBO;   // column group of the right-looking row solves (extra rows, gpk_trsm)
}  // namespace

extern "C" const char* gpk_version(void) {
#ifdef GPK_EXPERIMENTAL
  return "gpk 0.4 (gfx950, fp64 MFMA) [A/B build: environment tunables enabled]";
#else
  return "gpk 0.4 (gfx950, fp64 MFMA)";
#endif
}

extern "C" size_t gpk_invd_elems(int n, int batch) {
  return (size_t)(batch > 0 ? batch : 1) * gpk_cdiv(n, NB) * NB * NB;
}

namespace {
// gpk.h, "invd": the block inverses are stored and staged 16 bytes at a time (leaf2_device.h, group_solve.hip), whatever the
// alignment of the factor -- checked on the host by every entry point that takes one, before anything is launched
bool invd_aligned(const double* invd) { return (reinterpret_cast<uintptr_t>(invd) & 15) == 0; }
}  // namespace

// ---- per-device internal state (created lazily, once; see gpk.h "Internal state and threading") -------------------
// The factorisation runs on streams of its own, forked from / joined to the caller's stream with events only:
//   P   "panel" stream, high priority: the latency-bound critical path (leaf, panel solve, inner updates, strip) of
//       the NEXT outer panel (look-ahead);
//   B   bulk stream, CU-masked in hardware: its mask leaves 8 compute units (one per XCD; mask bit i is CU i/8 of XCD
//       i%8 on MI355X, tools/cumask_test.hip) to the panel stream -- without that the one-workgroup leaf kernel, which
//       needs a whole CU's LDS, queues behind thousands of resident GEMM workgroups (a 2 ms stall per panel at
//       N = 16384) and the look-ahead never overlaps.  Large factorisations (n >= 4096) only: the big MFMA GEMMs of the
//       outer trailing updates and of the extra rows;
//   Bs  rest-updates of SMALL factorisations and of the single-leaf panels at the end of large ones (they are ON the
//       critical path there): all CUs.  (Rounds 1-2 ran that end of a large factorisation with wide panels and a second
//       masked stream over half the CUs; round 3 measured every hand-off from that stream to P at ~55 us while both are
//       busy -- their hardware queues share a microengine pipe -- and replaced it: potrf_plan.h, "Panel boundaries".)
//   X   bulk stream of small factorisations: the right-looking solve of the extra rows (the SVGP minibatch).  Unmasked:
//       CU-masked queues dispatch its short kernels slowly and quantise its big updates badly (profiles/r03_*).
// One std::recursive_mutex per device serialises the ENQUEUE of factorisations (shared streams, event pool); the
// enqueued work of successive calls is ordered by the streams themselves.
namespace {
struct Aux {
  std::recursive_mutex mu;
  bool ready = false;
  int init_rc = 0;  // sticky: a failed stream set-up is reported by every later call instead of being retried
  hipStream_t P = nullptr, B = nullptr, Bs = nullptr, X = nullptr, pad = nullptr;
  hipEvent_t* ev = nullptr;
  int nev = 0;
  int ncu = 0, bulk_cus = 0;
  // stream-layout self-check (aux_get): microseconds per cross-stream hand-off P<->X, P<->Bs, X<->Bs as first measured and
  // after a possible re-creation of the streams; recreated = 1 if the first layout failed the check
  double check_us[3] = {0, 0, 0}, check_first_us[3] = {0, 0, 0};
  int recreated = 0;
  hipStream_t shift = nullptr;   // (kept alive: the extra stream that moved the re-created set onto other hardware queues)
  // packet-free hand-offs of the latency chain (ChainSync, "Chain flags"): one word per panel for "panel solved" (F) and for
  // "rest-update done" (R), written with the epoch of the factorisation that owns them (monotonic per device)
  int* flags = nullptr;
  int epoch = 0;
  int concurrent = -1;   // 1: kernels of two streams were seen running at the same time (init-time probe); 0: serialised by a tool
};
Aux g_aux[16];

int masked_stream(hipStream_t* out, int ncu, int first, int last) {  // CUs [first, last)
  if (first <= 0 && last >= ncu) return (int)hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  uint32_t mask[32] = {0};
  for (int i = first; i < last; ++i) mask[i >> 5] |= 1u << (i & 31);
  return (int)hipExtStreamCreateWithCUMask(out, (uint32_t)((ncu + 31) / 32), mask);
}

int aux_create(Aux& a, int dev) {
  int lo = 0, hi = 0;
  GPK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  hipDeviceProp_t prop;
  GPK_HIP(hipGetDeviceProperties(&prop, dev));
  const int ncu = prop.multiProcessorCount;
  a.ncu = ncu;
  // Stream -> hardware queue -> microengine pipe.  Two facts measured on MI355X (rocprofv3 kernel timelines of the
  // SVGP step, profiles/r02_*): (1) HIP keeps a pool of GPU_MAX_HW_QUEUES hardware queues per priority level: a new
  // stream opens a new queue while the pool is not full, afterwards it shares the queue with the fewest streams
  // (ties: the most recently opened queue); CU-masked and non-default-priority streams get queues of their own.
  // (2) Hardware queues are spread round-robin over FOUR pipes in creation order, and two queues of one pipe that
  // are active at the same time slow each other down badly: every kernel start / cross-queue event hand-off on them
  // then takes ~50 us instead of ~5 (queues 1 and 5, or 2 and 6: the step went from 2.2 to 3.3 - 4.4 ms).
  // Hence this creation order -- default stream = queue 1 (pipe 0) exists already:
  //   P -> queue 2 (pipe 1);  X -> queue 3 (pipe 2);  one unused stream, then Bs: with the usual pool of 2 the unused
  //   one shares X's queue and Bs lands on the default stream's (idle) queue 1, with a pool of 4 they open queues 4
  //   and 5 (pipes 3 and 0);  then the masked B -> pipe 3 (or 1).
  // The chain (P), its rest-updates (Bs) and the bulk stream (X or B) are then always on three different pipes.
  GPK_HIP(hipStreamCreateWithPriority(&a.P, hipStreamNonBlocking, hi));
  GPK_HIP(hipStreamCreateWithFlags(&a.X, hipStreamNonBlocking));
  GPK_HIP(hipStreamCreateWithFlags(&a.pad, hipStreamNonBlocking));
  GPK_HIP(hipStreamCreateWithFlags(&a.Bs, hipStreamNonBlocking));
  int reserved = GPK_TUNE(RESERVED_CUS, 32);   // (8 until round 6: see the tile queue of the trailing updates, potrf_plan.h)
  if (ncu > 1024 || reserved < 0 || reserved >= ncu) reserved = 0;
  int rc = masked_stream(&a.B, ncu, reserved, ncu);
  if (rc) return rc;
  a.bulk_cus = ncu - reserved;
  return 0;
}

// Cost of one cross-stream hand-off (kernel on a -> event -> kernel on b -> event -> ...), microseconds: ~5 when the two
// hardware queues sit on different microengine pipes, ~50 when they share one.
int handoff_us(hipStream_t a, hipStream_t b, double* us) {
  const int n = 24;
  hipEvent_t e0, e1, ea, eb;
  GPK_HIP(hipEventCreate(&e0));
  GPK_HIP(hipEventCreate(&e1));
  GPK_HIP(hipEventCreateWithFlags(&ea, hipEventDisableTiming));
  GPK_HIP(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
  int rc = 0;
  for (int rep = 0; rep < 2 && !rc; ++rep) {  // (first repetition warms the queues up)
    GPK_HIP(hipEventRecord(e0, a));
    for (int i = 0; i < n && !rc; ++i) {
      rc = gpk_launch_noop(a);
      if (!rc) rc = (int)hipEventRecord(ea, a);
      if (!rc) rc = (int)hipStreamWaitEvent(b, ea, 0);
      if (!rc) rc = gpk_launch_noop(b);
      if (!rc) rc = (int)hipEventRecord(eb, b);
      if (!rc) rc = (int)hipStreamWaitEvent(a, eb, 0);
    }
    if (!rc) rc = (int)hipEventRecord(e1, a);
    if (!rc) rc = (int)hipEventSynchronize(e1);
  }
  float ms = 0.f;
  if (!rc) rc = (int)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
  *us = (double)ms * 1e3 / (2.0 * n);
  return rc;
}

// Per-kernel cost (microseconds) of n empty kernels on EACH of the given streams while all of them are being fed at the
// same time -- two active hardware queues on one microengine pipe show up here ("pipes").
int concurrent_us(hipStream_t* st, int ns, double* us) {
  const int n = 48;
  hipEvent_t e0[4], e1[4];
  for (int i = 0; i < ns; ++i) {
    GPK_HIP(hipEventCreate(&e0[i]));
    GPK_HIP(hipEventCreate(&e1[i]));
  }
  int rc = 0;
  for (int rep = 0; rep < 2 && !rc; ++rep) {
    for (int i = 0; i < ns && !rc; ++i) rc = (int)hipEventRecord(e0[i], st[i]);
    for (int k = 0; k < n && !rc; ++k)
      for (int i = 0; i < ns && !rc; ++i) rc = gpk_launch_noop(st[i]);
    for (int i = 0; i < ns && !rc; ++i) rc = (int)hipEventRecord(e1[i], st[i]);
    for (int i = 0; i < ns && !rc; ++i) rc = (int)hipEventSynchronize(e1[i]);
  }
  for (int i = 0; i < ns; ++i) {
    float ms = 0.f;
    if (!rc) rc = (int)hipEventElapsedTime(&ms, e0[i], e1[i]);
    us[i] = (double)ms * 1e3 / n;
    (void)hipEventDestroy(e0[i]);
    (void)hipEventDestroy(e1[i]);
  }
  return rc;
}

// (caller holds a.mu)
int aux_get(int dev, Aux** out) {
  Aux& a = g_aux[dev];
  if (!a.ready) {
    if (a.init_rc) return a.init_rc;
    const int rc = aux_create(a, dev);
    if (rc) {  // no half-built stream set: give back what was created, remember the error
      for (hipStream_t* s : {&a.P, &a.X, &a.pad, &a.Bs, &a.B}) {
        if (*s) (void)hipStreamDestroy(*s);
        *s = nullptr;
      }
      a.init_rc = rc;
      return rc;
    }
    // Init-time self-check of the stream -> hardware-queue -> pipe layout ("pipes"): two of the three concurrently
    // active queues on one microengine pipe cost ~50 us per cross-stream hand-off instead of ~5-15, and a whole process then
    // runs 10-17 % slow at every problem size (seen on 2 of ~12 boxes in round 3).  Measured once here (a few hundred empty
    // kernels, ~1 ms, the only place the library synchronises); if any pair is slow the streams are created again behind
    // one more placeholder stream -- which shifts every stream of the set to the next hardware queue -- and measured again.
    {
      auto measure = [&](double* us) {
        (void)handoff_us(a.P, a.X, &us[0]); (void)handoff_us(a.P, a.Bs, &us[1]); (void)handoff_us(a.X, a.Bs, &us[2]);
      };
      measure(a.check_us);
      for (int i = 0; i < 3; ++i) a.check_first_us[i] = a.check_us[i];
      const double limit = (double)GPK_TUNE(HANDOFF_LIMIT_US, 30);
      if (a.check_us[0] > limit || a.check_us[1] > limit || a.check_us[2] > limit) {
        for (hipStream_t* st : {&a.P, &a.X, &a.pad, &a.Bs, &a.B}) {
          if (*st) (void)hipStreamDestroy(*st);
          *st = nullptr;
        }
        (void)hipStreamCreateWithFlags(&a.shift, hipStreamNonBlocking);
        const int rc2 = aux_create(a, dev);
        if (rc2) { a.init_rc = rc2; return rc2; }
        a.recreated = 1;
        measure(a.check_us);
      }
    }
    if (kGpkExp && GPK_TUNE(STREAM_SELFTEST, 0)) {
      double pm = 0;
      (void)handoff_us(a.P, a.B, &pm);
      hipStream_t trio[3] = {a.P, a.X, a.Bs};
      double cu[3] = {0, 0, 0};
      (void)concurrent_us(trio, 3, cu);
      fprintf(stderr, "[gpk] stream hand-off us: P<->X %.1f  P<->Bs %.1f  X<->Bs %.1f  P<->B(masked) %.1f (first layout %.1f %.1f %.1f, recreated %d) | concurrent noop us/kernel: P %.1f X %.1f Bs %.1f\n",
              a.check_us[0], a.check_us[1], a.check_us[2], pm, a.check_first_us[0], a.check_first_us[1], a.check_first_us[2], a.recreated, cu[0], cu[1], cu[2]);
    }
    a.ready = true;
  }
  if (!a.flags) {
    GPK_HIP(hipMalloc((void**)&a.flags, sizeof(int) * 2 * kMaxFlagPanels));   // F, R
    GPK_HIP(hipMemset(a.flags, 0, sizeof(int) * 2 * kMaxFlagPanels));
    // in-kernel hand-offs need kernels of two streams to RUN concurrently: under rocprofv3 --pmc (or any tool that serialises
    // kernels) they would deadlock, so the chain then keeps its events (gpk_probe_concurrent_kernels: <= 2 ms, once per device)
    int conc = 0;
    const int rcp = gpk_probe_concurrent_kernels(a.X, a.P, a.flags, &conc);
    a.concurrent = (rcp == 0 && conc) ? 1 : 0;
  }
  *out = &a;
  return 0;
}

// grow the event pool to `need` (caller holds a.mu)
int aux_reserve_events(Aux& a, int need) {
  if (a.nev >= need) return 0;
  hipEvent_t* n = (hipEvent_t*)realloc(a.ev, sizeof(hipEvent_t) * need);
  if (!n) return GPK_E_ARG;
  a.ev = n;
  // The events only order streams of ONE device against each other (never inspected from the host), so they carry no
  // system-scope fence: the producing kernels' own release at the end of their dispatch makes the data visible to the
  // device.  Round 3, same box: chain of n = 2048 alone 0.98 -> 0.925 ms, SVGP step 2.085 -> 2.063 ms, GPR N = 16384
  // 32.75 -> 32.45 ms, the 1024-row rank shard 1.447 -> 1.388 ms, all bit-identical (profiles/r03_ab_svgp_schedules.log).
  // (Round 1 had measured this flag slower on a different schedule: 283 vs 308 steps/s.)
  for (int i = a.nev; i < need; ++i) {
    GPK_HIP(hipEventCreateWithFlags(&a.ev[i], hipEventDisableTiming | (GPK_TUNE(EV_NOFENCE, 1) ? hipEventDisableSystemFence : 0)));
    a.nev = i + 1;
  }
  return 0;
}

int current_device(int* dev) {
  GPK_HIP(hipGetDevice(dev));
  if (*dev < 0 || *dev >= 16) return GPK_E_UNSUPPORTED;
  return 0;
}

// factor the outer panel [c0,c1) of the square part (rows up to `rows`) on stream s
int factor_panel(hipStream_t s, double* A, int rows, int c0, int c1, long lda, int batch, long strideA,
                 double* invd, long strideInv, int* info, int chain_wgs = 0) {
  int rc;
  for (int j0 = c0; j0 < c1; j0 += NB) {
    const int j1 = (j0 + NB < c1) ? j0 + NB : c1;
    const int nb = j1 - j0;
    double* invb = invd + (long)(j0 / NB) * NB * NB;
    rc = gpk_launch_leaf(s, A + (long)j0 * lda + j0, lda, strideA, nb, invb, strideInv, info, j0, batch, 0);
    if (rc) return rc;
    const int below = rows - j1;
    if (below <= 0) continue;
    double* panel = A + (long)j1 * lda + j0;
    // in-place panel solve X = panel * inv(L11)^T: one column tile, so each workgroup only
    // overwrites rows that it alone has read
    GemmArgs g = gemm_base(below, nb, nb, 1.0, panel, lda, invb, NB, 0.0, panel, lda, batch, strideA,
                           strideInv, strideA);
    g.b_tri = 2;
    g.max_wgs = chain_wgs;
    rc = gpk_launch_gemm(s, g);
    if (rc) return rc;
    const int ncols = c1 - j1;
    if (ncols > 0) {
      GemmArgs u = gemm_base(below, ncols, nb, -1.0, panel, lda, panel, lda, 1.0,
                             A + (long)j1 * lda + j1, lda, batch, strideA, strideA, strideA);
      u.c_lower = 1;
      rc = gpk_launch_gemm(s, u);
      if (rc) return rc;
    }
  }
  return 0;
}

// Rows E [rows, n] against the finished columns [c0,c1) of the factor L (ldl), right-looking:
//   S[:,c0:c1] = E[:,c0:c1] L[c0:c1,c0:c1]^-T             (NB-blocked, diagonal-block inverses; after block j is solved
//                                                          ALL remaining columns of the group get one K = 128 update --
//                                                          the left-looking form was latency-bound at 44 / 58 / 74 us)
//   E[:,c1:n] -= S[:,c0:c1] L[c1:n,c0:c1]^T                (one large GEMM, K = c1 - c0)
// The solved columns S are written to Eo (ldeo) -- the same matrix as E for the in-place form, a separate one when the
// caller wants A^T apart from the consumed input rows.  Used for the extra rows of the factorisation and, group after
// group, by gpk_trsm(trans = 0).
// part_j0 >= 0 (progressive form, first group of an SVGP-size factorisation): only leaf block part_j0 of the group is solved by
// this call -- it has just been factored -- and the group's later blocks get its K = 128 update; the large GEMM follows the LAST block.
bool group_solve_fused_ok(int nbk, int c0, int c1, int rows, const double* L, long ldl, const double* invd, int batch, long strideL,
                          long strideInv) {
  const bool batch_ok = batch <= 1 || (GPK_TUNE(GROUP_FUSED_BATCH, 1) && !(strideL & 1) && !(strideInv & 1));
  return batch_ok && nbk >= 2 && nbk <= 4 && nbk * NB == c1 - c0 && (c0 % NB) == 0 && rows >= GPK_TUNE(GROUP_FUSED_MIN_ROWS, 1024) &&
         !(ldl & 1) && !(reinterpret_cast<uintptr_t>(L + (long)c0 * ldl + c0) & 15) &&
         !(reinterpret_cast<uintptr_t>(invd + (long)(c0 / NB) * NB * NB) & 15) && GPK_TUNE(GROUP_FUSED, 1);
}

int solve_group_fwd(hipStream_t s, const PotrfBulk& bulk, double* E, long lde, double* Eo, long ldeo, int rows, const double* L,
                    long ldl, const double* invd, long strideInv, int n, int c0, int c1, int batch, long strideE,
                    long strideEo, long strideL, int part_j0 = -1, int part_cap = 0) {
  int rc;
  const int nbk = (c1 - c0) / NB;
  if (part_j0 >= 0) {
    rc = gpk_launch_group_solve(s, E + c0, lde, Eo + c0, ldeo, rows, L + (long)c0 * ldl + c0, ldl, invd + (long)(c0 / NB) * NB * NB,
                                nbk, batch, strideE, strideEo, strideL, strideInv, part_cap, part_j0, part_j0 + 1);
    if (rc) return rc;
    if (part_j0 + 1 < nbk) return 0;
  } else
  // (a batch of problems: blockIdx.y walks them; C5 with separate kernels 2.14 -> 2.07 ms against the tiled per-block launches)
  if (group_solve_fused_ok(nbk, c0, c1, rows, L, ldl, invd, batch, strideL, strideInv)) {
    // (the fused kernel stages its operand tiles by 16-byte LDS-DMA: an 8-byte-aligned factor takes the per-block loop below)
    // the whole in-group phase (nbk solves + nbk - 1 updates of the latency kernel) as ONE launch with the same arithmetic
    rc = gpk_launch_group_solve(s, E + c0, lde, Eo + c0, ldeo, rows, L + (long)c0 * ldl + c0, ldl, invd + (long)(c0 / NB) * NB * NB,
                                nbk, batch, strideE, strideEo, strideL, strideInv, bulk.group_cap);
    if (rc) return rc;
  } else {
    for (int j0 = c0; j0 < c1; j0 += NB) {
      const int j1 = (j0 + NB < c1) ? j0 + NB : c1;
      const int nb = j1 - j0;
      GemmArgs g = gemm_base(rows, nb, nb, 1.0, E + j0, lde, invd + (long)(j0 / NB) * NB * NB, NB, 0.0,
                             Eo + j0, ldeo, batch, strideE, strideInv, strideEo);
      g.b_tri = 2;
      bulk.apply(g);
      rc = gpk_launch_gemm(s, g);
      if (rc) return rc;
      if (j1 < c1) {
        GemmArgs u = gemm_base(rows, c1 - j1, nb, -1.0, Eo + j0, ldeo, L + (long)j1 * ldl + j0, ldl, 1.0,
                               E + j1, lde, batch, strideEo, strideL, strideE);
        bulk.apply(u);
        // K = 128 updates inside a group: the one-shot latency kernel with its workgroups walking the row blocks (B tile
        // staged once) instead of the tiled kernel, which runs K = 128 at 16-24 TFLOP/s (33-45 us per launch at 8192 rows).
        // Same-box A/B: SVGP step 2.251 -> 2.222 ms, GPR predict 56.5 -> 56.0 ms, cached posterior 20.9 -> 20.7 ms
        // (512 workgroups; 256: 2.238, 768: 2.246).
        if (GPK_TUNE(XSMALL, 1) && batch <= 1) {
          u.small_loop = 1;
          u.max_wgs = GPK_TUNE(XSMALL_WGS, 512);
        }
        rc = gpk_launch_gemm(s, u);
        if (rc) return rc;
      }
    }
  }
  if (c1 < n) {
    GemmArgs u = gemm_base(rows, n - c1, c1 - c0, -1.0, Eo + c0, ldeo, L + (long)c1 * ldl + c0, ldl, 1.0,
                           E + c1, lde, batch, strideEo, strideL, strideE);
    // (round 6, late: this update on the CU-masked stream B with TWO persistent workgroups per compute unit of its mask -- K loop at 88 %
    //  instead of 79 %, the 32 CUs outside the mask free for the chain, hand-over by events -- makes every SVGP workload 10 - 20 % SLOWER:
    //  Cm 1.94 - 1.96 against 1.75 - 1.79 ms, profiles/r06_ab_xbulk_masked.log.  A third active hardware queue, as in rounds 2 - 3.)
    bulk.apply(u);
    rc = gpk_launch_gemm(s, u);
    if (rc) return rc;
  }
  return 0;
}

// The mirror image for  B <- B L^-1  with LT = L^T (upper, row-major) and the transposed block inverses: columns
// [c0,c1) are solved from the last block to the first, then ONE K = c1 - c0 update of all columns to their left.
int solve_group_bwd(hipStream_t s, double* Bm, long ldb, int rows, const double* LT, long ldl, const double* invdT,
                    long strideInv, int c0, int c1, int batch, long strideB, long strideL) {
  int rc;
  for (int j1 = c1; j1 > c0;) {
    const int j0 = (j1 - c0 > NB) ? c0 + ((j1 - c0 - 1) / NB) * NB : c0;
    const int nb = j1 - j0;
    GemmArgs g = gemm_base(rows, nb, nb, 1.0, Bm + j0, ldb, invdT + (long)(j0 / NB) * NB * NB, NB, 0.0, Bm + j0,
                           ldb, batch, strideB, strideInv, strideB);
    g.b_tri = 1;
    rc = gpk_launch_gemm(s, g);
    if (rc) return rc;
    if (j0 > c0) {  // B[:, c0:j0] -= X[:, j0:j1] (LT[c0:j0, j0:j1])^T
      GemmArgs u = gemm_base(rows, j0 - c0, nb, -1.0, Bm + j0, ldb, LT + (long)c0 * ldl + j0, ldl, 1.0, Bm + c0,
                             ldb, batch, strideB, strideL, strideB);
      rc = gpk_launch_gemm(s, u);
      if (rc) return rc;
    }
    j1 = j0;
  }
  if (c0 > 0) {  // B[:, 0:c0] -= X[:, c0:c1] (LT[0:c0, c0:c1])^T
    GemmArgs u = gemm_base(rows, c0, c1 - c0, -1.0, Bm + c0, ldb, LT + c0, ldl, 1.0, Bm, ldb, batch, strideB,
                           strideL, strideB);
    rc = gpk_launch_gemm(s, u);
    if (rc) return rc;
  }
  return 0;
}
}  // namespace

// ---- how the streams of one factorisation hand over to each other -------------------------------------------------------------
// Chain flags (round 5).  Between two kernels of the panel stream an event record costs 4.6 us and an event wait 6.3 us of
// queue-packet processing (rocprofv3 timelines, profiles/r05_rows1024_events_timeline.txt, r05_ab_chain_flags.log); two kernels back to back start
// 0.3 us apart.  Single-leaf panels (the SVGP sizes and the narrow tail of a large factorisation: leaf -> solve -> strip,
// 16 - 32 times per factorisation) therefore hand over WITHOUT packets on this stream:
//   "panel p solved"     the strip kernel stores the epoch into F[p] on entry (its predecessor, the solve, has completed
//                        and released); the rest-update and extra-row streams wait for it with hipStreamWaitValue32;
//   "rest-update done"   hipStreamWriteValue32(R[p]) behind the rest-update on ITS stream; the next strip's workgroups
//                        spin on it in-kernel (normally already there: the rest-update has a leaf's time of slack).
// (stream memory operations only on the plain streams: on the CU-masked bulk stream of large factorisations a
// hipStreamWriteValue32 was observed to overtake the kernel queued before it -- wrong factor at n = 5000 -- so a panel whose
// extra-row group waits on that stream keeps its event, and so does a strip whose rest-update ran there: PotrfPanel::flag_candidate
// and rest_flag, potrf_plan.h)
// WHICH hand-off is a flag word is the plan's decision (AND what the operands allow); this struct issues it and remembers what the
// next hand-off needs to know.  One per call of gpk_potrf_core, on its stack.
namespace {
struct ChainSync {
  hipStream_t P;
  hipEvent_t* evF;   // [npanels] panel p factored, rows below solved (recorded on P)
  hipEvent_t* evR;   // [npanels] rest of the trailing update of panel p done (on B)
  hipEvent_t evFork, evJoinP, evJoinB, evJoinX;
  int* flagF;        // [kMaxFlagPanels] "panel p solved", written with the epoch of the factorisation that owns it
  int* flagR;        // [kMaxFlagPanels] "rest-update p done"
  int epoch;
  int* info;         // the status word: receives INT_MAX if a bounded in-kernel wait expires
  bool gate_kernels;
  // (A/B build only, GPK_FAULT_DROP_REST_FLAG=p: the "rest-update p done" word is never written -- the next strip's bounded
  //  in-kernel wait must expire, the status word become INT_MAX and the call return instead of hanging: tests/test_gpu_handoff.py)
  int drop_rest_flag;
  bool panel_flagged = false;   // the panel solved most recently announces itself by F[p], not by evF[p]
  bool rest_flagged = false;    // the most recent rest-update was followed by a write of R[last_rest]
  bool evr_recorded = false;
  int last_rest = -1;           // panel index whose evR marks the most recent rest-update
  hipStream_t last_bulk;        // ... and the stream it ran on

  ChainSync(Aux& aux, const PotrfPlan& plan, hipStream_t B, int* info_)
      : P(aux.P), evF(aux.ev), evR(aux.ev + plan.npanels()), evFork(aux.ev[2 * plan.npanels()]), evJoinP(aux.ev[2 * plan.npanels() + 1]),
        evJoinB(aux.ev[2 * plan.npanels() + 2]), evJoinX(aux.ev[2 * plan.npanels() + 3]), flagF(aux.flags),
        flagR(aux.flags + kMaxFlagPanels), epoch(++aux.epoch), info(info_), gate_kernels(plan.gate_kernels),
        drop_rest_flag(kGpkExp ? GPK_TUNE(FAULT_DROP_REST_FLAG, -1) : -1), last_bulk(B) {}

  // fork: everything already queued on S comes first (X = nullptr: no extra-row stream of its own)
  int fork(hipStream_t S, hipStream_t B, hipStream_t X) {
    GPK_HIP(hipEventRecord(evFork, S));
    GPK_HIP(hipStreamWaitEvent(P, evFork, 0));
    if (B != S) GPK_HIP(hipStreamWaitEvent(B, evFork, 0));
    if (X) GPK_HIP(hipStreamWaitEvent(X, evFork, 0));
    return 0;
  }

  // Panel p is solved on P; `strip` (the look-ahead update, launched next on P) announces it on entry if the panel is flagged,
  // else the event is recorded here.  (What the other streams wait for: the flag word of a flagged panel, else the event.)
  int panel_solved(int p, bool flagged, GemmArgs& strip) {
    panel_flagged = flagged;
    if (flagged) {
      strip.sig_ptr = flagF + p;
      strip.sig_val = epoch;
    } else GPK_HIP(hipEventRecord(evF[p], P));
    return 0;
  }

  // columns c1:c2 also received the most recent rest-update (on a bulk stream): order the two -- the strip's workgroups wait for
  // R[last_rest] in-kernel, or P waits for the event
  int strip_waits_for_rest(GemmArgs& strip) {
    if (last_rest < 0) return 0;
    if (panel_flagged && rest_flagged) {
      strip.wait_ptr = flagR + last_rest;
      strip.wait_val = epoch;
      strip.wait_info = info;
      return 0;
    }
    GPK_TRY(need_evr());
    GPK_HIP(hipStreamWaitEvent(P, evR[last_rest], 0));
    return 0;
  }

  // stream st waits for "panel p solved" (p: the panel of the last panel_solved)
  // (a flagged panel: our own one-wave gate kernel, 0.3 us behind its predecessor, instead of the runtime's wait packet, 5 - 7 us;
  //  never on the CU-masked stream, whose stream memory operations were seen out of order -- see above)
  int wait_panel(hipStream_t st, int p) {
    if (panel_flagged) {
      if (gate_kernels) return gpk_launch_wait_flag(st, flagF + p, epoch, info);
      GPK_HIP(hipStreamWaitValue32(st, flagF + p, (uint32_t)epoch, hipStreamWaitValueGte, 0xffffffffu));
    } else GPK_HIP(hipStreamWaitEvent(st, evF[p], 0));
    return 0;
  }

  // the event of the most recent rest-update, recorded when first needed: its stream is in order, so a record issued later covers it
  int need_evr() {
    if (!evr_recorded && last_rest >= 0) {
      GPK_HIP(hipEventRecord(evR[last_rest], last_bulk));
      evr_recorded = true;
    }
    return 0;
  }

  // the most recent rest-update ran on st (or there was none): a rest-update on st needs no hand-off from it
  bool previous_rest_on(hipStream_t st) const { return last_rest < 0 || last_bulk == st; }
  // ... else st waits for it.  (Only where the narrow panels of a large factorisation take over from the wide ones: the rest-updates
  // change from the masked stream to Bs once, and never back -- wide panels come before narrow ones.)
  int order_rest_after_previous(hipStream_t st) {
    if (previous_rest_on(st)) return 0;
    GPK_TRY(need_evr());
    GPK_HIP(hipStreamWaitEvent(st, evR[last_rest], 0));
    return 0;
  }

  // How "rest-update p done" is announced: by the event (recorded now); by a write of R[p] behind the update on its stream (set-flag
  // kernel or stream write); or by the update's last kernel itself ON ENTRY (rest_flag_on_entry: the remainder of a split
  // rest-update, which follows the column the next strip needs).  A flagged rest-update gets its event only if somebody asks
  // for it: need_evr.
  enum RestSignal { kEvent, kFlagWrite, kFlagOnEntry };
  void rest_flag_on_entry(int p, GemmArgs& g) const {
    if (p == drop_rest_flag) return;
    g.sig_ptr = flagR + p;
    g.sig_val = epoch;
  }
  int rest_done(hipStream_t st, int p, RestSignal how) {
    rest_flagged = how != kEvent;
    evr_recorded = !rest_flagged;
    last_bulk = st;
    last_rest = p;
    if (how == kEvent) GPK_HIP(hipEventRecord(evR[p], st));
    if (how != kFlagWrite || p == drop_rest_flag) return 0;
    if (gate_kernels) return gpk_launch_set_flag(st, flagR + p, epoch);
    GPK_HIP(hipStreamWriteValue32(st, flagR + p, (uint32_t)epoch, 0));
    return 0;
  }

  // join: P has waited for every rest-update it depends on; B's last event covers the rest (X = nullptr: as fork)
  int join(hipStream_t S, hipStream_t X) {
    GPK_HIP(hipEventRecord(evJoinP, P));
    GPK_HIP(hipStreamWaitEvent(S, evJoinP, 0));
    if (last_bulk != S) {
      GPK_HIP(hipEventRecord(evJoinB, last_bulk));  // rest-updates are chained through evR, the last one covers all
      GPK_HIP(hipStreamWaitEvent(S, evJoinB, 0));
    }
    if (X && X != last_bulk) {
      GPK_HIP(hipEventRecord(evJoinX, X));
      GPK_HIP(hipStreamWaitEvent(S, evJoinX, 0));
    }
    return 0;
  }
};

// ---- one factorisation being enqueued: the plan, the operands, the streams -----------------------------------------------------
struct PotrfRun {
  const PotrfPlan& plan;
  ChainSync& sync;
  double* A; long lda; int batch; long strideA;
  double* invd; long strideInv;
  int* info;
  hipStream_t P, B_masked, Bs, X;   // X: the stream of the extra rows (plan.X)
  bool progressive;                 // plan.progressive_candidate AND what the operands allow
  double* E() const { return A + (long)plan.n * lda; }   // the extra rows
  hipStream_t rest_stream(const PotrfPanel& q) const { return q.rest_stream == PotrfStream::B_masked ? B_masked : Bs; }

  int enqueue_chain(int p);
  int enqueue_rest_update(int p);
  int enqueue_extra_rows(int p);
};

// ---- P: the critical path.  Panel p, then the strip = columns of panel p+1 (look-ahead) -----------
int PotrfRun::enqueue_chain(int p) {
  const PotrfPanel& q = plan.panels[p];
  const int c0 = q.c0, c1 = q.c1, c2 = q.c2, R = plan.R;
  GPK_TRY(factor_panel(P, A, R, c0, c1, lda, batch, strideA, invd, strideInv, info, plan.chain_wgs));
  const bool has_strip = c1 < plan.n;
  const double* Pn = A + (long)c1 * lda + c0;  // rows c1.. of the solved panel
  GemmArgs strip{};
  if (has_strip) {
    strip = gemm_base(R - c1, c2 - c1, c1 - c0, -1.0, Pn, lda, Pn, lda, 1.0, A + (long)c1 * lda + c1, lda, batch, strideA,
                      strideA, strideA);
    strip.c_lower = 1;
    strip.max_wgs = plan.chain_wgs;
  }
  // (operand-dependent, so not in the plan: only the one-shot latency kernel honours sig_ptr / wait_ptr, and whether the strip
  //  runs on it depends on gemm.hip's limits and the alignment of A)
  const bool flagged = q.flag_candidate && gpk_gemm_takes_latency_kernel(strip);
  GPK_TRY(sync.panel_solved(p, flagged, strip));
  if (!has_strip) return 0;
  GPK_TRY(sync.strip_waits_for_rest(strip));
  // A strip that waits in-kernel holds a compute unit per workgroup while it waits (150 KB of LDS each: nothing else fits beside one),
  // and it is the high-priority stream's.  With as many waiting workgroups as compute units -- 480 for four problems of M = 2048, 249
  // behind the first narrow panel of n = 4736 -- a rest-update that is late finds no compute unit, its word is never written and the
  // bounded wait expires: the status word at INT_MAX of NEXT.md section 5.  So the waiters of one launch stay within the compute units of
  // the bulk stream's mask (all but the 32 the chain keeps anyway) and walk their row blocks; launches below that are as before.
  // (tests/test_potrf_schedule.py, assertion 7)
  if (strip.wait_ptr && plan.bulk_cus > 0) {
    const int room = std::max(1, plan.bulk_cus / batch);
    if (strip.max_wgs <= 0 || strip.max_wgs > room) strip.max_wgs = room;
  }
  return gpk_launch_gemm(P, strip);
}

// ---- B: rest of the outer trailing update  A[c2:, c2:] -= P[c2:] P[c2:]^T, lower tiles only --------
// While the trailing matrix is large the factorisation is bound by these GEMMs (masked stream B); they start as soon
// as panel p is solved.  (Which regime -- tiled, 64 x 64 tiles, tile queue, walking workgroups -- and why: potrf_plan.h.)
int PotrfRun::enqueue_rest_update(int p) {
  const PotrfPanel& q = plan.panels[p];
  const int c0 = q.c0, c1 = q.c1, c2 = q.c2, c3 = q.c3, n = plan.n, R = plan.R;
  if (c2 >= n) return 0;
  hipStream_t Bp = rest_stream(q);
  const double* P2 = A + (long)c2 * lda + c0;
  GemmArgs u = gemm_base(R - c2, n - c2, c1 - c0, -1.0, P2, lda, P2, lda, 1.0,
                         A + (long)c2 * lda + c2, lda, batch, strideA, strideA, strideA);
  u.c_lower = 1;
  if (q.rest_tile64_candidate) {
    u.no_small = 1;
    u.tile64 = plan.rest_tile64;
  }
  else if (q.rest_small_loop) { u.small_loop = 1; u.max_wgs = plan.rest_small_wgs; }
  if (q.rest_tile_queue) {
    u.stagger_first = plan.bulk_cus;
    u.tile_queue = plan.trail_queue;
  }
  // Split rest-update (round 6).  With the 25-us leaf the chain of a single-leaf panel is leaf 25 + solve 7 + strip 8 = 40 us,
  // and the rest-update stream had become the longer one: wait packet 6 + one 30-us tiled launch + write packet 7 + the
  // in-kernel wait of the next strip = 45 us per panel (profiles/r06_rows1024_new_leaf_timeline.txt).  The next strip only
  // needs the NEXT block column of the rest-update, so that column goes first, on the one-shot latency kernel (~8 us, beside
  // strip p) behind a gate on "panel p solved"; the remainder follows on the same stream and announces the
  // column on ITS entry (GemmArgs::sig_ptr) -- no packet in between, and the remainder has a whole panel period of slack.
  // ("waiting for panel p solved": the one-wave gate kernel of wait_panel.)
  GemmArgs ua = gemm_base(R - c2, c3 - c2, c1 - c0, -1.0, P2, lda, P2, lda, 1.0, A + (long)c2 * lda + c2, lda, batch, strideA,
                          strideA, strideA);
  ua.c_lower = 1;
  // (operand-dependent, so not in the plan: the first column must run on the one-shot latency kernel -- gemm.hip's limits, the
  //  alignment of A; the panel must really have been flagged; and the previous rest-update must have run on this stream)
  const bool split = q.rest_split_candidate && sync.panel_flagged && gpk_gemm_takes_latency_kernel(ua) && sync.previous_rest_on(Bp);
  // (the gate, not an in-kernel wait: up to 120 workgroups of 150 KB spinning from the moment they are enqueued -- a leaf and
  //  a solve before their flag -- would hold the compute units the chain and the extra-row stream need)
  GPK_TRY(sync.wait_panel(Bp, p));
  if (!split) {
    GPK_TRY(sync.order_rest_after_previous(Bp));
    GPK_TRY(gpk_launch_gemm(Bp, u));
    return sync.rest_done(Bp, p, q.rest_flag ? ChainSync::kFlagWrite : ChainSync::kEvent);
  }
  GPK_TRY(gpk_launch_gemm(Bp, ua));
  if (c3 >= n) return sync.rest_done(Bp, p, ChainSync::kFlagWrite);
  const double* P3 = A + (long)c3 * lda + c0;
  GemmArgs ub = gemm_base(R - c3, n - c3, c1 - c0, -1.0, P3, lda, P3, lda, 1.0, A + (long)c3 * lda + c3, lda, batch,
                          strideA, strideA, strideA);
  ub.c_lower = 1;
  ub.no_small = u.no_small;
  ub.tile64 = u.tile64;
  sync.rest_flag_on_entry(p, ub);
  GPK_TRY(gpk_launch_gemm(Bp, ub));
  return sync.rest_done(Bp, p, ChainSync::kFlagOnEntry);
}

// ---- X: the extra rows against the finished columns, in groups of up to 512 columns (so that the big
// right-looking update is a K = 512 GEMM).  Where the groups end, the shrinking groups at the end of the small sizes and the
// progressive first group: potrf_plan.h, plan_extra_rows.
int PotrfRun::enqueue_extra_rows(int p) {
  const PotrfPanel& q = plan.panels[p];
  const int n = plan.n, extra = plan.extra, tri = plan.tri;
  if (progressive && q.x_progressive_block >= 0) {
    GPK_TRY(sync.wait_panel(X, p));
    const int xrows = tri ? extra - tri + plan.prog_end : extra;
    return solve_group_fwd(X, plan.bulk, E(), lda, E(), lda, xrows, A, lda, invd, strideInv, n, 0, plan.prog_end, batch, strideA, strideA,
                           strideA, q.x_progressive_block, plan.prog_cap);
  }
  if (!q.x_group_end) return 0;
  GPK_TRY(sync.wait_panel(X, p));
  // (columns [g0, c1) may span several 512-groups when the outer panel is wider than a group)
  for (int h0 = q.x_group_begin; h0 < q.c1; h0 += NBO) {
    const int h1 = std::min(h0 + NBO, q.c1);
    const int xrows = tri ? extra - tri + h1 : extra;  // (identity rows below column h1 are still exactly zero here)
    GPK_TRY(solve_group_fwd(X, plan.bulk, E(), lda, E(), lda, xrows, A, lda, invd, strideInv, n, h0, h1, batch, strideA, strideA,
                            strideA));
  }
  return 0;
}

// n <= NB: one leaf on the caller's stream; nothing to overlap, no device state
int potrf_single_leaf(hipStream_t S, const PotrfPlan& plan, double* A, long lda, int batch, long strideA, double* invd, long strideInv,
                      int zero_upper, int* info, const PotrfHooks& hooks) {
  const int n = plan.n;
  for (const StreamWork* w : {&hooks.p_prologue, &hooks.x_prologue, &hooks.late_work}) {
    if (*w) GPK_TRY((*w)(S));
  }
  GPK_TRY(factor_panel(S, A, plan.R, 0, n, lda, batch, strideA, invd, strideInv, info));
  if (plan.useX) {
    double* E = A + (long)n * lda;
    GPK_TRY(solve_group_fwd(S, PotrfBulk{}, E, lda, E, lda, plan.extra, A, lda, invd, strideInv, n, 0, n, batch, strideA, strideA, strideA));
  }
  return zero_upper ? gpk_launch_zero_upper(S, A, n, lda, batch, strideA) : 0;
}
}  // namespace

// (the hooks, tri and tri_prefilled: gpk_internal.h)
int gpk_potrf_core(hipStream_t S, double* A, int n, int extra, long lda, int batch, long strideA, double* invd, int zero_upper,
                   int* info, const PotrfHooks& hooks, int tri, bool tri_prefilled) {
  if (!A || !invd || n < 0 || extra < 0 || lda < n) return GPK_E_ARG;
  if (tri && (tri != n || extra < n || batch > 1)) return GPK_E_ARG;
  if (batch <= 0) batch = 1;
  // (the status word is reset by the leaf of column 0 -- leaf2_device.h -- not by a memset packet ahead of the fork below)
  if (n == 0) {
    if (info) GPK_HIP(hipMemsetAsync(info, 0, sizeof(int) * batch, S));
    return 0;
  }
  if (tri && !tri_prefilled) GPK_TRY(gpk_launch_set_identity(S, A + (long)(n + extra - tri) * lda, n, lda));
  const long strideInv = (long)gpk_cdiv(n, NB) * NB * NB;
  // the per-device streams, events and flag words (held to the end of the enqueue); a single leaf needs none of them
  Aux* aux = nullptr;
  std::unique_lock<std::recursive_mutex> lock;
  if (n > NB) {
    int dev = 0;
    GPK_TRY(current_device(&dev));
    lock = std::unique_lock<std::recursive_mutex>(g_aux[dev].mu);
    GPK_TRY(aux_get(dev, &aux));
  }
  PotrfPlan plan = make_potrf_plan(PotrfShape{n, extra, batch, tri},
                                   aux ? PotrfDevice{aux->bulk_cus, aux->flags != nullptr && aux->concurrent == 1} : PotrfDevice{0, false});
  if (plan.single_leaf) return potrf_single_leaf(S, plan, A, lda, batch, strideA, invd, strideInv, zero_upper, info, hooks);
  GPK_TRY(aux_reserve_events(*aux, plan.nevents));
  // (operand-dependent, so not in the plan: the progressive first group needs the partial in-group solve of gemm.hip and operands the
  //  fused in-group kernel takes -- 16-byte-aligned factor and block inverses, even lda)
  const bool progressive = plan.progressive_candidate && gpk_group_solve_takes_parts() &&
                           group_solve_fused_ok(plan.prog_end / NB, 0, plan.prog_end, tri ? extra - tri + plan.prog_end : extra, A, lda, invd,
                                                batch, strideA, strideInv);
  if (plan.progressive_candidate && !progressive) plan.plan_extra_rows(false);
  hipStream_t B = plan.large ? aux->B : aux->Bs;
  hipStream_t X = plan.large ? aux->B : aux->X;
  hipStream_t Xown = (plan.useX && X != B) ? X : nullptr;   // the extra rows have a stream of their own to fork and join

  const bool p_on_panel = hooks.p_prologue && GPK_TUNE(KUU_ON_PANEL, 1);
  if (hooks.p_prologue && !p_on_panel) GPK_TRY(hooks.p_prologue(S));
  // the extra rows ride through the panel solves: they must exist before the first one
  if (hooks.x_prologue && !plan.useX) GPK_TRY(hooks.x_prologue(S));
  ChainSync sync(*aux, plan, B, info);
  PotrfRun run{plan, sync, A, lda, batch, strideA, invd, strideInv, info, aux->P, aux->B, aux->Bs, X, progressive};
  GPK_TRY(sync.fork(S, B, Xown));
  if (p_on_panel) GPK_TRY(hooks.p_prologue(aux->P));
  for (int p = 0; p < plan.npanels(); ++p) {
    GPK_TRY(run.enqueue_chain(p));
    GPK_TRY(run.enqueue_rest_update(p));
    if (p == 0 && hooks.x_prologue && plan.useX) GPK_TRY(hooks.x_prologue(X));
    // (on the stream of the most recent rest-update, whose last event the join below waits for)
    if (hooks.late_work && p == plan.late_panel) GPK_TRY(hooks.late_work(sync.last_bulk));
    GPK_TRY(run.enqueue_extra_rows(p));
  }
  GPK_TRY(sync.join(S, plan.useX ? X : nullptr));
  return zero_upper ? gpk_launch_zero_upper(S, A, n, lda, batch, strideA) : 0;
}

extern "C" int gpk_stream_selfcheck(double* us_now, double* us_first, int* recreated) {
  int dev = 0;
  const int rc = current_device(&dev);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lock(g_aux[dev].mu);
  const Aux& a = g_aux[dev];
  if (!a.ready) return GPK_E_UNSUPPORTED;   // no factorisation with n > 128 has been issued on this device yet
  for (int i = 0; i < 3; ++i) {
    if (us_now) us_now[i] = a.check_us[i];
    if (us_first) us_first[i] = a.check_first_us[i];
  }
  if (recreated) *recreated = a.recreated;
  return 0;
}

extern "C" int gpk_chain_handoff_mode(void) {
  int dev = 0;
  if (current_device(&dev)) return -1;
  std::lock_guard<std::recursive_mutex> lock(g_aux[dev].mu);
  const Aux& a = g_aux[dev];
  if (!a.ready || a.concurrent < 0) return -1;
  if (!(GPK_TUNE(CHAIN_FLAGS, 1) && a.concurrent == 1)) return 0;
  return GPK_TUNE(GATE_KERNELS, 1) ? 2 : 1;
}

extern "C" int gpk_potrf(void* stream, double* A, int n, int extra, long lda, int batch,
                         long strideA, double* invd, int zero_upper, int* info) {
  if (!invd_aligned(invd)) return GPK_E_ARG;
  return gpk_potrf_core((hipStream_t)stream, A, n, extra, lda, batch, strideA, invd, zero_upper, info);
}

extern "C" int gpk_potrf_inv(void* stream, double* A, int n, int extra, long lda, double* invd, int zero_upper,
                             int* info) {
  if (!invd_aligned(invd)) return GPK_E_ARG;
  return gpk_potrf_core((hipStream_t)stream, A, n, extra + n, lda, 1, 0, invd, zero_upper, info, PotrfHooks(), n);
}

extern "C" int gpk_trtri_blocks(void* stream, const double* L, int n, long ldl, int batch,
                                long strideL, double* invd) {
  if (!L || !invd || n < 0 || !invd_aligned(invd)) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (batch <= 0) batch = 1;
  const int nblk = gpk_cdiv(n, NB);
  const long strideInv = (long)nblk * NB * NB;
  const int nfull = n / NB;
  for (int b = 0; b < batch; ++b) {
    double* Lb = const_cast<double*>(L) + (long)b * strideL;  // FACTORED leaf never writes A
    double* ib = invd + (long)b * strideInv;
    if (nfull > 0) {
      int rc = gpk_launch_leaf(s, Lb, ldl, (long)NB * (ldl + 1), NB, ib, (long)NB * NB, nullptr, 0,
                               nfull, 1);
      if (rc) return rc;
    }
    if (nfull < nblk) {
      const int j0 = nfull * NB;
      int rc = gpk_launch_leaf(s, Lb + (long)j0 * (ldl + 1), ldl, 0, n - j0, ib + (long)nfull * NB * NB,
                               0, nullptr, 0, 1, 1);
      if (rc) return rc;
    }
  }
  return 0;
}

// trans = 0:  B <- B L^-T  with (L, invd);   trans = 1:  B <- B L^-1 with (LT = L^T, invdT).
// Right-looking in column groups of 512: inside a group the 128-blocks are solved with their explicit inverses and
// each is followed by one K = 128 update of the rest of the group; then ONE K = 512 GEMM updates every column still
// to be solved.  (The left-looking form -- for every 128 columns a GEMM with 32 output tiles per 4096 rows and K up to
// n -- ran the N = 16384, T = 4096 predict solve at 7 TFLOP/s.)
extern "C" int gpk_trsm(void* stream, int trans, const double* L, long ldl, const double* invd,
                        int n, double* B, int m, long ldb, int batch, long strideL, long strideB) {
  if (n < 0 || m < 0 || !invd_aligned(invd)) return GPK_E_ARG;
  if (n == 0 || m == 0) return 0;
  if (!L || !invd || !B) return GPK_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (batch <= 0) batch = 1;
  const long strideInv = (long)gpk_cdiv(n, NB) * NB * NB;
  int rc;
  if (trans == 0) {
    for (int g0 = 0; g0 < n; g0 += NBO) {
      rc = solve_group_fwd(s, PotrfBulk{}, B, ldb, B, ldb, m, L, ldl, invd, strideInv, n, g0, std::min(g0 + NBO, n), batch,
                           strideB, strideB, strideL);
      if (rc) return rc;
    }
  } else {
    const int ng = gpk_cdiv(n, NBO);
    for (int g = ng - 1; g >= 0; --g) {
      rc = solve_group_bwd(s, B, ldb, m, L, ldl, invd, strideInv, g * NBO, std::min((g + 1) * NBO, n), batch, strideB,
                           strideL);
      if (rc) return rc;
    }
  }
  return 0;
}

extern "C" int gpk_transpose_factor(void* stream, const double* L, long ldl, const double* invd,
                                    int n, double* LT, long ldlt, double* invdT) {
  if (!L || !invd || !LT || !invdT || n < 0 || !invd_aligned(invd) || !invd_aligned(invdT)) return GPK_E_ARG;
  if (n == 0) return 0;
  int rc = gpk_transpose(stream, L, n, n, ldl, LT, ldlt, 1, 1, 0, 0);
  if (rc) return rc;
  const int nblk = gpk_cdiv(n, NB);
  return gpk_transpose(stream, invd, NB, NB, NB, invdT, NB, 0, nblk, (long)NB * NB, (long)NB * NB);
}
