// The schedule of the trapezoidal Cholesky (potrf.hip, gpk_potrf_core) as DATA: everything the scheduler decides from the shape
// (n, extra, batch, tri) and two device facts, before a single HIP call is made.  Plain C++17 and no HIP header, so the plan can be
// printed and tested on a machine without a GPU (tests/test_potrf_plan.py, tests/potrf_plan_dump.cpp).  potrf.hip enqueues what the
// plan says; a change of the SCHEDULE -- panel cuts, group widths, which kernel regime, which stream -- is a change to this file.
//
// What is NOT here, because it depends on the operands (pointer alignment, parity of lda) or on gemm.hip's own limits:
// gpk_gemm_takes_latency_kernel(strip / ua) and group_solve_fused_ok(...).  potrf.hip evaluates them at enqueue time and ANDs them
// with the `*_candidate` fields below.
#pragma once
#include <algorithm>
#include <vector>
#include "../../include/gpk.h"   // GPK_NB
#include "gpk_tune.h"

constexpr int kPotrfNB = GPK_NB;
constexpr int kPotrfNBO = 512;          // column group of the right-looking row solves (extra rows, gpk_trsm)
constexpr int kMaxFlagPanels = 512;     // hand-off words per kind (F, R): panels beyond keep their events

struct PotrfShape {
  int n, extra, batch, tri;
};
// what the plan needs from the per-device state (potrf.hip, Aux)
struct PotrfDevice {
  int bulk_cus;        // compute units inside the mask of the bulk stream
  bool flags_usable;   // the hand-off words exist and kernels of two streams were seen running concurrently
};

// the internal streams by role (potrf.hip, "per-device internal state"); the panel stream P is implied
enum class PotrfStream : unsigned char { B_masked, Bs, X };

// how a bulk GEMM beside the latency chain is launched
struct PotrfBulk {
  int cap = 0;         // cap on the persistent workgroups of the big (K >= 256) updates, 0 = one workgroup per tile
  int group_cap = 0;   // cap on the workgroups of the fused in-group solve, 0 = one per 16-row sliver
  int kmin = 256;      // updates with K below this are not capped
  template <class Gemm>
  void apply(Gemm& g) const {
    if (cap > 0 && g.k >= kmin) g.max_wgs = cap;
  }
};

struct PotrfPanel {
  int c0, c1, c2, c3;           // columns [c0, c1) of this panel; c2, c3: ends of the next two (n beyond the last)
  bool narrow;                  // single-leaf panel in the chain-bound end of a large factorisation
  // ---- extra rows (useX) ----
  bool x_group_end;             // the extra-row group [x_group_begin, c1) is solved behind this panel (progressive: its last block)
  int x_group_begin;
  int x_progressive_block;      // >= 0: this panel's leaf block of the progressive first group is solved behind it; else -1
  bool tail_zone;               // ... and that group is one of the two shrinking single-block groups at the end
  // ---- chain hand-off ----
  bool flag_candidate;          // "panel solved" may be a flag word instead of an event (AND gpk_gemm_takes_latency_kernel(strip))
  // ---- rest-update  A[c2:, c2:] -= P[c2:] P[c2:]^T  (only when c2 < n) ----
  PotrfStream rest_stream;
  bool rest_tile_queue;         // on the masked stream: staggered start and persistent workgroups on the tile queue
  bool rest_tile64_candidate;   // tiled regime: never the latency kernel, 64 x 64 tiles of the generic one (PotrfPlan::rest_tile64)
  bool rest_small_loop;         // latency kernel with rest_small_wgs walking workgroups
  bool rest_flag;               // "rest-update done" is a flag word (when the update is not split), else an event
  bool rest_split_candidate;    // next block column first (AND panel flagged, gpk_gemm_takes_latency_kernel(ua), same stream as before)
};

struct PotrfPlan {
  // ---- whole call ----
  int n = 0, extra = 0, batch = 1, tri = 0;
  bool single_leaf = false;     // n <= NB: one leaf on the caller's stream, nothing to overlap
  bool large = false;           // n >= 4096: wide outer panels, masked bulk stream
  int nbo = kPotrfNB;           // outer panel width
  bool ride = false;            // the extra rows ride through the panel solves and trailing updates
  bool useX = false;            // ... or are solved right-looking, group by group, beside the chain
  int R = 0;                    // rows handled together with the square part
  PotrfStream B = PotrfStream::Bs, X = PotrfStream::X;
  PotrfBulk bulk;
  int chain_wgs = 0;
  int xgroup = kPotrfNBO, xgroup_first = kPotrfNBO;
  bool tail_zone = false;       // the extra-row groups shrink towards the end (.., n-256, n-128, n)
  bool rest_tiled = false;
  int rest_tiled_min_wgs = 0, rest_small_wgs = 0, rest_tile64 = 0, trail_queue = 0, bulk_cus = 0;
  bool progressive_candidate = false;   // AND gpk_group_solve_takes_parts() and group_solve_fused_ok(first group)
  int prog_end = 0, prog_cap = 0;
  int late_panel = 0;
  bool use_flags = false, gate_kernels = false;
  bool rest_split_enabled = false;
  int nevents = 0;              // events the call needs: F and R per panel, fork, three joins (+ spare)
  // ---- per panel ----
  std::vector<PotrfPanel> panels;
  int npanels() const { return (int)panels.size(); }

  // The extra-row fields of the panels (x_group_end, x_group_begin, x_progressive_block, tail_zone).  `progressive` = the first
  // group is solved block by block behind its panels.  make_potrf_plan calls this with progressive_candidate; potrf.hip calls it
  // again with false when the operands rule the progressive form out.
  void plan_extra_rows(bool progressive);
};

inline void PotrfPlan::plan_extra_rows(bool progressive) {
  constexpr int NB = kPotrfNB;
  int xg0 = 0;   // first column of the current extra-row group
  for (int p = 0; p < npanels(); ++p) {
    PotrfPanel& q = panels[p];
    const int c1 = q.c1;
    q.x_group_end = false;
    q.x_group_begin = xg0;
    q.x_progressive_block = -1;
    q.tail_zone = false;
    const int xgroup_now = (xg0 == 0 && !large) ? xgroup_first : xgroup;
    if (progressive && xg0 == 0 && c1 <= prog_end) {
      q.x_progressive_block = q.c0 / NB;
      if (c1 == prog_end) {   // (the group's last block: group [0, prog_end) is solved behind this panel)
        q.x_group_end = true;
        xg0 = c1;
      }
    } else {
      // THE predicate "an extra-row group ends at this panel": the X stream waits for the panel here, and a panel whose group waits
      // on the masked stream may not be flagged (flag_candidate below).
      const bool tail_group = tail_zone && (c1 == n - 2 * NB || c1 == n - NB);
      const bool full_group = ((c1 - xg0) >= xgroup_now || (large && c1 - xg0 >= nbo)) && !(tail_zone && c1 > n - 2 * NB && c1 < n);
      if (useX && (c1 == n || full_group || tail_group)) {
        q.x_group_end = true;
        q.tail_zone = tail_group;
        xg0 = c1;
      }
    }
  }
}

inline PotrfPlan make_potrf_plan(const PotrfShape& shape, const PotrfDevice& dev) {
  constexpr int NB = kPotrfNB, NBO = kPotrfNBO;
  PotrfPlan pl;
  const int n = pl.n = shape.n, extra = pl.extra = shape.extra, batch = pl.batch = shape.batch > 0 ? shape.batch : 1;
  pl.tri = shape.tri;   // (no decision depends on it: the identity rows only shorten the groups' row ranges at enqueue time)
  pl.single_leaf = n <= NB;
  const bool large = pl.large = n >= 4096;
  // outer panel width for n >= 4096 (A/B at N = 16384, profiles/r03_ab_gpr_nbo.log); one leaf block for the SVGP sizes,
  // where the whole factorisation is a latency chain
  const int nbo_large = (GPK_TUNE(NBO, 640) / NB) * NB;
  const int nbo = pl.nbo = large ? (nbo_large >= NB ? nbo_large : NBO) : NB;
  // Panel boundaries.  The END of a large factorisation is a latency chain again (trailing matrix too small to hide the
  // panel): there a wide panel costs 5 leaves + 4 in-panel updates + one K = 640 look-ahead strip of < 256 tiles, i.e. ONE
  // under-filled tile time of ~170 us -- 450 - 480 us per 640 columns (in-kernel time stamps, tools/leaf_phase_probe.py) --
  // while single-leaf panels cost 56 - 63 us each once their K = 128 rest-updates keep up.  So the last `narrow_tail`
  // columns are factored with the SVGP-size scheme (nbo = NB).  A/B at N = 16384, same box (profiles/r03_ab_gpr_nbo.log):
  // off 32.7 ms, 2048 -> 32.65, 3072 -> 32.4, 4096 -> 31.9, 5120 -> 32.2, 6144 -> 32.5, 8192 -> 33.2.
  const int narrow_tail = (nbo > NB) ? (GPK_TUNE(NARROW_TAIL, 4096) / NB) * NB : 0;
  int npanels = 0;
  for (int c = 0; c < n; ++npanels) c += (nbo > NB && n - c > narrow_tail) ? nbo : NB;
  pl.panels.reserve((size_t)npanels);
  for (int c = 0; c < n;) {
    PotrfPanel q{};
    q.c0 = c;
    c += (nbo > NB && n - c > narrow_tail) ? nbo : NB;
    q.c1 = std::min(c, n);
    pl.panels.push_back(q);
  }
  for (int p = 0; p < npanels; ++p) {
    pl.panels[p].c2 = (p + 1 < npanels) ? pl.panels[p + 1].c1 : n;
    pl.panels[p].c3 = (p + 2 < npanels) ? pl.panels[p + 2].c1 : n;
  }
  // Few extra rows (GPR: the P columns of Y) simply ride along through the panel solves and trailing
  // updates of the square part; many extra rows (SVGP: the minibatch; GPR: the test rows of predict_f) are solved
  // right-looking, group by group, as bulk work overlapped with the factorisation.
  pl.ride = extra > 0 && extra <= 256;
  const int R = pl.R = pl.ride ? n + extra : n;
  const bool useX = pl.useX = extra > 0 && !pl.ride;
  pl.B = large ? PotrfStream::B_masked : PotrfStream::Bs;
  // ONE bulk stream beside the chain: for large factorisations the extra rows share the (hardware-masked) stream of the
  // trailing updates; for small ones they have the unmasked stream X.  Round 3 re-measured every alternative on the SVGP
  // step (profiles/r03_ab_svgp_schedules.log): a masked extra-row stream with 8 ... 128 reserved CUs, two row halves on
  // two streams, the projection streamed or split onto a side stream, one GEMM per column group against an explicit
  // group inverse -- each 5 ... 40 % slower than this scheme.
  pl.X = large ? PotrfStream::B_masked : PotrfStream::X;
  // cap on the persistent workgroups of the big extra-row updates, so that some CUs stay free for the panel stream's
  // one-shot kernels (A/B on the SVGP step, round 1: cap 320 -> 448 steps/s, no cap 435, cap 224 -> 431; round 3: 256 ->
  // 419, 320 -> 441, 384 -> 447)
  // (round 5, with the packet-free chain: 224 -- one workgroup on 224 compute units, 32 left to the chain's one-shot kernels --
  //  is level with 320 on the whitened step and 2 - 5 % faster on the un-whitened one, whose extra-row stream is a quarter
  //  longer; a batch of problems keeps 320: C5 separate 2.04 against 2.02 ms; 240 / 248 lose 5 %, profiles/r05_ab_caps.log)
  if (!large) pl.bulk.cap = batch > 1 ? GPK_TUNE(EXTRA_MAX_WGS_BATCHED, 320) : GPK_TUNE(EXTRA_MAX_WGS, 224);
  if (!large) pl.bulk.group_cap = GPK_TUNE(GROUP_SOLVE_MAX_WGS, 0);
  if (!large) pl.bulk.kmin = GPK_TUNE(EXTRA_CAP_KMIN, 256);
  pl.chain_wgs = (!large && batch == 1) ? GPK_TUNE(CHAIN_MAX_WGS, 0) : 0;
  pl.nevents = 2 * npanels + 8;   // (+ fork, three joins)
  // Chain flags (round 5): single-leaf panels hand over with flag words instead of event packets -- potrf.hip, ChainSync.
  pl.use_flags = GPK_TUNE(CHAIN_FLAGS, 1) && (batch == 1 || GPK_TUNE(CHAIN_FLAGS_BATCHED, 1)) && dev.flags_usable;
  pl.gate_kernels = GPK_TUNE(GATE_KERNELS, 1) != 0;
  // (512 columns for M = 2048: 256 / 384 measured slower there.  For M <= 1024 the extra-row stream would start after half of
  // the chain: 256 columns for a batch of problems -- C5 separate 2.036 -> 1.977 ms -- and 128 for a single one -- C3 0.834 ->
  // 0.803 ms, C5 shared 1.314 -> 1.30 ms, but C5 separate 1.97 -> 2.11; profiles/r04_ab_c5.log, r04_ab_xgroup_small.log)
  // (round 6, with the chain at 41 us per panel instead of 62 the extra-row stream is the longer of the two at M = 1024 and wider groups
  //  -- fewer, longer-K updates of its 8192 rows -- win: 128 / 256 / 384 / 512 columns: C3 0.757 / 0.713 / 0.688 / 0.716 ms, C5 shared
  //  1.24 / 1.20 / 1.19 / 1.21 ms, two repetitions each on one box, profiles/r06_ab_extra_row_groups.log)
  const int xgroup_small = batch > 1 ? GPK_TUNE(XGROUP_SMALL_BATCH, 256) : GPK_TUNE(XGROUP_SMALL, 384);
  // (round 6: with FEW extra rows -- a rank's shard of a strong-scaled step -- M = 2048 prefers 256-column groups too: 4096 / 2048 / 1024
  //  rows 1.353 / 1.049 / 0.938 -> 1.308 / 1.019 / 0.918 ms, while 8192 rows lose 5 %: tools/strong_scaling_emulation.py under GPK_XGROUP,
  //  profiles/r06_ab_extra_row_groups.log)
  const int xgroup_wide = (batch == 1 && n < 4096 && extra < GPK_TUNE(XGROUP_FEW_ROWS_BELOW, 6144)) ? GPK_TUNE(XGROUP_FEW_ROWS, 256) : GPK_TUNE(XGROUP, NBO);
  pl.xgroup = std::max(NB, ((n <= 1024 ? xgroup_small : xgroup_wide) / NB) * NB);
  // (round 5 knobs: width of the FIRST extra-row group -- the extra-row stream idles until it is factored -- and the row count above
  //  which the shrinking groups at the end are dropped: with many rows that stream, not the chain, finishes last)
  pl.xgroup_first = std::max(NB, (GPK_TUNE(XGROUP_FIRST, 0) > 0 ? (GPK_TUNE(XGROUP_FIRST, 0) / NB) * NB : pl.xgroup));
  // (A/B, profiles/r05_ab_extra_row_stream.log: M = 2048 x 8192 rows 1.97 - 1.99 -> 1.934 ms without the shrinking groups;
  //  M = 1024, whose every panel is a group already, keeps them: 0.76 against 0.78 ms)
  // (round 6, late: with the 41-us chain period the extra-row stream finishes last at M = 1024 too -- the two single-block groups at the end ran as
  //  three launches BEHIND the last leaf: C3 0.683 - 0.690 -> 0.662 - 0.678 ms, C5 shared 1.18 -> 1.15, profiles/r06_ab_tail_zone_small.log)
  const int tail_zone_max_rows = n > 1024 ? GPK_TUNE(XTAIL_ZONE_MAX_ROWS, 6144) : GPK_TUNE(XTAIL_ZONE_MAX_ROWS_SMALL, 6144);
  // For the small sizes the groups shrink towards the end (.., n-256, n-128, n): whatever is left of the extra-row work when the
  // LAST leaf finishes is exposed latency.
  pl.tail_zone = useX && !large && (nbo == NB) && (n >= 8 * NB) && (extra < tail_zone_max_rows);
  // (A/B, profiles/r05_ab_extra_row_stream.log: latency kernel everywhere 1.903 1.907 | tiled from 150 workgroups 1.867 1.869 |
  //  from 250: 1.886 1.896 | always: 1.883 1.897; caps of 16 / 32 / 64 walking workgroups on the latency kernel: 2.41 / 2.06 / 1.94)
  // (all three "many extra rows" switches -- this one, the progressive first group, no shrinking groups at the end -- were measured
  //  at 8192 rows (gain) and 4096 rows (loss: 1.71 -> 1.82 ms for this one, tools/strong_scaling_emulation.py): threshold 6144)
  pl.rest_tiled = useX && !large && batch == 1 && extra >= GPK_TUNE(REST_TILED_MIN_ROWS, 3000);   // (6144 until the 64 x 64 tiles below: 4096 rows 1.33 -> 1.27 ms with them, profiles/r06_ab_rest_update_tile64.log)
  pl.rest_tiled_min_wgs = n > 1024 ? GPK_TUNE(REST_TILED_MIN_WGS, 30) : GPK_TUNE(REST_TILED_MIN_WGS_SMALL, 150);
  pl.rest_small_wgs = (useX && !large && batch == 1 && extra >= 6144) ? GPK_TUNE(REST_SMALL_WGS, 0) : 0;
  pl.rest_tile64 = GPK_TUNE(REST_TILE64, 1);     // (the per-panel loop below: rest_tile64_candidate)
  pl.trail_queue = GPK_TUNE(TRAIL_QUEUE, 1);     // (the per-panel loop below: rest_tile_queue)
  pl.bulk_cus = dev.bulk_cus;
  // Progressive first group (round 5).  The extra-row stream has nothing to do until the first group (four panels, ~245 us) is
  // factored, and then spends ~100 us on that group's in-group solve before its first large update can start.  Instead, as soon
  // as panel j of the first group is solved, ONE leaf block of the in-group solve runs (S_j = E_j X_j^T and the K = 128 update of
  // the group's later blocks: 4 + 3 + 2 + 1 block products), on a capped number of workgroups so that the chain -- alone on the
  // critical path there -- keeps its compute units.  When the fourth panel is done only one block product is left.
  pl.prog_end = std::min(pl.xgroup_first, n);
  pl.prog_cap = GPK_TUNE(XFIRST_PART_WGS, 128);
  pl.progressive_candidate = useX && !large && nbo == NB && batch == 1 && GPK_TUNE(XFIRST_PROGRESSIVE, 1) && pl.prog_end >= 2 * NB &&
                             extra >= GPK_TUNE(XFIRST_PROGRESSIVE_MIN_ROWS, 6144);
  pl.late_panel = std::min(npanels - 1, GPK_TUNE(LATE_WORK_PANEL, 5));
  // Split rest-update (round 6): potrf.hip, enqueue_rest_update.
  pl.rest_split_enabled = GPK_TUNE(REST_SPLIT, 1) && pl.use_flags;

  pl.plan_extra_rows(pl.progressive_candidate);
  for (int p = 0; p < npanels; ++p) {
    PotrfPanel& q = pl.panels[p];
    q.narrow = large && (q.c1 - q.c0 <= NB) && nbo > NB;
    // (stream memory operations only on the plain streams: on the CU-masked bulk stream of large factorisations a
    // hipStreamWriteValue32 was observed to overtake the kernel queued before it -- wrong factor at n = 5000 -- so a panel whose
    // extra-row group waits on that stream keeps its event, and so does a strip whose rest-update ran there)
    // (x_group_end matters on the masked stream only, i.e. for large factorisations, which have no progressive group: a second
    //  plan_extra_rows(false) leaves this as it is)
    q.flag_candidate = pl.use_flags && p < kMaxFlagPanels && q.c1 < n && (q.c1 - q.c0) <= NB && !(q.x_group_end && pl.X == PotrfStream::B_masked);
    // Bs: the unmasked stream of the SVGP-size scheme.  (A stream masked to half the CUs would keep CUs free for the leaf,
    // but its hand-offs to P took ~55 us instead of ~5: 190 us per panel instead of 56, GPR N = 16384 36.6 vs 32.0 ms.)
    q.rest_stream = q.narrow ? PotrfStream::Bs : pl.B;
    const bool masked = q.rest_stream == PotrfStream::B_masked;
    // (round 6) persistent workgroups -- two per compute unit of the bulk stream -- that take their tiles from a device counter
    // (gemm.hip, "Tile QUEUE"): no workgroup launch per tile and no drift between static tile lists; the kernel alone gains 7 %
    // (as dispatched 0.591 -> 0.632 of the chip's peak from 240 CUs).  They never leave their CUs, though, so the look-ahead panel no
    // longer finds gaps there and needs more CUs of its own: with 8 reserved the whole factorisation LOSES 7 % (33.0 against 30.8 ms),
    // with 32 (four per XCD) it gains 1.7 % (29.94 / 30.07 against 30.58 / 30.43 ms; 24: 32.0, 40: 31.6;
    // profiles/r06_ab_gpr_tile_queue.log).
    q.rest_tile_queue = masked && large;
    // (round 5) While the extra-row stream's capped updates hold 224 compute units, a rest-update on the one-shot latency kernel
    // -- up to 512 workgroups of 150 KB each -- queues through the 32 free ones for ~140 us and the chain's strips queue behind
    // it; the tiled kernel's 74-KB workgroups fit beside the capped ones.
    // (round 6, late) ... and there a 128 x 128 tile of the rest-update shares its compute unit with a capped MFMA-bound workgroup of the
    // extra-row stream and takes 60 - 95 us instead of 30 -- longer than the chain's period, and every strip WAITS for the previous
    // rest-update (the strips of the step timeline: 30 - 67 us, of which 8 are work).  As 64 x 64 tiles of the generic kernel (four times
    // the workgroups, 36 KB of LDS: they fit anywhere) it is short again: Cm 1.771 -> 1.750 ms, with the tiled regime from 30
    // workgroups on (M > 1024) 1.72 - 1.74; 32 x 64 and 64 x 128 tiles lose (profiles/r06_ab_rest_update_tile64.log).
    // (no_small = 1 and tile64 = PotrfPlan::rest_tile64)
    const int um = R - q.c2, un = n - q.c2;   // the rest-update is [um x un]
    q.rest_tile64_candidate = q.c2 < n && pl.rest_tiled && (long)((um + 15) / 16) * ((un + 127) / 128) >= pl.rest_tiled_min_wgs;
    q.rest_small_loop = !q.rest_tile64_candidate && pl.rest_small_wgs > 0;
    q.rest_flag = pl.use_flags && p < kMaxFlagPanels && !masked;
    q.rest_split_candidate = pl.rest_split_enabled && q.flag_candidate && !masked && !q.rest_tile64_candidate && !q.rest_small_loop &&
                             (q.c2 - q.c1) <= NB;
  }
  return pl;
}
