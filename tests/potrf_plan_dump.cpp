// Prints the schedule plan of the trapezoidal Cholesky for one shape: tests/test_potrf_plan.py builds this with plain g++ (no ROCm
// include path -- which is the check that potrf_plan.h needs no HIP header) and reads the lines back.
//   potrf_plan_dump n extra batch tri bulk_cus flags_usable [replan]
// replan != 0: the extra-row groups as gpk_potrf_core plans them again (plan_extra_rows(false)) when the operands rule the progressive
// first group out.
#include <cstdio>
#include <cstdlib>
#include "../gpflow_amd/csrc/potrf_plan.h"

static const char* name(PotrfStream s) { return s == PotrfStream::B_masked ? "B_masked" : s == PotrfStream::Bs ? "Bs" : "X"; }

int main(int argc, char** argv) {
  if (argc != 7 && argc != 8) return 2;
  const PotrfShape shape{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
  const PotrfDevice dev{atoi(argv[5]), atoi(argv[6]) != 0};
  PotrfPlan pl = make_potrf_plan(shape, dev);
  if (argc == 8 && atoi(argv[7]) != 0) pl.plan_extra_rows(false);
#define I(f) printf(#f " %d\n", (int)pl.f)
  I(single_leaf); I(large); I(nbo); I(ride); I(useX); I(R); I(chain_wgs); I(xgroup); I(xgroup_first); I(tail_zone); I(rest_tiled);
  I(rest_tiled_min_wgs); I(rest_small_wgs); I(rest_tile64); I(trail_queue); I(bulk_cus); I(progressive_candidate); I(prog_end);
  I(prog_cap); I(late_panel); I(use_flags); I(gate_kernels); I(rest_split_enabled); I(nevents); I(bulk.cap); I(bulk.group_cap);
  I(bulk.kmin);
#undef I
  printf("B %s\nX %s\nnpanels %d\n", name(pl.B), name(pl.X), pl.npanels());
  for (const PotrfPanel& q : pl.panels)
    printf("panel c0=%d c1=%d c2=%d c3=%d narrow=%d x_group_end=%d x_group_begin=%d x_progressive_block=%d tail_zone=%d flag_candidate=%d "
           "rest_stream=%s rest_tile_queue=%d rest_tile64_candidate=%d rest_small_loop=%d rest_flag=%d rest_split_candidate=%d\n",
           q.c0, q.c1, q.c2, q.c3, (int)q.narrow, (int)q.x_group_end, q.x_group_begin, q.x_progressive_block, (int)q.tail_zone,
           (int)q.flag_candidate, name(q.rest_stream), (int)q.rest_tile_queue, (int)q.rest_tile64_candidate, (int)q.rest_small_loop,
           (int)q.rest_flag, (int)q.rest_split_candidate);
  return 0;
}
