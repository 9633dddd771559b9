#!/bin/bash
# A/B of the q_sqrt projection's tunables on the SVGP step (same box):  tools/ab_proj.sh "GPK_PROJ_SNAKE=0" ...
# (written for the streamed projection of round 2, GPK_STREAM_PROJ, which no longer exists; the first line is the baseline)
run() {
  for rep in 1 2; do
    env $1 python bench.py --full --steps 40 --warmup 5 --no-cpu-baseline --no-gpr 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read())
r=d['roofline']
print('cfg=[$1] rep=$rep steps/s=%.1f ms=%.3f big_gemm_TF=%.1f all_gemm_us=%.0f' % (d['value'], d['ms_per_step'], r['big_gemm_launches']['tflops_over_summed_durations'], r['all_gemm_launches']['avg_launch_us']*r['all_gemm_launches']['launches_per_step']))" || echo "cfg=[$1] rep=$rep FAILED"
  done
}
run "AB_BASELINE=1"   # (no tunable: the defaults)
for cfg in "$@"; do run "$cfg"; done
