#!/bin/bash
# Runs on an MI355X machine: kernel trace of the bench.py command with every leg (--full) + PMC passes on the short
# profiling workload.  Raw rocpd DBs land in $PROFILE_OUT/<tag>_*/ (default profile_out/ in the repository) ; summaries
# are made here by tools/rocpd_summary.py and tools/pmc_summary.py (text files next to them) and copied to profiles/ by hand.
tag=${1:-r02}
root=${GRAFT_REPO_ROOT:-$(pwd)}
out=${PROFILE_OUT:-$root/profile_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $out/${tag}_bench -o bench -- python $root/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-other > $out/${tag}_bench_under_rocprof.json 2> $out/${tag}_bench.err
timeout 150 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $out/${tag}_pmc_fetch -o pmc -- python $root/tools/prof_run.py both > $out/${tag}_pmc_fetch.log 2>&1
timeout 150 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $out/${tag}_pmc_write -o pmc -- python $root/tools/prof_run.py both > $out/${tag}_pmc_write.log 2>&1
timeout 150 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE -d $out/${tag}_pmc_mfma -o pmc -- python $root/tools/prof_run.py both > $out/${tag}_pmc_mfma.log 2>&1
timeout 120 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $out/${tag}_pmc_kb_write -o pmc -- python $root/tools/kb_probe.py > $out/${tag}_pmc_kb_write.log 2>&1
timeout 120 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $out/${tag}_pmc_kb_fetch -o pmc -- python $root/tools/kb_probe.py > $out/${tag}_pmc_kb_fetch.log 2>&1
cd $root
python tools/rocpd_summary.py $(find $out/${tag}_bench -name "*.db" | head -1) > $out/${tag}_bench_kernel_stats.txt 2>&1
for k in fetch write mfma kb_write kb_fetch; do
  python tools/pmc_summary.py $(find $out/${tag}_pmc_$k -name "*.db" | head -1) > $out/${tag}_pmc_$k.txt 2>&1
done
db=$(find $out/${tag}_bench -name "*.db" | head -1)
python tools/timeline.py $db rbf_kernel 20 130 > $out/${tag}_step_timeline.txt 2>&1
rm -rf $out/${tag}_bench $out/${tag}_pmc_fetch $out/${tag}_pmc_write $out/${tag}_pmc_mfma $out/${tag}_pmc_kb_write $out/${tag}_pmc_kb_fetch
ls -la $out/${tag}_*
tail -c 600 $out/${tag}_bench_under_rocprof.json
