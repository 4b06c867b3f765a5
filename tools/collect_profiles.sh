#!/bin/bash
# Runs ON the GPU box (through tools/gpu.sh): the judged evidence for one tree, written under gpurun_out/<tag>/.
#   bench_n1.json                  python bench.py --full
#   bench_under_rocprof.json       the same step loop (a plain run: warm-up + timed steps, full-size launches only) under rocprofv3 --kernel-trace --stats
#   bench_kernel_stats.csv         its per-kernel summary (tools/summarize_rocpd.py)
#   pmc_traffic.json               HBM bytes per launch: FETCH_SIZE / WRITE_SIZE passes of tools/run_kernels.py (separate runs)
#   pmc_sq_*.json                  SQ counters (MFMA busy, LDS conflicts, issue / wait shares) of the conv and routing kernels
# usage: bash tools/collect_profiles.sh <tag> [steps]
set -o pipefail
TAG=${1:-rXX}; STEPS=${2:-10}
R=$PWD; O=$R/gpurun_out/$TAG; mkdir -p $O
HEAD=$(cat .bench_head 2>/dev/null)
python3 bench.py --full > $O/bench_n1.json 2> $O/bench_n1.err || { tail -5 $O/bench_n1.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python3 $R/bench.py --steps $STEPS --warmup 3 > $O/bench_under_rocprof.json 2> $O/bench_under_rocprof.err || { tail -5 $O/bench_under_rocprof.err; exit 1; }
DB=$(ls $O/prof/*.db $O/prof/*/*.db 2>/dev/null | head -1)
[ -n "$DB" ] && python3 $R/tools/summarize_rocpd.py $DB $((STEPS + 3)) > $O/bench_kernel_stats.csv
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_f -o p --output-format csv -- python3 $R/tools/run_kernels.py all 32 1 > $O/pmc_f.log 2>&1 &&
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_w -o p --output-format csv -- python3 $R/tools/run_kernels.py all 32 1 > $O/pmc_w.log 2>&1 &&
python3 $R/tools/pmc_traffic.py $(ls $O/pmc_f/*counter_collection.csv $O/pmc_f/*/*counter_collection.csv 2>/dev/null | head -1) $(ls $O/pmc_w/*counter_collection.csv $O/pmc_w/*/*counter_collection.csv 2>/dev/null | head -1) "$HEAD" > $O/pmc_traffic.json
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY -d $O/pmc_m -o p --output-format csv -- python3 $R/tools/run_kernels.py all 32 1 > $O/pmc_m.log 2>&1 &&
rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM -d $O/pmc_l -o p --output-format csv -- python3 $R/tools/run_kernels.py all 32 1 > $O/pmc_l.log 2>&1
M=$(ls $O/pmc_m/*counter_collection.csv $O/pmc_m/*/*counter_collection.csv 2>/dev/null | head -1)
L=$(ls $O/pmc_l/*counter_collection.csv $O/pmc_l/*/*counter_collection.csv 2>/dev/null | head -1)
if [ -n "$M" ] && [ -n "$L" ]; then
  python3 $R/tools/pmc_sq.py $M $L > $O/pmc_sq.json
  python3 $R/tools/pmc_sq_any.py caps $M $L > $O/pmc_sq_routing.json
fi
cd $R; rm -rf $O/pmc_f $O/pmc_w $O/pmc_m $O/pmc_l $O/prof
ls -la $O; cat $O/bench_n1.json | head -c 1500
