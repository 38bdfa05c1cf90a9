#!/bin/bash
# One GPU call that refreshes the round's profile set (on the GPU box; writes under the directory given as the second argument,
# default out/ in the repository root):
#   bench line (bench.py --full), rocprofv3 --kernel-trace --stats of the bench command, one step's kernel timeline, in-kernel stamps, PMC traffic passes.
set -u
R=${1:-r05}
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
OUT=${2:-out}
mkdir -p "$OUT"
CMD="bench.py --no-cpu-baseline --no-extras --no-configs --steps 100 --warmup 10"
timeout -k 10 480 python bench.py --full > $OUT/${R}_bench_n1.json 2> $OUT/${R}_bench_n1.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_prof -- python3 $CMD > $OUT/${R}_prof.log 2>&1
s=$(find $OUT/${R}_prof -name "*kernel_stats.csv" | head -1)
k=$(find $OUT/${R}_prof -name "*kernel_trace.csv" | head -1)
python tools/stats_summary.py "$s" "rocprofv3 --kernel-trace --stats -- python3 $CMD" 30 > $OUT/${R}_kernel_stats_step_bf16_graph.md
cp "$s" $OUT/${R}_kernel_stats_step_bf16_graph.csv
python tools/step_timeline.py "$k" subsample_fused_kernel > $OUT/${R}_step_timeline_bf16.md
rm -rf $OUT/${R}_prof
timeout -k 10 200 python tools/persist2_stamps.py 0.2 > $OUT/${R}_persist2_stamps.txt 2>&1
timeout -k 10 200 python tools/persist2x_stamps.py 0.2 > $OUT/${R}_persist2x_stamps_raw.txt 2>&1
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/${R}_pmc_fetch -- python3 tools/run_lstm2_steps.py > $OUT/${R}_pmc.log 2>&1 && \
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/${R}_pmc_write -- python3 tools/run_lstm2_steps.py >> $OUT/${R}_pmc.log 2>&1
f=$(find $OUT/${R}_pmc_fetch -name "*counter_collection.csv" | head -1); w=$(find $OUT/${R}_pmc_write -name "*counter_collection.csv" | head -1)
python tools/pmc_traffic.py "$f" "$w" $OUT/${R}_lstm2_chain_traffic.json $OUT/${R}_lstm2_chain_traffic.md > /dev/null
rm -rf $OUT/${R}_pmc_fetch $OUT/${R}_pmc_write
echo done; tail -c 300 $OUT/${R}_bench_n1.json
