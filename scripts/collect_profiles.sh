#!/bin/bash
# Collects the records of a round on the GPU box: the full bench line (headline + CPU baseline + long window), the rocprofv3
# --kernel-trace --stats summary of the headline's command (per-kernel average durations) and the cross-check of bench.py's
# HIP-event timing of k_flush against the trace.
# usage: bash scripts/collect_profiles.sh r02 [OUTDIR]   -> OUTDIR/r02_*.{json,csv} (default build/records); copy what is to be judged into profiles/
tag=${1:-rXX}
out=${2:-build/records}
mkdir -p "$out"
export TMPDIR=/tmp
python3 bench.py --full > $out/${tag}_bench_smid.json 2> $out/${tag}_bench_smid.err || exit 1
python3 bench.py --full --workload S-small --no-pair > $out/${tag}_bench_ssmall.json 2>> $out/${tag}_bench_smid.err || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag} -o ${tag} -- python3 bench.py --no-cpu-baseline --no-long-window > $out/${tag}_bench_smid_profiled.json 2> $out/${tag}_prof.err || exit 1
ks=$(find $out/prof_${tag} -name "*kernel_stats.csv" | head -1)
kt=$(find $out/prof_${tag} -name "*kernel_trace.csv" | head -1)
cp "$ks" $out/${tag}_bench_smid_kernel_stats.csv
python3 scripts/roofline_check.py "$kt" $out/${tag}_bench_smid_profiled.json > $out/${tag}_k_flush_trace_vs_events.json
rm -rf $out/prof_${tag}
head -12 $out/${tag}_bench_smid_kernel_stats.csv | cut -c1-160
cat $out/${tag}_k_flush_trace_vs_events.json
