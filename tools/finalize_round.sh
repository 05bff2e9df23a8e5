#!/bin/bash
# The LAST act of a round, on the GPU box (bash tools/finalize_round.sh r05): rocprofv3 kernel-trace + SQ + FETCH_SIZE /
# WRITE_SIZE passes of cfg 4, cfg 3, cfg 5 and associated-press with the kernels as they are NOW, the traffic files bench.py ties
# to the hash of the device headers, then the full bench line (bench.py --full, which therefore carries roofline.traffic), the
# --steps 20 --warmup 5 line and the GPU suite.  Everything lands under $RESULTS (default results/, as for
# tools/profile_bench.sh); copy into profiles/ with
#   bash tools/finalize_round.sh --collect r05        (once $RESULTS holds the records of that run)
TAG=${1:-rXX}
RESULTS=${RESULTS:-results}
export RESULTS
if [ "$TAG" = "--collect" ]; then
    set -euo pipefail      # a missing record must not leave a stale profiles/traffic_*.json behind
    TAG=$2
    for n in cfg4 cfg3; do
        cp $RESULTS/prof_${TAG}_$n/summary.txt profiles/${TAG}_${n}_rocprof_summary.txt
        cp $RESULTS/prof_${TAG}_$n/kernel_stats.csv profiles/${TAG}_${n}_kernel_stats.csv
    done
    cp $RESULTS/prof_${TAG}_nips/summary.txt profiles/${TAG}_nips_k500_rocprof_summary.txt
    cp $RESULTS/prof_${TAG}_nips/kernel_stats.csv profiles/${TAG}_nips_k500_kernel_stats.csv
    cp $RESULTS/prof_${TAG}_ap/summary.txt profiles/${TAG}_ap_k10_rocprof_summary.txt
    cp $RESULTS/prof_${TAG}_ap/kernel_stats.csv profiles/${TAG}_ap_k10_kernel_stats.csv
    cp $RESULTS/prof_${TAG}_cfg4/traffic.json profiles/traffic_synth1m.json
    cp $RESULTS/prof_${TAG}_cfg3/traffic.json profiles/traffic_synth100k.json
    cp $RESULTS/bench_final.json profiles/${TAG}_bench_default.json
    cp $RESULTS/bench_steps20.json profiles/${TAG}_bench_steps20_warmup5.json
    python -c "import json, bench; t = json.load(open('profiles/traffic_synth1m.json')); print('traffic hash', t['kernel_source_hash'], 'tree', bench.kernel_source_hash())"
    exit 0
fi
mkdir -p $RESULTS
bash tools/profile_bench.sh ${TAG}_cfg4 --workload synth1m > $RESULTS/prof_${TAG}_cfg4.log 2>&1
bash tools/profile_bench.sh ${TAG}_cfg3 --workload synth100k > $RESULTS/prof_${TAG}_cfg3.log 2>&1
bash tools/profile_cmd.sh ${TAG}_nips python bench.py --workload nips --no-cpu-baseline --no-extras --steps 5 --warmup 3 > $RESULTS/prof_${TAG}_nips.log 2>&1
bash tools/profile_cmd.sh ${TAG}_ap python bench.py --workload ap --no-cpu-baseline --no-extras --steps 20 --warmup 5 > $RESULTS/prof_${TAG}_ap.log 2>&1
cp $RESULTS/prof_${TAG}_cfg4/traffic.json profiles/traffic_synth1m.json
cp $RESULTS/prof_${TAG}_cfg3/traffic.json profiles/traffic_synth100k.json
( time python bench.py --full > $RESULTS/bench_final.json 2> $RESULTS/bench_final.err ) 2>&1 | tail -3
python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline > $RESULTS/bench_steps20.json 2>/dev/null
python -m pytest tests -x -q -m gpu 2>&1 | grep -E "passed|failed|rror" | head -5
