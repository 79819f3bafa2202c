#!/bin/bash
# A change against its parent commit on one box in one session (run on the GPU box from the repository root):
#     bash tools/ab_parent.sh <checkout of the parent commit, library built> <output directory>
# Headline bench lines alternating parent / new, the 262 144-cf batch, bs128 as the control, kernel traces with
# per-kernel stats (two steps in flight and one) with tools/phase_trace.py's view of them, and the region histograms of
# tools/bench_regions.py without and with the start gate.  Every GPU command runs under its own timeout and the
# script stops at the first that fails.
set -o pipefail
R=$PWD
P=$(cd "$1" && pwd)
mkdir -p "$2"
O=$(cd "$2" && pwd)
export TMPDIR=/tmp
line() {    # checkout tag bench-args...
  local d=$1 tag=$2; shift 2
  ( cd $d && timeout -k 10 200 python3 bench.py "$@" > $O/$tag.log 2> $O/$tag.err ) || { echo "FAILED $tag"; tail -5 $O/$tag.err; exit 1; }
  grep '^{"metric"' $O/$tag.log | tail -1 > $O/bench_$tag.json
  python3 - $O/bench_$tag.json $tag <<'PY'
import json, sys
d = json.load(open(sys.argv[1])); c = d["config"]
print("%-22s median of regions %.2f M cf/s  value %.2f M  one step in flight %.2f M  verified %s  quantiles %s" % (
    sys.argv[2], c["value_median_regions"] / 1e6, d["value"] / 1e6, c["value_one_step_in_flight"] / 1e6, d["verified_cf"],
    {k: round(v, 4) for k, v in c["ms_per_step_quantiles"].items()}), flush=True)
PY
  rm -f $O/$tag.log $O/$tag.err
}
for i in 1 2 3 4; do
  line $P parent_scalar128_$i --full --no-cpu-baseline
  line $R new_scalar128_$i --full --no-cpu-baseline
done
for i in 1 2; do
  line $P parent_scalar128_262144_$i --full --no-cpu-baseline --frames 131072 --host-stream-frames 0
  line $R new_scalar128_262144_$i --full --no-cpu-baseline --frames 131072 --host-stream-frames 0
  line $P parent_bs128_$i --full --no-cpu-baseline --workload bs128 --host-stream-frames 0
  line $R new_bs128_$i --full --no-cpu-baseline --workload bs128 --host-stream-frames 0
done
trace() {   # checkout tag extra-bench-args...
  local d=$1 tag=$2; shift 2
  ( cd $d && timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $O/tr_$tag -o t --output-format csv -- python3 bench.py --full --no-cpu-baseline --no-verify --no-decode-leg --min-seconds 0.25 --host-stream-frames 0 "$@" > $O/trace_$tag.log 2>&1 ) || { echo "FAILED trace $tag"; tail -5 $O/trace_$tag.log; exit 1; }
  cp $(find $O/tr_$tag -name 't_kernel_stats.csv' | head -1) $O/${tag}_kernel_stats.csv
  python3 $R/tools/phase_trace.py $(find $O/tr_$tag -name 't_kernel_trace.csv' | head -1) > $O/${tag}_phase_trace.txt 2>&1 || echo "phase_trace.py failed for $tag"
  rm -rf $O/tr_$tag $O/trace_$tag.log
}
trace $P parent_scalar128
trace $R new_scalar128
trace $P parent_scalar128_one_in_flight --pipeline 1 --no-graph
trace $R new_scalar128_one_in_flight --pipeline 1 --no-graph
for g in 0 20; do
  ( cd $P && timeout -k 10 200 python3 tools/bench_regions.py parent gate $g us -- --gate-us $g ) | tee -a $O/regions.txt || exit 1
  ( cd $R && timeout -k 10 200 python3 tools/bench_regions.py new gate $g us -- --gate-us $g ) | tee -a $O/regions.txt || exit 1
done
