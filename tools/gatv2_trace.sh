#!/bin/bash
# usage: tools/gatv2_trace.sh <tag>
# rocprofv3 kernel trace + stats (no counters in the run) of tools/gatv2_probe.py:
# the GATv2 forward / backward kernels next to GATConv's aggregation and
# backward at the batch-32 shapes.  Leaves $VGAN_TRACE_OUT/gatv2_trace_<tag>/ (default ab_out/)
# {probe.json, kernel_stats.csv, summary.txt}; summary.txt holds the average
# duration per kernel instantiation and, from the bytes probe.json lists, its
# rate over compulsory traffic.
set -o pipefail
TAG=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${VGAN_TRACE_OUT:-$R/ab_out}/gatv2_trace_$TAG
mkdir -p "$OUT"
export TMPDIR=/tmp
cd /tmp || exit 1
rm -rf "/tmp/gatv2_trace_$TAG"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "/tmp/gatv2_trace_$TAG" -o run --output-format csv -- \
  python3 "$R/tools/gatv2_probe.py" "$@" > "$OUT/probe.json" 2> "$OUT/probe.log" || exit $?
T=$(find "/tmp/gatv2_trace_$TAG" -name "*kernel_trace.csv" | head -1)
S=$(find "/tmp/gatv2_trace_$TAG" -name "*kernel_stats.csv" | head -1)
[ -n "$S" ] && cp "$S" "$OUT/kernel_stats.csv"
[ -n "$T" ] || { echo "no kernel_trace.csv"; exit 1; }
python3 - "$T" "$OUT/probe.json" > "$OUT/summary.txt" <<'EOF'
import csv, json, re, sys
from collections import defaultdict
pat = re.compile(r"(k_gatv2_\w+|k_gat_fwd_\w+|k_gat_bwd_\w+|k_fold_cols)(<[^>]*>)?")
by = defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    m = pat.search(r["Kernel_Name"])
    if m:
        by[m.group(1) + (m.group(2) or "")].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
probe = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(f"rows {probe['rows']}, edges {probe['edges']}, {probe['reps']} launches per kernel and width")
print("compulsory bytes per launch:", json.dumps(probe["bytes"]))
for k, v in sorted(by.items()):
    v = sorted(v)
    print(f"  {k:40s} {len(v):5d} x  avg {sum(v) / len(v):8.3f} us  median {v[len(v) // 2]:8.3f} us  min {v[0]:8.3f} us")
EOF
cat "$OUT/summary.txt"
