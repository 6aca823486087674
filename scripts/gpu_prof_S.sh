#!/usr/bin/env bash
# Dev tool: kernel durations of the tracker iteration at workload S (graph replay), rocprofv3 kernel trace.
set -o pipefail
export OUT=${OUT:-run_out}  # output folder of this script
mkdir -p "$OUT"
R=$(pwd)
cd /tmp && export TMPDIR=/tmp && cd "$R"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_S -o st --output-format csv -- python3 bench.py --workload S --no-cpu-baseline --no-variants --steps 30 --warmup 5 --full > $OUT/prof_S.log 2>&1
rc=$?; if [ $rc -ge 124 ]; then exit $rc; fi
f=$(find $OUT/prof_S -name "*kernel_stats.csv" | head -1)
python3 - "$f" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if float(r["Percentage"]) > 0.3: print(f'{r["Name"][:60]:60s} calls {r["Calls"]:>6s} avg {float(r["AverageNs"])/1e3:8.2f} us  {r["Percentage"]}%')
PY
