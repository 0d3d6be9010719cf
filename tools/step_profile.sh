#!/bin/bash
# tools/step_profile.sh <tag> -- kernel-level profile of 40 bench steps and the legs of `bench.py --full` after them
# (rocprofv3 --kernel-trace --stats) on a GPU machine; output under $OUT/prof_<tag>/ (default OUT=build).
set -e
tag=${1:-x}
out=${OUT:-build}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_$tag" -o run -- python3 bench.py --full --steps 40 --warmup 60 --no-cpu-baseline > "$out/prof_$tag.log" 2>&1
python3 - "$out/prof_$tag" <<'PY'
import csv, glob, sys
f = glob.glob(f"{sys.argv[1]}/**/*kernel_stats.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
for r in rows[:28]:
    print(f"{r['Name'][:96]:96s} n={r['Calls']:>6s} avg_us={float(r['AverageNs'])/1e3:8.1f} pct={float(r['Percentage']):5.1f}")
PY
tail -1 "$out/prof_$tag.log" | cut -c1-300
