#!/bin/bash
# tools/profile_extras.sh <tag> -- rocprofv3 kernel-trace of bench.py INCLUDING its "extra" workloads (Merkle 2^24,
# XFE coset evaluation, fast_multiply, LDE, table hashing): per-kernel dispatch counts and durations, grouped by grid size.
# Output: gpurun_out/prof_<tag>/extras_summary.json (copy to profiles/).
set -u
TAG=${1:-r01}
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$REPO/gpurun_out/prof_$TAG
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
CMD="python $REPO/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/extras" -o all -- $CMD > "$OUT/extras.log" 2>&1
python3 - "$OUT" <<'PY'
import csv, glob, json, os, statistics, sys
out = sys.argv[1]
g = glob.glob(os.path.join(out, "extras/**/*kernel_trace.csv"), recursive=True)
summary = {"command": "bench.py --steps 10 --warmup 3 --full --no-cpu-baseline (headline + extra workloads)"}
if g:
    per = {}
    for r in csv.DictReader(open(g[0])):
        k = r["Kernel_Name"]
        grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0))
        per.setdefault(k, {}).setdefault(grid, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    rows = []
    for k, grids in per.items():
        total = sum(sum(v) for v in grids.values())
        top = sorted(grids.items(), key=lambda kv: -sum(kv[1]))[:4]
        rows.append({"kernel": k, "dispatches": sum(len(v) for v in grids.values()), "total_ms": total / 1e6,
                     "by_grid_size_x": [{"grid_x": gx, "dispatches": len(v), "avg_us": sum(v) / len(v) / 1e3,
                                         "median_us": statistics.median(v) / 1e3, "min_us": min(v) / 1e3} for gx, v in top]})
    rows.sort(key=lambda r: -r["total_ms"])
    summary["kernels"] = rows[:24]
# (bench.py's own step time under the profiler is NOT a timing reference: rocprofv3 stalls the host for ~120 ms whenever it
# flushes its trace buffer, sometimes inside the timed region; the kernel durations above are what this file records)
json.dump(summary, open(os.path.join(out, "extras_summary.json"), "w"), indent=1)
print(json.dumps(summary, indent=1)[:6000])
PY
