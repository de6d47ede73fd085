#!/bin/bash
# tools/bench_repeats.sh [runs] [outfile] -- python bench.py --full (every leg, CPU legs included in the first run only) N times back
# to back on one box: the run-to-run spread of every leg, one line per run, from each line's `summary` block.  The first run's full line is
# kept beside the table (bench_final.json in the outfile's folder).
set -u
REPO=$(cd "$(dirname "$0")/.." && pwd)
cd "$REPO"
N=${1:-5}
OUT=${2:-gpurun_out/r06_bench_repeats.txt}
DIR=$(dirname "$OUT"); REP=$DIR/_rep.json
mkdir -p "$DIR"
H=$(python -c "import twenty_first_amd as tf; print(tf.lib().tf_source_hash().decode())" 2>/dev/null)
echo "# python bench.py --full, $N runs back to back on one MI355X, library $H (run 1 with the CPU legs, the others --no-cpu-baseline): run-to-run spread of every leg" > "$OUT"
for i in $(seq 1 "$N"); do
  if [ "$i" = 1 ]; then python bench.py --full > "$REP" 2> /dev/null; cp "$REP" "$DIR/bench_final.json"
  else python bench.py --full --no-cpu-baseline > "$REP" 2> /dev/null; fi
  python - "$REP" >> "$OUT" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
s = d["summary"]
print(f"headline GFelts/s {s['headline']['value']} ms {s['headline']['ms']} frac {s['headline']['frac']} | merkle G leaves/s {s['merkle']['value'] / 1e9:.3f} ms {s['merkle']['ms']} | "
      f"coset ms {s['coset_eval']['ms']} frac {s['coset_eval']['frac']} | config5 GFelts/s {s['config5']['value']} trees G leaves/s {s['config5']['trees_leaves_per_s'] / 1e9:.3f} | commit ms {s['commit_pipeline']['ms']}")
PY
done
rm -f "$REP"
cat "$OUT"
