#!/bin/bash
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
# usage: gpu_bench_full.sh <output dir>: the --full bench line (CPU baseline included) and its wall time
OUT=${1:?usage: gpu_bench_full.sh <output dir>}
mkdir -p "$OUT"
SECONDS=0; timeout 1500 python bench.py --steps 3 --warmup 1 --full > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
OUT="$OUT" python - <<'PY'
import json, os
r = json.loads(open(os.path.join(os.environ["OUT"], "bench.json")).read().strip().split("\n")[-1])
print(r["value"], r["ms_per_step"], json.dumps(r["cpu_baseline"], indent=1)[:2500])
PY
echo "wall ${SECONDS}s"; tail -3 "$OUT/bench.err"
