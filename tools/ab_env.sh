#!/bin/bash
# A/B of one environment switch on ONE box: bench.py with VAR=0 and VAR=1 alternating, 2 rounds, full extras (per-stage numbers).
# usage (via gpurun): bash tools/ab_env.sh DRT_HIT_SEED [bench args]
export DRT_BENCH_REPEATS=${DRT_BENCH_REPEATS:-3}      # (several timed regions back to back, the line reports the median repeat: steadier than bench.py's single region)
var=$1; shift
O=${BENCH_OUT:-bench_out}/ab; mkdir -p "$O"      # (the JSON lines of the runs)
for r in 1 2; do
  for v in 0 1; do
    env $var=$v timeout 600 python bench.py --full --no-cpu-baseline "$@" > "$O/${var}_${v}_$r.json" 2> "$O/${var}_${v}_$r.err"
    echo "== $var=$v round $r"; python tools/benchsum.py "$O/${var}_${v}_$r.json" | grep -E "Mrays|trace|raster|cull"
    python - <<PY
import json
d=json.loads(open("$O/${var}_${v}_$r.json").read().strip().splitlines()[-1])
e=d.get("establish_mode") or {}
print("   repeats:", d.get("repeats",{}).get("ms_per_step"), " tight:", (d.get("tight_framing") or {}).get("ms_per_step"), " establish:", e.get("ms_per_step"), (e.get("stages_ms_per_step") or {}).get("cull"), " fused:", (d.get("fused_mode") or {}).get("ms_per_step"))
PY
  done
done
