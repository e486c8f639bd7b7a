#!/bin/bash
# usage: tools/abrun.sh <stage-regex> variant1 variant2 ...   (variants = names of drt_amd/_ab/<name>.so; "base" = the in-tree library)
export DRT_BENCH_REPEATS=${DRT_BENCH_REPEATS:-5}      # (several timed regions back to back, the line reports the median repeat: steadier than bench.py's single region)
pat=$1; shift
O=${BENCH_OUT:-bench_out}; mkdir -p "$O"      # (the JSON lines of the runs)
for v in "$@" "$@"; do
  if [ "$v" = base ]; then unset DRT_HIP_LIB; else export DRT_HIP_LIB=$PWD/drt_amd/_ab/$v.so; fi
  python bench.py --full --no-cpu-baseline > "$O/ab_$v.json" 2>/dev/null
  echo "== $v"; python tools/benchsum.py "$O/ab_$v.json" | grep -E "Mrays|$pat"
done
