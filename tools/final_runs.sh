#!/bin/bash
# The measurement batch whose outputs go to profiles/ at the end of a round (run on the GPU box through gpurun).
# usage: bash tools/final_runs.sh <prefix>      e.g. r02
set -u
P=${1:-r06}
O=gpurun_out/final_$P; mkdir -p $O
python -m pytest tests -m gpu -q > $O/gputest.log 2>&1      # the whole GPU suite on this box, first
export DRT_BENCH_REPEATS=5      # (the many small runs of this batch: five repeats of the timed region each; the bench lines at the end unset it and take the sustained measurement from --full)
{
  for cfg in "--mesh hand --res 512 --views 72" "--mesh mouse --res 1024 --views 72" "--mesh horse --res 1024 --views 72" "--mesh monkey --res 1024 --views 72" "--mesh monkey --res 1024 --views 144"; do
    python bench.py $cfg --no-cpu-baseline --no-extras --steps 10 --warmup 3 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$cfg ::', d['ms_per_step'], 'ms/step', d['value'], 'M rays/s ;', d['config']['workload'])"
  done
} > $O/configs.txt 2>&1
{
  bash tools/scaling_proxy.sh
  # the one-kernel path (k_path, opt-in) at the same shares: the negative result of DESIGN_HISTORY.md A.1
  for v in 18 9; do
    DRT_MEGA_MAX_LOG2=25 DRT_BENCH_NOPROF=1 python bench.py --views $v --graph 0 --no-cpu-baseline --no-extras --steps 40 --warmup 5 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('views $v eager, DRT_MEGA_MAX_LOG2=25 (k_path)', d['ms_per_step'], 'ms/step')"
  done
} > $O/scaling_proxy.txt 2>&1
{
  # drt_tree_mode: full LBVH build per update (default) / its topology kept for 50 updates / binned-SAH topology from the host, refit per update
  for a in "" "--distance-factor 1.1" "--views 18" "--views 9"; do
    for e in "DRT_TREE=0" "DRT_TREE=1 DRT_REBUILD_EVERY=50" "DRT_TREE=2"; do
      echo "bench.py $a :: $e :: $(env $e DRT_BENCH_NOPROF=1 python bench.py $a --no-cpu-baseline --no-extras --steps 20 --warmup 5 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], 'ms/step')")"
    done
  done
  # outputs recycled (default) / zeroed ahead of time (round 3) / filled inside the call
  for e in "DRT_RECYCLE_OUTPUTS=1" "DRT_RECYCLE_OUTPUTS=0" "DRT_RECYCLE_OUTPUTS=0 DRT_PREFILL_NEXT=0"; do
    echo "bench.py :: $e :: $(env $e python bench.py --no-cpu-baseline --no-extras --steps 20 --warmup 5 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], 'ms/step')")"
  done
} > $O/modes.txt 2>&1
# soak: the fuzz tests of the suite over seeds it does not hold (round 6: 1600-1899 / 700-759 / 1000-1149; with RECYCLE + binding defaults)
{ python tools/fuzz_soak.py 1600 300; python tools/fuzz_soak_path.py 700 60; python tools/fuzz_soak_raster.py 1000 150;
  DRT_DETERMINISTIC=1 python tools/fuzz_soak_path.py 760 20; python tools/fuzz_soak_remesh.py 6 80 | grep 'FAILED\|AssertionError\|failures'; } 2>&1 | grep -v amdgpu > $O/soak.txt
python tools/ubench/trace_repeat.py 9 2>&1 | grep -v amdgpu > $O/trace_repeat.txt
python tools/ubench/remesh_probe.py 0.9 2>&1 | grep -v amdgpu > $O/remesh_probe.txt
# the kernels of the remesh probe (five un-instrumented calls + one bracketed = six remesh calls: rocprofv3 --stats summary, names cut)
( export TMPDIR=/tmp; rm -rf /tmp/rp_rm; rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_rm -o t -- python tools/ubench/remesh_probe.py 0.9 > /tmp/rp_rm.log 2>&1;
  f=$(find /tmp/rp_rm -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && python tools/kstats_top.py "$f" 40 ) > $O/remesh_kernels.txt 2>&1
python tools/recon_error_map.py 2>&1 | grep -v amdgpu > $O/recon_error_map.txt
python tools/ubench/vh_probe.py 2>&1 | grep -v amdgpu | head -3 > $O/vh_probe.txt
for r in gpu host; do REMESH=$r python tools/recon_trend.py 2>&1 | grep -v amdgpu > $O/recon_trend_$r.txt; done
python -m drt_amd.reconstruct --name monkey --views 144 --res 1024 2>&1 | grep -v amdgpu > $O/recon_monkey_144views.txt
# the launch line of the driver's multi-GPU runs, two ranks on this box's one GPU (gloo instead of RCCL): functional check of bench.py's N > 1 path
DRT_DIST_BACKEND=gloo timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 5 --warmup 2 --full > $O/bench_2rank_gloo.json 2> $O/bench_2rank_gloo.err
# the driver's N = 8 line (BASELINE config 4: 9 views per rank), eight ranks on this one GPU over gloo, full size: functional check, memory of eight scenes
DRT_DIST_BACKEND=gloo timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29541 bench.py --gpus 8 --steps 3 --warmup 2 --repeats 2 --full --no-cpu-baseline --no-extras > $O/bench_8rank_gloo.json 2> $O/bench_8rank_gloo.err
python tools/iter_bench.py > $O/iter_bench.txt 2>&1
{
  # explicit ray binding (default) vs the drop-in signature's identity heuristics; deterministic accumulation mode (drt_deterministic)
  for a in "--bind 1" "--bind 0"; do
    for e in "DRT_DETERMINISTIC=0" "DRT_DETERMINISTIC=1"; do
      echo "bench.py $a :: $e :: $(env $e python bench.py $a --full --no-cpu-baseline --no-extras --steps 20 --warmup 5 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], 'ms/step', d['repeats']['ms_per_step'], 'backward', d['roofline']['stages']['backward']['ms_per_step'])")"
    done
  done
  echo "bench.py --distance-factor 1.1 :: DRT_DETERMINISTIC=1 :: $(DRT_DETERMINISTIC=1 python bench.py --distance-factor 1.1 --no-cpu-baseline --no-extras --steps 10 --warmup 5 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], 'ms/step')")"
  DRT_DETERMINISTIC=1 python tools/iter_bench.py 2>&1 | grep -v amdgpu | grep "ms/iteration" | sed 's/^/DRT_DETERMINISTIC=1 iter_bench: /'
} > $O/bind_det.txt 2>&1
bash tools/profile.sh $P > $O/profile.log 2>&1
PROFILE_SKIP_PMC=1 DRT_STREAMS=1 DRT_FILL_OVERLAP=0 DRT_PREFILL_NEXT=0 bash tools/profile.sh ${P}_serial > $O/profile_serial.log 2>&1
# the regime real captures live in: the object fills the image (camera at 1.1 extents)
bash tools/profile.sh ${P}_tight --distance-factor 1.1 > $O/profile_tight.log 2>&1
PROFILE_SKIP_PMC=1 DRT_STREAMS=1 DRT_FILL_OVERLAP=0 DRT_PREFILL_NEXT=0 bash tools/profile.sh ${P}_tight_serial --distance-factor 1.1 > $O/profile_tight_serial.log 2>&1
bash tools/step_timeline.sh $O/step_timeline_tight.txt --distance-factor 1.1 > /dev/null 2>&1
# the bench lines LAST, with this build's own counters: bench.py prices k_trace's live launch time against SQ_INSTS_VALU of profiles/pmc.json
python tools/make_pmc_json.py gpurun_out/$P profiles/pmc.json dropin > /dev/null
PMC_WORKLOAD="horse res 1024 views 72 streams default, cameras at 1.1 extents" python tools/make_pmc_json.py gpurun_out/${P}_tight profiles/pmc.json tight > /dev/null
cp profiles/pmc.json $O/pmc.json
# (measured twice: right after the counter passes above the same box runs the step 3 % slower -- 2.40 vs 2.33 ms -- than in a call of its own; let it settle)
sleep 30
unset DRT_BENCH_REPEATS          # the bench lines: everything --full reports, the sustained measurement (`sustained`) among it
python bench.py --full > $O/bench.json 2> $O/bench.err
python bench.py --full --mode fused --no-cpu-baseline > $O/bench_fused.json 2> /dev/null
tail -n 3 $O/configs.txt $O/scaling_proxy.txt $O/iter_bench.txt; python tools/benchsum.py $O/bench.json | head -3
