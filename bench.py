#!/usr/bin/env python3
"""Headline benchmark: camera rays traced + differentiated per second (BASELINE.json metric).

A "step" is one full-batch optimisation iteration over the synthetic 72-view capture of a
~50k-triangle mesh (horse_vh.ply after one midpoint subdivision = 50 248 triangles,
1024x1024 rays per view):

    vertices = init + parameter                      (reference optim.py:202)
    scene.update_verticex(vertices)                  LBVH rebuild on the GPU (DiffRender.py:378-380)
    for each local view: render_transparent + ray_loss          (optim.py:91-108)
    loss.backward()  -> grad[V,3]; all-reduce over ranks (views are sharded round-robin)
    limit_hook + SGD(nesterov) step                  (optim.py:155-171, 215)

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--mode dropin|fused] [--res R] [--views V] [--full] [--dump-outputs DIR]
For N > 1 launch under torch.distributed.run (one rank per GPU, RCCL).  Rank 0 prints ONE JSON line.

A plain run sets up, takes W untimed steps (at least 3), times exactly K steps, writes the last step's outputs if --dump-outputs is
given and prints the line.  --full adds everything else the line can carry: a sustained measurement, the roofline and per-stage tables,
the fused / establish / tight-framing / route-B extras, the drop-in vs fused loss check and the CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from drt_amd import diffrender as Render, dist as ddist, mesh_io, views  # noqa: E402

IOR = 1.4723
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md); 6290 GB/s measured achievable
B_FWD = 48 + 51              # render_transparent kernel: read origin+dir, write out_ori+out_dir+mask (float64 signature)
B_STEP = 148                 # whole fwd + loss + bwd per ray


def load_workload(name, subdiv=None):
    path = os.path.join(ROOT, "data", f"{name}_vh.ply")
    if os.path.exists(path):
        base = mesh_io.read_ply(path)
        src = f"{name}_vh.ply"
    else:                                   # licence-free stand-in with a similar triangle count
        base = mesh_io.icosphere(4, radius=60.0, noise=0.01)
        src = "icosphere(4)"
    if subdiv is None:
        subdiv = 1 if name in ("horse", "mouse") else 0
    mesh = base
    for _ in range(subdiv):
        mesh = mesh_io.subdivide_midpoint(mesh)
    return mesh, f"{src} x{4 ** subdiv} ({subdiv} midpoint subdivision{'s' if subdiv != 1 else ''})"


def per_view_mesh_bytes(V, F):
    # float64 vertices + float32 copy + faces + triangle records + BVH nodes + gradient write
    return 24 * V + 12 * V + 12 * F + 48 * F + 64 * (F - 1) + 24 * V


VALU_PEAK = 256 * 4 * 2.4e9 / 2     # wave64 VALU instructions/s: 256 CUs x 4 SIMD-32 units, two cycles per wave-instruction (MI355X_MICROARCH.md)
# What this chip sustains on streams of ONE instruction at 8 waves per SIMD (tools/ubench/valu_rate.hip, G wave-instructions/s): only the
# fma class comes near the two-cycle figure; compares, selects, min/max, permutes -- three quarters of an inner visit -- take four cycles,
# and packed float32 fmas are slower per fma than plain ones.  `frac` is priced against VALU_PEAK all the same.
VALU_MEASURED = {"v_fma_f32": 834.0, "v_max_f32": 563.8, "v_pk_fma_f32 (x2 fmas)": 246.6, "source": "tools/ubench/valu_rate.hip"}
# which bench.py stage is which kernel(s) in a rocprofv3 trace
KERNELS = {"k_trace<closest>": ("trace1", "trace2"), "k_trace<any>": ("trace3",), "fill + k_cull": ("fill", "cull"), "k_raster": ("raster",),
           "k_shade1": ("shade1",), "k_shade2": ("shade2",), "k_finish": ("finish",), "k_render_bwd": ("backward", "collect"),
           "k_loss_bwd_fused": ("loss_bwd_fused",), "build": ("build",), "k_path": ("path",)}
# (the third template argument -- temporal hit seeds -- since round 5; the record with the most launches is the steady state's)
PMC_NAMES = {"k_trace<closest>": ("k_trace<false, 0, false>", "k_trace<false, 0, true>", "k_trace<false, 0>"),
             "k_trace<any>": ("k_trace<true, 0, false>", "k_trace<true, 0>")}


def _pmc(mode, workload):
    """(per-launch PMC means of profiles/pmc.json, provenance) -- only for the workload they were collected on.  The file is stamped
    with a sha256 of the kernel sources (tools/make_pmc_json.py, drt_amd.build.source_hash): counters of OTHER kernels than the ones
    this run timed are not mixed with its launch times -- `stale` says so and the issue-rate figures fall back to the live estimate."""
    path = os.path.join(ROOT, "profiles", "pmc.json")
    prov = {"file": "profiles/pmc.json", "git_head": None, "source_sha256": None, "stale": True}
    try:
        rec = json.load(open(path))
        from drt_amd import build as _build
        now = _build.source_hash()
        prov.update(git_head=rec.get("git_head"), source_sha256=rec.get("source_sha256"), sources_now_sha256=now,
                    stale=rec.get("source_sha256") != now)
        return (rec.get(mode, {}) if rec.get("workloads", {}).get(mode, rec.get("workload")) == workload else {}), prov
    except Exception:
        return {}, prov


# VALU wave-instructions of one wave-step of k_trace<closest> (static counts of the inner-node visit and of the one-triangle leaf visit in
# this build's ISA, loop bookkeeping included: DESIGN.md section 6): with the wave-steps the statistics mode counts live, an estimate of
# SQ_INSTS_VALU that does not depend on a committed counter file -- reported next to the PMC figure, and used instead of it when that
# file was collected on other kernel sources.
VALU_PER_INNER_STEP, VALU_PER_LEAF_STEP = 103, 72


def projection_pass(pmc, fresh, launches_per_step, alg_bytes_per_step):
    """The projection pass against its algorithmic bytes (48 B per (image, triangle) + 40 B per written key): HBM traffic of its kernels from
    the PMC passes (profiles/pmc.json, same kernel sources), per step = stage launches x (2 k_raster + 2 k_raster_big launches each)."""
    out = {"alg_bytes_per_step": int(alg_bytes_per_step), "traffic_bytes_per_step": None, "ratio": None}
    if pmc and fresh and all(k in pmc and "hbm_bytes_per_launch" in pmc[k] for k in ("k_raster", "k_raster_big")):
        t = 2.0 * launches_per_step * (pmc["k_raster"]["hbm_bytes_per_launch"] + pmc["k_raster_big"]["hbm_bytes_per_launch"])
        out.update(traffic_bytes_per_step=int(t), ratio=round(t / max(1.0, alg_bytes_per_step), 2))
    return out


def roofline(prof, args, P, n_local_views, V, F, elapsed, world, prof_alone=None, live=None, wave_steps=None, recycled=False):
    """Per-kernel live timing (hipEvents on the launch streams, drt_profile_*) -> the kernel that takes the most time, BY
    KERNEL NAME (the two closest-hit traversals are one kernel), with the bound that applies to it, and the HBM-streaming
    stage beside it.

    * `k_trace` walks an L2-resident tree: its bound is VALU issue (measured: doubling the slab arithmetic of an inner visit
      costs +24 %).  achieved = VALU wave-instructions per launch (rocprofv3 SQ_INSTS_VALU of the same
      command, profiles/pmc.json) / the live launch time; peak = 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles.
    * `fill + k_cull` (dead values into the dense float64 outputs + the patches that matter) is the HBM stage: algorithmic
      bytes = 51 B per ray written + (48 read + 36 list + 8 key) per primary hit, DESIGN.md section 4.  `recycled`: the call renders into
      the outputs of the previous one (diffrender.RECYCLE_OUTPUTS) and the "fill" is 51 B per COMPLETED PATH of that call (the rows it had
      set), not per ray: the stage is then a latency-bound scatter and no longer a bandwidth figure worth a roofline.
    Stage times of the timed region overlap (two internal streams); `alone` = the same steps with the streams serialised."""
    n = P * n_local_views * args.steps                 # rays through the pipeline in the timed region
    it = {k: v[2] for k, v in prof.items()}
    h0 = it["shade1"]                                  # primary hits (list R0)
    c, h, s2 = it["trace1"], it["trace2"], it["trace3"]          # rays left to the tree, refracted primary hits, exit rays
    v = it["loss_bwd_fused"] if args.mode == "fused" else it["backward"]
    fused = args.mode == "fused"
    # bytes per item: list entry = 4 (index) + 24 (float32 ray) + 4 (face); float64 ray = 48; dense outputs = 51 + 8 (face ids)
    alg = {
        "fill": 0 if fused else (55 * v if recycled else 51 * n),      # dense outputs 24 + 24 + 3 B per ray (face ids only where mask = 1); recycled outputs: the rows of the previous call's list (4 B read + 51 B written each)
        "cull": (48 + 36 + 8) * h0 + (0 if it.get("fill", 0) or fused else 51 * n),
        "trace1": 28 * c, "trace2": 28 * h, "trace3": 28 * s2,
        "shade1": (8 + 48 + 4) * h0 + 28 * h,
        "shade2": (8 + 48 + 4) * h + 28 * s2 + (4 * h if fused else 59 * h),
        "finish": 8 * s2 + 4 * v,
        "collect": 4 * n + 4 * v,
        "backward": (4 + 48 + 8 + 24) * v + 144 * v,
        "loss_bwd_fused": (8 + 48 + 8 + 24) * s2 + 144 * s2,
        "build": per_view_mesh_bytes(V, F) * args.steps,
        # projected primary visibility: every image reads the triangle records once; per written key a 24-byte ray and a 16-byte atomic
        "raster": 48 * F * n_local_views * args.steps + 40 * h0,
    }

    def table(pr):
        st = {}
        for k, (ms, launches, items) in pr.items():
            if launches == 0:
                continue
            mesh_b = per_view_mesh_bytes(V, F) * launches if k in ("trace1", "trace2", "trace3") else 0
            gbs = (alg.get(k, 0) + mesh_b) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            st[k] = {"ms_per_step": round(ms / args.steps, 4), "avg_launch_ms": round(ms / launches, 4), "launches": launches,
                     "items_per_launch": items // launches, "alg_GBps": round(gbs, 1)}
        return st

    stages = table(prof)
    alone = table(prof_alone) if prof_alone else {}
    by_kernel = {}
    for name, members in KERNELS.items():
        ms = sum(stages[m]["ms_per_step"] for m in members if m in stages)
        if ms > 0:
            by_kernel[name] = {"ms_per_step": round(ms, 4), "launches": sum(stages[m]["launches"] for m in members if m in stages),
                               "alone_ms_per_step": round(sum(alone[m]["ms_per_step"] for m in members if m in alone), 4) if alone else None}
    dom = max((k for k in by_kernel if k != "build"), key=lambda k: by_kernel[k]["ms_per_step"])
    pmc, pmc_prov = _pmc(args.mode, f"{args.mesh} res {args.res} views {n_local_views} streams default")
    pmc_fresh = bool(pmc) and not pmc_prov["stale"]

    def issue_entry(name):
        """VALU-issue bound of a traversal kernel: wave-instructions per launch (PMC) over the live launch time."""
        members = [m for m in KERNELS[name] if m in stages and stages[m]["items_per_launch"] > 0]
        launches = sum(stages[m]["launches"] for m in members)
        ms = sum(stages[m]["ms_per_step"] for m in members) * args.steps
        rec = max((pmc[q] for q in PMC_NAMES.get(name, ()) if q in pmc), key=lambda r: r.get("launches", 0), default=None)
        out = {"kernel": name, "bound": "valu-issue", "unit": "G wave-instr/s", "peak": round(VALU_PEAK / 1e9, 1), "avg_launch_ms": round(ms / max(1, launches), 4),
               "achieved": None, "frac": None, "traffic": None, "valu_instr_per_launch": None, "pmc_stale": pmc_prov["stale"], "pmc": pmc_prov}
        # live estimate: wave-steps of one (untimed, statistics-mode) step x the static instruction counts of a wave-step
        ws = [wave_steps[m] for m in members if wave_steps and m in wave_steps]
        est = None
        if ws and name == "k_trace<closest>":
            inner = sum(w["inner"] for w in ws) / max(1, sum(w["launches"] for w in ws)); leaf = sum(w["leaf"] for w in ws) / max(1, sum(w["launches"] for w in ws))
            est = inner * VALU_PER_INNER_STEP + leaf * VALU_PER_LEAF_STEP
            out["wave_steps_per_launch"] = {"inner": round(inner), "leaf": round(leaf)}
            out["valu_instr_per_launch_est"] = int(est)
            if launches and ms > 0:
                out["est"] = {"achieved": round(est / (ms / launches * 1e-3) / 1e9, 1), "frac": round(est / (ms / launches * 1e-3) / VALU_PEAK, 4),
                              "what": f"wave-steps counted live x ({VALU_PER_INNER_STEP} VALU per inner visit, {VALU_PER_LEAF_STEP} per leaf visit)"}
        if not pmc_fresh:
            # counters of other kernel sources (or none): not mixed with this run's launch times
            if est and launches and ms > 0:
                out.update(achieved=out["est"]["achieved"], frac=out["est"]["frac"], frac_source="live wave-step estimate (profiles/pmc.json is stale: re-run tools/final_runs.sh)")
            return out
        if rec and launches and ms > 0 and "SQ_INSTS_VALU" in rec:
            ach = rec["SQ_INSTS_VALU"] / (ms / launches * 1e-3)
            out.update(achieved=round(ach / 1e9, 1), frac=round(ach / VALU_PEAK, 4), valu_instr_per_launch=int(rec["SQ_INSTS_VALU"]),
                       valu_busy_quadcycles_per_launch=rec.get("SQ_ACTIVE_INST_VALU"), salu_instr_per_launch=rec.get("SQ_INSTS_SALU"),
                       l2_hit=round(rec["TCC_HIT_sum"] / (rec["TCC_HIT_sum"] + rec["TCC_MISS_sum"]), 4) if "TCC_HIT_sum" in rec and "TCC_MISS_sum" in rec else None,
                       hbm_bytes_per_launch=rec.get("hbm_bytes_per_launch"), traffic=rec.get("hbm_bytes_per_launch"))     # (`traffic`: the contract's name for the PMC bytes)
            if rec.get("SQ_ACTIVE_INST_VALU") and rec.get("GRBM_GUI_ACTIVE"):
                # share of the launch during which a SIMD's vector ALU is occupied: SQ_ACTIVE_INST_VALU counts quad-cycles summed over the
                # 1024 SIMDs, GRBM_GUI_ACTIVE the launch's cycles summed over the 8 XCDs (both from the serialised PMC passes)
                out["valu_pipe_busy"] = round(rec["SQ_ACTIVE_INST_VALU"] * 4 * 8 / (1024 * rec["GRBM_GUI_ACTIVE"]), 3)
                out["valu_lanes_useful"] = round(rec["SQ_THREAD_CYCLES_VALU"] / (64 * rec["SQ_ACTIVE_INST_VALU"]), 3) if rec.get("SQ_THREAD_CYCLES_VALU") else None
            out["measured_issue_rates"] = VALU_MEASURED
            out["frac_source"] = "rocprofv3 SQ_INSTS_VALU (profiles/pmc.json, same kernel sources)"
            if est:
                out["est_over_pmc"] = round(est / rec["SQ_INSTS_VALU"], 3)
            if alone:
                ms_a = sum(alone[m]["ms_per_step"] for m in members if m in alone) * args.steps
                out["alone"] = {"avg_launch_ms": round(ms_a / launches, 4), "achieved": round(rec["SQ_INSTS_VALU"] / (ms_a / launches * 1e-3) / 1e9, 1),
                                "frac": round(rec["SQ_INSTS_VALU"] / (ms_a / launches * 1e-3) / VALU_PEAK, 4)}
        return out

    def hbm_entry(_stage=None):
        """The HBM stage: pre-fill of the dense outputs (memsets) + k_patch_list + k_cull_listed, per sub-batch."""
        members = [m for m in ("fill", "cull") if m in stages]
        launches = stages["cull"]["launches"]
        ms = sum(stages[m]["ms_per_step"] for m in members) * args.steps
        bytes_ = sum(alg[m] for m in members)
        ach = bytes_ / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        traffic = None
        if pmc and pmc_fresh:       # HBM bytes of the kernels of the stage (memset fills + k_patch_list + k_cull_listed), per sub-batch
            names = [q for q in pmc if q.startswith(("__amd_rocclr_fill", "k_patch_list", "k_cull_listed"))]    # (k_cull<...> is the establishing step's kernel)
            if names and all("hbm_bytes_per_launch" in pmc[q] for q in names):
                per_step = sum(pmc[q]["hbm_bytes_per_launch"] * pmc[q]["launches"] for q in names)
                ref_launches = pmc.get("k_patch_list", {}).get("launches")
                traffic = round(per_step / ref_launches) if ref_launches else None
        out = {"kernel": "k_unwrite_rows + k_cull (outputs recycled: no dense fill)" if recycled else "fill + k_cull", "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
               "traffic": traffic, "pmc_stale": pmc_prov["stale"], "alg_bytes_per_launch": round(bytes_ / max(1, launches)), "avg_launch_ms": round(ms / max(1, launches), 4)}
        if alone and all(m in alone for m in members):
            ms_a = sum(alone[m]["ms_per_step"] for m in members) * args.steps
            out["alone"] = {"achieved": round(bytes_ / (ms_a * 1e-3) / 1e9, 1), "frac": round(bytes_ / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                            "avg_launch_ms": round(ms_a / max(1, launches), 4)}
        return out

    step_alg = ((73 if fused else B_STEP) * P + per_view_mesh_bytes(V, F)) * args.views
    top = issue_entry(dom) if dom.startswith("k_trace") else hbm_entry("cull")
    top.update({"dominant_by_kernel_name": dom, "kernels": by_kernel, "hbm": hbm_entry("cull"),
                "traversal": {k: issue_entry(k) for k in ("k_trace<closest>", "k_trace<any>") if k in by_kernel},
                "stages": stages, "stages_alone_avg_launch_ms": {k: v["avg_launch_ms"] for k, v in alone.items()} if alone else None,
                "whole_step_alg_GBps_per_gpu": round(step_alg / (elapsed / args.steps) / 1e9 / world, 1),
                "projection_pass": projection_pass(pmc, pmc_fresh, stages["raster"]["launches"] / args.steps, alg["raster"] / args.steps) if "raster" in stages else None,
                "live_stages": list(live) if live else None,
                "note": "the closest-hit traversal of the refracted rays (stage trace2 = every launch of the dominant kernel) is timed by hipEvent pairs on its launch streams INSIDE the timed region (N = 1); the other stages are "
                        "timed in an immediate repeat of the same steps with every stage's events on; sub-batches run on two internal streams, so stage "
                        "durations overlap (`alone`: the same steps, untimed, with the streams serialised). The kernel that takes the most time is "
                        "the closest-hit traversal: VALU-issue bound on an L2-resident tree (see node_visits_per_ray, lane_utilisation); the HBM "
                        "stage is the fill of the dense outputs + k_cull."})
    return top


def usable_cpus():
    """CPUs this process may run on: its affinity mask, capped by OMP_NUM_THREADS when that is set (os.cpu_count() counts the
    whole host, and a pool sized by it on a share of the host only oversubscribes that share)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def cpu_baseline(mesh, center, extent):
    """the oracle (port of the reference's CPU path: brute-force float32 tracer + float64 PyTorch
    autograd, `BASELINE.json:configs[0]`) on the GPU box's host cores, forward + backward, median of 3:
      (i)  config 1 in full: hand_vh.ply, one view, 256x256;
      (ii) the timed workload's mesh on a one-view 256x256 slice (cost is O(rays x faces): rays/s carries over to 72 x 1024^2).
    `value` is (ii).  For context also a 768x768 slice and the same path with a BVH tracer instead of the brute force."""
    import statistics
    from oracle import diffrender_oracle as orc
    cores = usable_cpus()
    orc.TRACER_THREADS = cores                       # the C tracers use every core ...
    orc.TORCH_THREADS = min(32, cores)               # ... PyTorch's float64 ops do not scale past a few dozen threads (they collapse at 256)
    torch.set_num_threads(orc.TORCH_THREADS)
    rng = np.random.default_rng(0)

    def run(m, c, ext, res, repeats):
        R, K, Rinv, Kinv = views.turntable_cameras(c, ext, 72, res, res)[0]
        o, d = views.generate_ray(res, res, Kinv, Rinv)
        sp = torch.tensor(rng.standard_normal((res * res, 3)) * 40.0 + c)
        valid = torch.ones(res * res, dtype=torch.bool)
        times = []
        for _ in range(repeats):
            V = torch.tensor(m.vertices, dtype=torch.float64, requires_grad=True)
            t0 = time.perf_counter()
            om = orc.Mesh(m.faces, V)
            oo, od, mk = orc.render_transparent(om, o, d, IOR)
            loss = orc.ray_loss(oo, od, mk, sp, valid)
            if loss.requires_grad:
                loss.backward()
            times.append(time.perf_counter() - t0)
        return statistics.median(times), times

    threads = f"brute-force f32 tracer on {cores} threads + f64 autograd on {orc.TORCH_THREADS}"
    hand = mesh_io.read_ply(os.path.join(ROOT, "data", "hand_vh.ply"))
    hc, hext = views.mesh_frame(hand.vertices)
    run(hand, hc, hext, 64, 1)                       # thread pools, first-touch
    t1, _ = run(hand, hc, hext, 256, 3)
    t2, _ = run(mesh, center, extent, 256, 3)
    t3, _ = run(mesh, center, extent, 768, 3)
    # `value`: the 256 x 256 slice BASELINE.md section 3 defines as the baseline of record (kept comparable from round to round).  That
    # slice is dominated by fixed costs (thread pools, autograd set-up: it under-states the CPU path by almost a factor two), so a 768 x 768
    # slice of the same view is reported beside it as `slice_768`.
    out = {"value": round(256 ** 2 / t2 / 1e6, 6), "unit": "M camera-rays/s", "cores": cores, "kind": "port", "baseline_slice": "256x256 (BASELINE.md section 3)",
           "sample": f"oracle ({threads}), 1 view 256x256 of the same {len(mesh.faces)}-triangle mesh, forward+backward, median of 3 ({t2:.3f} s each)",
           "config1": {"value": round(256 ** 2 / t1 / 1e6, 6), "unit": "M camera-rays/s",
                       "sample": f"hand_vh.ply ({len(hand.faces)} triangles), 1 view 256x256 in full, forward+backward, median of 3 ({t1:.3f} s)"},
           "slice_768": {"value": round(768 ** 2 / t3 / 1e6, 6), "unit": "M camera-rays/s", "cores": cores,
                         "sample": f"same mesh and threads, 1 view 768x768, median of 3 ({t3:.2f} s each): the fixed costs of a call amortised"}}
    # context: the same CPU path with a reasonable tracer (oracle/bvh_tracer.c: same contract, median-split BVH instead of the
    # loop over every face, bit-identical hits) on a larger slice -- what a CPU implementation that is not brute force does
    res_b, n_b = 1024, 8
    orc.TRACER_THREADS = orc.TORCH_THREADS = min(64, cores)     # one pool size for both: no resize between the short tracer calls
    torch.set_num_threads(orc.TORCH_THREADS)
    cams = views.turntable_cameras(center, extent, 72, res_b, res_b)
    rays_b = [views.generate_ray(res_b, res_b, cams[9 * k][3], cams[9 * k][2]) for k in range(n_b)]
    sp = torch.tensor(rng.standard_normal((res_b ** 2, 3)) * 40.0 + center)
    valid = torch.ones(res_b ** 2, dtype=torch.bool)
    orc.USE_BVH = True
    try:
        times = []
        for _ in range(2):
            V = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
            t0 = time.perf_counter()
            om = orc.Mesh(mesh.faces, V)
            for o, d in rays_b:
                oo, od, mk = orc.render_transparent(om, o, d, IOR)
                orc.ray_loss(oo, od, mk, sp, valid).backward()
            times.append(time.perf_counter() - t0)
    finally:
        orc.USE_BVH = False
    tb = min(times)
    out["bvh_variant"] = {"value": round(n_b * res_b ** 2 / tb / 1e6, 6), "unit": "M camera-rays/s", "cores": orc.TORCH_THREADS,
                          "sample": f"same oracle with its BVH tracer (bit-identical hits; tree rebuilt per trace call), {n_b} views of "
                                    f"{res_b}x{res_b}, forward+backward, best of 2 ({tb:.2f} s); on {orc.TORCH_THREADS} threads, not the {cores} of `value` "
                                    "(one pool size for tracer and autograd: no pool resize between its short tracer calls)"}
    return out


def regime_roofline(scene, step_fn, kk, n_rays_per_step, verify_every_ray, pmc_mode=None, pmc_workload=None, n_faces=0, n_views=0):
    """A regime's own roofline row (the `establish_mode` / `tight_framing` keys of the line): `kk` untimed steps with every stage's hipEvent
    pairs on, then one step in statistics mode.  The closest-hit traversal is priced like the headline's (VALU issue; wave-instructions from
    the wave-steps counted live x the static instruction counts of a wave-step, since profiles/pmc.json holds the headline workload's
    counters only); the stage that reads every ray (`k_cull`, when nothing is trusted) against HBM: 48 B ray + 8 B key per camera ray."""
    om = scene.optix_mesh
    om.profile_select(None)
    om.profile_enable(1); om.profile_read()
    for _ in range(kk):
        step_fn()
    pr = om.profile_read()
    om.profile_enable(2)
    step_fn()
    pr2 = om.profile_read()
    ts = om.trace_stats()
    # ... and `kk` steps with the two internal pipelines serialised on one stream: every kernel with the GPU to itself
    prefill, Render.PREFILL_NEXT = Render.PREFILL_NEXT, False
    om.profile_enable(3)
    step_fn()
    om.profile_read()
    for _ in range(kk):
        step_fn()
    pa = om.profile_read()
    Render.PREFILL_NEXT = prefill
    om.profile_enable(0)
    alone = {k: ms / kk for k, (ms, l, it) in pa.items() if l}
    stages = {k: {"ms_per_step": round(ms / kk, 4), "avg_launch_ms": round(ms / l, 4), "launches_per_step": round(l / kk, 2), "items_per_launch": it // l}
              for k, (ms, l, it) in pr.items() if l}
    rows = {}
    ws, ls, lf, mx = ts.get("trace2", (0, 0, 0, 0))
    if ws and "trace2" in stages and pr2["trace2"][1]:
        l2 = pr2["trace2"][1]
        est = (ws - lf) / l2 * VALU_PER_INNER_STEP + lf / l2 * VALU_PER_LEAF_STEP
        t = stages["trace2"]["avg_launch_ms"] * 1e-3
        rows["k_trace<closest>"] = {"kernel": "k_trace<closest>", "bound": "valu-issue", "unit": "G wave-instr/s", "peak": round(VALU_PEAK / 1e9, 1),
                                    "avg_launch_ms": stages["trace2"]["avg_launch_ms"], "ms_per_step": stages["trace2"]["ms_per_step"],
                                    "achieved": round(est / t / 1e9, 1), "frac": round(est / t / VALU_PEAK, 4), "traffic": None,
                                    "valu_instr_per_launch_est": int(est), "node_visits_per_ray": round(ls / max(1, pr2["trace2"][2]), 2),
                                    "lane_utilisation": round(ls / (64.0 * ws), 3),
                                    "frac_source": f"wave-steps counted live x ({VALU_PER_INNER_STEP} VALU per inner visit, {VALU_PER_LEAF_STEP} per leaf visit)"}
        if alone.get("trace2"):
            ta = alone["trace2"] / max(1.0, stages["trace2"]["launches_per_step"]) * 1e-3
            rows["k_trace<closest>"]["alone"] = {"avg_launch_ms": round(ta * 1e3, 4), "achieved": round(est / ta / 1e9, 1), "frac": round(est / ta / VALU_PEAK, 4)}
    if verify_every_ray and "cull" in stages:
        h0 = pr["shade1"][2] / kk
        b = 56.0 * n_rays_per_step + 36.0 * h0
        t = stages["cull"]["ms_per_step"] * 1e-3
        rows["k_cull"] = {"kernel": "k_cull (every ray loaded and verified)", "bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "ms_per_step": stages["cull"]["ms_per_step"],
                          "achieved": round(b / t / 1e9, 1), "frac": round(b / t / 1e9 / HBM_PEAK_GBS, 4), "traffic": None, "alg_bytes_per_step": int(b)}
        if alone.get("cull"):
            rows["k_cull"]["alone"] = {"ms_per_step": round(alone["cull"], 4), "achieved": round(b / (alone["cull"] * 1e-3) / 1e9, 1),
                                       "frac": round(b / (alone["cull"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    proj = None
    if pmc_mode:
        # this regime's own counters (profiles/pmc.json[pmc_mode], collected by tools/final_runs.sh on the same kernel sources): HBM traffic of
        # the traversal launch and of the projection pass, and the closest-hit kernel priced with its own SQ_INSTS_VALU
        pmc, prov = _pmc(pmc_mode, pmc_workload)
        fresh = bool(pmc) and not prov["stale"]
        rec = max((pmc[q] for q in PMC_NAMES["k_trace<closest>"] if q in pmc), key=lambda r: r.get("launches", 0), default=None) if fresh else None
        if rec and "k_trace<closest>" in rows:
            r = rows["k_trace<closest>"]
            r["traffic"] = rec.get("hbm_bytes_per_launch")
            if rec.get("SQ_INSTS_VALU"):
                t = r["avg_launch_ms"] * 1e-3
                r.update(achieved=round(rec["SQ_INSTS_VALU"] / t / 1e9, 1), frac=round(rec["SQ_INSTS_VALU"] / t / VALU_PEAK, 4), valu_instr_per_launch=int(rec["SQ_INSTS_VALU"]),
                         frac_source=f"rocprofv3 SQ_INSTS_VALU (profiles/pmc.json[{pmc_mode}], same kernel sources)")
                if rec.get("SQ_THREAD_CYCLES_VALU") and rec.get("SQ_ACTIVE_INST_VALU"):
                    r["valu_lanes_useful"] = round(rec["SQ_THREAD_CYCLES_VALU"] / (64 * rec["SQ_ACTIVE_INST_VALU"]), 3)
        if "raster" in stages:
            h0 = pr["shade1"][2] / kk
            proj = projection_pass(pmc, fresh, stages["raster"]["launches_per_step"], 48.0 * n_faces * n_views + 40.0 * h0)
    dom = max(rows, key=lambda k: rows[k]["ms_per_step"]) if rows else None
    return {"roofline": dict(rows[dom], others={k: v for k, v in rows.items() if k != dom}) if dom else None, "projection_pass": proj,
            "stages_ms_per_step": {k: v["ms_per_step"] for k, v in stages.items()},
            "stages_alone_ms_per_step": {k: round(v, 4) for k, v in alone.items()}}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """Write every array as `dirname/<name>.npy` in float64.  If the set would take more than `limit` bytes, every array of more
    than one row is cut to the same fraction of its rows, chosen by a fixed seed: the same rows in every run with the same arguments."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > limit and a.ndim > 0 and len(a) > 1:
            keep = max(1, int(len(a) * (limit - (1 << 16)) / total))       # (64 KiB left for the .npy headers and the one-row arrays)
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", choices=["dropin", "fused"], default="dropin")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--mesh", default="horse")
    ap.add_argument("--no-grid-cache", action="store_true",
                    help="diffrender.GRID_CACHE = False for the whole run (every call fits and verifies every image again: the `establish_mode` extra as the main line, for its stage table)")
    ap.add_argument("--distance-factor", type=float, default=2.5,
                    help="camera distance in mesh extents (views.turntable_cameras; 2.5 = SURVEY 8d's framing, the headline; 1.1 = the object fills the image: for stage tables of that case)")
    ap.add_argument("--subdiv", type=int, default=None, help="midpoint subdivisions of the input hull (default: 1 for horse/mouse)")
    ap.add_argument("--batch-views", type=int, default=0,
                    help="views concatenated into one render_transparent call (0 = all local views; 1 = the reference's per-view loop)")
    ap.add_argument("--graph", type=int, default=-1,
                    help="1: capture the whole step (rebuild, pipelines, autograd, all-reduce, SGD) in a HIP graph and replay it; 0: eager; "
                         "-1 (default): graph when N > 1 AND the rank's share is below 24 views x 1024^2 camera rays (a chain of small launches: "
                         "9 views 0.655 vs 0.691 ms eager, 18 views 0.792 vs 0.819; above, the eager step is the faster one: 36 views 1.177 vs 1.204) "
                         "-- eager otherwise; falls back to eager if the capture fails")
    ap.add_argument("--repeats", type=int, default=int(os.environ.get("DRT_BENCH_REPEATS", "1")),
                    help="the timed region (exactly --steps steps between two barrier + synchronize pairs) is run this many times back to back, "
                         "and `value` / `ms_per_step` are those of the median repeat.  1 (default): one region, exactly --steps timed steps.  "
                         "0: SUSTAINED mode -- at least 5 repeats and as many as it takes for --min-seconds of timed steps; `value` / "
                         "`ms_per_step` are then those of the median repeat among the ones that STARTED after the first --settle-seconds of timed "
                         "steps (the chip's clocks settle over the first few hundred milliseconds of sustained load), the first repeat's figure "
                         "is reported beside it.  (--full with R > 0 runs a sustained measurement after the headline and reports it as `sustained`)")
    ap.add_argument("--min-seconds", type=float, default=float(os.environ.get("DRT_BENCH_MIN_SECONDS", "3.0")),
                    help="sustained mode: total length of the timed regions (s)")
    ap.add_argument("--settle-seconds", type=float, default=1.0, help="sustained mode: repeats that start before this much timed time has passed do not count for `value`")
    ap.add_argument("--reset-every", type=int, default=50,
                    help="the parameter and the momentum buffer are put back to their initial state once this many steps (untimed ones included) were "
                         "taken since the last reset -- between two repeats, or inside a longer timed region as two in-place fills enqueued in front of "
                         "the next step (timed with it, no drain) -- so that a long "
                         "run stays within the first iterations of a pass (BASELINE.json: 200 iterations per pass) instead of timing whatever mesh 2 000 "
                         "steps of descent on synthetic targets produce.  50: the float64 atomics of the gradient sums differ in the last bits from run to "
                         "run, and this descent amplifies that (two runs 8e-13 apart after 70 steps from the same state, 3e-3 after 130), so a shorter "
                         "horizon keeps the last step's outputs (--dump-outputs) equal to rounding from run to run; 0 = never")
    ap.add_argument("--bind", type=int, default=1,
                    help="1 (default): the views' rays and targets are handed to the scene ONCE (scene.bind_rays -> diffrender.RayBinding) and every step "
                         "renders through the handle: trusted grids and recycled outputs by contract; 0: the drop-in signature render_transparent(origin, "
                         "ray_dir) on the same tensors every step, which reaches the same kernels through tensor-identity heuristics and torch's storage use counts")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the line can carry: the sustained measurement, the roofline and per-stage tables, "
                         "the fused / establish / tight-framing / route-B extras, the drop-in vs fused loss check, the CPU baseline.  "
                         "Off by default: a plain run does only what `value` and `ms_per_step` need")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned -- the loss of all views, the parameter after the "
                         "optimiser step and the gradient it applied -- as DIR/<name>.npy (float64; a fixed, seeded sample of the rows above "
                         f"{DUMP_LIMIT_BYTES >> 20} MB in all).  The inputs are identical from run to run with the same arguments")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the extras after the timed region (sustained measurement, fused-mode comparison, traversal "
                         "statistics); the roofline and stage tables are still taken")
    ap.add_argument("--displaced-targets", action="store_true", help="targets from a noise-displaced hull even when data/<mesh>_scan.ply exists")
    ap.add_argument("--random-targets", action="store_true",
                    help="skip the ground-truth render of the setup (targets = random points); used for PMC passes so that every "
                         "traced kernel dispatch belongs to a step")
    args = ap.parse_args()

    rank, local_rank, world = ddist.init()
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run --nproc-per-node N")
        args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU fallback"
    if local_rank >= torch.cuda.device_count():
        # more ranks than GPUs: only for functional checks of the multi-rank path on one GPU (DRT_DIST_BACKEND=gloo)
        assert os.environ.get("DRT_DIST_BACKEND") == "gloo", "one rank per GPU"
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    mesh, mesh_src = load_workload(args.mesh, args.subdiv)
    n_faces, n_verts = len(mesh.faces), len(mesh.vertices)
    center, extent = views.mesh_frame(mesh.vertices)
    res = args.res
    P = res * res
    Render.intIOR = IOR
    Render.resx = Render.resy = res
    if args.no_grid_cache:
        Render.GRID_CACHE = False

    # ---- synthetic capture (untimed): targets from a displaced ground-truth mesh through the same path
    scene = Render.Scene(mesh, local_rank)
    # targets: the scanned object traced through the same path; meshes without a scan in data/ use a
    # noise-displaced copy of the hull
    scan_path = os.path.join(ROOT, "data", f"{args.mesh}_scan.ply")
    if os.path.exists(scan_path) and not args.displaced_targets:
        gt, target_src = mesh_io.read_ply(scan_path), f"{args.mesh}_scan.ply"
    else:
        gt, target_src = views.displaced_ground_truth(mesh, sigma=0.3, seed=0), "hull displaced along vertex normals, sigma 0.3"
    gt_scene = Render.Scene(gt, local_rank)
    my_views = ddist.shard_views(args.views, rank, world)
    cams = views.turntable_cameras(center, extent, args.views, res, res, distance_factor=args.distance_factor)
    data = []
    with torch.no_grad():
        for k in my_views:
            o, d = views.generate_ray(res, res, cams[k][3], cams[k][2], device=dev)
            if args.random_targets:
                gen = torch.Generator(device=dev).manual_seed(k)
                sp = torch.randn(o.shape, dtype=torch.float64, device=dev, generator=gen) * 40.0 + torch.tensor(center, device=dev)
                sp = sp * (torch.rand(P, device=dev, generator=gen) < 0.05).unsqueeze(1)
            else:
                oo, od, mk = gt_scene.render_transparent(o, d)
                sp = views.screen_targets(oo, od, mk, cams[k], center, extent)
            data.append((sp.contiguous(), (sp[:, 0] != 0).contiguous(), o, d))
    del gt_scene
    valid_frac = float(np.mean([v.float().mean().item() for _, v, _, _ in data]))
    # render_transparent takes any ray set: concatenating views into one call keeps every CU busy
    # (one 1024x1024 view of this object has only ~1.3k wavefronts that hit anything)
    bv = args.batch_views if args.batch_views > 0 else len(data)
    data = [tuple(torch.cat([v[j] for v in data[i:i + bv]]).contiguous() for j in range(4)) for i in range(0, len(data), bv)]
    torch.cuda.empty_cache()

    from drt_amd import optim as O
    init_vertices, parameter, opt = O.setup_opt(scene, 0.1, O.HyperParams, hook=False, fused=True)    # reference optim.py:164-171; limit_hook + SGD in one kernel
    limit_hook = O.limit_hook
    w_ray = O.loss_weights(O.HyperParams, res, scene.mean_len)[0]     # 40 * 217.5 / res^2 (reference optim.py:127, config.py defaults)
    local_views = [(sp, valid, scene.bind_rays(o, d, sp, valid)) if args.bind else (sp, valid, o, d) for sp, valid, o, d in data]

    def step(record):
        """drt_amd.optim.full_batch_step: rebuild, every local view's render_transparent + ray_loss, backward, ONE
        all-reduce of grad[V,3], limit_hook, SGD(nesterov) -- the same function the 2-rank tests run."""
        return O.full_batch_step(scene, local_views, init_vertices, parameter, opt, w_ray, fused=args.mode == "fused")

    if args.graph < 0:
        # Measured per share on one GPU (profiles/r05_scaling_proxy.txt; r03 / r04 for the history).  Since round 5 a capture takes a pooled
        # output set for good (diffrender `graph_set`: replay = recycle, no dense fill inside the graph), so eager and replayed steps do the
        # same GPU work and differ by the host's enqueue and the gaps between ~60 dependent launches: the replay wins where the step is a chain
        # of small launches (9 views: 0.655 vs 0.691 ms; 18: 0.792 vs 0.819) and loses where the two pipelines' overlap matters more than the
        # launch gaps (36 views: 1.204 vs 1.177; 72: 1.83 vs 1.79).  So: a graph for shares below 24 views x 1024^2 rays.
        # (Not over gloo -- the functional two-ranks-on-one-GPU check: its all-reduce goes through the host and cannot be captured.)
        small = len(my_views) * P < (3 << 23)
        args.graph = 1 if world > 1 and small and os.environ.get("DRT_BENCH_GRAPH", "1") != "0" and os.environ.get("DRT_DIST_BACKEND") != "gloo" else 0
    graph = None
    untimed = 0                                      # steps taken before the timed region, each of them an optimiser step (--reset-every counts them)
    if args.graph:
        # The step has no host-side data dependence (every list size lives on the device), so it can be
        # captured once and replayed: one graph launch per step instead of ~60 kernel launches.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(3, args.warmup)):
                step(False)
                untimed += 1
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):      # (the process group's watchdog thread may query events meanwhile)
                static_loss = step(False)
            graph.replay()
            untimed += 1                             # (the capture itself runs nothing; its first replay is a step)
            torch.cuda.synchronize()
            ok = torch.tensor([1.0], device=dev)
        except Exception as e:                      # (a capture that fails must fail on every rank alike: the ranks agree below)
            print(f"[bench] rank {rank}: whole-step graph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr, flush=True)
            graph = None
            ok = torch.tensor([0.0], device=dev)
        if world > 1:
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
        if ok.item() == 0.0:
            graph, args.graph = None, 0
    if graph is not None:
        run = lambda: (graph.replay(), static_loss)[1]
    else:
        run = lambda: step(True)
    # at least three untimed steps whatever --warmup says: the first call on a capture's ray tensors ESTABLISHES the grid verdict, the second
    # reads it back (one host sync per ray tensor, ever), and the caching allocator has its steady set of blocks from the third on
    for _ in range(max(args.warmup, 3)):
        untimed += 1
        loss = run()     # (held like in the timed loop: the previous step's loss keeps its autograd nodes -- and the face-id / path-list arrays they
                         #  reference -- alive while the next step allocates, so the caching allocator must see THAT pattern before the timed region:
                         #  a first hipMalloc of a 1.8 GB block inside it costs 30 ms on a box whose driver clears the memory first)
    # N = 1, --full: the per-kernel hipEvent pairs are recorded live inside the timed region (the roofline contract).  N > 1: they
    # are recorded in an eager repeat right after it, so that ~120 event records per step do not sit in a 1.7 ms step.
    live_profile = args.full and not args.graph and world == 1 and not os.environ.get('DRT_BENCH_NOPROF')
    # the launches of the kernel the roofline is about (k_trace<closest> on the refracted rays: the closest-hit launch on rays outside the grid
    # is not even issued when every ray is a verified grid ray).  Every event pair is a stream marker that keeps the next kernel from
    # starting under the previous one's tail (~8 us each): with the occlusion launches and the empty first-traversal stage timed live too,
    # 12 records per step cost 0.1 ms of a 2.4 ms step; those rows come from the repeat below like every other stage.
    LIVE = ("trace2",)
    if live_profile:
        scene.optix_mesh.profile_select(LIVE)   # hipEvent pairs around the traversal kernels only (the other stages are
        scene.optix_mesh.profile_enable(True)   # timed in the repeat below: ~50 more event records per step cost 0.15 ms of 3.3)
        scene.optix_mesh.profile_read()

    def timed_region(n_repeats, since_reset):
        """The timed region -- exactly K steps between two (barrier, synchronize) pairs, max over ranks -- run `n_repeats` times back to
        back (0: sustained mode, see --repeats); `elapsed` is the MEDIAN repeat's, every repeat is listed.  `loss` is rebound every step like
        in the warm-up: the previous step's loss (and what its autograd nodes reference) lives while the next step allocates.
        Every --reset-every steps (untimed ones included) parameter and momentum go back to their initial state -- between two repeats
        (untimed), or inside a region longer than that: there two in-place fills on the compute stream, ordered like the optimiser's own
        in-place update and timed with the step (no drain) -- so that a run of any length times the first iterations of a pass, and its
        last step starts at most --reset-every steps after a state that is the same in every run."""
        nonlocal loss
        repeats, starts = [], []                     # (seconds, host enqueue ms per step) of each repeat; timed seconds in front of it
        sustained = n_repeats <= 0
        timed_total, n_resets = 0.0, 0

        def reset():
            # (in place, so that a captured graph sees it too: momentum buffer 0 = a first step)
            nonlocal since_reset, n_resets
            with torch.no_grad():
                parameter.zero_()
                if getattr(opt, "buf", None) is not None:
                    opt.buf.zero_()
            since_reset, n_resets = 0, n_resets + 1
        while True:
            rep = len(repeats)
            if (not sustained and rep >= n_repeats) or (sustained and rep >= 5 and timed_total >= args.min_seconds) or rep >= 2000:
                break
            if args.reset_every > 0 and since_reset + args.steps > args.reset_every and rep > 0:
                reset()                              # (untimed, between two regions)
            if live_profile:
                scene.optix_mesh.profile_read()          # (drops the event pairs of the previous repeat: the stage rows are the last repeat's)
            ddist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_ms = []
            for _ in range(args.steps):
                ts = time.perf_counter()
                if args.reset_every > 0 and since_reset >= args.reset_every:
                    reset()                          # (a region longer than --reset-every; every rank at the same step)
                loss = run()
                since_reset += 1
                host_ms.append(1e3 * (time.perf_counter() - ts))
                if os.environ.get("DRT_BENCH_ALLOC_TRACE"):
                    m = torch.cuda.memory_stats(dev)
                    print("step", len(host_ms), "device_alloc", m["num_device_alloc"], "reserved_GB", round(m["reserved_bytes.all.current"] / 2 ** 30, 3),
                          "active_GB", round(m["active_bytes.all.current"] / 2 ** 30, 3), "peak_active_GB", round(m["active_bytes.all.peak"] / 2 ** 30, 3), file=sys.stderr, flush=True)
            ddist.barrier()
            torch.cuda.synchronize()
            repeats.append((ddist.allreduce_max_float(time.perf_counter() - t0, dev), host_ms))
            starts.append(timed_total)
            timed_total += repeats[-1][0]                # (the max over ranks: every rank takes the same number of repeats)
        counted = [k for k in range(len(repeats)) if sustained and starts[k] >= args.settle_seconds] or list(range(len(repeats)))
        order = sorted(counted, key=lambda k: repeats[k][0])
        elapsed, host_ms = repeats[order[(len(order) - 1) // 2]]      # the median repeat (the lower one of an even count) among the counted ones
        summary = {"n": len(repeats), "reported": f"median of the {len(counted)} repeats that started after {args.settle_seconds} s of timed steps" if sustained and len(counted) < len(repeats) else "median",
                   "ms_per_step": [round(1e3 * t / args.steps, 3) for t, _ in repeats],
                   "min": round(1e3 * min(repeats[k][0] for k in counted) / args.steps, 3), "median": round(1e3 * elapsed / args.steps, 3),
                   "max": round(1e3 * max(repeats[k][0] for k in counted) / args.steps, 3), "timed_region_ms_total": round(1e3 * sum(t for t, _ in repeats), 1),
                   "first_repeat": round(1e3 * repeats[0][0] / args.steps, 3), "sustained": sustained, "n_counted": len(counted),
                   # the plateau, visibly: median ms/step of the repeats that started within each successive half second of timed steps
                   "by_half_second": [round(1e3 * sorted(repeats[k][0] for k in ks)[(len(ks) - 1) // 2] / args.steps, 3)
                                      for ks in ([k for k in range(len(repeats)) if int(starts[k] / 0.5) == b] for b in range(int(timed_total / 0.5) + 1)) if ks],
                   "parameter_resets": n_resets, "reset_every_steps": args.reset_every}
        return elapsed, host_ms, summary, since_reset

    ms0 = torch.cuda.memory_stats(dev)
    elapsed, host_ms, repeats_summary, since_reset = timed_region(args.repeats, untimed)
    ms1 = torch.cuda.memory_stats(dev)
    final_loss = float(ddist.allreduce_sum_(loss.detach().clone().reshape(1).double()).item())     # (summed over the ranks: the loss of all views)
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller: the loss, the parameter it updated in place, the gradient it applied (identical on every rank)
        dump_outputs(args.dump_outputs, {"loss": np.array([final_loss]), "parameter": parameter.detach().cpu().numpy(),
                                         "grad": parameter.grad.detach().cpu().numpy()})
    # the host's own pace (enqueue only): a step whose enqueue takes as long as the step itself means the host, not the GPU, set the time
    # device-level allocator traffic inside the timed region (a hipMalloc / hipFree there would be a host-side stall of milliseconds)
    alloc_stats = {k: int(ms1.get(k, 0) - ms0.get(k, 0)) for k in ("num_device_alloc", "num_device_free", "num_alloc_retries")}
    alloc_stats["reserved_GB"] = round(ms1.get("reserved_bytes.all.current", 0) / 2 ** 30, 2)
    alloc_stats["host_enqueue_ms_per_step"] = {"median": round(sorted(host_ms)[len(host_ms) // 2], 3), "max": round(max(host_ms), 3)}

    total_rays = args.views * P * args.steps
    value = total_rays / elapsed / 1e6
    out = {
        "metric": "M camera-rays/s (forward+backward) on 50k-tri mesh, 72 views",
        "value": round(value, 3), "unit": "M camera-rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "strong",
        "repeats": repeats_summary,
        "vs_baseline": None, "dtype": "f32 traversal + f64 shading/gradients", "data": "synthetic",
        "config": {"workload": f"{mesh_src} = {n_faces} tris / {n_verts} verts, {args.views} turntable views, "
                               f"{res}x{res} rays/view, LBVH rebuilt every step, forward+ray_loss+backward+all-reduce+SGD"
                               + ("" if args.distance_factor == 2.5 else f", cameras at {args.distance_factor} extents")
                               + (", no grid verdict cache" if args.no_grid_cache else ""),
                   "targets": "random" if args.random_targets else target_src, "mode": args.mode, "hip_graph": bool(args.graph), "outputs_recycled": bool(args.mode == "dropin" and (args.bind or (Render.RECYCLE_OUTPUTS and P * len(my_views) >= Render.RECYCLE_MIN_RAYS and (not args.graph or Render.cache_report().get("recycle_graph_set", 0) > 0)))), "ray_binding": bool(args.bind), "views_per_gpu": len(my_views), "views_per_call": min(bv, len(my_views)), "ior": IOR, "valid_pixel_fraction": round(valid_frac, 4), "untimed_steps": untimed, "allocator_in_timed_region": alloc_stats,
                   "final_loss": final_loss},
    }
    if args.full and not args.no_extras and args.repeats > 0:
        # the sustained measurement (--repeats 0) after the headline: >= --min-seconds of timed steps, the median of the repeats after the clocks settled
        s_elapsed, _, s_summary, since_reset = timed_region(0, since_reset)
        out["sustained"] = {"value": round(total_rays / s_elapsed / 1e6, 3), "ms_per_step": round(1e3 * s_elapsed / args.steps, 3), "repeats": s_summary}
    # N > 1: what the line says about the exchange itself, so that the first run on a multi-GPU node explains itself -- the process group as
    # torch.distributed sees it, and the step's one all-reduce (grad[V,3] float64) timed alone on every rank, after the timed region
    if world > 1 or os.environ.get("DRT_DIST_FORCE", "") not in ("", "0"):
        import torch.distributed as tdist
        g_probe = torch.zeros_like(parameter)
        for _ in range(3):
            ddist.allreduce_sum_(g_probe)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ddist.barrier(); torch.cuda.synchronize()
        n_ar = 20
        ev[0].record()
        for _ in range(n_ar):
            ddist.allreduce_sum_(g_probe)
        ev[1].record()
        torch.cuda.synchronize()
        mine = torch.tensor([ev[0].elapsed_time(ev[1]) / n_ar, float(len(my_views)), float(torch.cuda.current_device())], dtype=torch.float64, device=dev)
        per_rank = [torch.zeros_like(mine) for _ in range(world)]
        if tdist.is_initialized() and world > 1:
            tdist.all_gather(per_rank, mine)
        else:
            per_rank = [mine]
        try:
            nccl_ver = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception:
            nccl_ver = None
        out["multi_gpu"] = {
            "backend": tdist.get_backend() if tdist.is_initialized() else None, "world_size_seen_by_torch_distributed": tdist.get_world_size() if tdist.is_initialized() else 1,
            "rccl_version": nccl_ver, "visible_devices": torch.cuda.device_count(), "partition": "view k -> rank k mod world; no data-path collective but ONE all-reduce(sum) of grad[V,3] float64 per step",
            "allreduce_bytes": int(parameter.numel() * 8),
            "allreduce_ms_per_rank": [round(float(t[0]), 4) for t in per_rank], "views_per_rank": [int(t[1]) for t in per_rank], "device_of_rank": [int(t[2]) for t in per_rank],
            "allreduce_share_of_step": round(max(float(t[0]) for t in per_rank) / (1e3 * elapsed / args.steps), 4),
            "note": "the all-reduce figure is the collective alone (20 back-to-back calls after the timed region); inside the step it is one launch in the chain",
        }
    prof_live = scene.optix_mesh.profile_read() if live_profile else None
    if live_profile:
        scene.optix_mesh.profile_select(None)
    # everything below is --full only.  The two modes at ONE parameter state (no optimiser step in between): same loss to rounding, or one
    # of them is wrong
    loss_check = None
    if args.full and not args.graph:
        scene.optix_mesh.profile_enable(0)
        opt.zero_grad(set_to_none=True)
        l_drop = float(O.local_loss_backward(scene, local_views, init_vertices, parameter, w_ray, fused=False).item())
        g_drop = parameter.grad.clone() if parameter.grad is not None else None
        opt.zero_grad(set_to_none=True)
        l_fus = float(O.local_loss_backward(scene, local_views, init_vertices, parameter, w_ray, fused=True).item())
        g_fus = parameter.grad.clone() if parameter.grad is not None else None
        opt.zero_grad(set_to_none=True)
        rel = abs(l_drop - l_fus) / max(abs(l_drop), 1e-300)
        g_rel = float(((g_drop - g_fus).abs().max() / g_drop.abs().max().clamp_min(1e-300)).item()) if g_drop is not None and g_fus is not None else None
        loss_check = {"final_loss_dropin": l_drop, "final_loss_fused": l_fus, "rel_diff": rel, "grad_max_rel_diff": g_rel}
        assert rel <= 1e-10, f"drop-in and fused losses disagree at the same parameters: {loss_check}"
        assert g_rel is None or g_rel <= 1e-9, f"drop-in and fused gradients disagree at the same parameters: {loss_check}"
        out["config"]["loss_check"] = loss_check
        if live_profile:
            scene.optix_mesh.profile_enable(True)
            scene.optix_mesh.profile_read()
    fused_extra = None
    if args.full and args.mode == "dropin" and not args.graph and not args.no_extras:   # (N = 1 and N > 1 alike)
        # same K steps through the one-pass API (Scene.ray_loss_fused: no dense out_ori/out_dir/mask, rays of
        # pixels without a target dropped before tracing) -- reported next to the headline, never as `value`
        def fused_step():
            O.full_batch_step(scene, local_views, init_vertices, parameter, opt, w_ray, fused=True)
        scene.optix_mesh.profile_enable(0)
        fused_step()
        ddist.barrier(); torch.cuda.synchronize()
        tf = time.perf_counter()
        for _ in range(args.steps):
            fused_step()
        ddist.barrier(); torch.cuda.synchronize()
        tf = ddist.allreduce_max_float(time.perf_counter() - tf, dev)
        fused_extra = {"M_rays_per_s": round(total_rays / tf / 1e6, 3), "ms_per_step": round(1e3 * tf / args.steps, 3),
                       "alg_bytes_per_ray": 73, "api": "Scene.ray_loss_fused (render_transparent + ray_loss + backward in one pass)"}
        scene.optix_mesh.profile_enable(1)
        scene.optix_mesh.profile_read()
    establish_extra = tight_extra = None
    if args.full and args.mode == "dropin" and not args.graph and not args.no_extras:
        # (a) the same steps WITHOUT the verdict cache: every call fits the image models and verifies every single ray again, as a caller
        #     does whose capture layer hands out fresh ray tensors per call (the reference's Data.get_view, captured_data.py:44-59)
        scene.optix_mesh.profile_enable(0)
        Render.GRID_CACHE = False
        try:
            for _ in range(2):
                step(False)
            ke = min(args.steps, 20)
            te = float("inf")
            for _ in range(2):            # (best of two: an extra is a description of the mode, not the contract's timed region)
                ddist.barrier(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(ke):
                    step(False)
                ddist.barrier(); torch.cuda.synchronize()
                te = min(te, ddist.allreduce_max_float(time.perf_counter() - t0, dev))
            est_roof = regime_roofline(scene, lambda: step(False), min(ke, 5), len(my_views) * P, True)
        finally:
            Render.GRID_CACHE = True
        establish_extra = {"M_rays_per_s": round(args.views * P * ke / te / 1e6, 3), "ms_per_step": round(1e3 * te / ke, 3), "steps": ke, "repeats": "best of 2", **est_roof,
                           "what": "diffrender.GRID_CACHE = False: no trusted-grid shortcut -- every ray of every image is loaded and verified against the fitted pinhole model in every call"}
        # (b) tight framing: the same mesh seen from 1.1 extents instead of 2.5 (the object fills the image: primary hit fraction 0.2-0.4 instead of 0.04)
        cams_t = views.turntable_cameras(center, extent, args.views, res, res, distance_factor=float(os.environ.get("DRT_TIGHT_FACTOR", "1.1")))
        gt_t = Render.Scene(gt, local_rank)
        tv = []
        with torch.no_grad():
            for k in my_views:
                o, d = views.generate_ray(res, res, cams_t[k][3], cams_t[k][2], device=dev)
                oo, od, mk = gt_t.render_transparent(o, d)
                sp = views.screen_targets(oo, od, mk, cams_t[k], center, extent)
                tv.append((sp.contiguous(), (sp[:, 0] != 0).contiguous(), o, d))
        del gt_t
        tight_views = [tuple(torch.cat([v[j] for v in tv[i:i + bv]]).contiguous() for j in range(4)) for i in range(0, len(tv), bv)]
        if args.bind:
            tight_views = [(sp, valid, scene.bind_rays(o, d, sp, valid)) for sp, valid, o, d in tight_views]
        del tv
        torch.cuda.empty_cache()

        def tight_step():
            return O.full_batch_step(scene, tight_views, init_vertices, parameter, opt, w_ray, fused=False)
        for _ in range(6):            # (establish + read back the verdict of the new ray tensors, grow the lists to this hit fraction, settle the allocator)
            lt = tight_step()
        scene.optix_mesh.profile_enable(1); scene.optix_mesh.profile_read()
        tight_step()
        pt = scene.optix_mesh.profile_read()
        scene.optix_mesh.profile_enable(0)
        kt = min(args.steps, 10)
        tt = float("inf")
        for _ in range(2):                # (best of two, as above)
            ddist.barrier(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(kt):
                lt = tight_step()
            ddist.barrier(); torch.cuda.synchronize()
            tt = min(tt, ddist.allreduce_max_float(time.perf_counter() - t0, dev))
        hits_t = pt["shade1"][2]
        tight_roof = regime_roofline(scene, tight_step, min(kt, 5), len(my_views) * P, False, pmc_mode="tight",
                                     pmc_workload=f"{args.mesh} res {args.res} views {len(my_views)} streams default, cameras at {os.environ.get('DRT_TIGHT_FACTOR', '1.1')} extents",
                                     n_faces=n_faces, n_views=len(my_views))
        tight_extra = {"M_rays_per_s": round(args.views * P * kt / tt / 1e6, 3), "ms_per_step": round(1e3 * tt / kt, 3), "steps": kt, "repeats": "best of 2", **tight_roof,
                       "primary_hit_fraction": round(hits_t / (len(my_views) * P), 4), "M_paths_per_s": round(hits_t * world / (tt / kt) / 1e6, 1),
                       "exit_rays_per_step_per_gpu": int(pt["trace3"][2]),
                       "what": f"turntable_cameras(distance_factor={os.environ.get('DRT_TIGHT_FACTOR', '1.1')}): same mesh, same step, the object fills the frame"}
        del tight_views
        torch.cuda.empty_cache()
        scene.optix_mesh.profile_enable(1)
        scene.optix_mesh.profile_read()
    route_b = None
    if args.full and rank == 0 and world == 1 and not args.no_extras and args.mode == "dropin":
        # INTEGRATION.md route B: the reference's own DiffRender structure -- Dintersect / refract_ray / trace2 as float64
        # torch ops with autograd, the occlusion query, boolean-mask compaction between the steps -- on top of the HIP tracer
        # class only (drt_intersect behind optix_mesh.intersect), one view per call like the reference's loop.
        o1, d1 = data[0][2][:P].contiguous(), data[0][3][:P].contiguous()
        sp1, va1 = data[0][0][:P].contiguous(), data[0][1][:P].contiguous()

        def route_b_view():
            verts = (init_vertices + parameter).detach().requires_grad_(True)
            scene.update_verticex(verts)
            out = scene.trace2(Render.Ray(o1, d1))
            _, occluded = scene.optix_intersect(out)
            keep = torch.logical_not(occluded)
            idx = out.ray_ind[keep]
            target = sp1[idx] - out.origin[keep].detach()
            target = target / target.norm(dim=1, keepdim=True)
            vm = va1[idx]
            loss = (out.direction[keep] - target)[vm].pow(2).sum()
            loss.backward()
            return loss

        for _ in range(2):
            route_b_view()
        torch.cuda.synchronize()
        tb = time.perf_counter()
        nb = 10
        for _ in range(nb):
            route_b_view()
        torch.cuda.synchronize()
        tb = (time.perf_counter() - tb) / nb
        route_b = {"M_rays_per_s": round(P / tb / 1e6, 3), "ms_per_view": round(1e3 * tb, 3),
                   "what": f"one {res}x{res} view per call: update_vert + Scene.trace2 (stepwise float64 torch ops, autograd) + occlusion query + ray loss + "
                           "backward, all traversals through optix_mesh.intersect (drt_intersect) -- the reference's DiffRender.py shape on the HIP tracer"}
    # every stage's event pairs: the same K steps repeated eagerly right after the timed region (same kernels, same inputs, same
    # launch streams).  N = 1: the traversal kernels' rows are then replaced by the ones recorded live INSIDE the timed region;
    # N > 1 and graph replay (no events inside a replayed graph): all rows come from this repeat.
    prof = None
    if args.full:
        scene.optix_mesh.profile_enable(1)
        scene.optix_mesh.profile_read()
        for _ in range(args.steps):
            step(True)
        prof = scene.optix_mesh.profile_read()
        if prof_live:
            prof.update({k: prof_live[k] for k in LIVE if prof_live[k][1] > 0})
    # one extra, untimed step (on every rank: it contains the all-reduce) with the traversal statistics
    # switched on -- they cost contended atomics, so they are kept out of the timed region
    tstats, prof2 = {}, None
    if args.full and not args.no_extras:
        scene.optix_mesh.profile_enable(2)
        step(False)
        prof2 = scene.optix_mesh.profile_read()
        tstats = scene.optix_mesh.trace_stats()
    # and K more untimed steps with the two internal pipelines serialised on one stream (profile level 3): every kernel
    # timed ALONE.  In the timed region the HBM-bound k_cull of one sub-batch overlaps the latency-bound k_trace of the
    # other, which makes the step faster and each of the two kernels look slower.
    prof_iso = None
    if args.full and not args.no_extras:
        # (the next call's out_ori / mask are zeroed beside THIS call's loss + backward kernel by default, diffrender.PREFILL_NEXT: off
        # here, so that the fills and that kernel are each timed with the GPU to themselves like every other stage)
        prefill, Render.PREFILL_NEXT = Render.PREFILL_NEXT, False
        scene.optix_mesh.profile_enable(3)
        step(False)
        scene.optix_mesh.profile_read()
        for _ in range(args.steps):
            step(False)
        prof_iso = scene.optix_mesh.profile_read()
        Render.PREFILL_NEXT = prefill
    if args.full:
        scene.optix_mesh.profile_enable(0)
    if rank == 0 and args.full:
        wave_steps = {k: {"inner": ws - lf, "leaf": lf, "launches": max(1, prof2[k][1])} for k, (ws, ls, lf, mx) in tstats.items() if ws} if prof2 else None
        out["roofline"] = roofline(prof, args, P, len(my_views), n_verts, n_faces, elapsed, world, prof_iso, LIVE if prof_live else None, wave_steps,
                                   recycled=args.mode == "dropin" and not args.graph and (bool(args.bind) or (Render.RECYCLE_OUTPUTS and P * len(my_views) >= Render.RECYCLE_MIN_RAYS)))
        # what the step actually traces: paths that start at a primary hit (every pixel counts in `value`, SURVEY section 8d, but 96 % of
        # the benchmark's pixels see the background)
        h0 = prof["shade1"][2] / max(1, args.steps)
        out["paths"] = {"primary_hits_per_step_per_gpu": int(h0), "primary_hit_fraction": round(h0 / (len(my_views) * P), 4),
                        "M_paths_per_s": round(h0 * world / (elapsed / args.steps) / 1e6, 1),
                        "exit_rays_per_step_per_gpu": int(prof["trace3"][2] / max(1, args.steps))}
        if establish_extra:
            out["establish_mode"] = establish_extra
        if tight_extra:
            out["tight_framing"] = tight_extra
        if tstats.get("trace2", (0,))[0] and "path" in out["roofline"]["stages"] and "trace2" not in out["roofline"]["stages"]:
            tstats["path"] = tstats.pop("trace2")         # (k_path reports in trace2's slot)
        for k, (ws, ls, lf, mx) in tstats.items():
            if ws and k in out["roofline"]["stages"]:
                out["roofline"]["stages"][k].update({"wave_steps": ws, "node_visits_per_ray": round(ls / max(1, prof2[k][2]), 2),
                                                     "lane_utilisation": round(ls / (64.0 * ws), 3), "longest_wave_visits": mx})
        if fused_extra:
            out["fused_mode"] = fused_extra
        if route_b:
            out["route_b"] = route_b
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(mesh, center, extent)
    # RCCL writes its version banner through C stdio, which sits in libc's buffer until exit when stdout is a pipe: every rank
    # flushes it now and rank 0 prints after a barrier, so that the JSON line is the LAST line of the job's stdout
    import ctypes
    ctypes.CDLL(None).fflush(None)
    sys.stdout.flush()
    ddist.barrier()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
