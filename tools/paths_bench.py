#!/usr/bin/env python3
"""Time of one view's refraction term -- forward + loss + backward to the vertex gradient -- under the K-interaction law, by route:

    (a) dense    Scene.render_paths + Render.ray_loss + backward()       (dense outputs, tape fill, finish pass, dense loss gradient)
    (b) one-pass Scene.paths_ray_loss_fused + backward()                 (drt_render_paths_ray_loss_fused: nothing dense)
    (c) two-bounce one-pass kernel Scene.ray_loss_fused + backward()     at (2, drop) only: the pipeline the fast loops use today

    python tools/paths_bench.py [--mesh horse] [--res 1024] [--views 0,18,36,54] [--reps 15] [--warmup 3] [--refraction reference|snell]

Input as bench.py's: <mesh>_vh x4 (one midpoint subdivision), targets from <mesh>_scan traced with the law under test, 72-camera
turntable, at the bench camera (2.5 extents) and at 1.1 extents (the object fills the image).  Laws (2, drop), (4, reflect), (8, reflect),
each under the refraction formula of --refraction (targets and fit alike; route (c) is always the reference's formula).
The routes are alternated inside one process on the same tensors, after a warm-up of every route; each timed window is one view through
one route and ends in a device synchronise; the figure is the median over views x repetitions (min and max alongside).  Prints a table
and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from drt_amd import diffrender as Render, mesh_io, views  # noqa: E402

LAWS = [(2, "drop"), (4, "reflect"), (8, "reflect")]
IOR = 1.4723


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", default="horse")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--views", default="0,18,36,54")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--refraction", choices=("reference", "snell"), default="reference")
    a = ap.parse_args()
    view_ids = [int(v) for v in a.views.split(",")]
    res = a.res
    Render.intIOR = IOR
    Render.resx = Render.resy = res
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.mesh}_vh.ply")))
    center, extent = views.mesh_frame(mesh.vertices)
    scene = Render.Scene(mesh, 0)
    gt = Render.Scene(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.mesh}_scan.ply")), 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)

    def dense(o, d, sp, valid, law):
        out_ori, out_dir, mask = scene.render_paths(o, d, *law)
        Render.ray_loss(out_ori, out_dir, mask, sp, valid).backward()

    def one_pass(o, d, sp, valid, law):
        scene.paths_ray_loss_fused(o, d, sp, valid, *law).backward()

    def two_bounce(o, d, sp, valid, law):
        scene.ray_loss_fused(o, d, sp, valid).backward()

    results = []
    print(f"{a.mesh}_vh x4 ({len(mesh.faces)} triangles), {res} x {res}, views {view_ids}, {a.reps} repetitions after {a.warmup} warm-up rounds; "
          "ms per view, forward + loss + backward: median [min .. max]")
    for factor in (2.5, 1.1):
        cams = views.turntable_cameras(center, extent, 72, res, res, distance_factor=factor)
        for law in [l + (a.refraction,) for l in LAWS]:
            data = []
            with torch.no_grad():
                for k in view_ids:
                    o, d = views.generate_ray(res, res, cams[k][3], cams[k][2], device="cuda")
                    oo, od, mk = gt.render_paths(o, d, *law)
                    sp = views.screen_targets(oo, od, mk, cams[k], center, extent).contiguous()
                    data.append((o, d, sp, (sp[:, 0] != 0).contiguous()))
            routes = [("dense", dense), ("one_pass", one_pass)] + ([("two_bounce_one_pass", two_bounce)] if law[:2] == (2, "drop") else [])
            times = {name: [] for name, _ in routes}
            contributing = []
            for rep in range(a.warmup + a.reps):
                for view in data:
                    for name, fn in routes:                    # alternated: every route sees the same clocks and cache state
                        V.grad = None
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(*view, law)
                        torch.cuda.synchronize()
                        if rep >= a.warmup:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                        if rep == 0 and name == "one_pass":
                            contributing.append(int(scene.last_path_count))
            row = {"distance_factor": factor, "max_bounces": law[0], "tir": law[1], "refraction": law[2], "contributing_rays_per_view": contributing}
            for name, ts in times.items():
                row[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "windows": len(ts)}
            results.append(row)
            print(f"cameras at {factor} extents, law {law}: contributing rays per view {contributing}")
            for name, ts in times.items():
                print(f"    {name:20s} {statistics.median(ts):8.3f} [{min(ts):.3f} .. {max(ts):.3f}]")
    print(json.dumps({"tool": "paths_bench", "mesh": a.mesh, "res": res, "views": view_ids, "reps": a.reps, "device": torch.cuda.get_device_name(0),
                      "results": results}))


if __name__ == "__main__":
    main()
