"""Whole reconstruction, end to end -- the reference's ``python optim.py`` (optim.py:173-229).

    python -m drt_amd.reconstruct --name horse [--capture horse.npz] [--res 512] [--passes 20] [--iters 200]
    python -m torch.distributed.run --nproc-per-node 8 -m drt_amd.reconstruct --name monkey --views 144 --res 1024 --views-per-step all
    python -m drt_amd.reconstruct --name horse --max-bounces 6 --tir reflect --fused-paths

``optimize(HyperParams)`` of the reference builds the scene from ``<data>/<name>_vh.ply``, loads the capture,
runs Pass x Iters iterations with a remesh before every pass and writes ``<result>/<name>_recons.ply``
(optim.py:173-229); its README then measures the result against ``<name>_scan.ply`` with MeshLab.  This
module does the same on the HIP path.  The captures (HDF5) are not distributed with the reference: when
``--capture`` is not given, a synthetic capture is traced through the scanned mesh (or, without a scan,
through a displaced copy of the hull) with the same tuple layout.

``--views-per-step`` (or a launch with more than one rank) runs the multi-rank loop, optim.optimize_sharded: each rank renders and
evaluates only its own views, one all-reduce per iteration, and rank 0 alone prints, writes the PLY and ``<name>_report.json``.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from . import captured_data, diffrender as Render, mesh_io, metrics, optim, views, visual_hull


def _refraction_of(law):
    return law[2] if law is not None and len(law) > 2 else "reference"


def run(HyperParams, data_path="./data/", result_path="./result/", capture=None, res=None, fused=True, output=True, device=0, n_views=72,
        views_per_step=None, ior_start=None, path_law=None, hull_from_capture=None):
    """``views_per_step=None``: the single-process loop (optim.optimize).  An int, or "all" (one epoch of the refraction schedule per
    iteration), goes through optim.optimize_sharded on every rank of the default process group (one process without one).
    ``HyperParams["ior_lr"] > 0``: the IOR is fitted too (the drop-in loop, optim.optimize), starting at ``ior_start`` (default
    ``HyperParams["IOR"]``, which is also the IOR the synthetic capture is traced with); the report gains ``ior``, the fitted value.
    ``HyperParams["max_bounces"]`` / ``["tir"]`` other than 2 / "drop" (optim.path_law): the synthetic capture AND the fit trace paths of up
    to that many interactions (the drop-in loop); the report echoes both.
    ``path_law=(K, tir)`` (the keyword of optim.optimize / optimize_sharded; the ``HyperParams`` keys stay at their defaults): the same
    law for the capture, and the fit runs it in the ONE-PASS loop (unless ``fused=False``).  Either spelling may carry the refraction
    formula (``HyperParams["refraction"]``, or a third element of the keyword: "reference" / "snell"); the report echoes it.  ``report["path_route"]`` says which route the
    refraction term took: "fused" (one-pass kernels) or "dropin".
    ``hull_from_capture=N``: do not read ``<name>_vh.ply`` as the start; build the visual hull of the run's own capture on an N-corner grid
    (drt_amd.visual_hull) and start from that; ``report["hull"]`` describes it.  Single process only (a rank holds only its own views)."""
    law_kw = optim.path_law_keyword(path_law, HyperParams, "reconstruct")
    law = optim.path_law(HyperParams) or law_kw
    if views_per_step is not None or torch.distributed.is_available() and torch.distributed.is_initialized():
        if hull_from_capture:
            raise ValueError(HULL_NEEDS_ONE_PROCESS)
        return run_sharded(HyperParams, data_path, result_path, capture, res, output, device, n_views, views_per_step or 1, path_law=law_kw)
    name = HyperParams["name"]
    hull_path = os.path.join(data_path, f"{name}_vh.ply")
    scan_path = os.path.join(data_path, f"{name}_scan.ply")
    Render.intIOR = HyperParams["IOR"]
    scene = None if hull_from_capture else Render.Scene(hull_path, device)
    scan_scene = Render.Scene(scan_path, device) if os.path.exists(scan_path) else None
    if capture is not None:
        data = captured_data.get_data(HyperParams, path=capture)
    else:
        resx = resy = int(res or 512)
        Render.resx, Render.resy = resx, resy
        gt = scan_scene if scan_scene is not None else Render.Scene(
            views.displaced_ground_truth(scene.mesh if scene is not None else mesh_io.load(hull_path), 0.5, 0), device)
        center, extent = views.mesh_frame(gt.mesh.vertices)
        data = captured_data.SyntheticData(gt, center, extent, resx, resy, num_view=min(HyperParams["num_view"], n_views), n_total=n_views, name=name,
                                           path_law=law)
    hull = {}
    if hull_from_capture:
        scene = Render.Scene(visual_hull.visual_hull(data, resolution=int(hull_from_capture), report=hull), device)
    report = {"name": name, "resx": data.resx, "resy": data.resy, "views": data.n_total, "hull_faces": int(scene.faces.shape[0]),
              "max_bounces": law[0] if law else 2, "tir": law[1] if law else "drop", "refraction": _refraction_of(law)}
    if hull_from_capture:
        report.update(hull_source="capture", hull=hull)
    if scan_scene is not None:
        report["hull_to_scan"] = metrics.hausdorff(scene, scan_scene)
    t0 = time.time()
    if float(HyperParams.get("ior_lr", 0) or 0) > 0:
        start = HyperParams["IOR"] if ior_start is None else float(ior_start)
        report["ior_start"] = start
        report["path_route"] = "dropin"
        scene, history, report["ior"] = optim.optimize(scene, data, dict(HyperParams, IOR=start), output=output, fused=False)
    else:
        one_pass = fused and (law is None or law_kw is not None)
        report["path_route"] = "fused" if one_pass else "dropin"
        scene, history = optim.optimize(scene, data, HyperParams, output=output, fused=one_pass, path_law=law_kw)
    torch.cuda.synchronize()
    report["optimize_seconds"] = time.time() - t0
    report["iterations"] = HyperParams["Pass"] * HyperParams["Iters"]
    report["result_faces"] = int(scene.faces.shape[0])
    if scan_scene is not None:
        report["result_to_scan"] = metrics.hausdorff(scene, scan_scene)
    os.makedirs(result_path, exist_ok=True)
    out = os.path.join(result_path, f"{name}_recons.ply")
    scene.mesh.export(out)
    report["result"] = out
    return scene, report


HULL_NEEDS_ONE_PROCESS = ("--hull-from-capture builds the hull from ALL views of the capture and a rank holds only its own: write the hull first with "
                          "`python -m drt_amd.visual_hull --name NAME -o DATA/NAME_vh.ply` (one process), then run the ranks without the flag")


def run_sharded(HyperParams, data_path="./data/", result_path="./result/", capture=None, res=None, output=True, device=0, n_views=72,
                views_per_step=1, path_law=None):
    """The reconstruction on every rank (optim.optimize_sharded): each rank renders only the views it owns of the synthetic capture; rank 0
    alone prints, measures and writes ``<name>_recons.ply`` and ``<name>_report.json``.  Returns (scene, report) -- the report on rank 0,
    None elsewhere.  ``path_law=(K, tir)``: capture and fit trace paths of up to K interactions (the one-pass form)."""
    from . import dist as ddist
    law = optim.path_law_keyword(path_law, HyperParams, "reconstruct")
    rank, world = ddist.rank_world()
    name = HyperParams["name"]
    hull_path = os.path.join(data_path, f"{name}_vh.ply")
    scan_path = os.path.join(data_path, f"{name}_scan.ply")
    Render.intIOR = HyperParams["IOR"]
    scene = Render.Scene(hull_path, device)
    scan_scene = Render.Scene(scan_path, device) if os.path.exists(scan_path) else None
    if capture is not None:
        data = captured_data.get_data(HyperParams, path=capture)
    else:
        resx = resy = int(res or 512)
        Render.resx, Render.resy = resx, resy
        num_view = min(HyperParams["num_view"], n_views)
        ray_ids = captured_data.ray_view_ids(n_views, num_view, name)
        mine = sorted(set(ddist.owned_views(ray_ids, rank, world)) | set(ddist.owned_views(captured_data.silh_view_ids(n_views), rank, world)))
        gt = scan_scene if scan_scene is not None else Render.Scene(views.displaced_ground_truth(scene.mesh, 0.5, 0), device)
        center, extent = views.mesh_frame(gt.mesh.vertices)
        data = captured_data.SyntheticData(gt, center, extent, resx, resy, num_view=num_view, n_total=n_views, name=name, view_ids=mine,
                                           path_law=law)
    k = len(data.ray_view_ids()) if views_per_step == "all" else int(views_per_step)
    report = {"name": name, "resx": data.resx, "resy": data.resy, "views": data.n_total, "hull_faces": int(scene.faces.shape[0]),
              "world": world, "views_per_step": k, "max_bounces": law[0] if law else 2, "tir": law[1] if law else "drop", "refraction": _refraction_of(law), "path_route": "fused"}
    if scan_scene is not None and rank == 0:
        report["hull_to_scan"] = metrics.hausdorff(scene, scan_scene)
    t0 = time.time()
    scene, history, stats = optim.optimize_sharded(scene, data, HyperParams, views_per_step=k, output=output, path_law=law)
    torch.cuda.synchronize()
    report["optimize_seconds"] = time.time() - t0
    report["iterations"] = stats["iterations"]
    report["seconds_per_iteration"] = stats["step_seconds"] / max(1, stats["iterations"])
    report["collectives_per_iteration"] = stats["allreduces_per_iteration"]
    report["broadcasts_per_pass"] = stats["broadcasts_per_pass"]
    report["collective_share"] = stats["collective_seconds"] / stats["step_seconds"] if stats["step_seconds"] > 0 else 0.0
    report["result_faces"] = int(scene.faces.shape[0])
    if rank != 0:
        return scene, None
    if scan_scene is not None:
        report["result_to_scan"] = metrics.hausdorff(scene, scan_scene)
    os.makedirs(result_path, exist_ok=True)
    out = os.path.join(result_path, f"{name}_recons.ply")
    scene.mesh.export(out)
    report["result"] = out
    with open(os.path.join(result_path, f"{name}_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return scene, report


def _views_per_step(text):
    if text == "all":
        return text
    k = int(text)
    if k < 1:
        raise argparse.ArgumentTypeError("--views-per-step takes a positive integer or 'all'")
    return k


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default=optim.HyperParams["name"])
    ap.add_argument("--data-path", default="./data/")
    ap.add_argument("--result-path", default="./result/")
    ap.add_argument("--capture", default=None, help=".npz / .h5 capture with the reference's datasets (default: synthetic capture)")
    ap.add_argument("--res", type=int, default=512, help="resolution of the synthetic capture")
    ap.add_argument("--passes", type=int, default=optim.HyperParams["Pass"])
    ap.add_argument("--iters", type=int, default=optim.HyperParams["Iters"])
    ap.add_argument("--num-view", type=int, default=optim.HyperParams["num_view"], help="views the refraction loss cycles through")
    ap.add_argument("--views", type=int, default=72, help="views of the synthetic capture (the real captures have 72)")
    ap.add_argument("--ior", type=float, default=optim.HyperParams["IOR"])
    ap.add_argument("--dropin", action="store_true", help="use the reference-shaped (unfused) loss terms")
    ap.add_argument("--fit-ior", type=float, default=0.0, metavar="LR",
                    help="also learn the index of refraction with this SGD learning rate (implies --dropin); the report gains \"ior\"")
    ap.add_argument("--ior-start", type=float, default=None, help="with --fit-ior: the IOR the fit starts from (default: --ior)")
    ap.add_argument("--max-bounces", type=int, default=2, metavar="K", help="surface interactions per light path, 2..8 (other than 2 / drop: "
                    "Scene.render_paths for the synthetic capture and the fit; implies --dropin)")
    ap.add_argument("--tir", choices=("drop", "reflect"), default="drop", help="what a hit with total internal reflection does to a path")
    ap.add_argument("--refraction", choices=("reference", "snell"), default="reference", help="how a refracting hit bends the ray: the "
                    "reference's formula, or Snell's law (alone: the two-bounce path under Snell's law through Scene.render_paths, drop-in)")
    ap.add_argument("--fused-paths", action="store_true", help="with --max-bounces / --tir / --refraction: fit with the one-pass form of the law "
                    "(Scene.paths_ray_loss_fused) in the one-pass loop, which also runs under torch.distributed.run")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--views-per-step", type=_views_per_step, default=None, metavar="N|all",
                    help="refraction views per iteration (all: every view of the schedule once) on the multi-rank loop; "
                         "under torch.distributed.run the default is 1")
    ap.add_argument("--hull-from-capture", type=int, nargs="?", const=256, default=None, metavar="N",
                    help="start from the visual hull of the run's own capture, built on an N-corner grid (default 256), instead of reading "
                         "<name>_vh.ply; single process only")
    a = ap.parse_args(argv)
    import numpy as np
    np.random.seed(a.seed)
    hp = dict(optim.HyperParams, name=a.name, Pass=a.passes, Iters=a.iters, num_view=a.num_view, IOR=a.ior)
    if a.fit_ior > 0:
        hp["ior_lr"] = a.fit_ior
    law_kw = None
    if a.fused_paths:         # the law as the explicit keyword: the HyperParams keys keep their defaults, the one-pass loop runs it
        law_kw = optim.path_law_keyword((a.max_bounces, a.tir, a.refraction), hp, "reconstruct")
    else:
        hp["max_bounces"], hp["tir"], hp["refraction"] = a.max_bounces, a.tir, a.refraction
    law = optim.path_law(hp)
    from . import dist as ddist
    if a.hull_from_capture is not None and (a.views_per_step is not None or ddist.env_world()[2] > 1):
        raise SystemExit(HULL_NEEDS_ONE_PROCESS)
    if a.views_per_step is None and ddist.env_world()[2] == 1:
        _, report = run(hp, a.data_path, a.result_path, a.capture, a.res, fused=not (a.dropin or a.fit_ior > 0), n_views=a.views,
                        ior_start=a.ior_start, path_law=law_kw, hull_from_capture=a.hull_from_capture)
        print(json.dumps(report))
        return
    if a.dropin or a.fit_ior > 0 or law is not None:
        raise SystemExit("--dropin / --fit-ior / --max-bounces / --tir have no multi-rank form: the sharded loop runs the one-pass terms")
    _, local_rank, world = ddist.init()
    device = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device)
    try:
        _, report = run_sharded(hp, a.data_path, a.result_path, a.capture, a.res, output=True, device=device, n_views=a.views,
                                views_per_step=a.views_per_step or 1, path_law=law_kw)
        if report is not None:
            print(json.dumps(report))
    finally:
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
