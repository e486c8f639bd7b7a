"""Calibration of a capture: fit the interior index of refraction of a FIXED mesh.

    python -m drt_amd.calibrate --name horse --max-bounces 6 --tir reflect --refraction snell --bracket 1.3 1.7

A capture comes with a nominal IOR, not a known one.  ``fit_ior`` finds the IOR at which the refraction loss of the given mesh against
the capture's targets is smallest, under any K-interaction law -- Snell's included -- from the exact derivative d loss / d IOR of
``Scene.paths_ray_loss_ior_fused(..., vertices=False)`` summed over the refraction views.  The loss as a function of the IOR is only
piecewise smooth (paths change face and validity), so a fixed-step optimiser rings around the minimum; the SIGN of the summed
derivative is right well away from it, and the fit bisects a bracket on that sign.
"""
from __future__ import annotations

import argparse
import json
import os

import torch

from . import optim


def _law(path_law):
    """(K, tir, refraction) by the rules of ``optim.path_law_keyword``; (2, "drop") under the reference formula -- no law to the loops
    -- is a law here: the IOR is fitted under today's formula."""
    law = optim.path_law_keyword(path_law, {}, "fit_ior")
    if law is None:
        return (2, "drop", "reference")
    return law if len(law) > 2 else (law[0], law[1], "reference")


def evaluate_views(scene, data, ior, law, view_ids, ior_ext=None):
    """(loss, d loss / d ior, contributing rays) summed over ``view_ids`` at the interior IOR ``ior``, as Python numbers."""
    x = torch.tensor(float(ior), dtype=torch.float64, requires_grad=True)
    total, rays = None, []
    for v in view_ids:
        screen_pixel, valid, _, origin, ray_dir, _ = data.get_view(v)
        loss = scene.paths_ray_loss_ior_fused(origin, ray_dir, screen_pixel, valid, x, ior_ext, *law, vertices=False)
        total = loss if total is None else total + loss
        rays.append(scene.last_path_count)
    if total is None:
        raise ValueError("fit_ior: no views to evaluate")
    g, = torch.autograd.grad(total, x)
    return float(total.detach()), float(g), int(sum(int(r) for r in rays))


def fit_ior(scene, data, path_law=(2, "drop", "snell"), bracket=(1.2, 1.8), halvings=14, view_ids=None, ior_ext=None):
    """The interior IOR of the fixed mesh of ``scene`` against the capture ``data``: bisection of ``bracket`` on the sign of
    d loss / d IOR, the refraction loss of ``path_law`` summed over ``view_ids`` (default: ``data.ray_view_ids()``).
    Returns dict(ior: the middle of the final bracket, bracket: the final one, evaluations, history: [(ior, loss, derivative,
    contributing rays)] per evaluation).  The bracket must hold a minimum -- derivative negative at its lower end, positive at its
    upper end -- else RuntimeError."""
    law = _law(path_law)
    lo, hi = (float(b) for b in bracket)
    if not (0.0 < lo < hi):
        raise ValueError(f"bracket must be (lo, hi) with 0 < lo < hi, got {bracket!r}")
    if isinstance(halvings, bool) or int(halvings) != halvings or int(halvings) < 0:
        raise ValueError(f"halvings must be a non-negative integer, got {halvings!r}")
    ids = list(data.ray_view_ids() if view_ids is None else view_ids)
    history = []

    def derivative(x):
        loss, g, rays = evaluate_views(scene, data, x, law, ids, ior_ext)
        history.append((x, loss, g, rays))
        return g

    g_lo, g_hi = derivative(lo), derivative(hi)
    if not (g_lo < 0.0 < g_hi):
        raise RuntimeError(f"fit_ior: the bracket ({lo}, {hi}) does not hold a minimum of the loss: d loss / d IOR is {g_lo:.6g} at its lower "
                           f"end and {g_hi:.6g} at its upper end (wanted: negative, positive)")
    for _ in range(int(halvings)):
        mid = 0.5 * (lo + hi)
        if derivative(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return {"ior": 0.5 * (lo + hi), "bracket": (lo, hi), "evaluations": len(history), "history": history}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fit the interior IOR of a fixed mesh against a capture (bisection on d loss / d IOR).")
    ap.add_argument("--name", default=optim.HyperParams["name"])
    ap.add_argument("--data-path", default="./data/")
    ap.add_argument("--capture", default=None, help=".npz / .h5 capture with the reference's datasets (default: a synthetic capture of "
                    "<name>_scan.ply, or of the hull without a scan, traced under the same law at --ior)")
    ap.add_argument("--mesh", default=None, help="the mesh to calibrate against (default: the mesh the synthetic capture was traced on; "
                    "required with --capture)")
    ap.add_argument("--ior", type=float, default=optim.HyperParams["IOR"], help="the IOR the synthetic capture is traced with")
    ap.add_argument("--bracket", type=float, nargs=2, default=(1.2, 1.8), metavar=("LO", "HI"))
    ap.add_argument("--halvings", type=int, default=14)
    ap.add_argument("--max-bounces", type=int, default=2, metavar="K")
    ap.add_argument("--tir", choices=("drop", "reflect"), default="drop")
    ap.add_argument("--refraction", choices=("reference", "snell"), default="snell")
    ap.add_argument("--res", type=int, default=256, help="resolution of the synthetic capture")
    ap.add_argument("--views", type=int, default=72, help="views of the synthetic capture")
    ap.add_argument("--num-view", type=int, default=optim.HyperParams["num_view"], help="views the refraction loss cycles through")
    args = ap.parse_args(argv)
    from . import captured_data, diffrender as Render, views
    law = (args.max_bounces, args.tir, args.refraction)
    if args.capture is not None:
        if args.mesh is None:
            ap.error("--capture needs --mesh: the mesh the IOR is fitted on")
        data = captured_data.get_data(dict(optim.HyperParams, name=args.name, num_view=args.num_view), path=args.capture)
        scene = Render.Scene(args.mesh, 0)
    else:
        scan = os.path.join(args.data_path, f"{args.name}_scan.ply")
        scene = Render.Scene(args.mesh or (scan if os.path.exists(scan) else os.path.join(args.data_path, f"{args.name}_vh.ply")), 0)
        Render.intIOR = args.ior
        Render.resx = Render.resy = args.res
        center, extent = views.mesh_frame(scene.mesh.vertices)
        data = captured_data.SyntheticData(scene, center, extent, args.res, args.res, num_view=min(args.num_view, args.views), n_total=args.views,
                                           name=args.name, path_law=law)
    fit = fit_ior(scene, data, law, tuple(args.bracket), args.halvings)
    report = {"name": args.name, "max_bounces": law[0], "tir": law[1], "refraction": law[2], "ior": fit["ior"], "bracket": list(fit["bracket"]),
              "evaluations": fit["evaluations"]}
    if args.capture is None:
        report["ior_true"] = args.ior
        report["error"] = fit["ior"] - args.ior
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
