"""Cost of the camera gradient of Scene.image_loss_fused at capture size: horse50k (horse_vh.ply after one midpoint
subdivision, 50 248 triangles), one 1080 x 1920 turntable view, Fresnel on, supersample 1 and 3, the three laws of
tests/test_gpu_image.py.  Per law and supersample four calls are timed:

    today            image_loss_fused without the keyword, with its vertex and IOR gradients (drt_render_image_loss)
    + screen         screen_param requires grad: DESIGN.md 10.4's row, the yardstick of the next one
    + camera         camera_param = (Rinv, Kinv), both require grad (k_image_loss_bwd with CAMERA, k_image_camera_bwd)
    camera only      camera_param alone: vertices=False and plain IOR floats (against today's call: what a camera fit pays per step)

    python tools/image_camera_bench.py [--repeat 9] [--today-only] [--deterministic] [--out profiles/render_image_loss_camera.txt]

``--today-only`` times the first call alone: what a build from before the keyword can run (select it with DRT_HIP_LIB), the yardstick
the first row is held against.  ``--deterministic`` times the same calls with the fixed-point accumulators (drt_amd.det).  Times are
hipEvent intervals on the current stream: median (min .. max) of ``--repeat`` runs after one warm-up; nothing is asserted."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAWS = [(2, "drop", "reference"), (6, "reflect", "reference"), (6, "reflect", "snell")]


def timed(fn, repeat):
    fn()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--resx", type=int, default=1920)
    ap.add_argument("--resy", type=int, default=1080)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--today-only", action="store_true")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss_camera.txt"))
    a = ap.parse_args(argv)
    from drt_amd import det, diffrender as Render, mesh_io, render, views
    det.enable(a.deterministic)
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    Render.intIOR = 1.4723
    center, extent = views.mesh_frame(mesh.vertices)
    H, W = a.resy, a.resx
    cam = views.turntable_cameras(center, extent, 72, W, H)[a.view]
    texture = torch.as_tensor(render.checker(1024, 1024, 16), device="cuda")
    screen = render.Screen.behind(cam, center, extent, 1024, 1024)
    lines = [f"image_loss_fused with camera_param, {a.name} ({len(mesh.faces)} triangles), one {H} x {W} view, Fresnel on"
             f"{', deterministic mode' if a.deterministic else ''}: {torch.cuda.get_device_name(0)}; median (min .. max) of {a.repeat} runs after one warm-up, hipEvent ms", ""]
    for law in LAWS:
        kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
        Render.intIOR = 1.55                          # the photograph: the same view at another IOR
        target = scene.render_image(cam, H, W, screen, texture, supersample=3, **kw)
        Render.intIOR = 1.4723
        ior = torch.tensor(1.4723, dtype=torch.float64, requires_grad=True)
        for s in (1, 3):
            def call(with_screen=False, camera=False, only=False):
                wrt, extra = ([], dict(vertices=False)) if only else ([V, ior], dict(ior_int=ior))
                if with_screen:
                    P = torch.tensor(screen.packed().reshape(3, 3), requires_grad=True)
                    extra["screen_param"] = P
                    wrt.append(P)
                if camera:
                    R = torch.tensor(cam[2], dtype=torch.float64, requires_grad=True)
                    K = torch.tensor(cam[3], dtype=torch.float64, requires_grad=True)
                    extra["camera_param"] = (R, K)
                    wrt += [R, K]
                loss = scene.image_loss_fused(None if camera else cam, H, W, None if with_screen else screen, texture, target, supersample=s, **kw, **extra)
                return torch.autograd.grad(loss, wrt)

            rows = [("today", lambda: call())]
            if not a.today_only:
                rows += [("+ screen", lambda: call(with_screen=True)), ("+ camera", lambda: call(camera=True)),
                         ("camera only", lambda: call(camera=True, only=True))]
            base = None
            for label, fn in rows:
                ms, lo, hi = timed(fn, a.repeat)
                base = ms if base is None else base
                lines.append(f"s={s} {str(law):32s} {label:16s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f})" + ("" if label == "today" else f"   {ms - base:+.3f} ms on today's call"))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
