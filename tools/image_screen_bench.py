"""Cost of the screen-pose and texture gradients of Scene.image_loss_fused at capture size: horse50k (horse_vh.ply after
one midpoint subdivision, 50 248 triangles), one 1080 x 1920 turntable view, Fresnel on, supersample 1 and 3, the three laws of
tests/test_gpu_image.py.  Per law and supersample five calls are timed, each with the vertex and IOR gradients of today's call:

    today            image_loss_fused without the new keywords (drt_render_image_loss)
    + screen         screen_param requires grad                     (k_image_screen_bwd without its table)
    + texture 1024   texture_param requires grad, a 1024 x 1024 x 1 texture
    + texture 64     the same with a 64 x 64 x 1 texture: sixteen times fewer texels under the same pixels
    + both           screen_param and the 1024 x 1024 texture_param

    python tools/image_screen_bench.py [--repeat 9] [--today-only] [--out profiles/render_image_loss_screen.txt]

``--today-only`` times the first call alone: what a build from before the keywords can run (select it with DRT_HIP_LIB), the yardstick
the first row is held against.  Times are hipEvent intervals on the current stream: median (min .. max) of ``--repeat`` runs after one
warm-up; nothing is asserted."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss_screen.txt"))
    a = ap.parse_args(argv)
    from drt_amd import diffrender as Render, mesh_io, render, views
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    Render.intIOR = 1.4723
    center, extent = views.mesh_frame(mesh.vertices)
    H, W = a.resy, a.resx
    cam = views.turntable_cameras(center, extent, 72, W, H)[a.view]
    textures = {n: torch.as_tensor(render.checker(n, n, 16), device="cuda") for n in (1024, 64)}
    screens = {n: render.Screen.behind(cam, center, extent, n, n) for n in (1024, 64)}
    lines = [f"image_loss_fused with screen_param / texture_param, {a.name} ({len(mesh.faces)} triangles), one {H} x {W} view, Fresnel on: "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.repeat} runs after one warm-up, hipEvent ms", ""]
    for law in LAWS:
        kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
        Render.intIOR = 1.55                          # the photograph: the same view at another IOR
        target = scene.render_image(cam, H, W, screens[1024], textures[1024], supersample=3, **kw)
        Render.intIOR = 1.4723
        ior = torch.tensor(1.4723, dtype=torch.float64, requires_grad=True)
        for s in (1, 3):
            def call(n=1024, screen=False, texture=False):
                wrt, extra = [V, ior], {}
                if screen:
                    P = torch.tensor(screens[n].packed().reshape(3, 3), requires_grad=True)
                    extra["screen_param"] = P
                    wrt.append(P)
                if texture:
                    T = textures[n].detach().requires_grad_(True)
                    extra["texture_param"] = T
                    wrt.append(T)
                loss = scene.image_loss_fused(cam, H, W, None if screen else screens[n], None if texture else textures[n], target, ior_int=ior,
                                              supersample=s, **kw, **extra)
                return torch.autograd.grad(loss, wrt)

            rows = [("today", lambda: call())]
            if not a.today_only:
                rows += [("+ screen", lambda: call(screen=True)), ("+ texture 1024", lambda: call(texture=True)),
                         ("+ texture 64", lambda: call(64, texture=True)), ("+ both", lambda: call(screen=True, texture=True))]
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
