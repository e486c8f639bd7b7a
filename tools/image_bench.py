"""Samples per second of Scene.render_image at capture size: horse50k (horse_vh.ply after one midpoint subdivision, 50 248 triangles), one
1080 x 1920 turntable view, supersample 1 and 3, the three laws of tests/test_gpu_image.py -- beside the route the library offered before
the call existed, at supersample 1 and without Fresnel: views.generate_ray on the device, Scene.render_paths, Scene.render_mask for the
"any interaction" flag, then the screen plane and torch's grid_sample.

    python tools/image_bench.py [--name horse] [--view 11] [--repeat 5] [--out profiles/render_image.txt]

Times are hipEvent intervals on the current stream, the median of `--repeat` runs after one warm-up; nothing is asserted."""
import argparse
import os
import statistics
import sys

import numpy as np
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
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), out


def parent_route(scene, cam, H, W, screen, tex, law, void, invalid, stages=None):
    """The same pixels through the calls that existed before render_image (supersample 1, no Fresnel); float32 [H, W, C]."""
    from drt_amd import views

    def stage(name, fn):
        if stages is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        stages[name] = stages.get(name, 0.0) + a.elapsed_time(b)
        return out

    o, d = stage("generate_ray", lambda: views.generate_ray(H, W, cam[3], cam[2], device="cuda"))
    with torch.no_grad():
        oo, od, mask = stage("render_paths", lambda: scene.render_paths(o, d, *law))
        hit = stage("render_mask", lambda: scene.render_mask(o, d) > 0)

    def shade():
        through = mask[:, 0]
        eo, ed = torch.where(through[:, None], oo, o), torch.where(through[:, None], od, d)
        p0, eu, ev = (torch.as_tensor(a, device="cuda") for a in (screen.p0, screen.eu, screen.ev))
        n = torch.linalg.cross(eu, ev)
        dn = ed @ n
        t = ((p0 - eo) @ n) / dn
        r = eo + t[:, None] * ed - p0
        u, v = (r @ eu) / (eu @ eu), (r @ ev) / (ev @ ev)
        th, tw = tex.shape[:2]
        on = (dn != 0) & (t > 0) & (u >= 0) & (u <= tw - 1) & (v >= 0) & (v <= th - 1)
        grid = torch.stack([2 * u / (tw - 1) - 1, 2 * v / (th - 1) - 1], dim=1).to(torch.float32).view(1, H, W, 2)
        col = torch.nn.functional.grid_sample(tex.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        col = col.permute(1, 2, 0).reshape(H * W, -1)
        col = torch.where(on[:, None], col, torch.full_like(col, void))
        col = torch.where((hit & ~through)[:, None], torch.full_like(col, invalid), col)
        return col.view(H, W, -1)

    return stage("plane + grid_sample", shade)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--resx", type=int, default=1920)
    ap.add_argument("--resy", type=int, default=1080)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image.txt"))
    a = ap.parse_args(argv)
    from drt_amd import diffrender as Render, mesh_io, render, views
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    Render.intIOR = 1.4723
    center, extent = views.mesh_frame(mesh.vertices)
    H, W = a.resy, a.resx
    cam = views.turntable_cameras(center, extent, 72, W, H)[a.view]
    tex_host = render.ramp(a.texture, a.texture)
    tex = torch.as_tensor(tex_host, device="cuda")
    screen = render.Screen.behind(cam, center, extent, a.texture, a.texture)
    lines = [f"render_image, {a.name} ({len(mesh.faces)} triangles), one {H} x {W} view: {torch.cuda.get_device_name(0)}; median (best) of {a.repeat} runs after "
             "one warm-up, hipEvent ms", ""]
    single = {}
    for s in (1, 3):
        for law in LAWS:
            for fresnel in (True, False):
                med, best, out = timed(lambda: scene.render_image(cam, H, W, screen, tex, supersample=s, max_bounces=law[0], tir=law[1], refraction=law[2],
                                                                  fresnel=fresnel, void=0.0, invalid=0.5, want_planes=True), a.repeat)
                n = H * W * s * s
                if s == 1 and not fresnel:
                    single[law] = (med, out)
                lines.append(f"render_image s={s} {str(law):32s} {'fresnel ' if fresnel else 'geometry'} {med:9.3f} ms ({best:.3f})   {n / med / 1e3:8.1f} M samples/s   "
                             f"hit {float(out[1].mean()):.4f} through {float(out[2].mean()):.4f}   bands {len(render.plan_bands(H, W, s, 1 << 22))}")
    lines += ["", "the route before this call (supersample 1, no Fresnel): generate_ray on the device + render_paths + render_mask + plane and grid_sample in torch"]
    for law in LAWS:
        med, best, img = timed(lambda: parent_route(scene, cam, H, W, screen, tex, law, 0.0, 0.5), a.repeat)
        stages = {}
        for _ in range(a.repeat):
            parent_route(scene, cam, H, W, screen, tex, law, 0.0, 0.5, stages)
        mine, out = single[law]
        diff = (img - out[0]).abs()
        lines.append(f"composition  s=1 {str(law):32s} geometry {med:9.3f} ms ({best:.3f})   render_image / composition = {mine / med:.3f}   "
                     f"stages (mean ms): " + ", ".join(f"{k} {v / a.repeat:.3f}" for k, v in stages.items()) +
                     f"   pixels that differ by more than 1e-4: {int((diff.amax(2) > 1e-4).sum())} of {H * W} (float32 grid_sample against the float64 law)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
