"""Time of Scene.image_loss_fused (loss + vertex gradient + IOR partials of the refracted image) at capture size: horse50k (horse_vh.ply
after one midpoint subdivision, 50 248 triangles), one 1080 x 1920 turntable view, supersample 1 and 3, the three laws of
tests/test_gpu_image.py, Fresnel on -- beside two yardsticks that exist without it, on the same view: Scene.render_image (the forward
alone) and Scene.paths_ray_loss_ior_fused on views.generate_ray's rays (one wavefront trace plus the path adjoint, supersample 1).
The expectation was roughly their sum; the call traces once (its backward recomputes from the face tape), so it comes out below it.

    python tools/image_loss_bench.py [--name horse] [--view 11] [--repeat 3] [--out profiles/render_image_loss.txt]

Times are hipEvent intervals on the current stream, the median of `--repeat` runs after one warm-up; nothing is asserted."""
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
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--resx", type=int, default=1920)
    ap.add_argument("--resy", type=int, default=1080)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss.txt"))
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
    tex = torch.as_tensor(render.checker(a.texture, a.texture, 16), device="cuda")
    screen = render.Screen.behind(cam, center, extent, a.texture, a.texture)
    o, d = views.generate_ray(H, W, cam[3], cam[2], device="cuda")
    lines = [f"image_loss_fused, {a.name} ({len(mesh.faces)} triangles), one {H} x {W} view, Fresnel on: {torch.cuda.get_device_name(0)}; median (best) of "
             f"{a.repeat} runs after one warm-up, hipEvent ms", ""]
    for law in LAWS:
        kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
        # the photograph: the same view at another IOR
        Render.intIOR = 1.55
        target = scene.render_image(cam, H, W, screen, tex, supersample=3, **kw)
        Render.intIOR = 1.4723
        with torch.no_grad():
            oo, od, mask = scene.render_paths(o, d, *law)
            sp, valid = (oo + 50.0 * od).clone(), mask[:, 0].clone()
        ior = torch.tensor(1.4723, dtype=torch.float64, requires_grad=True)

        def ray_term():
            loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, ior, None, *law)
            return loss, torch.autograd.grad(loss, [V, ior])

        ray_ms, ray_best, _ = timed(ray_term, a.repeat)
        lines.append(f"paths_ray_loss_ior_fused  s=1 {str(law):32s} {ray_ms:9.3f} ms ({ray_best:.3f})   valid rays {int(valid.sum())}")
        for s in (1, 3):
            fwd_ms, fwd_best, _ = timed(lambda: scene.render_image(cam, H, W, screen, tex, supersample=s, **kw), a.repeat)

            def image_term(vertices=True):
                loss = scene.image_loss_fused(cam, H, W, screen, tex, target, ior_int=ior, supersample=s, vertices=vertices, **kw)
                return loss, torch.autograd.grad(loss, [V, ior] if vertices else [ior])

            ms, best, out = timed(image_term, a.repeat)
            fixed_ms, fixed_best, _ = timed(lambda: image_term(False), a.repeat)
            count = int(scene.last_image_count)
            n = H * W * s * s
            lines.append(f"render_image              s={s} {str(law):32s} {fwd_ms:9.3f} ms ({fwd_best:.3f})   bands {len(render.plan_bands(H, W, s, 1 << 22))}")
            lines.append(f"image_loss_fused          s={s} {str(law):32s} {ms:9.3f} ms ({best:.3f})   {n / ms / 1e3:8.1f} M samples/s   samples with a gradient {count}   "
                         f"loss {float(out[0].detach()):.6e}   / render_image = {ms / fwd_ms:.2f}" +
                         (f"   / (render_image + paths_ray_loss_ior_fused) = {ms / (fwd_ms + ray_ms):.2f}" if s == 1 else "") +
                         f"   vertices=False {fixed_ms:.3f} ms ({fixed_best:.3f})")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
