"""Cost of absorption: Scene.render_image and Scene.image_loss_fused (loss + vertex gradient + IOR partials; the
absorbing call also the sigma partials) with and without ``absorption``, in the same build and the same process, on horse50k
(horse_vh.ply after one midpoint subdivision, 50 248 triangles): one 256 x 256 and one 1080 x 1920 turntable view, supersample 1, the
three laws of tests/image_cases.py, Fresnel on, the one-channel checker texture of the other image benchmarks.

    python tools/image_absorb_bench.py [--name horse] [--view 11] [--repeat 9] [--out profiles/render_image_absorb.txt]

The clear and the absorbing call are timed alternately -- clear, absorbing, clear, absorbing, ... -- after a warm-up of both.  A timed
run is a hipEvent interval on the current stream around ``inner`` back-to-back calls (so many that a window lasts about 20 ms), divided
by ``inner``.  Reported: the median of ``--repeat`` runs with the run-to-run spread (max - min) beside it, and the ratio of the medians.
Nothing is asserted and no threshold is fixed."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAWS = [(2, "drop", "reference"), (6, "reflect", "reference"), (6, "reflect", "snell")]
SIGMA = {3: (0.004, 0.012, 0.03), 1: (0.012,)}          # per texture channel count; the procedural checker has one channel
WINDOW_MS = 20.0


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternately(clear, absorbing, repeat):
    """((median, spread) of the clear call, (median, spread) of the absorbing one, inner), in ms per call."""
    clear(), absorbing()
    inner = max(1, math.ceil(WINDOW_MS / max(window(clear, 1), window(absorbing, 1), 1e-3)))
    window(clear, inner), window(absorbing, inner)
    ms = ([], [])
    for _ in range(repeat):
        ms[0].append(window(clear, inner))
        ms[1].append(window(absorbing, inner))
    return tuple((statistics.median(m), max(m) - min(m)) for m in ms) + (inner,)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_absorb.txt"))
    a = ap.parse_args(argv)
    from drt_amd import diffrender as Render, mesh_io, render, views
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    center, extent = views.mesh_frame(mesh.vertices)
    tex = torch.as_tensor(render.checker(a.texture, a.texture, 16), device="cuda")
    sigma_host = SIGMA[int(tex.shape[2])]
    lines = [f"render_image / image_loss_fused with and without absorption {sigma_host}, {a.name} ({len(mesh.faces)} triangles, extent {extent:.1f}), supersample 1, "
             f"Fresnel on: {torch.cuda.get_device_name(0)}",
             f"ms per call: median of {a.repeat} runs (spread: max - min) after a warm-up; a run is a hipEvent window of `inner` calls; clear and absorbing "
             "calls alternate", ""]
    for H, W in ((256, 256), (1080, 1920)):
        cam = views.turntable_cameras(center, extent, 72, W, H)[a.view]
        screen = render.Screen.behind(cam, center, extent, a.texture, a.texture)
        for law in LAWS:
            kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
            Render.intIOR = 1.55          # the photograph: the same view at another IOR, clear glass
            target = scene.render_image(cam, H, W, screen, tex, **kw)
            Render.intIOR = 1.4723
            ior = torch.tensor(1.4723, dtype=torch.float64, requires_grad=True)
            sigma = torch.tensor(sigma_host, dtype=torch.float64, requires_grad=True)

            def loss_term(absorption):
                loss = scene.image_loss_fused(cam, H, W, screen, tex, target, ior_int=ior, absorption=absorption, **kw)
                return torch.autograd.grad(loss, [V, ior] + ([sigma] if absorption is not None else []))

            rows = (("render_image", lambda: scene.render_image(cam, H, W, screen, tex, **kw),
                     lambda: scene.render_image(cam, H, W, screen, tex, absorption=sigma_host, **kw)),
                    ("image_loss_fused", lambda: loss_term(None), lambda: loss_term(sigma)))
            for what, clear, absorbing in rows:
                (c_ms, c_spread), (a_ms, a_spread), inner = alternately(clear, absorbing, a.repeat)
                lines.append(f"{H:4d} x {W:4d} {str(law):32s} {what:17s} clear {c_ms:8.3f} ms (spread {c_spread:.3f})   absorbing {a_ms:8.3f} ms (spread {a_spread:.3f})   "
                             f"absorbing / clear = {a_ms / c_ms:.3f}   inner {inner}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
