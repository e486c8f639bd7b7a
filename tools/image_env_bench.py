"""Cost of the environment map and of the outer-surface reflection: Scene.render_image and Scene.image_loss_fused (loss
+ vertex gradient + IOR partials) as before (clear), with an environment behind the screen, and with environment and reflection, in
the same build and the same process, on horse50k (horse_vh.ply after one midpoint
subdivision, 50 248 triangles): one 256 x 256 and one 1080 x 1920 turntable view, supersample 1, the three laws of
tests/image_cases.py, Fresnel on, the one-channel checker texture of the other image benchmarks and a random one-channel
512 x 1024 environment turned by Rx(0.3) Ry(0.7).

    python tools/image_env_bench.py [--name horse] [--view 11] [--repeat 9] [--out profiles/render_image_env.txt]

tools/image_absorb_bench.py's protocol: the forms are timed alternately -- clear, environment, environment + reflection, clear, ... -- after a
warm-up of all.  A timed run is a hipEvent interval on the current stream around ``inner`` back-to-back calls (so many that a window
lasts about 20 ms), divided by ``inner``.  Reported: the median of ``--repeat`` runs with the run-to-run spread (max - min) beside it,
and the ratios of the medians.  Nothing is asserted and no threshold is fixed."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAWS = [(2, "drop", "reference"), (6, "reflect", "reference"), (6, "reflect", "snell")]
WINDOW_MS = 20.0


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternately(forms, repeat):
    """([(median, spread) per form], inner), in ms per call."""
    for fn in forms:
        fn()
    inner = max(1, math.ceil(WINDOW_MS / max([window(fn, 1) for fn in forms] + [1e-3])))
    for fn in forms:
        window(fn, inner)
    ms = [[] for _ in forms]
    for _ in range(repeat):
        for m, fn in zip(ms, forms):
            m.append(window(fn, inner))
    return [(statistics.median(m), max(m) - min(m)) for m in ms], inner


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_env.txt"))
    a = ap.parse_args(argv)
    from drt_amd import diffrender as Render, mesh_io, render, views
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    center, extent = views.mesh_frame(mesh.vertices)
    tex = torch.as_tensor(render.checker(a.texture, a.texture, 16), device="cuda")
    cx, sx, cy, sy = math.cos(0.3), math.sin(0.3), math.cos(0.7), math.sin(0.7)
    rot = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    env = render.Environment(torch.as_tensor(np.random.default_rng(11).random((512, 1024, 1)).astype(np.float32), device="cuda"), rot)
    Render.intIOR = 1.4723
    lines = [f"render_image / image_loss_fused as before, with an environment behind the screen, and with environment and reflection, {a.name} ({len(mesh.faces)} triangles, "
             f"extent {extent:.1f}), supersample 1, Fresnel on: {torch.cuda.get_device_name(0)}",
             f"ms per call: median of {a.repeat} runs (spread: max - min) after a warm-up; a run is a hipEvent window of `inner` calls; the three forms "
             "alternate", ""]
    for H, W in ((256, 256), (1080, 1920)):
        cam = views.turntable_cameras(center, extent, 72, W, H)[a.view]
        screen = render.Screen.behind(cam, center, extent, a.texture, a.texture)
        for law in LAWS:
            kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
            Render.intIOR = 1.55          # the photograph: the same view at another IOR, clear glass in front of the screen alone
            target = scene.render_image(cam, H, W, screen, tex, **kw)
            Render.intIOR = 1.4723
            ior = torch.tensor(1.4723, dtype=torch.float64, requires_grad=True)

            def loss_term(**more):
                loss = scene.image_loss_fused(cam, H, W, screen, tex, target, ior_int=ior, **more, **kw)
                return torch.autograd.grad(loss, [V, ior])

            rows = (("render_image", [lambda: scene.render_image(cam, H, W, screen, tex, **kw), lambda: scene.render_image(cam, H, W, screen, tex, environment=env, **kw),
                                      lambda: scene.render_image(cam, H, W, screen, tex, environment=env, reflection=True, **kw)]),
                    ("image_loss_fused", [lambda: loss_term(), lambda: loss_term(environment=env), lambda: loss_term(environment=env, reflection=True)]))
            for what, forms in rows:
                ((c_ms, c_sp), (e_ms, e_sp), (n_ms, n_sp)), inner = alternately(forms, a.repeat)
                lines.append(f"{H:4d} x {W:4d} {str(law):32s} {what:17s} clear {c_ms:8.3f} ms (spread {c_sp:.3f})   environment {e_ms:8.3f} ms (spread {e_sp:.3f})   "
                             f"environment + reflection {n_ms:8.3f} ms (spread {n_sp:.3f})   environment / clear = {e_ms / c_ms:.3f}   + reflection / clear = {n_ms / c_ms:.3f}   inner {inner}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
