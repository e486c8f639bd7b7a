"""Cost of the environment's texel and rotation gradients: Scene.image_loss_fused (loss + vertex gradient + IOR
partial) in front of an environment without the new keywords, with the rotation gradient, with the texel gradient and with both, in the
same build and the same process, on horse50k (horse_vh.ply after one midpoint subdivision, 50 248 triangles): one 256 x 256 and one
1080 x 1920 turntable view, supersample 1, the three laws of tests/image_cases.py, Fresnel on, reflection off and on, the one-channel
checker texture of the other image benchmarks and a random one-channel 512 x 1024 environment turned by Rx(0.3) Ry(0.7).

    python tools/image_env_param_bench.py [--name horse] [--view 11] [--repeat 9] [--out profiles/render_image_loss_env_param.txt]

tools/image_env_bench.py's protocol: the four forms are timed alternately after a warm-up of all.  A timed run is a hipEvent interval on the
current stream around ``inner`` back-to-back calls (so many that a window lasts about 20 ms), divided by ``inner``.  Reported: the median
of ``--repeat`` runs with the run-to-run spread (max - min) beside it, and the differences of the medians from the call without the
keywords.  Nothing is asserted and no threshold is fixed."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from image_env_bench import LAWS, alternately      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--view", type=int, default=11)
    ap.add_argument("--texture", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss_env_param.txt"))
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
    texels = torch.as_tensor(np.random.default_rng(11).random((512, 1024, 1)).astype(np.float32), device="cuda")
    env = render.Environment(texels, rot)
    tp = texels.clone().requires_grad_(True)
    rp = torch.tensor(rot, dtype=torch.float64, requires_grad=True)
    Render.intIOR = 1.4723
    lines = [f"image_loss_fused in front of an environment: without the new keywords, + rotation gradient, + texel gradient, + both, {a.name} ({len(mesh.faces)} triangles, "
             f"extent {extent:.1f}), supersample 1, Fresnel on, a 512 x 1024 one-channel environment: {torch.cuda.get_device_name(0)}",
             f"ms per call: median of {a.repeat} runs (spread: max - min) after a warm-up; a run is a hipEvent window of `inner` calls; the four forms "
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
            for reflection in (False, True):
                def loss_term(wrt=(), **more):
                    loss = scene.image_loss_fused(cam, H, W, screen, tex, target, ior_int=ior, environment=env, reflection=reflection, **more, **kw)
                    return torch.autograd.grad(loss, [V, ior] + list(wrt))

                forms = [lambda: loss_term(), lambda: loss_term([rp], env_rotation_param=rp), lambda: loss_term([tp], env_texels_param=tp),
                         lambda: loss_term([tp, rp], env_texels_param=tp, env_rotation_param=rp)]
                ((b_ms, b_sp), (r_ms, r_sp), (t_ms, t_sp), (a_ms, a_sp)), inner = alternately(forms, a.repeat)
                lines.append(f"{H:4d} x {W:4d} {str(law):32s} {'reflection' if reflection else 'no reflection':13s} without {b_ms:8.3f} ms (spread {b_sp:.3f})   "
                             f"+ rotation {r_ms:8.3f} ms (spread {r_sp:.3f}, {r_ms - b_ms:+.3f})   + texels {t_ms:8.3f} ms (spread {t_sp:.3f}, {t_ms - b_ms:+.3f})   "
                             f"+ both {a_ms:8.3f} ms (spread {a_sp:.3f}, {a_ms - b_ms:+.3f})   inner {inner}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
