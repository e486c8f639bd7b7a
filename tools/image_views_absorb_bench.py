"""Cost of absorbing glass in the image term of eight views in ONE call (drt_render_image_loss_views_absorb): horse50k
(horse_vh.ply after one midpoint subdivision, 50 248 triangles), 8 turntable views of 256 x 256 object crops, each with its screen, a
512 x 1024 environment, Fresnel on, supersample 1, the three laws of tests/test_gpu_image.py, vertex, IOR and sigma gradients.  Everything
goes through the C ABI, so that no side pays for autograd; the protocol is tools/image_views_env_bench.py's:

    screens   8 calls            drt_render_image_loss_absorb, view after view (the chain of DESIGN.md 10.7)
              1 call             drt_render_image_loss_views_absorb over the eight views, no environment        (the batching)
              1 call, clear      drt_render_image_loss_views                                                    (the payload)
    room      1 call, clear      drt_render_image_loss_views_env, reflection off and on
              1 call             drt_render_image_loss_views_absorb, the same                                   (the payload)

and one optim.PhotoIteration.step (8 views of 256 x 256 per step, all three terms, in the room with the reflection) with clear glass, with
sigma fixed and with absorption_lr > 0 -- the last reads C numbers back and synchronises once per step.

    python tools/image_views_absorb_bench.py [--repeat 9] [--deterministic] [--out profiles/render_image_loss_views_absorb.txt]

Times are hipEvent intervals on the current stream: median (min .. max) of ``--repeat`` runs after one warm-up; nothing is asserted but
that the forms that compute the same thing agree on the loss and the count."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAWS = [(2, "drop", "reference"), (6, "reflect", "reference"), (6, "reflect", "snell")]
N_VIEWS = 8
ENV_H, ENV_W = 512, 1024
SIGMA = 0.012              # per unit of mesh length (tests/image_absorb_cases.py SIGMA1)


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


def room(channels, seed=11):
    """A smooth random panorama: an 8 x 16 random grid enlarged bilinearly to 512 x 1024, so that neighbouring texels differ little."""
    coarse = torch.as_tensor(np.random.default_rng(seed).random((1, channels, 8, 16)).astype(np.float32))
    fine = torch.nn.functional.interpolate(coarse, size=(ENV_H, ENV_W), mode="bilinear", align_corners=False)
    return np.ascontiguousarray(fine[0].permute(1, 2, 0).numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--name", default="horse")
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 256], help="H W")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--no-loop", action="store_true", help="skip the PhotoIteration rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss_views_absorb.txt"))
    a = ap.parse_args(argv)
    from drt_amd import _lib, captured_data, det, diffrender as Render, mesh_io, optim, render, views
    det.enable(a.deterministic)
    lib = _lib.lib()
    mesh = mesh_io.subdivide_midpoint(mesh_io.read_ply(os.path.join(ROOT, "data", f"{a.name}_vh.ply")))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    scene.update_verticex(V)
    ior, ext = 1.4723, float(Render.extIOR)
    center, extent = views.mesh_frame(mesh.vertices)
    texture = torch.as_tensor(render.checker(1024, 1024, 16), device="cuda").contiguous()
    env = render.Environment(torch.as_tensor(room(1), device="cuda").contiguous(), render.Environment.yaw(30.0))
    rot = env.packed()
    fill = np.zeros(1), np.full(1, 0.5)
    sigma = np.full(1, SIGMA)
    stream = torch.cuda.current_stream().cuda_stream
    H, W = a.size
    lines = [f"drt_render_image_loss_views_absorb, {a.name} ({len(mesh.faces)} triangles), {N_VIEWS} turntable views of {H} x {W} with screens, a {ENV_H} x {ENV_W} "
             f"environment, sigma = {SIGMA}, Fresnel on, supersample 1, vertex, IOR and sigma gradients{', deterministic mode' if a.deterministic else ''}: "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.repeat} runs after one warm-up, hipEvent ms", ""]
    turntable = views.turntable_cameras(center, extent, 72, W, H)
    cams = [turntable[9 * k] for k in range(N_VIEWS)]
    screens = [render.Screen.behind(c, center, extent, 1024, 1024) for c in cams]
    ids = (ctypes.c_int * N_VIEWS)(*range(N_VIEWS))
    loss, grad, gi, gs = det.scalar(V.device), det.acc(V), det.acc(torch.empty(2, dtype=torch.float64, device="cuda")), det.acc(torch.empty(1, dtype=torch.float64, device="cuda"))
    count = torch.zeros((), dtype=torch.int64, device="cuda")

    def zero():
        for t in (loss, grad, gi, gs, count):
            t.zero_()

    for law in LAWS:
        flags = int(law[1] == "reflect") | (2 if law[2] == "snell" else 0)
        kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5)
        for in_room, reflection in ((False, 0), (True, 0), (True, 1)):
            more = dict(environment=env, reflection=bool(reflection)) if in_room else {}
            Render.intIOR = 1.55                          # the photographs: the same views of clear glass at another IOR
            photos = torch.stack([scene.render_image(c, H, W, sc, texture, supersample=1, **kw, **more) for c, sc in zip(cams, screens)])
            Render.intIOR = ior
            binding = scene.bind_image_views(cams, H, W, screens, photos, **({"environment": env} if in_room else {}))
            c21, s9 = binding.args["cameras"], binding.args["screens"]
            head = (scene.optix_mesh._h, V.data_ptr(), binding._h, ids, N_VIEWS, 0, N_VIEWS * H, 1, ior, ext, law[0], flags, 1, texture.data_ptr(), 1024, 1024, 1,
                    fill[0].ctypes.data, fill[1].ctypes.data, binding.targets.data_ptr(), None, loss.data_ptr(), grad.data_ptr(), gi.data_ptr(), count.data_ptr())
            env_args = (binding.env.data_ptr(), ENV_H, ENV_W, rot.ctypes.data, reflection) if in_room else (None, 0, 0, None, 0)

            def eight():
                zero()
                for k in range(N_VIEWS):
                    _lib.check(lib.drt_render_image_loss_absorb(scene.optix_mesh._h, V.data_ptr(), c21[k].ctypes.data, H, W, 0, H, 1, ior, ext, law[0], flags, 1,
                                                                s9[k].ctypes.data, texture.data_ptr(), 1024, 1024, 1, fill[0].ctypes.data, fill[1].ctypes.data,
                                                                binding.targets[k].data_ptr(), None, loss.data_ptr(), grad.data_ptr(), gi.data_ptr(), None,
                                                                count.data_ptr(), sigma.ctypes.data, gs.data_ptr(), stream))

            def absorbing():
                zero()
                _lib.check(lib.drt_render_image_loss_views_absorb(*head, sigma.ctypes.data, gs.data_ptr(), *env_args, None, stream))

            def clear():
                zero()
                if in_room:
                    _lib.check(lib.drt_render_image_loss_views_env(*head, *env_args, stream))
                else:
                    _lib.check(lib.drt_render_image_loss_views(*head, stream))

            where = f"room, reflection {reflection}" if in_room else "screens"
            rows = ([(f"{N_VIEWS} absorbing calls", eight, "absorb")] if not in_room else []) + [("1 call, clear", clear, "clear"), ("1 call, absorbing", absorbing, "absorb")]
            seen, times = {}, {}
            for label, fn, what in rows:
                ms, lo, hi = timed(fn, a.repeat)
                got = (float(det.value(loss)), int(count))
                check = seen.setdefault(what, got)
                assert got[1] == check[1] and abs(got[0] - check[0]) <= 1e-9 * abs(check[0]), (label, got, check)
                times[label] = ms
                note = ""
                if label == "1 call, absorbing":
                    note = f"   clear x{ms / times['1 call, clear']:.3f}" + (f"   chain / call x{times[f'{N_VIEWS} absorbing calls'] / ms:.2f}" if not in_room else "")
                lines.append(f"{H:5d} x {W:<5d} {str(law):32s} {where:22s} {label:20s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f}){note}")
            binding.release()
        lines.append("")
    if not a.no_loop:
        hp = dict(optim.HyperParams, IOR=ior, image_w=100.0)
        Render.intIOR = ior
        gt = Render.Scene(views.displaced_ground_truth(mesh), 0)
        law = LAWS[2]
        tex = texture.cpu().numpy()
        data = captured_data.SyntheticPhotoData(gt, center, extent, W, H, tex, num_view=N_VIEWS, path_law=law, supersample=1, environment=env, reflection=True,
                                                absorption=SIGMA)
        Render.resx, Render.resy = W, H
        for label, more in (("PhotoIteration.step in the room, reflection on, clear glass", {}),
                            ("PhotoIteration.step ..., sigma fixed", {"absorption": SIGMA}),
                            ("PhotoIteration.step ..., absorption_lr > 0 (C numbers read back per step)", {"absorption": 0.0, "absorption_lr": 1e-4})):
            scene.update_verticex(V.clone())
            it = optim.PhotoIteration(scene, data, hp, 0.01, views_per_step=N_VIEWS, path_law=law, reflection=True, **more)
            ms, lo, hi = timed(lambda: it.step(), a.repeat)
            lines.append(f"{label:78s} {str(law):28s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f})   all three terms, host enqueue included")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
