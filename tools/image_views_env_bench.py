"""Cost of the image term of eight views in front of one environment in ONE call (drt_render_image_loss_views_env) against
eight single-view calls into the same accumulators (drt_render_image_loss_env -- the chain of before): horse50k
(horse_vh.ply after one midpoint subdivision, 50 248 triangles), 8 turntable views, each with its screen, a 512 x 1024 environment,
Fresnel on, supersample 1, the three laws of tests/test_gpu_image.py, vertex and IOR gradients, the outer-surface reflection off and on,
at two sizes: 256 x 256 object crops (the fit loop's regime) and 1080 x 1920.  Both sides go through the C ABI, so that neither pays for
autograd; the protocol is tools/image_views_bench.py's:

    8 calls          drt_render_image_loss_env, view after view, one band each
    1 call           drt_render_image_loss_views_env over the eight views in bands of at most --max-samples samples
    1 call, 1 band   the same as a single band (the workspace then holds all eight views)

and one optim.PhotoIteration.step (8 views of 256 x 256 per step, all three terms) with the room and its reflection beside the same step
without the room.

    python tools/image_views_env_bench.py [--repeat 9] [--deterministic] [--out profiles/render_image_loss_views_env.txt]

Times are hipEvent intervals on the current stream: median (min .. max) of ``--repeat`` runs after one warm-up; nothing is asserted but
that the forms of a row agree on the loss and the count."""
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
    ap.add_argument("--max-samples", type=int, default=1 << 22)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 256, 1080, 1920], help="H W pairs")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--no-loop", action="store_true", help="skip the PhotoIteration rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_image_loss_views_env.txt"))
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
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"drt_render_image_loss_views_env against {N_VIEWS} drt_render_image_loss_env calls, {a.name} ({len(mesh.faces)} triangles), {N_VIEWS} turntable views with "
             f"screens, a {ENV_H} x {ENV_W} environment, Fresnel on, supersample 1, vertex and IOR gradients{', deterministic mode' if a.deterministic else ''}: "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.repeat} runs after one warm-up, hipEvent ms", ""]
    for H, W in zip(a.sizes[0::2], a.sizes[1::2]):
        turntable = views.turntable_cameras(center, extent, 72, W, H)
        cams = [turntable[9 * k] for k in range(N_VIEWS)]
        screens = [render.Screen.behind(c, center, extent, 1024, 1024) for c in cams]
        for law in LAWS:
            for reflection in (0, 1):
                kw = dict(max_bounces=law[0], tir=law[1], refraction=law[2], void=0.0, invalid=0.5, environment=env, reflection=bool(reflection))
                Render.intIOR = 1.55                          # the photographs: the same views at another IOR
                photos = torch.stack([scene.render_image(c, H, W, sc, texture, supersample=1, **kw) for c, sc in zip(cams, screens)])
                Render.intIOR = ior
                binding = scene.bind_image_views(cams, H, W, screens, photos, environment=env)
                flags = int(law[1] == "reflect") | (2 if law[2] == "snell" else 0)
                loss, grad, gi = det.scalar(V.device), det.acc(V), det.acc(torch.empty(2, dtype=torch.float64, device="cuda"))
                count = torch.zeros((), dtype=torch.int64, device="cuda")
                ids = (ctypes.c_int * N_VIEWS)(*range(N_VIEWS))
                c21, s9 = binding.args["cameras"], binding.args["screens"]
                env_args = (binding.env.data_ptr(), ENV_H, ENV_W, rot.ctypes.data, reflection)

                def zero():
                    for t in (loss, grad, gi, count):
                        t.zero_()

                def eight():
                    zero()
                    for k in range(N_VIEWS):
                        _lib.check(lib.drt_render_image_loss_env(scene.optix_mesh._h, V.data_ptr(), c21[k].ctypes.data, H, W, 0, H, 1, ior, ext, law[0], flags, 1,
                                                                 s9[k].ctypes.data, texture.data_ptr(), 1024, 1024, 1, fill[0].ctypes.data, fill[1].ctypes.data,
                                                                 binding.targets[k].data_ptr(), None, loss.data_ptr(), grad.data_ptr(), gi.data_ptr(), None,
                                                                 count.data_ptr(), *env_args, stream))

                def one(bands):
                    def run():
                        zero()
                        for r0, r1 in bands:
                            _lib.check(lib.drt_render_image_loss_views_env(scene.optix_mesh._h, V.data_ptr(), binding._h, ids, N_VIEWS, r0, r1, 1, ior, ext, law[0], flags,
                                                                           1, texture.data_ptr(), 1024, 1024, 1, fill[0].ctypes.data, fill[1].ctypes.data,
                                                                           binding.targets.data_ptr(), None, loss.data_ptr(), grad.data_ptr(), gi.data_ptr(),
                                                                           count.data_ptr(), *env_args, stream))
                    return run

                bands = render.plan_bands(N_VIEWS * H, W, 1, a.max_samples)
                rows = [(f"{N_VIEWS} calls", eight), (f"1 call, {len(bands)} band{'s' if len(bands) > 1 else ''}", one(bands))]
                if len(bands) > 1:
                    rows.append(("1 call, 1 band", one([(0, N_VIEWS * H)])))
                base, check = None, None
                for label, fn in rows:
                    ms, lo, hi = timed(fn, a.repeat)
                    base = ms if base is None else base
                    got = (float(det.value(loss)), int(count))
                    check = got if check is None else check
                    assert got[1] == check[1] and abs(got[0] - check[0]) <= 1e-9 * abs(check[0]), (label, got, check)
                    lines.append(f"{H:5d} x {W:<5d} {str(law):32s} reflection {reflection}  {label:18s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f})"
                                 + ("" if fn is eight else f"   x{base / ms:.2f}"))
                binding.release()
        lines.append("")
    if not a.no_loop:
        H = W = 256
        hp = dict(optim.HyperParams, IOR=ior, image_w=100.0)
        Render.intIOR = ior
        gt = Render.Scene(views.displaced_ground_truth(mesh), 0)
        law = LAWS[2]
        tex = texture.cpu().numpy()
        plain = captured_data.SyntheticPhotoData(gt, center, extent, W, H, tex, num_view=N_VIEWS, path_law=law, supersample=1)
        roomed = captured_data.SyntheticPhotoData(gt, center, extent, W, H, tex, num_view=N_VIEWS, path_law=law, supersample=1, environment=env, reflection=True)
        Render.resx = Render.resy = H
        for label, data, more in (("PhotoIteration.step, 8 views of 256 x 256, screen only", plain, {}),
                                  ("PhotoIteration.step, ... in the room, reflection off", roomed, {}),
                                  ("PhotoIteration.step, ... in the room, reflection on", roomed, {"reflection": True})):
            scene.update_verticex(V.clone())
            it = optim.PhotoIteration(scene, data, hp, 0.01, views_per_step=N_VIEWS, path_law=law, **more)
            ms, lo, hi = timed(lambda: it.step(), a.repeat)
            lines.append(f"{label:56s} {str(law):28s} {ms:9.3f} ms ({lo:.3f} .. {hi:.3f})   all three terms, host enqueue included")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
