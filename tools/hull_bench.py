"""Per-stage milliseconds of the visual hull at capture size: 72 views of 1080 x 1920 carved into a 256^3 grid (1.2 G projections),
surface extraction, and the whole `visual_hull` call with component selection and remesh.

    python tools/hull_bench.py [--name horse] [--views 72] [--resolution 256] [--repeat 5] [--out profiles/visual_hull.txt]

The masks are the silhouettes of `<name>_scan.ply` (or the shipped hull) on the phone camera's turntable, traced on the device.  Times are
hipEvent intervals around each stage on the current stream, the median of `--repeat` runs after one warm-up; nothing is asserted."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--resx", type=int, default=1920)
    ap.add_argument("--resy", type=int, default=1080)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visual_hull.txt"))
    a = ap.parse_args(argv)
    from drt_amd import _lib, diffrender as Render, views, visual_hull
    from drt_amd.optix_mesh import _stream
    scan = os.path.join(ROOT, "data", f"{a.name}_scan.ply")
    gt = Render.Scene(scan if os.path.exists(scan) else os.path.join(ROOT, "data", f"{a.name}_vh.ply"), 0)
    center, extent = views.mesh_frame(gt.mesh.vertices)
    masks, P = [], []
    for R, K, Rinv, Kinv in views.turntable_cameras(center, extent, a.views, a.resx, a.resy):
        o, d = views.generate_ray(a.resy, a.resx, Kinv, Rinv, device="cuda")
        masks.append((gt.render_mask(o, d) > 0).view(a.resy, a.resx).to(torch.uint8))
        P.append(K @ R[:3, :])
    masks, P = torch.stack(masks).contiguous(), np.stack(P)
    bounds = (center - 0.6 * extent, center + 0.6 * extent)
    lo, cell, dims = visual_hull.hull_grid(bounds, a.resolution)
    n = dims[0] * dims[1] * dims[2]
    rows = []
    med, best, field = timed(lambda: visual_hull.silhouette_field(masks, P, lo, cell, dims), a.repeat)
    rows.append(("k_hull_field", med, best, f"{a.views} x {a.resy} x {a.resx} masks, {dims[0]} x {dims[1]} x {dims[2]} corners, "
                 f"{a.views * n / 1e9:.2f} G projections at most; {a.views * n / med / 1e6:.1f} G projections/s if none were skipped"))
    lib = _lib.lib()
    em, nv_, nt_ = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    med, best, _ = timed(lambda: _lib.check(lib.drt_hull_mark(field.data_ptr(), *dims, 0.5, em.data_ptr(), nv_.data_ptr(), nt_.data_ptr(), _stream())), a.repeat)
    rows.append(("k_hull_mark", med, best, f"{n} corners, {n * 7 / med / 1e6:.1f} GB/s of field reads and byte writes at 4 + 3 B per corner"))
    med, best, sums = timed(lambda: (torch.cumsum(nv_, 0, dtype=torch.int32), torch.cumsum(nt_, 0, dtype=torch.int32)), a.repeat)
    rows.append(("2 x torch.cumsum", med, best, "uint8 -> int32, plumbing"))
    nv, nf = int(sums[0][-1]), int(sums[1][-1])
    V, F = torch.empty((nv, 3), dtype=torch.float64, device="cuda"), torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    med, best, _ = timed(lambda: _lib.check(lib.drt_hull_emit(field.data_ptr(), *dims, lo[0], lo[1], lo[2], cell, 0.5, em.data_ptr(), sums[0].data_ptr(),
                                                               sums[1].data_ptr(), nv, nf, V.data_ptr(), F.data_ptr(), _stream())), a.repeat)
    rows.append(("k_hull_emit", med, best, f"{nv} vertices, {nf} triangles"))
    med, best, _ = timed(lambda: visual_hull.extract_surface(field, lo, cell), a.repeat)
    rows.append(("extract_surface", med, best, "mark + sums + one read-back + emit, allocations included"))

    class _Views:                                        # the part of captured_data.Data that visual_hull reads
        resx, resy = a.resx, a.resy
        Views = list(range(a.views))

        def get_view(self, k):
            R, K = (torch.as_tensor(m) for m in views.turntable_cameras(center, extent, a.views, a.resx, a.resy)[k][:2])
            return (None, None, masks[k].to(torch.float64).reshape(-1), None, None, (R, K))

    report = {}
    visual_hull.visual_hull(_Views(), a.resolution, bounds=bounds, report=report)          # warm-up
    report = {}
    visual_hull.visual_hull(_Views(), a.resolution, bounds=bounds, report=report)
    lines = [f"visual hull, {a.name}: {torch.cuda.get_device_name(0)}; median (best) of {a.repeat} runs after one warm-up, hipEvent ms", ""]
    lines += [f"{name:18s} {med:10.3f} ms ({best:.3f})   {note}" for name, med, best, note in rows]
    lines += ["", "visual_hull(resolution=%d), host seconds per stage (synchronised; one run after a warm-up):" % a.resolution,
              "  " + json.dumps({k: round(v, 4) for k, v in report["seconds"].items()}),
              "  " + json.dumps({k: v for k, v in report.items() if k != "seconds"})]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
