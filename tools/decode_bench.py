"""Milliseconds per view of the pattern decode at capture size: 8 views of 44 frames at 1080 x 1920 with one shared background.

    python tools/decode_bench.py [--views 8] [--resx 1920] [--resy 1080] [--repeat 20] [--offset 0] [--per-view-background] [--label TEXT] [--out profiles/decode_patterns.txt] [--append]

The monitor is 1920 x 1080 texels (11 + 11 bits: 44 frames) and every camera pixel looks at its own texel, moved by a few texels per view,
so every pixel decodes and carries a target.  A shared background (91 MB) fits the Infinity Cache and is read from HBM once, not once per
view; --per-view-background reads every input byte from HBM.  Times are hipEvent intervals around `drt_decode_patterns` with all five outputs on the
current stream: the median, the best and the worst of `--repeat` launches after three warm-up launches.  GB/s is against the algorithmic
bytes, 2 F in (object and background frames) plus 4 + 1 + 1 + 1 + 24 out per pixel; the fraction is of the 8.0 TB/s HBM3E peak (6.29 TB/s
is what a float4 copy reaches).  DRT_HIP_LIB selects a library built with other -DDRT_DECODE_RUN / -DDRT_DECODE_INFLIGHT.  Nothing is asserted."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--resx", type=int, default=1920)
    ap.add_argument("--resy", type=int, default=1080)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--offset", type=int, default=0, help="start the object frames this many bytes into their buffer (1: no plane is aligned)")
    ap.add_argument("--per-view-background", action="store_true", help="one background stack per view: nothing of the input is read twice")
    ap.add_argument("--label", default="as built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_patterns.txt"))
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args(argv)
    from drt_amd import _lib, structured_light
    from drt_amd.optix_mesh import _stream
    n, H, W = a.views, a.resy, a.resx
    tex_h, tex_w = H, W
    F = structured_light.n_frames(tex_h, tex_w)
    pat = torch.as_tensor(structured_light.gray_patterns(tex_h, tex_w), device="cuda")
    buf = torch.empty(n * F * H * W + 16, dtype=torch.uint8, device="cuda")
    frames = buf[a.offset:a.offset + n * F * H * W].view(n, F, H, W)
    for v in range(n):
        frames[v] = torch.roll(pat, shifts=(3 * v, 5 * v), dims=(1, 2))
    background = pat.unsqueeze(0).repeat(n, 1, 1, 1).contiguous() if a.per_view_background else pat
    stride = F * H * W if a.per_view_background else 0
    screens = torch.tensor([[-960.0, -540.0, 2000.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n, dtype=torch.float64, device="cuda")
    codes = torch.empty((n, H, W, 2), dtype=torch.int16, device="cuda")
    contrast, mask, covered = (torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(3))
    positions = torch.empty((n, H * W, 3), dtype=torch.float64, device="cuda")
    lib = _lib.lib()

    def launch():
        _lib.check(lib.drt_decode_patterns(frames.data_ptr(), background.data_ptr(), stride, n, H, W, tex_h, tex_w, 16, 1, screens.data_ptr(), 1, codes.data_ptr(),
                                           contrast.data_ptr(), mask.data_ptr(), covered.data_ptr(), positions.data_ptr(), _stream()))

    for _ in range(3):
        launch()
    ms = []
    for _ in range(a.repeat):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    decoded = float((codes[..., 0] >= 0).float().mean())
    moved = float((mask[1:] != 0).float().mean()) if n > 1 else 0.0
    med, best, worst = statistics.median(ms), min(ms), max(ms)
    bytes_per_pixel = 2 * F + 4 + 1 + 1 + 1 + 24
    total = bytes_per_pixel * n * H * W
    rate = total / (med * 1e-3)
    text = (f"decode_patterns [{a.label}]: {torch.cuda.get_device_name(0)}; {n} views x {F} frames x {H} x {W}, {'one background per view' if a.per_view_background else 'shared background'}, "
            f"frames at byte offset {a.offset}; "
            f"{a.repeat} launches after 3 warm-up, hipEvent ms\n"
            f"  per launch  median {med:.3f} ms (best {best:.3f}, worst {worst:.3f});  per view {med / n:.3f} ms\n"
            f"  {bytes_per_pixel} algorithmic B per pixel ({2 * F} in, 31 out), {total / 1e9:.3f} GB per launch: {rate / 1e9:.0f} GB/s = "
            f"{100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s peak, {100 * rate / HBM_COPY:.1f} % of a float4 copy's 6.29 TB/s\n"
            f"  decoded {100 * decoded:.2f} % of the pixels; mask on {100 * moved:.2f} % of the pixels of the views after the first\n")
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
