"""Numpy restatement of the Gray-code decoding law (test only), written from the law and not from
drt_amd/csrc/drt_decode.h.

A screen of tex_w x tex_h texels shows F = 2 (nbx + nby) frames: frame 2k (k < nbx) is bit nbx - 1 - k of g(x) = x ^ (x >> 1) at texel
column x (white = 1), frame 2k + 1 its complement, then the same for rows.  Per pixel and bit: a = pattern frame, b = complement,
bit = a > b, c = |a - b|; contrast = min c; Gray -> binary by the prefix XOR; the pixel decodes iff contrast >= min_contrast and the code
lies inside the texture, else its code is (-1, -1).  Mask 255 iff the background decodes and the object frames do not or moved by
max(|dx|, |dy|) >= mask_shift.  Position (p0 + x eu) + y ev, an x component of exactly 0 -> 1e-12, zeros where nothing decodes (or, on
request, outside the mask).  Everything but the position is integer arithmetic; the position is elementwise float64 in that association."""
import numpy as np


def n_bits(n):
    """ceil(log2 n), at least 1."""
    return max(1, (int(n) - 1).bit_length())


def n_frames(tex_h, tex_w):
    return 2 * (n_bits(tex_w) + n_bits(tex_h))


def patterns(tex_h, tex_w):
    """uint8 [F, tex_h, tex_w], values 0 / 255."""
    out = []
    for size, axis in ((tex_w, 1), (tex_h, 0)):
        idx = np.arange(size)
        gray = idx ^ (idx >> 1)
        nb = n_bits(size)
        for k in range(nb):
            line = ((gray >> (nb - 1 - k)) & 1).astype(np.uint8) * 255
            plane = np.broadcast_to(line[None, :] if axis == 1 else line[:, None], (tex_h, tex_w))
            out += [plane, 255 - plane]
    return np.stack(out).astype(np.uint8)


def gray_to_binary(g):
    """Bit i of the result is the XOR of the bits i, i + 1, ... of g."""
    b = g.copy()
    shift = g >> 1
    while shift.any():
        b ^= shift
        shift = shift >> 1
    return b


def decode_stack(frames, tex_h, tex_w, min_contrast):
    """frames uint8 [..., F, H, W] -> (ok bool [..., H, W], x, y int64 (meaningless where not ok), contrast uint8)."""
    nbx, nby = n_bits(tex_w), n_bits(tex_h)
    assert frames.dtype == np.uint8 and frames.shape[-3] == 2 * (nbx + nby)
    f = np.moveaxis(frames, -3, 0).astype(np.int64)
    a, b = f[0::2], f[1::2]
    bit = (a > b).astype(np.int64)
    contrast = np.abs(a - b).min(0)
    gx = np.zeros(contrast.shape, np.int64)
    gy = np.zeros(contrast.shape, np.int64)
    for k in range(nbx):
        gx |= bit[k] << (nbx - 1 - k)
    for k in range(nby):
        gy |= bit[nbx + k] << (nby - 1 - k)
    x, y = gray_to_binary(gx), gray_to_binary(gy)
    ok = (contrast >= min_contrast) & (x < tex_w) & (y < tex_h)
    return ok, x, y, contrast.astype(np.uint8)


def decode(frames, tex_h, tex_w, screens=None, background=None, min_contrast=16, mask_shift=1, zero_outside_mask=False):
    """frames uint8 [n, F, H, W]; background None, [F, H, W] or [n, F, H, W]; screens None or float64 [n, 9].  dict(codes int16
    [n, H, W, 2], contrast uint8 [n, H, W], mask / covered uint8 [n, H, W] or None, positions float64 [n, H W, 3] or None)."""
    n, _, H, W = frames.shape
    ok, x, y, contrast = decode_stack(frames, tex_h, tex_w, min_contrast)
    codes = np.where(ok[..., None], np.stack([x, y], -1), -1).astype(np.int16)
    mask = covered = None
    if background is not None:
        okb, xb, yb, _ = decode_stack(background, tex_h, tex_w, min_contrast)
        okb, xb, yb = (np.broadcast_to(v, ok.shape) for v in (okb, xb, yb))
        moved = np.maximum(np.abs(x - xb), np.abs(y - yb)) >= mask_shift
        mask = np.where(okb & (~ok | moved), 255, 0).astype(np.uint8)
        covered = okb.astype(np.uint8)
    positions = None
    if screens is not None:
        s = np.asarray(screens, np.float64).reshape(n, 1, 1, 9)
        xf, yf = x.astype(np.float64)[..., None], y.astype(np.float64)[..., None]
        pos = (s[..., 0:3] + xf * s[..., 3:6]) + yf * s[..., 6:9]
        pos[..., 0] = np.where(pos[..., 0] == 0.0, 1e-12, pos[..., 0])
        keep = ok & (mask != 0) if zero_outside_mask else ok
        positions = np.where(keep[..., None], pos, 0.0).reshape(n, H * W, 3)
    return dict(codes=codes, contrast=contrast, mask=mask, covered=covered, positions=positions)


def background_frames(camera_M, height, width, screen, tex_h, tex_w, s=1):
    """The background photographs: the patterns seen by the camera with nothing in front of the screen (every sample is a direct one),
    three patterns per render as the three channels, fills 0, bytes by rint(clip * 255)."""
    return render_frames(np.zeros((0, 3), np.int64), np.zeros((0, 3)), camera_M, height, width, screen, tex_h, tex_w, s=s)[0]


def render_frames(faces, V, camera_M, height, width, screen, tex_h, tex_w, s=1, max_bounces=2, tir="drop", fresnel=False):
    """(frames uint8 [F, H, W], the last render's dict) through tests/image_ref.py and the oracle's tracer."""
    import image_ref
    pat = patterns(tex_h, tex_w)
    F = len(pat)
    out, r = [], None
    for i in range(0, F, 3):
        chunk = pat[i:i + 3]
        if len(chunk) < 3:
            chunk = np.concatenate([chunk, np.zeros((3 - len(chunk), tex_h, tex_w), np.uint8)])
        tex = np.ascontiguousarray(np.moveaxis(chunk, 0, 2).astype(np.float32) / np.float32(255.0))
        r = image_ref.render(faces, V, camera_M, height, width, screen, tex, s=s, max_bounces=max_bounces, tir=tir, fresnel=fresnel)
        img = r["image"].numpy().astype(np.float64)
        out.append(np.moveaxis(np.rint(np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8), 2, 0))
    return np.ascontiguousarray(np.concatenate(out)[:F]), r
