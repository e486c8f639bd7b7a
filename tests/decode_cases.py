"""Inputs of the pattern-decoding tests, shared by test_decode_host.py and test_gpu_decode.py; each is built once per process, with the
restatement's outputs (tests/decode_ref.py) computed once beside it and never modified afterwards."""
import functools

import numpy as np

import decode_ref
from conftest import data_path

SIZES = [(1, 1), (1, 67), (5, 7), (17, 23), (32, 20)]             # H x W: odd plane sizes are the point
TEXTURES = [(2, 2), (5, 3), (64, 40), (1024, 600)]                # tex_w x tex_h; 5 x 3: codes beyond the texture must come out invalid
MIN_CONTRAST = [1, 16, 255]
MASK_SHIFT = [1, 3]
BACKGROUND = ["none", "shared", "views"]
E2E = dict(res=24, tex=64, min_contrast=16, n_turntable=8, view=0, distance_factor=1.6)      # at the turntable's default 2.5 only 39 pixels carry a target


def _freeze(case):
    for a in list(case.values()) + list(case["expect"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _stack(rng, codes_x, codes_y, nbx, nby, force=None):
    """uint8 [n, F, H, W] whose pixels show the given codes with contrasts on both sides of every threshold the tests use."""
    shape = codes_x.shape
    gx, gy = codes_x ^ (codes_x >> 1), codes_y ^ (codes_y >> 1)
    bits = np.stack([(gx >> (nbx - 1 - k)) & 1 for k in range(nbx)] + [(gy >> (nby - 1 - k)) & 1 for k in range(nby)], 1).astype(bool)
    cls = np.broadcast_to(rng.random(shape)[:, None], bits.shape)
    good = rng.choice([40, 120, 254, 255], bits.shape)
    mixed = rng.choice([0, 1, 2, 15, 16, 17, 40, 255], bits.shape)
    delta = np.where(cls < 0.5, good, np.where(cls < 0.65, 255, mixed))
    if force is not None:
        delta[force] = 255
    hi = rng.integers(delta, 256)
    lo = hi - delta
    out = np.empty((shape[0], 2 * (nbx + nby)) + shape[1:], np.uint8)
    out[:, 0::2] = np.where(bits, hi, lo)
    out[:, 1::2] = np.where(bits, lo, hi)
    return out


def random_case(H, W, tex_w, tex_h, min_contrast=16, mask_shift=1, background="shared", screens=True, n=2, seed=0, zero_x=False, targets_object=False):
    rng = np.random.default_rng([seed, H, W, tex_w, tex_h])
    nbx, nby = decode_ref.n_bits(tex_w), decode_ref.n_bits(tex_h)
    cx, cy = rng.integers(0, 1 << nbx, (n, H, W)), rng.integers(0, 1 << nby, (n, H, W))
    force = None
    scr = None
    if screens:
        scr = rng.standard_normal((n, 9)) * np.array([20.0] * 3 + [0.5] * 6)
    if zero_x:                                                # (p0 + 3 eu) + y ev has an x component of exactly 0 at pixel (0, 0) of every view
        scr[:] = np.array([-3.0, 0.5, 2.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.0])
        cx[:, 0, 0], cy[:, 0, 0] = 3, 1
        force = (slice(None), slice(None), 0, 0)
    frames = _stack(rng, cx, cy, nbx, nby, force)
    bg = None
    if background != "none":
        m = n if background == "views" else 1
        kind = rng.random((m, H, W))
        bx = np.where(kind < 0.4, cx[:m], np.where(kind < 0.6, cx[:m] + rng.choice([-1, 1], (m, H, W)), np.where(kind < 0.8, cx[:m], rng.integers(0, 1 << nbx, (m, H, W)))))
        by = np.where((kind >= 0.6) & (kind < 0.8), cy[:m] + rng.integers(-3, 4, (m, H, W)), np.where(kind < 0.8, cy[:m], rng.integers(0, 1 << nby, (m, H, W))))
        bg = _stack(rng, np.clip(bx, 0, (1 << nbx) - 1), np.clip(by, 0, (1 << nby) - 1), nbx, nby, force)
        bg = bg if background == "views" else bg[0]
    zero = bool(targets_object and bg is not None and scr is not None)
    case = dict(frames=frames, background=bg, screens=scr, tex_h=tex_h, tex_w=tex_w, min_contrast=min_contrast, mask_shift=mask_shift, zero=zero)
    case["expect"] = decode_ref.decode(frames, tex_h, tex_w, scr, bg, min_contrast, mask_shift, zero)
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def grid_case(i):
    """Case i of the 5 sizes x 4 textures, with the contrasts, shifts, background forms and the absence of screens dealt over them."""
    (H, W), (tex_w, tex_h) = SIZES[i % 5], TEXTURES[i // 5]
    return random_case(H, W, tex_w, tex_h, MIN_CONTRAST[i % 3], MASK_SHIFT[(i // 3) % 2], BACKGROUND[(i + i // 3) % 3], screens=i % 4 != 3,
                       n=3 if i % 2 else 2, seed=i, targets_object=i % 2 == 0)


@functools.lru_cache(maxsize=None)
def zero_x_case():
    return random_case(5, 7, 64, 40, 16, 1, "shared", n=2, seed=99, zero_x=True)


@functools.lru_cache(maxsize=None)
def big_case(H, W):
    return random_case(H, W, 64, 40, 16, 1, "views" if H == 3 else "shared", n=2, seed=7, targets_object=True)


@functools.lru_cache(maxsize=None)
def hand_e2e():
    """The hand in front of a 64 x 64 screen (Screen.behind), a 24 x 24 image, s = 1, Fresnel off, law (2, "drop"): the photographs by
    tests/image_ref.py and the oracle's tracer, their background, the restatement's decode, and the traced truth per pixel."""
    import image_ref
    from drt_amd import mesh_io, render, views
    res, tex = E2E["res"], E2E["tex"]
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    center, extent = views.mesh_frame(mesh.vertices)
    cam = views.turntable_cameras(center, extent, E2E["n_turntable"], res, res, distance_factor=E2E["distance_factor"])[E2E["view"]]
    screen = render.Screen.behind(cam, center, extent, tex, tex)
    frames, r = decode_ref.render_frames(mesh.faces, mesh.vertices, cam, res, res, screen, tex, tex)
    background = decode_ref.background_frames(cam, res, res, screen, tex, tex)
    scr = screen.packed()[None]
    case = dict(frames=frames[None], background=background, screens=scr, tex_h=tex, tex_w=tex, min_contrast=E2E["min_contrast"], mask_shift=1, zero=False,
                camera=cam, screen=screen, center=center, extent=extent)
    case["expect"] = decode_ref.decode(case["frames"], tex, tex, scr, background, E2E["min_contrast"], 1, False)
    through = (r["cls"] == image_ref.THROUGH) & r["on"]
    case["truth"] = dict(valid=through.numpy(), u=r["u"].numpy(), v=r["v"].numpy(), hit=(r["hit"] > 0).numpy().reshape(-1),
                         target=(r["out_ori"] + r["t"].view(-1, 1) * r["out_dir"]).numpy())
    return _freeze(case)


def host_cases():
    """(id, thunk): the unaligned planes first."""
    order = sorted(range(20), key=lambda i: (SIZES[i % 5][0] * SIZES[i % 5][1]) % 8 == 0)
    cases = [(f"grid{i}-{SIZES[i % 5][0]}x{SIZES[i % 5][1]}-tex{TEXTURES[i // 5][0]}x{TEXTURES[i // 5][1]}", functools.partial(grid_case, i)) for i in order]
    return cases + [("zero-x", zero_x_case), ("hand-rendered", hand_e2e)]


def gpu_cases():
    return host_cases() + [("64x48", functools.partial(big_case, 64, 48)), ("3x1031", functools.partial(big_case, 3, 1031))]


def nearest_texel_check(truth, codes, positions, screen9, min_contrast):
    """The end-to-end assertions on one view: (share of valid pixels excluded by the margin, number checked).  Every pixel whose true
    (u, v) lie farther than (min_contrast + 2) / 510 texel from a half-integer on both axes must decode to exactly (round u, round v) --
    bilinear sampling of a pattern and its complement decodes to the nearer texel, with contrast |1 - 2 f| 255 less the two uint8
    roundings -- and its position must lie within half a texel diagonal (+ 1e-9) of the traced target."""
    margin = (min_contrast + 2) / 510.0
    u, v, valid = truth["u"], truth["v"], truth["valid"]
    far = lambda w: np.abs(w - np.floor(w) - 0.5) > margin          # noqa: E731
    sel = valid & far(np.where(valid, u, 0.25)) & far(np.where(valid, v, 0.25))
    assert valid.sum() > 50
    xy = codes.reshape(-1, 2)[sel]
    assert np.array_equal(xy[:, 0], np.rint(u[sel]).astype(np.int16)) and np.array_equal(xy[:, 1], np.rint(v[sel]).astype(np.int16))
    bound = 0.5 * np.sqrt((screen9[3:6] ** 2).sum() + (screen9[6:9] ** 2).sum()) + 1e-9
    assert np.linalg.norm(positions.reshape(-1, 3)[sel] - truth["target"][sel], axis=1).max() <= bound
    return 1.0 - sel.sum() / valid.sum(), int(sel.sum())
