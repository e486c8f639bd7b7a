"""Gray-code pattern photographs -> the ray targets and masks of a capture, on the device: the front end of a capture of one's own.

    python -m drt_amd.structured_light --frames capture_raw.npz -o name.h5 [--camera redmi|pointgray] [--min-contrast 16] [--mask-shift 1] [--force]

The ray loss needs, per camera pixel, the point on the background screen its light came from (``screen_position`` of a capture file)
and the silhouette ``mask``.  The captures hold them precomputed; neither they nor the code that made them are distributed.  Here a
monitor behind the object shows the stripe patterns of ``gray_patterns``, the camera photographs each one, and

    decode             photographs uint8 [n, F, H, W] -> codes, contrast, mask, covered, positions (k_decode_patterns, one pass)
    PatternData        a ``captured_data.Data`` over decoded photographs: the existing loops run on it unchanged
    capture_arrays     the dict ``captured_data.write_capture`` takes, so the existing loaders and ``visual_hull --capture`` read it
    synthetic_frames   the photographs of a known mesh through ``Scene.render_image``: the stand-in for the undistributed raw ones

The CLI's ``.npz`` holds ``frames``, ``background``, ``cam_proj``, ``cam_k``, ``screens`` and ``tex_hw``.  ``decode`` takes photographs
without background frames; the CLI does not, because the capture file it writes needs the ``mask`` and the mask comes from them.

The law is stated once, in csrc/drt_decode.h (and DESIGN.md section 10.12); tests/decode_ref.py restates it in numpy and the device
agrees with it bit for bit.  There is no CPU fallback: the kernel is the implementation."""
from __future__ import annotations

import argparse
import collections
import os

import numpy as np
import torch

from . import _lib, captured_data, render, views

MIN_TEX, MAX_TEX = 2, 32768
TARGETS = ("object", "all")

DecodeResult = collections.namedtuple("DecodeResult", "codes contrast mask covered positions")


# ---- the patterns ----------------------------------------------------------------------------------------------------------------------
def _tex(tex_h, tex_w):
    for v, name in ((tex_h, "tex_h"), (tex_w, "tex_w")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not MIN_TEX <= v <= MAX_TEX:
            raise ValueError(f"{name} must be an integer in [{MIN_TEX}, {MAX_TEX}], got {v!r}")
    return int(tex_h), int(tex_w)


def _bits(n):
    return max(1, (n - 1).bit_length())


def n_frames(tex_h, tex_w):
    """F = 2 (ceil(log2 tex_w) + ceil(log2 tex_h)): a pattern and its complement per bit of a texel's column and row."""
    tex_h, tex_w = _tex(tex_h, tex_w)
    return 2 * (_bits(tex_w) + _bits(tex_h))


def gray_patterns(tex_h, tex_w):
    """uint8 [F, tex_h, tex_w], values 0 / 255: the frames to show on the monitor, in order.  Frame 2k (k < nbx) is bit nbx - 1 - k of
    the Gray code x ^ (x >> 1) of the texel column, frame 2k + 1 its complement; then the same for the rows."""
    tex_h, tex_w = _tex(tex_h, tex_w)
    out = np.empty((n_frames(tex_h, tex_w), tex_h, tex_w), np.uint8)
    f = 0
    for size, along_x in ((tex_w, True), (tex_h, False)):
        idx = np.arange(size)
        gray = idx ^ (idx >> 1)
        for k in range(_bits(size) - 1, -1, -1):
            line = (((gray >> k) & 1) * 255).astype(np.uint8)
            out[f] = line[None, :] if along_x else line[:, None]
            out[f + 1] = 255 - out[f]
            f += 2
    return out


# ---- argument checks (before anything touches the device) ----------------------------------------------------------------------------
def _is_u8(a):
    return isinstance(a, (np.ndarray, torch.Tensor)) and str(a.dtype).endswith("uint8")


def _check_frames(frames, tex_h, tex_w):
    F = n_frames(tex_h, tex_w)
    if not (_is_u8(frames) and frames.ndim in (3, 4)):
        raise ValueError(f"frames must be a uint8 array [F, H, W] or [n, F, H, W], got {getattr(frames, 'dtype', type(frames))} "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    if frames.ndim == 3:
        frames = frames[None]
    n, f, H, W = (int(s) for s in frames.shape)
    if f != F:
        raise ValueError(f"frames holds {f} frames per view, a {tex_w} x {tex_h} texture needs n_frames = {F}")
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"frames must hold at least one view of at least 1 x 1 pixels, got shape {tuple(frames.shape)}")
    return frames


def _check_background(background, frames):
    if background is None:
        return None
    n, F, H, W = frames.shape
    if not (_is_u8(background) and tuple(background.shape) in ((F, H, W), (n, F, H, W))):
        raise ValueError(f"background must be a uint8 array [{F}, {H}, {W}] (one for all views) or [{n}, {F}, {H}, {W}], got "
                         f"{getattr(background, 'dtype', type(background))} {tuple(getattr(background, 'shape', ()))}")
    return background


def _check_screens(screens, n):
    """float64 numpy [n, 9] (p0, eu, ev per view) from a Screen, a sequence of them, or an array [9], [1, 9] or [n, 9]."""
    if screens is None:
        return None
    if isinstance(screens, render.Screen):
        screens = [screens]
    if isinstance(screens, (list, tuple)) and len(screens) > 0 and all(isinstance(s, render.Screen) for s in screens):
        a = np.stack([s.packed() for s in screens])
    else:
        try:
            a = np.array(screens.detach().cpu().numpy() if isinstance(screens, torch.Tensor) else screens, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"screens must be render.Screen objects or an array [n, 9], got {type(screens).__name__}") from None
        a = a.reshape(1, 9) if a.shape == (9,) else a
    if a.ndim != 2 or a.shape[1] != 9 or a.shape[0] not in (1, n) or not np.isfinite(a).all():
        raise ValueError(f"screens must be one screen or {n} of them as finite [n, 9] (p0, eu, ev), got shape {a.shape}")
    return np.array(np.broadcast_to(a, (n, 9)))


def _check_int(x, name, lo, hi):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= x <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {x!r}")
    return int(x)


def check_decode_args(frames, tex_h, tex_w, screens=None, background=None, min_contrast=16, mask_shift=1, targets=None):
    """The arguments of ``decode`` in the form the launch takes; raises a ValueError that names the bad one.  Needs no GPU."""
    tex_h, tex_w = _tex(tex_h, tex_w)
    frames = _check_frames(frames, tex_h, tex_w)
    background = _check_background(background, frames)
    screens = _check_screens(screens, frames.shape[0])
    min_contrast = _check_int(min_contrast, "min_contrast", 1, 255)
    mask_shift = _check_int(mask_shift, "mask_shift", 1, MAX_TEX)
    if targets is None:
        targets = "object" if background is not None else "all"
    if targets not in TARGETS:
        raise ValueError(f"targets must be one of {TARGETS} or None, got {targets!r}")
    if targets == "object" and background is None:
        raise ValueError("targets = 'object' needs a background: without one there is no mask to restrict the targets to")
    return dict(frames=frames, tex_h=tex_h, tex_w=tex_w, screens=screens, background=background, min_contrast=min_contrast, mask_shift=mask_shift,
                targets=targets)


# ---- the device pass -------------------------------------------------------------------------------------------------------------------
def _stream():
    from .optix_mesh import _stream as s
    return s()


def _device(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _resident(a):
    """A stack the kernel can read in place: a contiguous device tensor (whatever its base address)."""
    return isinstance(a, torch.Tensor) and a.is_cuda and a.is_contiguous()


def decode(frames, tex_h, tex_w, screens=None, background=None, min_contrast=16, mask_shift=1, targets=None):
    """Decode photographs of the patterns of ``gray_patterns(tex_h, tex_w)``: ``frames`` uint8 ``[n, F, H, W]`` or ``[F, H, W]`` (numpy
    or a tensor).  Returns ``DecodeResult`` of device tensors: ``codes`` int16 ``[n, H, W, 2]`` = texel (x, y), (-1, -1) where the pixel
    does not decode (some bit's |pattern - complement| below ``min_contrast``, or a code beyond the texture); ``contrast`` uint8
    ``[n, H, W]``, the smallest such difference.  ``background``: the same patterns photographed without the object, ``[F, H, W]`` for
    all views or ``[n, F, H, W]``; with it ``mask`` uint8 ``[n, H, W]`` is 255 where the background decodes and the object frames do
    not, or decode to a texel at least ``mask_shift`` away, and ``covered`` is 1 where the background decodes; None without.
    ``screens``: a ``render.Screen`` per view (or one for all, or ``[n, 9]``); with them ``positions`` float64 ``[n, H W, 3]`` is the
    world position of the decoded texel, (0, 0, 0) where nothing decodes and -- ``targets="object"``, the default with a background --
    outside the mask (``"all"``: wherever the pixel decodes); an x component of exactly 0 becomes 1e-12.  A stack that is not a
    contiguous device tensor goes to the device view by view, so a capture need not fit at once."""
    a = check_decode_args(frames, tex_h, tex_w, screens, background, min_contrast, mask_shift, targets)
    frames, background = a["frames"], a["background"]
    n, F, H, W = (int(s) for s in frames.shape)
    dev = _device(frames, background)
    shared = background is not None and background.ndim == 3
    zero = int(a["screens"] is not None and a["targets"] == "object")
    lib = _lib.lib()
    with torch.cuda.device(dev):
        codes = torch.empty((n, H, W, 2), dtype=torch.int16, device=dev)
        contrast = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        mask = covered = positions = scr = None
        if background is not None:
            mask, covered = (torch.empty((n, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
        if a["screens"] is not None:
            positions = torch.empty((n, H * W, 3), dtype=torch.float64, device=dev)
            scr = torch.as_tensor(a["screens"], device=dev)

        def launch(fr, bg, stride, v0, nv):
            _lib.check(lib.drt_decode_patterns(fr.data_ptr(), _lib.ptr(bg), stride, nv, H, W, a["tex_h"], a["tex_w"], a["min_contrast"], a["mask_shift"],
                                               None if scr is None else scr[v0:].data_ptr(), zero, codes[v0:].data_ptr(), contrast[v0:].data_ptr(),
                                               None if mask is None else mask[v0:].data_ptr(), None if covered is None else covered[v0:].data_ptr(),
                                               None if positions is None else positions[v0:].data_ptr(), _stream()))

        def up(x):
            if _resident(x):
                return x
            if isinstance(x, np.ndarray) and not x.flags.writeable:          # (torch cannot wrap a read-only array)
                return torch.tensor(x, device=dev)
            return torch.as_tensor(x).to(dev).contiguous()

        if _resident(frames) and (background is None or _resident(background)):
            launch(frames, background, 0 if shared or background is None else F * H * W, 0, n)
        else:
            bg_all = up(background) if shared else None
            for v in range(n):                                   # one view resident at a time
                launch(up(frames[v]), bg_all if shared else (None if background is None else up(background[v])), 0, v, 1)
    return DecodeResult(codes, contrast, mask, covered, positions)


# ---- a capture of decoded photographs --------------------------------------------------------------------------------------------------
def _cameras(cameras, n):
    try:
        cams = [tuple(render._host(m) for m in cam) for cam in cameras]
    except (TypeError, ValueError):
        raise ValueError("cameras must be a sequence of (R, K, R^-1, K^-1)") from None
    if len(cams) != n or any(len(c) != 4 or c[0].shape != (4, 4) or c[1].shape != (3, 3) or c[2].shape != (4, 4) or c[3].shape != (3, 3) for c in cams):
        raise ValueError(f"cameras must hold one (R [4, 4], K [3, 3], R^-1 [4, 4], K^-1 [3, 3]) per view ({n}), got {len(cams)}")
    return cams


class PatternData(captured_data.Data):
    """A capture made of pattern photographs: per view a camera ``(R, K, R^-1, K^-1)``, a ``render.Screen`` and the ``F`` photographs
    of ``gray_patterns(tex_h, tex_w)`` on it (``frames`` uint8 ``[n, F, resy, resx]``), with the ``background`` photographs without the
    object (``[F, resy, resx]`` or per view).  ``get_view`` returns the standard tuple ``(screen_pixel, valid, soft mask, origin,
    ray_dir, camera_M)`` at whatever resolution the photographs have: targets and mask from ``decode``, rays from
    ``views.generate_ray``, the soft mask from ``views.process_mask``.  Built on the device and resident there, like ``SyntheticData``."""

    def __init__(self, cameras, screens, frames, tex_h, tex_w, background, resx, resy, min_contrast=16, mask_shift=1, targets=None, num_view=None,
                 device="cuda", seed=0, name="pattern"):
        a = check_decode_args(frames, tex_h, tex_w, screens, background, min_contrast, mask_shift, targets)
        n, _, H, W = a["frames"].shape
        if (int(resy), int(resx)) != (H, W):
            raise ValueError(f"resy x resx = {resy} x {resx} but the frames are {H} x {W}")
        if a["background"] is None or a["screens"] is None:
            raise ValueError("background and screens are both needed: the mask comes from the background, the targets from the screens")
        cams = _cameras(cameras, n)
        self.resx, self.resy, self.n_total = int(resx), int(resy), n
        self.num_view = n if num_view is None else int(num_view)
        self.name, self.device = name, device
        self.rng = np.random.RandomState(seed)
        r = decode(a["frames"], tex_h, tex_w, a["screens"], a["background"], min_contrast, mask_shift, a["targets"])
        self.decoded = r
        dev = r.codes.device
        binary = r.mask.cpu().numpy()
        self.Views = []
        for v, cam in enumerate(cams):
            origin, ray_dir = views.generate_ray(H, W, cam[3], cam[2], device=dev)
            sp = r.positions[v]
            soft = torch.as_tensor(views.process_mask(binary[v]), dtype=captured_data.Float, device=dev).reshape(-1)
            camera_M = tuple(torch.as_tensor(m, dtype=captured_data.Float, device=dev) for m in cam)
            self.Views.append((sp, (sp[:, 0] != 0).contiguous(), soft, origin, ray_dir, camera_M))
        self._resident = dict(enumerate(self.Views))


def capture_arrays(cameras, screens, frames, tex_h, tex_w, background, camera="redmi", min_contrast=16, mask_shift=1, targets=None):
    """Decode and return the datasets of a capture file as numpy arrays, the dict ``captured_data.write_capture`` takes: ``cam_proj``
    [n, 4, 4], ``cam_k`` [3, 3], ``screen_position`` and ``mask`` (uint8, 0 / 255) in the layout of the named camera class
    (``captured_data.CAMERAS``), and for the PointGrey layout the pinhole rays ``ray_origin`` / ``ray_dir``.  The photographs must have
    that class's resolution, and all views one K."""
    if camera not in captured_data.CAMERAS:
        raise ValueError(f"camera must be one of {tuple(captured_data.CAMERAS)}, got {camera!r}")
    cls = captured_data.CAMERAS[camera]
    a = check_decode_args(frames, tex_h, tex_w, screens, background, min_contrast, mask_shift, targets)
    n, _, H, W = a["frames"].shape
    if (H, W) != (cls.resy, cls.resx):
        raise ValueError(f"camera {camera!r} is {cls.resy} x {cls.resx}, the frames are {H} x {W}")
    if a["background"] is None or a["screens"] is None:
        raise ValueError("background and screens are both needed: the mask comes from the background, the targets from the screens")
    cams = _cameras(cameras, n)
    if any(not np.array_equal(c[1], cams[0][1]) for c in cams):
        raise ValueError("cameras: a capture file holds one cam_k, every view must have the same K")
    r = decode(a["frames"], tex_h, tex_w, a["screens"], a["background"], min_contrast, mask_shift, a["targets"])
    sp = r.positions.cpu().numpy()
    out = {"cam_proj": np.stack([c[0] for c in cams]), "cam_k": cams[0][1].copy(),
           "screen_position": sp if cls.rays_from_file else sp.reshape(n, H, W, 3), "mask": r.mask.cpu().numpy()}
    if cls.rays_from_file:
        rays = [views.generate_ray(H, W, c[3], c[2]) for c in cams]
        out["ray_origin"] = np.stack([o.numpy() for o, _ in rays])
        out["ray_dir"] = np.stack([d.numpy() for _, d in rays])
    return out


# ---- synthetic photographs -------------------------------------------------------------------------------------------------------------
def _unseen_copy(scene_gt, camera_M):
    """The scene's mesh moved behind the camera: a scene the camera does not see, so every pixel looks straight at the screen.  It is a
    second ``Scene`` on the same device, with an acceleration structure of its own: one more build per camera, the price of background
    frames that equal a direct pixel's frames bit for bit (``Scene`` takes no empty mesh)."""
    from . import diffrender, mesh_io
    R = render._host(camera_M[0])
    V = np.asarray(scene_gt.mesh.vertices, np.float64)
    eye = render._host(camera_M[2])[:3, 3]
    zc = R[2, :3] / np.linalg.norm(R[2, :3])
    reach = float(np.linalg.norm(V - eye, axis=1).max())
    return diffrender.Scene(mesh_io.TriMesh(V - (2.0 * reach + 1.0) * zc, np.asarray(scene_gt.mesh.faces)), scene_gt.cuda_device)


def synthetic_frames(scene_gt, camera_M, H, W, screen, tex_h, tex_w, path_law=(2, "drop"), supersample=1, fresnel=False, with_background=True):
    """(frames, background) uint8 ``[F, H, W]`` device tensors (background None without ``with_background``): the photographs of
    ``gray_patterns(tex_h, tex_w)`` on ``screen`` through ``scene_gt``, by ``Scene.render_image`` under ``path_law`` = (max_bounces,
    tir[, refraction]) -- three patterns per call as the three channels, fills 0 (a pixel that sees no screen has contrast 0), bytes by
    ``render.to_bytes``.  The background frames are the same calls on the mesh moved behind the camera, where no ray meets it (a second
    ``Scene`` and its build per call: make the backgrounds once per camera, not per use)."""
    pat = gray_patterns(tex_h, tex_w)
    law = tuple(path_law) + ("reference",) * (3 - len(path_law))

    def photographs(scene):
        out = []
        for i in range(0, len(pat), 3):
            chunk = pat[i:i + 3]
            if len(chunk) < 3:
                chunk = np.concatenate([chunk, np.zeros((3 - len(chunk),) + chunk.shape[1:], np.uint8)])
            tex = np.ascontiguousarray(np.moveaxis(chunk, 0, 2).astype(np.float32) / np.float32(255.0))
            image = scene.render_image(camera_M, H, W, screen, tex, supersample=supersample, max_bounces=law[0], tir=law[1], refraction=law[2],
                                       fresnel=fresnel, void=0.0, invalid=0.0)
            out.append(np.moveaxis(render.to_bytes(image), 2, 0))
        return torch.as_tensor(np.ascontiguousarray(np.concatenate(out)[:len(pat)]), device=scene._dev)

    frames = photographs(scene_gt)
    return frames, (photographs(_unseen_copy(scene_gt, camera_M)) if with_background else None)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description="Decode Gray-code pattern photographs into a capture file (screen_position, mask, cameras).")
    ap.add_argument("--frames", required=True, help=".npz with frames [n, F, H, W] uint8, optional background [F, H, W] or [n, F, H, W], cam_proj "
                    "[n, 4, 4], cam_k [3, 3], screens [n or 1, 9] (p0, eu, ev) and tex_hw (tex_h, tex_w)")
    ap.add_argument("-o", "--output", required=True, help=".h5 or .npz capture file")
    ap.add_argument("--camera", choices=tuple(captured_data.CAMERAS), default="redmi", help="layout (and resolution) of the capture file")
    ap.add_argument("--min-contrast", type=int, default=16)
    ap.add_argument("--mask-shift", type=int, default=1)
    ap.add_argument("--targets", choices=TARGETS, default=None)
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    a = ap.parse_args(argv)
    if os.path.exists(a.output) and not a.force:
        raise SystemExit(f"{a.output} exists: pass --force to overwrite it")
    raw = np.load(a.frames)
    for key in ("frames", "cam_proj", "cam_k", "screens", "tex_hw"):
        if key not in raw.files:
            raise SystemExit(f"{a.frames}: dataset {key!r} is missing")
    if "background" not in raw.files:
        raise SystemExit(f"{a.frames}: no 'background' frames; a capture file needs the mask, and the mask comes from them")
    tex_h, tex_w = (int(v) for v in raw["tex_hw"])
    K = np.asarray(raw["cam_k"], np.float64)
    cams = [(R, K, np.linalg.inv(R), np.linalg.inv(K)) for R in np.asarray(raw["cam_proj"], np.float64)]
    arrays = capture_arrays(cams, raw["screens"], raw["frames"], tex_h, tex_w, raw["background"], a.camera, a.min_contrast, a.mask_shift, a.targets)
    sp = arrays["screen_position"].reshape(len(cams), -1, 3)
    for v in range(len(cams)):
        print(f"view {v}: {100.0 * float((sp[v, :, 0] != 0).mean()):.2f} % of the pixels carry a target, {100.0 * float((arrays['mask'][v] != 0).mean()):.2f} % "
              "are mask")
    captured_data.write_capture(a.output, arrays)
    print(f"wrote {a.output}")
    return arrays


if __name__ == "__main__":
    main()
