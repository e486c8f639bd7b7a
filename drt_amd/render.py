"""The refracted image of a mesh in front of a textured screen: what a camera sees THROUGH the glass object.

    python -m drt_amd.render --name horse [--mesh result.ply] [--capture horse.h5 | --views N] --view-ids 0 9 18 --res H W
                             --supersample 3 --max-bounces 6 --tir reflect --refraction snell [--no-fresnel]
                             [--background checker|ramp|FILE] [--environment FILE [--env-rotation ...] [--no-screen] [--reflection]] -o DIR [--force]

``Scene.render_image`` (drt_amd.diffrender) is the entry point; this module holds what goes with it: the screen, procedural
textures, image files, the band plan and the command line.  The law is stated once, in csrc/drt_image.h (and DESIGN.md section 10.2):
s x s sample rays per pixel made in the kernel, the K-interaction path law of ``Scene.render_paths`` with a Fresnel throughput, the
exit ray's bilinear sample of the screen's texture, the mean per pixel.  Forward only: the image has no gradient.  There is no CPU
fallback: the kernels are the implementation (tests/image_ref.py restates the law for the tests)."""
from __future__ import annotations

import argparse
import json
import os
import re

import numpy as np

MAX_SUPERSAMPLE = 4
ORTHO_TOL = 1e-12


class Screen:
    """A textured planar screen: ``p0`` the world position of texel (0, 0), ``eu`` / ``ev`` the world vectors of one texel step along the
    texture's x and y.  The axes must be orthogonal (|eu . ev| <= 1e-12 |eu| |ev|) and non-zero; the screen has two faces."""

    def __init__(self, p0, eu, ev):
        self.p0, self.eu, self.ev = (_vec3(a, n) for a, n in ((p0, "p0"), (eu, "eu"), (ev, "ev")))
        lu, lv = float(np.linalg.norm(self.eu)), float(np.linalg.norm(self.ev))
        if not (lu > 0.0 and lv > 0.0):
            raise ValueError(f"screen: eu and ev must be non-zero, got |eu| = {lu}, |ev| = {lv}")
        if abs(float(self.eu @ self.ev)) > ORTHO_TOL * lu * lv:
            raise ValueError(f"screen: eu and ev must be orthogonal, got eu . ev = {float(self.eu @ self.ev)!r} with |eu| |ev| = {lu * lv!r}")

    def packed(self):
        """The nine doubles of the C ABI: p0, eu, ev."""
        return np.ascontiguousarray(np.concatenate([self.p0, self.eu, self.ev]), dtype=np.float64)

    @classmethod
    def behind(cls, camera_M, center, extent, tex_w, tex_h, plane_factor=1.5, span=2.0):
        """A screen perpendicular to the view axis of ``camera_M`` = (R, K, R^-1, K^-1), centred behind the object where
        ``views.screen_targets`` places its plane (``center + plane_factor * extent * z_camera``) and spanning ``span * extent`` along both
        camera axes: texel (0, 0) is the corner the image's top-left looks at, x runs along the camera's x, y along its y.  A calibrated R
        is orthonormal to 1e-7 or so, not to the 1e-12 a screen asks for: the y axis is made orthogonal to the x axis here (Gram-Schmidt),
        and the plane's normal is their cross product rather than R's third row."""
        tex_w, tex_h = _int(tex_w, "tex_w"), _int(tex_h, "tex_h")
        if tex_w < 2 or tex_h < 2:
            raise ValueError(f"tex_w, tex_h must be at least 2, got {(tex_w, tex_h)}")
        span, extent, plane_factor = float(span), float(extent), float(plane_factor)
        if not (span > 0.0 and extent > 0.0 and np.isfinite(span * extent)):
            raise ValueError(f"span and extent must be positive and finite, got span = {span!r}, extent = {extent!r}")
        R = _mat(camera_M[0], (4, 4), "camera_M[0] (R)")
        xc, yc, zc = R[0, :3], R[1, :3], R[2, :3]
        if not (np.linalg.norm(xc) > 0.0 and np.linalg.norm(zc) > 0.0):
            raise ValueError("camera_M[0] (R) must have non-zero rows")
        xc = xc / np.linalg.norm(xc)
        yc = yc - (yc @ xc) * xc
        yc = yc - (yc @ xc) * xc                          # twice: the first pass leaves a residue of the order of the defect squared
        if not np.linalg.norm(yc) > 0.0:
            raise ValueError("camera_M[0] (R): its first two rows must not be parallel")
        yc = yc / np.linalg.norm(yc)
        zc = zc / np.linalg.norm(zc)
        mid = _vec3(center, "center") + (plane_factor * extent) * zc
        eu = xc * (span * extent / (tex_w - 1))
        ev = yc * (span * extent / (tex_h - 1))
        return cls(mid - eu * ((tex_w - 1) / 2.0) - ev * ((tex_h - 1) / 2.0), eu, ev)


def _vec3(a, name):
    try:
        a = _host(a)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three finite numbers, got {a!r}") from None
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite numbers, got {a!r}")
    return a


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=np.float64)


def _mat(a, shape, name):
    try:
        a = _host(a)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite {shape[0]} x {shape[1]} matrix, got {type(a).__name__}") from None
    if a.shape != shape or not np.isfinite(a).all():
        raise ValueError(f"{name} must be a finite {shape[0]} x {shape[1]} matrix, got shape {a.shape}")
    return a


def _int(x, name):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {x!r}")
    return int(x)


# ---- procedural textures ---------------------------------------------------------------------------------------------------------------
def checker(tex_h, tex_w, squares=8):
    """float32 [tex_h, tex_w, 1]: a checkerboard of ``squares`` squares along the longer side, values 0.1 and 0.9."""
    tex_h, tex_w, squares = _int(tex_h, "tex_h"), _int(tex_w, "tex_w"), _int(squares, "squares")
    if tex_h < 2 or tex_w < 2 or squares < 1:
        raise ValueError(f"checker needs tex_h, tex_w >= 2 and squares >= 1, got {(tex_h, tex_w, squares)}")
    side = max(tex_h, tex_w) / squares
    yy, xx = np.meshgrid(np.arange(tex_h), np.arange(tex_w), indexing="ij")
    odd = (np.floor(yy / side) + np.floor(xx / side)) % 2
    return (0.1 + 0.8 * odd).astype(np.float32)[:, :, None]


def ramp(tex_h, tex_w):
    """float32 [tex_h, tex_w, 3]: red grows along x, green along y, blue marks a 16-texel grid -- every texel tells where it is."""
    tex_h, tex_w = _int(tex_h, "tex_h"), _int(tex_w, "tex_w")
    if tex_h < 2 or tex_w < 2:
        raise ValueError(f"ramp needs tex_h, tex_w >= 2, got {(tex_h, tex_w)}")
    yy, xx = np.meshgrid(np.arange(tex_h), np.arange(tex_w), indexing="ij")
    grid = ((yy % 16 == 0) | (xx % 16 == 0)).astype(np.float64)
    return np.stack([xx / (tex_w - 1), yy / (tex_h - 1), 0.25 + 0.5 * grid], axis=2).astype(np.float32)


# ---- image files -----------------------------------------------------------------------------------------------------------------------
def _read_netpbm(path):
    with open(path, "rb") as f:
        raw = f.read()
    tokens, pos = [], 0
    while len(tokens) < 4:
        while raw[pos:pos + 1].isspace():
            pos += 1
        if raw[pos:pos + 1] == b"#":
            pos = raw.index(b"\n", pos) + 1
            continue
        end = pos
        while not raw[end:end + 1].isspace():
            end += 1
        tokens.append(raw[pos:end])
        pos = end
    magic, w, h, top = tokens[0], int(tokens[1]), int(tokens[2]), int(tokens[3])
    if magic not in (b"P5", b"P6") or top != 255:
        raise ValueError(f"{path}: only binary 8-bit PGM / PPM files are read, got {magic!r} with maximum {top}")
    c = 1 if magic == b"P5" else 3
    return np.frombuffer(raw, np.uint8, h * w * c, pos + 1).reshape(h, w, c)


def load_texture(path):
    """float32 [Th, Tw, C] in [0, 1] from ``.npy`` (float arrays as they are, uint8 scaled by 1 / 255), binary ``.ppm`` / ``.pgm``, or
    any image file PIL reads when it is importable."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
    elif ext in (".ppm", ".pgm"):
        a = _read_netpbm(path)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise ValueError(f"{path}: reading {ext or 'this'} files needs PIL; without it use .npy, .ppm or .pgm") from None
        with Image.open(path) as im:
            a = np.asarray(im.convert("L" if im.mode in ("L", "1", "I", "F") else "RGB"))
    a = a.astype(np.float32) / np.float32(255.0) if a.dtype == np.uint8 else a.astype(np.float32)
    return check_texture(a)


def _read_hdr(path):
    """float32 [H, W, 3] of a Radiance ``.hdr`` / ``.pic`` file (RGBE, ``-Y H +X W``; flat or run-length encoded scanlines): a pixel
    (r, g, b, e) with e > 0 is (r + 0.5, g + 0.5, b + 0.5) * 2^(e - 136), Radiance's own colr_color; e = 0 is black."""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.startswith((b"#?RADIANCE", b"#?RGBE")):
        raise ValueError(f"{path}: not a Radiance picture (it does not begin with #?RADIANCE)")
    blank = re.search(rb"\r?\n\r?\n", raw)
    if blank is None:
        raise ValueError(f"{path}: the Radiance header does not end")
    for line in raw[:blank.start()].split(b"\n"):
        if line.startswith(b"FORMAT=") and line.strip() != b"FORMAT=32-bit_rle_rgbe":
            raise ValueError(f"{path}: only FORMAT=32-bit_rle_rgbe is read, got {line.strip().decode(errors='replace')}")
    pos = raw.find(b"\n", blank.end())
    if pos < 0:
        raise ValueError(f"{path}: the size line (-Y H +X W) behind the Radiance header is missing or does not end")
    size = raw[blank.end():pos].split()
    if len(size) == 4 and (size[0], size[2]) != (b"-Y", b"+X") and size[0][1:] in (b"Y", b"X") and size[2][1:] in (b"Y", b"X"):
        raise ValueError(f"{path}: only the standard orientation -Y H +X W is read, got {raw[blank.end():pos].decode(errors='replace')!r}")
    try:
        if len(size) != 4 or (size[0], size[2]) != (b"-Y", b"+X"):
            raise ValueError
        h, w = int(size[1]), int(size[3])
    except ValueError:
        raise ValueError(f"{path}: the size line must read -Y H +X W with two integers, got {raw[blank.end():pos].decode(errors='replace')!r}") from None
    pos += 1
    data = np.frombuffer(raw, np.uint8, offset=pos)
    rgbe = np.empty((h, w, 4), np.uint8)
    if h < 1 or w < 1:
        raise ValueError(f"{path}: empty picture ({h} x {w})")
    encoded = 8 <= w <= 32767 and len(data) >= 4 and data[0] == 2 and data[1] == 2 and data[2] < 128
    if not encoded:
        if len(data) < h * w * 4:
            raise ValueError(f"{path}: the file ends before its {h} x {w} pixels do")
        rgbe[:] = data[:h * w * 4].reshape(h, w, 4)
    else:
        p = 0
        for y in range(h):
            if p + 4 > len(data) or data[p] != 2 or data[p + 1] != 2 or (int(data[p + 2]) << 8 | int(data[p + 3])) != w:
                raise ValueError(f"{path}: scanline {y} is not run-length encoded for a width of {w}")
            p += 4
            for ch in range(4):
                x = 0
                while x < w:
                    if p >= len(data):
                        raise ValueError(f"{path}: the file ends inside scanline {y}")
                    n = int(data[p])
                    if n > 128:                          # a run: n - 128 copies of the next byte
                        n -= 128
                        if n == 0 or x + n > w or p + 1 >= len(data):
                            raise ValueError(f"{path}: bad run in scanline {y}")
                        rgbe[y, x:x + n, ch] = data[p + 1]
                        p += 2
                    else:                                # n literal bytes
                        if n == 0 or x + n > w or p + 1 + n > len(data):
                            raise ValueError(f"{path}: bad literal in scanline {y}")
                        rgbe[y, x:x + n, ch] = data[p + 1:p + 1 + n]
                        p += 1 + n
                    x += n
    e = rgbe[:, :, 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return ((rgbe[:, :, :3].astype(np.float64) + 0.5) * scale[:, :, None]).astype(np.float32)


class Environment:
    """An environment map at infinity: ``texels`` float32 ``[Eh, Ew, C]`` (or ``[Eh, Ew]``), C in {1, 3}, at least
    2 x 2, numpy or a device tensor -- a lat-long panorama whose row 0 looks along +y of the environment frame and whose columns run once
    around it; ``rotation``: 3 x 3, world -> environment frame, y up (None: the identity), orthonormal to 1e-12
    (max |R R^T - I|).  The values are radiances: they are not clipped to [0, 1]."""

    def __init__(self, texels, rotation=None):
        t = texels
        if not (hasattr(t, "shape") and hasattr(t, "dtype")):
            try:
                t = np.asarray(t)
            except (TypeError, ValueError):
                raise ValueError(f"environment texels must be a float array [Eh, Ew, C], got {type(texels).__name__}") from None
        if t.ndim == 2:
            t = t[:, :, None]
        if t.ndim != 3 or t.shape[2] not in (1, 3):
            raise ValueError(f"environment texels must be [Eh, Ew], [Eh, Ew, 1] or [Eh, Ew, 3], got shape {tuple(t.shape)}")
        if t.shape[0] < 2 or t.shape[1] < 2:
            raise ValueError(f"environment must be at least 2 x 2 texels, got {tuple(t.shape[:2])}")
        if "float" not in str(t.dtype):
            raise ValueError(f"environment texels must be a float array (float32 is used), got dtype {t.dtype}")
        self.texels = np.ascontiguousarray(t, dtype=np.float32) if isinstance(t, np.ndarray) else t
        R = np.eye(3) if rotation is None else _mat(rotation, (3, 3), "environment rotation")
        defect = float(np.abs(R @ R.T - np.eye(3)).max())
        if not defect <= ORTHO_TOL:
            raise ValueError(f"environment rotation must be orthonormal: max |R R^T - I| = {defect!r} exceeds {ORTHO_TOL}")
        self.rotation = np.ascontiguousarray(R, dtype=np.float64)

    @property
    def channels(self):
        return int(self.texels.shape[2])

    def packed(self):
        """The nine doubles of the C ABI: the rotation, row-major."""
        return np.ascontiguousarray(self.rotation.reshape(-1), dtype=np.float64)

    @staticmethod
    def yaw(degrees):
        """The rotation that turns the panorama by ``degrees`` about the world's y axis."""
        a = np.deg2rad(float(degrees))
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])

    @classmethod
    def load(cls, path, rotation=None):
        """An environment from a file: Radiance ``.hdr`` / ``.pic`` (read here with numpy), or whatever ``load_texture`` reads."""
        ext = os.path.splitext(path)[1].lower()
        return cls(_read_hdr(path) if ext in (".hdr", ".pic") else load_texture(path), rotation)


def to_bytes(image):
    """uint8 [H, W, C] of a float image: clipped to [0, 1], scaled by 255, rounded to nearest."""
    a = _host(image)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"image must be [H, W], [H, W, 1] or [H, W, 3], got shape {a.shape}")
    return np.rint(np.clip(np.nan_to_num(a, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_image(path, image, force=False):
    """Write a float image ([H, W], [H, W, 1] or [H, W, 3], values in [0, 1]) as 8 bits per channel and return the path written:
    ``.ppm`` / ``.pgm`` as binary netpbm; anything else through PIL when it is importable, otherwise as netpbm next to the requested name
    (extension replaced).  An existing file is only replaced with ``force``."""
    a = to_bytes(image)
    ext = os.path.splitext(path)[1].lower()
    pil = None
    if ext not in (".ppm", ".pgm"):
        try:
            from PIL import Image as pil
        except ImportError:
            path = os.path.splitext(path)[0] + (".pgm" if a.shape[2] == 1 else ".ppm")
    if os.path.exists(path) and not force:
        raise FileExistsError(f"{path} exists: pass force=True (--force) to overwrite it")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if pil is not None:
        pil.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(path)
    else:
        with open(path, "wb") as f:
            f.write(b"%s\n%d %d\n255\n" % (b"P5" if a.shape[2] == 1 else b"P6", a.shape[1], a.shape[0]))
            f.write(a.tobytes())
    return path


# ---- the call's arguments (checked before anything touches the device) -----------------------------------------------------------------
def plan_bands(height, width, s, max_samples):
    """Rows [y0, y1) of the bands of an image of ``height`` x ``width`` pixels with ``s`` x ``s`` samples each: consecutive, covering every
    row once, each of at most ``max_samples`` samples -- except that a band is never less than one row."""
    height, width, s, max_samples = _int(height, "height"), _int(width, "width"), _int(s, "supersample"), _int(max_samples, "max_samples")
    if height < 1 or width < 1:
        raise ValueError(f"height, width must be at least 1, got {(height, width)}")
    if not 1 <= s <= MAX_SUPERSAMPLE:
        raise ValueError(f"supersample must be in 1..{MAX_SUPERSAMPLE}, got {s}")
    if max_samples < 1:
        raise ValueError(f"max_samples must be at least 1, got {max_samples}")
    rows = max(1, max_samples // (width * s * s))
    return [(y0, min(height, y0 + rows)) for y0 in range(0, height, rows)]


def check_texture(texture):
    """The texture as a contiguous float32 array [Th, Tw, C] (numpy) -- or, a device tensor, as it is after the same checks."""
    t = texture
    if not (hasattr(t, "shape") and hasattr(t, "dtype")):
        t = np.asarray(t)
    if t.ndim == 2:
        t = t[:, :, None]
    if t.ndim != 3 or t.shape[2] not in (1, 3):
        raise ValueError(f"texture must be [Th, Tw], [Th, Tw, 1] or [Th, Tw, 3], got shape {tuple(t.shape)}")
    if t.shape[0] < 2 or t.shape[1] < 2:
        raise ValueError(f"texture must be at least 2 x 2 texels, got {tuple(t.shape[:2])}")
    kind = str(t.dtype)
    if "float" not in kind:
        raise ValueError(f"texture must be a float array (float32 is used), got dtype {kind}")
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t, dtype=np.float32)
    return t


def _fill(x, channels, name):
    try:
        a = _host(x).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be one finite number or {channels} of them (one per channel), got {x!r}") from None
    if a.size == 1:
        a = np.repeat(a, channels)
    if a.size != channels or not np.isfinite(a).all():
        raise ValueError(f"{name} must be one finite number or {channels} of them (one per channel), got {x!r}")
    return np.ascontiguousarray(a, dtype=np.float64)


def check_absorption(absorption, channels):
    """An ``absorption`` argument as C float64 coefficients on the host: one number (the same for every channel), C
    numbers, or a float64 tensor [C] on any device (its value is read here); each finite and >= 0.  None stays None."""
    if absorption is None:
        return None
    what = f"absorption must be one finite number >= 0, {channels} of them (one per channel) or a float64 tensor [{channels}]"
    if _is_tensor(absorption):
        kind = str(absorption.dtype).replace("torch.", "")
        if kind != "float64" or tuple(absorption.shape) != (channels,):
            raise ValueError(f"{what}, got a {kind} tensor of shape {tuple(absorption.shape)}")
    elif isinstance(absorption, (bool, np.bool_, str, bytes)):
        raise ValueError(f"{what}, got {absorption!r}")
    try:
        a = np.asarray(_host(absorption), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}, got {absorption!r}") from None
    if a.size == 1 and not _is_tensor(absorption):
        a = np.repeat(a, channels)
    if a.size != channels or not np.isfinite(a).all() or (a < 0).any():
        raise ValueError(f"{what}, got {absorption!r}")
    return np.ascontiguousarray(a, dtype=np.float64)


def check_render_args(camera_M, height, width, screen, texture, supersample=1, max_bounces=2, tir="drop", refraction="reference",
                      fresnel=True, void=0.0, invalid=0.0, max_samples=1 << 22, want_planes=False, absorption=None, environment=None, reflection=False):
    """Every argument check of ``Scene.render_image``, none of which needs a device.  Returns a dict: camera (21 doubles: K^-1, then the
    top 3 x 4 of R^-1), screen (9 doubles), texture, void / invalid (C doubles), bands, law_flags, the scalars, absorption (C doubles,
    or None: clear glass) and environment (an ``Environment``, or None).  With an environment ``screen`` and ``texture`` may both be
    None (screen and texture are then None in the dict, and C is the environment's); absorption does not go with one.  ``reflection``
    (the outer-surface reflection) needs an environment and ``fresnel=True``."""
    try:
        n_cam = len(camera_M)
    except TypeError:
        raise ValueError(f"camera_M must be the tuple (R, K, R^-1, K^-1), got {type(camera_M).__name__}") from None
    if n_cam != 4:
        raise ValueError(f"camera_M must be the tuple (R, K, R^-1, K^-1), got {n_cam} entries")
    rinv, kinv = _mat(camera_M[2], (4, 4), "camera_M[2] (R^-1)"), _mat(camera_M[3], (3, 3), "camera_M[3] (K^-1)")
    bands = plan_bands(height, width, supersample, max_samples)
    if isinstance(max_bounces, bool) or not isinstance(max_bounces, (int, np.integer)) or not 2 <= int(max_bounces) <= 8:
        raise ValueError(f"max_bounces must be an integer in 2..8, got {max_bounces!r}")
    if tir not in ("drop", "reflect"):
        raise ValueError(f"tir must be 'drop' or 'reflect', got {tir!r}")
    if not isinstance(refraction, str) or refraction not in ("reference", "snell"):
        raise ValueError(f"refraction must be 'reference' or 'snell', got {refraction!r}")
    if not isinstance(fresnel, (bool, np.bool_)):
        raise ValueError(f"fresnel must be True or False, got {fresnel!r}")
    if not isinstance(want_planes, (bool, np.bool_)):
        raise ValueError(f"want_planes must be True or False, got {want_planes!r}")
    if not isinstance(reflection, (bool, np.bool_)):
        raise ValueError(f"reflection must be True or False, got {reflection!r}")
    if reflection and environment is None:
        raise ValueError("reflection=True needs an environment: the reflected rays almost never meet a screen behind the object")
    if reflection and not fresnel:
        raise ValueError("reflection=True needs fresnel=True: the reflected share is the complement of what the Fresnel term transmits")
    if environment is not None:
        if not isinstance(environment, Environment):
            raise ValueError(f"environment must be a drt_amd.render.Environment, got {type(environment).__name__}")
        if absorption is not None:
            raise ValueError("environment cannot be combined with absorption: the absorbing image has no environment form")
        if (screen is None) != (texture is None):
            raise ValueError("environment: screen and texture must be given together or both be None (no screen: every ray sees the environment)")
    if environment is not None and screen is None:
        tex, channels = None, environment.channels
    else:
        if not isinstance(screen, Screen):
            raise ValueError(f"screen must be a drt_amd.render.Screen, got {type(screen).__name__}")
        tex = check_texture(texture)
        channels = int(tex.shape[2])
        if environment is not None and environment.channels != channels:
            raise ValueError(f"environment has {environment.channels} channels, the texture has {channels}: they must agree")
    return dict(camera=np.ascontiguousarray(np.concatenate([kinv.reshape(-1), rinv[:3, :].reshape(-1)]), dtype=np.float64),
                screen=None if tex is None else screen.packed(), texture=tex, environment=environment, reflection=bool(reflection), channels=channels, void=_fill(void, channels, "void"),
                invalid=_fill(invalid, channels, "invalid"), bands=bands, height=int(height), width=int(width), supersample=int(supersample),
                max_bounces=int(max_bounces), law_flags=int(tir == "reflect") | (2 if refraction == "snell" else 0), fresnel=int(bool(fresnel)),
                want_planes=bool(want_planes), absorption=check_absorption(absorption, channels))


def _plane(x, shape, name, allow_bytes):
    """A float32 plane of ``shape`` for the device: numpy (checked for finite values, made contiguous; uint8 scaled by 1 / 255 where
    allowed) or a device tensor (shape and dtype checked, converted by the caller)."""
    if x is None or not (hasattr(x, "shape") and hasattr(x, "dtype")):
        try:
            x = None if x is None else np.asarray(x)
        except (TypeError, ValueError):
            x = None
        if x is None or x.dtype == object:
            raise ValueError(f"{name} must be an array of shape {shape}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    kind = str(x.dtype).replace("torch.", "")
    if kind not in (("float32", "uint8") if allow_bytes else ("float32",)):
        raise ValueError(f"{name} must be float32{' or uint8 (read as value / 255)' if allow_bytes else ''}, got dtype {kind}")
    if isinstance(x, np.ndarray):
        x = x.astype(np.float32) / np.float32(255.0) if kind == "uint8" else x
        if not np.isfinite(x).all():
            raise ValueError(f"{name} must be finite")
        return np.ascontiguousarray(x, dtype=np.float32)
    return x


def _ior_arg(x, name):
    """An IOR argument of ``Scene.image_loss_fused``: None, a positive finite float (returned), or a 0-dim tensor (None returned: its
    value is read by the caller)."""
    if x is None:
        return None
    if hasattr(x, "numel") and hasattr(x, "dtype"):
        if x.numel() != 1:
            raise ValueError(f"{name} must be a float or a 0-dim tensor, got shape {tuple(x.shape)}")
        return None
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) or not x > 0:
        raise ValueError(f"{name} must be a positive finite float or a 0-dim tensor, got {x!r}")
    return float(x)


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "requires_grad")


def screen_of_param(screen_param):
    """The ``Screen`` of a ``screen_param``: a float64 tensor [3, 3] with rows p0, eu, ev on any device, read to the host here, finite,
    and with axes that pass the ``Screen`` constructor's checks."""
    if not _is_tensor(screen_param):
        raise ValueError(f"screen_param must be a float64 tensor of shape (3, 3) with rows p0, eu, ev, got {type(screen_param).__name__}")
    if tuple(screen_param.shape) != (3, 3):
        raise ValueError(f"screen_param must have shape (3, 3) with rows p0, eu, ev, got {tuple(screen_param.shape)}")
    kind = str(screen_param.dtype).replace("torch.", "")
    if kind != "float64":
        raise ValueError(f"screen_param must be float64, got dtype {kind}")
    rows = screen_param.detach().cpu().numpy()
    if not np.isfinite(rows).all():
        raise ValueError(f"screen_param must be finite, got {rows!r}")
    try:
        return Screen(rows[0], rows[1], rows[2])
    except ValueError as e:
        raise ValueError(f"screen_param: {e}") from None


def check_texture_param(texture_param):
    """A ``texture_param``: a float32 or float64 tensor [Th, Tw, C] or [Th, Tw], C in {1, 3}, at least 2 x 2 texels; finite where that
    can be seen without a device (a host tensor)."""
    if not _is_tensor(texture_param):
        raise ValueError(f"texture_param must be a float32 or float64 tensor [Th, Tw, C] or [Th, Tw], got {type(texture_param).__name__}")
    kind = str(texture_param.dtype).replace("torch.", "")
    if kind not in ("float32", "float64"):
        raise ValueError(f"texture_param must be float32 or float64, got dtype {kind}")
    shape = tuple(texture_param.shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] not in (1, 3)):
        raise ValueError(f"texture_param must be [Th, Tw], [Th, Tw, 1] or [Th, Tw, 3], got shape {shape}")
    if shape[0] < 2 or shape[1] < 2:
        raise ValueError(f"texture_param must be at least 2 x 2 texels, got {shape[:2]}")
    if texture_param.device.type == "cpu" and not np.isfinite(texture_param.detach().numpy()).all():
        raise ValueError("texture_param must be finite")
    return texture_param


def camera_of_param(camera_param):
    """The ``camera_M`` 4-tuple ``(None, None, R^-1 [4, 4], K^-1)`` of a ``camera_param`` = ``(Rinv, Kinv)``: float64 tensors on any device,
    ``Rinv`` [4, 4] or [3, 4] (its top three rows are what the renderer reads; a [3, 4] one is completed by the row (0, 0, 0, 1)),
    ``Kinv`` [3, 3]; read to the host here, finite."""
    try:
        n = len(camera_param)
    except TypeError:
        n = -1
    if isinstance(camera_param, (str, bytes)) or _is_tensor(camera_param) or n != 2:
        raise ValueError(f"camera_param must be the pair (Rinv, Kinv) of float64 tensors, got {type(camera_param).__name__}"
                         + (f" of {n} entries" if n >= 0 and not _is_tensor(camera_param) else ""))
    mats = []
    for x, shapes, name in ((camera_param[0], ((4, 4), (3, 4)), "Rinv"), (camera_param[1], ((3, 3),), "Kinv")):
        want = " or ".join(str(sh) for sh in shapes)
        if not _is_tensor(x):
            raise ValueError(f"camera_param: {name} must be a float64 tensor of shape {want}, got {type(x).__name__}")
        if tuple(x.shape) not in shapes:
            raise ValueError(f"camera_param: {name} must have shape {want}, got {tuple(x.shape)}")
        kind = str(x.dtype).replace("torch.", "")
        if kind != "float64":
            raise ValueError(f"camera_param: {name} must be float64, got dtype {kind}")
        m = x.detach().cpu().numpy()
        if not np.isfinite(m).all():
            raise ValueError(f"camera_param: {name} must be finite, got {m!r}")
        mats.append(m)
    rinv = mats[0] if mats[0].shape == (4, 4) else np.concatenate([mats[0], np.array([[0.0, 0.0, 0.0, 1.0]])])
    return (None, None, rinv, mats[1])


def environment_of_params(environment, env_texels_param=None, env_rotation_param=None):
    """The ``Environment`` of ``environment`` with ``env_texels_param`` in the place of its texels and ``env_rotation_param`` in the place
    of its rotation.  ``env_texels_param``: a float32 or float64 tensor shaped like the environment's texels,
    ``[Eh, Ew, C]`` (or ``[Eh, Ew]`` with one channel); finite where that can be seen without touching a device.  ``env_rotation_param``:
    a float64 tensor ``[3, 3]`` on any device, read to the host here, through ``Environment``'s own rotation check."""
    given = [n for n, p in (("env_texels_param", env_texels_param), ("env_rotation_param", env_rotation_param)) if p is not None]
    if not isinstance(environment, Environment):
        raise ValueError(f"{' / '.join(given)} needs an environment: a drt_amd.render.Environment, got {type(environment).__name__}")
    texels, rotation = environment.texels, environment.rotation
    if env_texels_param is not None:
        p = env_texels_param
        if not _is_tensor(p):
            raise ValueError(f"env_texels_param must be a float32 or float64 tensor [Eh, Ew, C] or [Eh, Ew], got {type(p).__name__}")
        kind = str(p.dtype).replace("torch.", "")
        if kind not in ("float32", "float64"):
            raise ValueError(f"env_texels_param must be float32 or float64, got dtype {kind}")
        want = tuple(environment.texels.shape)
        if tuple(p.shape) != want and not (want[2] == 1 and tuple(p.shape) == want[:2]):
            raise ValueError(f"env_texels_param must have the shape of the environment's texels, {want}" + (f" or {want[:2]}" if want[2] == 1 else "") +
                             f", got shape {tuple(p.shape)}")
        if p.device.type == "cpu" and not np.isfinite(p.detach().numpy()).all():
            raise ValueError("env_texels_param must be finite")
        texels = p.detach()
    if env_rotation_param is not None:
        p = env_rotation_param
        if not _is_tensor(p):
            raise ValueError(f"env_rotation_param must be a float64 tensor of shape (3, 3), got {type(p).__name__}")
        if tuple(p.shape) != (3, 3):
            raise ValueError(f"env_rotation_param must have shape (3, 3), got {tuple(p.shape)}")
        kind = str(p.dtype).replace("torch.", "")
        if kind != "float64":
            raise ValueError(f"env_rotation_param must be float64, got dtype {kind}")
        rotation = p.detach().cpu().numpy()
    try:
        return Environment(texels, rotation)
    except ValueError as e:
        raise ValueError(f"{' / '.join(given)}: {e}") from None


def check_image_loss_args(camera_M, height, width, screen, texture, target, weight=None, ior_int=None, ior_ext=None, vertices=True,
                          want_image=False, supersample=1, max_bounces=2, tir="drop", refraction="reference", fresnel=True, void=0.0,
                          invalid=0.0, max_samples=1 << 22, screen_param=None, texture_param=None, camera_param=None, absorption=None, environment=None,
                          reflection=False, env_texels_param=None, env_rotation_param=None):
    """Every argument check of ``Scene.image_loss_fused``, none of which needs a device: ``check_render_args``' dict plus target
    (float32 [H, W, C]; uint8 is read as value / 255; [H, W] with a one-channel texture), weight (float32 [H, W] or None), ior (the float
    of each IOR given as a number, else None), vertices and want_image.  ``screen_param`` / ``texture_param`` (tensors a gradient is
    wanted for) take the place of ``screen`` / ``texture``, which must then be None: exactly one form of each is given; so does
    ``camera_param`` = ``(Rinv, Kinv)`` for ``camera_M``.  ``absorption`` (``check_absorption``) goes with none of the three.  ``environment`` / ``reflection``
    (``check_render_args``): with an environment ``screen`` and ``texture`` may both be None; it goes with none of
    ``absorption``, ``screen_param``, ``texture_param``, ``camera_param``.  ``env_texels_param`` / ``env_rotation_param``
    (``environment_of_params``) need an environment and take the place of its texels / rotation: ``a["environment"]`` is
    then the environment the call renders."""
    if env_texels_param is not None or env_rotation_param is not None:
        environment = environment_of_params(environment, env_texels_param, env_rotation_param)
    if environment is not None or reflection is not False:
        for name, given in (("absorption", absorption), ("screen_param", screen_param), ("texture_param", texture_param), ("camera_param", camera_param)):
            if given is not None:
                raise ValueError(f"environment / reflection cannot be combined with {name}: the loss over an environment has vertex and IOR gradients only")
        if camera_M is None:
            raise ValueError("camera_M is None and no camera_param is given: one of the two must supply the camera")
        a = check_render_args(camera_M, height, width, screen, texture, supersample, max_bounces, tir, refraction, fresnel, void, invalid, max_samples,
                              environment=environment, reflection=reflection)
        return _loss_planes(a, target, weight, ior_int, ior_ext, vertices, want_image)
    if absorption is not None:
        for name, given in (("screen_param", screen_param), ("texture_param", texture_param), ("camera_param", camera_param)):
            if given is not None:
                raise ValueError(f"absorption cannot be combined with {name}: the absorbing loss has no screen, texture or camera gradient")
    if camera_param is not None:
        if camera_M is not None:
            raise ValueError("camera_param is given: the positional camera_M must be None (one of the two supplies the camera)")
        camera_M = camera_of_param(camera_param)
    elif camera_M is None:
        raise ValueError("camera_M is None and no camera_param is given: one of the two must supply the camera")
    if screen_param is not None:
        if screen is not None:
            raise ValueError("screen_param is given: the positional screen must be None (one of the two supplies the screen)")
        screen = screen_of_param(screen_param)
    elif screen is None:
        raise ValueError("screen is None and no screen_param is given: one of the two must supply the screen")
    if texture_param is not None:
        if texture is not None:
            raise ValueError("texture_param is given: the positional texture must be None (one of the two supplies the texture)")
        texture = check_texture_param(texture_param).detach()
    elif texture is None:
        raise ValueError("texture is None and no texture_param is given: one of the two must supply the texture")
    a = check_render_args(camera_M, height, width, screen, texture, supersample, max_bounces, tir, refraction, fresnel, void, invalid, max_samples,
                          absorption=absorption)
    return _loss_planes(a, target, weight, ior_int, ior_ext, vertices, want_image)


def _loss_planes(a, target, weight, ior_int, ior_ext, vertices, want_image):
    """``check_image_loss_args`` behind ``check_render_args``: target, weight, ior, vertices and want_image into the dict ``a``."""
    H, W, C = a["height"], a["width"], a["channels"]
    if target is not None and hasattr(target, "shape") and len(target.shape) == 2 and C == 1:
        target = target[:, :, None]
    a["target"] = _plane(target, (H, W, C), "target", True)
    a["weight"] = None if weight is None else _plane(weight, (H, W), "weight", False)
    a["ior"] = (_ior_arg(ior_int, "ior_int"), _ior_arg(ior_ext, "ior_ext"))
    for name, flag in (("vertices", vertices), ("want_image", want_image)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, got {flag!r}")
    a["vertices"], a["want_image"] = bool(vertices), bool(want_image)
    return a


# ---- several views in one call (Scene.bind_image_views / image_loss_views_fused) ---------------------------------------
MAX_VIEWS_PER_CALL = 16


def _camera21(camera_M, name):
    try:
        n_cam = len(camera_M)
    except TypeError:
        raise ValueError(f"{name} must be the tuple (R, K, R^-1, K^-1), got {type(camera_M).__name__}") from None
    if n_cam != 4:
        raise ValueError(f"{name} must be the tuple (R, K, R^-1, K^-1), got {n_cam} entries")
    rinv, kinv = _mat(camera_M[2], (4, 4), f"{name}[2] (R^-1)"), _mat(camera_M[3], (3, 3), f"{name}[3] (K^-1)")
    return np.concatenate([kinv.reshape(-1), rinv[:3, :].reshape(-1)])


# the table row of a view without a screen: never evaluated (the environment call then runs with no screen), it only has to pass the
# library's check of a screen
NO_SCREEN_ROW = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def check_image_views_args(cameras, height, width, screens, targets, weights=None, environment=None):
    """Every argument check of ``Scene.bind_image_views``, none of which needs a device.  Returns a dict: n, height, width, channels,
    cameras (float64 [n, 21]: K^-1, then the top 3 x 4 of R^-1, per view), screens (float64 [n, 9]), targets (float32 [n, H, W, C];
    uint8 is read as value / 255; [n, H, W] is one channel) and weights (float32 [n, H, W] or None) -- numpy arrays made contiguous, or
    device tensors as they are after the shape and dtype checks --, environment (an ``Environment`` or None; its channels must be the
    targets') and has_screens.  ``screens=None`` goes with an environment only: the capture has no screen, the rows of
    ``screens`` are then placeholders that are never read."""
    height, width = _int(height, "height"), _int(width, "width")
    if height < 1 or width < 1:
        raise ValueError(f"height, width must be at least 1, got {(height, width)}")
    if environment is not None and not isinstance(environment, Environment):
        raise ValueError(f"environment must be a drt_amd.render.Environment, got {type(environment).__name__}")
    has_screens = screens is not None
    if not has_screens and environment is None:
        raise ValueError("screens is None and no environment is given: a capture without screens needs an environment to look at")
    try:
        cameras = list(cameras)
        screens = list(screens) if has_screens else [Screen(NO_SCREEN_ROW[0:3], NO_SCREEN_ROW[3:6], NO_SCREEN_ROW[6:9])] * len(cameras)
    except TypeError:
        raise ValueError("cameras must be a list of camera_M tuples and screens a list of Screen objects") from None
    n = len(cameras)
    if n < 1:
        raise ValueError("cameras must list at least one view")
    if len(screens) != n:
        raise ValueError(f"screens must list one Screen per camera: {len(screens)} screens for {n} cameras")
    cams = np.ascontiguousarray(np.stack([_camera21(c, f"cameras[{k}]") for k, c in enumerate(cameras)]), dtype=np.float64)
    rows = []
    for k, sc in enumerate(screens):
        if not isinstance(sc, Screen):
            raise ValueError(f"screens[{k}] must be a drt_amd.render.Screen, got {type(sc).__name__}")
        try:
            rows.append(Screen(sc.p0, sc.eu, sc.ev).packed())          # (checked again: the attributes of a Screen can be assigned)
        except ValueError as e:
            raise ValueError(f"screens[{k}]: {e}") from None
    if targets is None or not (hasattr(targets, "shape") and hasattr(targets, "dtype")):
        try:
            targets = None if targets is None else np.asarray(targets)
        except (TypeError, ValueError):
            targets = None
        if targets is None or targets.dtype == object:
            raise ValueError(f"targets must be an array of shape ({n}, {height}, {width}, C)")
    if len(targets.shape) == 3:
        targets = targets[:, :, :, None]
    if len(targets.shape) != 4 or targets.shape[3] not in (1, 3):
        raise ValueError(f"targets must be [n, H, W], [n, H, W, 1] or [n, H, W, 3], got shape {tuple(targets.shape)}")
    channels = int(targets.shape[3])
    if environment is not None and environment.channels != channels:
        raise ValueError(f"environment has {environment.channels} channels, the targets have {channels}: they must agree")
    return dict(n=n, height=height, width=width, channels=channels, cameras=cams, screens=np.ascontiguousarray(np.stack(rows), dtype=np.float64),
                targets=_plane(targets, (n, height, width, channels), "targets", True),
                weights=None if weights is None else _plane(weights, (n, height, width), "weights", False), environment=environment,
                has_screens=has_screens)


def check_view_ids(view_ids, n_views):
    """The view list of one ``image_loss_views_fused`` call as a list of ints: 1 .. 16 ids, each in [0, n_views), repeats allowed."""
    try:
        ids = [_int(v, "view_ids entry") for v in view_ids]
    except TypeError:
        raise ValueError(f"view_ids must be a list of view numbers, got {view_ids!r}") from None
    if not 1 <= len(ids) <= MAX_VIEWS_PER_CALL:
        raise ValueError(f"view_ids must list 1..{MAX_VIEWS_PER_CALL} views, got {len(ids)}")
    for v in ids:
        if not 0 <= v < n_views:
            raise ValueError(f"view_ids: view {v} is outside the binding's views 0..{n_views - 1}")
    return ids


def check_image_views_law(binding, view_ids, texture, ior_int=None, ior_ext=None, vertices=True, supersample=1, max_bounces=2, tir="drop",
                          refraction="reference", fresnel=True, void=0.0, invalid=0.0, max_samples=1 << 22, reflection=False, absorption=None,
                          want_images=False):
    """Every argument check of ``Scene.image_loss_views_fused`` behind the binding: ``check_render_args``' dict for the tall image of
    ``len(view_ids) * H`` rows (camera and screen are the first listed view's and stand for nothing), plus ids, ior and vertices.  The
    environment is the binding's (``a["environment"]``, or None); ``texture`` is None exactly when the binding has no screens;
    ``reflection`` needs the binding's environment and ``fresnel``.  ``absorption``: ``check_absorption``'s forms,
    C float64 coefficients or None in the dict -- here, unlike in the single-view calls, it goes with the binding's environment;
    ``want_images``: True or False."""
    if not isinstance(binding, ImageViews):
        raise ValueError(f"binding must be a drt_amd.render.ImageViews (Scene.bind_image_views), got {type(binding).__name__}")
    ids = check_view_ids(view_ids, binding.n)
    cam = binding.args["cameras"][ids[0]]
    rinv = np.concatenate([cam[9:].reshape(3, 4), np.array([[0.0, 0.0, 0.0, 1.0]])])
    sc = binding.args["screens"][ids[0]]
    env = binding.args.get("environment")
    if binding.args.get("has_screens", True):
        if texture is None:
            raise ValueError("texture is None: the binding has screens, and the views share one texture")
        screen = Screen(sc[0:3], sc[3:6], sc[6:9])
    else:
        if texture is not None:
            raise ValueError("texture must be None: the binding was made with screens=None (every ray sees the environment)")
        screen = None
    a = check_render_args((None, None, rinv, cam[:9].reshape(3, 3)), len(ids) * binding.height, binding.width, screen, texture,
                          supersample, max_bounces, tir, refraction, fresnel, void, invalid, max_samples, environment=env, reflection=reflection)
    if a["channels"] != binding.channels:
        raise ValueError(f"texture has {a['channels']} channels, the binding's targets have {binding.channels}")
    a["ids"] = ids
    a["ior"] = (_ior_arg(ior_int, "ior_int"), _ior_arg(ior_ext, "ior_ext"))
    if not isinstance(vertices, (bool, np.bool_)):
        raise ValueError(f"vertices must be True or False, got {vertices!r}")
    a["vertices"] = bool(vertices)
    a["absorption"] = check_absorption(absorption, a["channels"])
    if not isinstance(want_images, (bool, np.bool_)):
        raise ValueError(f"want_images must be True or False, got {want_images!r}")
    if want_images and a["absorption"] is None:
        raise ValueError("want_images=True needs absorption (0.0 renders clear glass): the clear multi-view calls write no image")
    a["want_images"] = bool(want_images)
    return a


class ImageViews:
    """The views of a capture for ``Scene.image_loss_views_fused``, made by ``Scene.bind_image_views``: the device table of cameras and
    screens (drt_image_views_create; owned here, freed with this object or with the scene, whichever goes first) and the resident
    target and weight stacks.  ``n`` views of ``height`` x ``width`` pixels and ``channels`` channels.  A binding made with an
    environment also keeps its texels resident (``env``, float32 [Eh, Ew, C]) and holds the packed rotation
    (``env_rot``, nine doubles); without one both are None."""

    def __init__(self, scene, args):
        import ctypes
        import torch
        from . import _lib
        from .optix_mesh import _on
        self.scene, self.args = scene, args
        self.n, self.height, self.width, self.channels = args["n"], args["height"], args["width"], args["channels"]
        dev = scene._dev
        h = ctypes.c_void_p()
        with _on(dev):
            t = torch.as_tensor(args["targets"], device=dev)
            self.targets = (t.to(torch.float32) / 255.0 if t.dtype == torch.uint8 else t).reshape(self.n, self.height, self.width, self.channels).contiguous()
            self.weights = None if args["weights"] is None else torch.as_tensor(args["weights"], device=dev).contiguous()
            environment = args.get("environment")
            self.env = None if environment is None else torch.as_tensor(environment.texels, device=dev).to(torch.float32).contiguous()
            self.env_rot = None if environment is None else environment.packed()
            _lib.check(_lib.lib().drt_image_views_create(scene.optix_mesh._h, self.n, args["cameras"].ctypes.data, args["screens"].ctypes.data,
                                                         self.height, self.width, ctypes.byref(h)))
        self._h = h.value
        self._mesh = scene.optix_mesh          # (the scene handle outlives the table)

    def release(self):
        """Frees the device table now; the object cannot be used afterwards."""
        h, self._h = self._h, None
        if h and getattr(self._mesh, "_h", None):
            from . import _lib
            _lib.lib().drt_image_views_destroy(h)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def _background(spec, tex):
    if spec == "checker":
        return checker(tex, tex, 16)
    if spec == "ramp":
        return ramp(tex, tex)
    return load_texture(spec)


def capture_cameras(path, view_ids):
    """(height, width, {view: camera_M}) of a capture file (``captured_data``'s formats and datasets): ``cam_proj`` [n, 4, 4] world ->
    camera, ``cam_k`` [3, 3], the image size from ``mask`` [n, H, W].  Only these are read: the renderer makes its own rays."""
    from . import captured_data
    cap = captured_data._open_capture(path)
    try:
        K = np.asarray(cap["cam_k"][:], dtype=np.float64)
        n, height, width = (int(v) for v in cap["mask"].shape)
        cams = {}
        for k in view_ids:
            if not 0 <= k < n:
                raise ValueError(f"view {k}: the capture has views 0..{n - 1}")
            R = np.asarray(cap["cam_proj"][k], dtype=np.float64)
            cams[k] = (R, K, np.linalg.inv(R), np.linalg.inv(K))
    finally:
        if hasattr(cap, "close"):
            cap.close()
    return height, width, cams


def main(argv=None):
    ap = argparse.ArgumentParser(description="Render what a camera sees of a textured screen through the glass object and write one image per view.")
    ap.add_argument("--name", default="horse")
    ap.add_argument("--data-path", default="./data/")
    ap.add_argument("--mesh", default=None, help="the mesh to look through (default: <data-path>/<name>_vh.ply)")
    ap.add_argument("--capture", default=None, help=".npz / .h5 capture: its cameras (cam_proj, cam_k) and its resolution are used")
    ap.add_argument("--views", type=int, default=72, help="views of the turntable used without --capture")
    ap.add_argument("--view-ids", type=int, nargs="+", default=[0])
    ap.add_argument("--res", type=int, nargs=2, default=[512, 512], metavar=("H", "W"), help="image size of the turntable cameras (a capture has its own)")
    ap.add_argument("--supersample", type=int, default=2)
    ap.add_argument("--max-bounces", type=int, default=6)
    ap.add_argument("--tir", choices=("drop", "reflect"), default="reflect")
    ap.add_argument("--refraction", choices=("reference", "snell"), default="snell")
    ap.add_argument("--no-fresnel", action="store_true")
    ap.add_argument("--ior", type=float, default=None, help="index of refraction of the object (default: the package's intIOR)")
    ap.add_argument("--absorption", type=float, nargs="+", default=None, metavar="A",
                    help="Beer-Lambert absorption per unit of mesh length: one number, or one per channel (default: clear glass)")
    ap.add_argument("--background", default="checker", help="checker, ramp, or a texture file (.npy, .ppm, .pgm, or what PIL reads)")
    ap.add_argument("--texture-size", type=int, default=1024, help="texels per side of a procedural background")
    ap.add_argument("--span", type=float, default=2.0, help="side of the screen in units of the object's extent")
    ap.add_argument("--environment", default=None, metavar="FILE",
                    help="a lat-long panorama seen where the screen is not: Radiance .hdr, .npy, .ppm, .pgm, or what PIL reads")
    ap.add_argument("--env-rotation", nargs="+", default=None, metavar="R",
                    help="world -> environment frame, y up: nine numbers (row-major), or `yaw DEG`")
    ap.add_argument("--no-screen", action="store_true", help="render without a screen: every ray sees the environment")
    ap.add_argument("--reflection", action="store_true", help="add the light reflected off the outer surface (needs --environment and the Fresnel term)")
    ap.add_argument("--invalid", type=float, nargs="+", default=[0.0], help="colour of samples whose path does not complete")
    ap.add_argument("--void", type=float, nargs="+", default=[0.0], help="colour of samples that miss the screen")
    ap.add_argument("-o", "--output", required=True, help="directory the images are written to")
    ap.add_argument("--format", default="png", help="png (needs PIL; netpbm is written without it), ppm / pgm")
    ap.add_argument("--force", action="store_true", help="overwrite existing images")
    a = ap.parse_args(argv)
    if (a.env_rotation is not None or a.no_screen or a.reflection) and a.environment is None:
        raise SystemExit("--env-rotation, --no-screen and --reflection need --environment")
    if a.reflection and a.no_fresnel:
        raise SystemExit("--reflection cannot be combined with --no-fresnel")
    if a.environment is not None and a.absorption is not None:
        raise SystemExit("--environment cannot be combined with --absorption")
    rotation = None
    if a.env_rotation is not None:
        try:
            if a.env_rotation[0] == "yaw" and len(a.env_rotation) == 2:
                rotation = Environment.yaw(float(a.env_rotation[1]))
            elif len(a.env_rotation) == 9:
                rotation = np.array([float(x) for x in a.env_rotation]).reshape(3, 3)
            else:
                raise ValueError
        except ValueError:
            raise SystemExit(f"--env-rotation takes nine numbers or `yaw DEG`, got {' '.join(a.env_rotation)!r}") from None
    stem = os.path.join(a.output, a.name + "_view{:03d}")
    for k in a.view_ids:
        for ext in {a.format, "ppm", "pgm"}:
            if os.path.exists(stem.format(k) + "." + ext) and not a.force:
                raise SystemExit(f"{stem.format(k)}.{ext} exists: pass --force to overwrite it")
    from . import diffrender as Render, views
    scene = Render.Scene(a.mesh or os.path.join(a.data_path, f"{a.name}_vh.ply"), 0)
    if a.ior is not None:
        Render.intIOR = a.ior
    center, extent = views.mesh_frame(scene.mesh.vertices)
    if a.capture is not None:
        height, width, cams = capture_cameras(a.capture, a.view_ids)
    else:
        height, width = a.res
        turntable = views.turntable_cameras(center, extent, a.views, width, height)
        cams = {k: turntable[k] for k in a.view_ids}
    texture = None if a.no_screen else _background(a.background, a.texture_size)
    more = {} if a.environment is None else {"environment": Environment.load(a.environment, rotation), "reflection": a.reflection}      # (without it: the call of before)
    report = {"name": a.name, "height": height, "width": width, "views": []}
    for k in a.view_ids:
        screen = None if a.no_screen else Screen.behind(cams[k], center, extent, texture.shape[1], texture.shape[0], span=a.span)
        image, hit, through = scene.render_image(cams[k], height, width, screen, texture, supersample=a.supersample, max_bounces=a.max_bounces,
                                                 tir=a.tir, refraction=a.refraction, fresnel=not a.no_fresnel, void=a.void, invalid=a.invalid,
                                                 want_planes=True, absorption=a.absorption, **more)[:3]
        path = write_image(stem.format(k) + "." + a.format, image, force=a.force)
        report["views"].append({"view": k, "image": path, "hit_share": float(hit.mean()), "through_share": float(through.mean())})
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
