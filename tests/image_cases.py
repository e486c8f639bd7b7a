"""Scenes of the forward renderer's tests (Scene.render_image): small views of data/hand_vh.ply in front of a random texture, and the
restatement's result for each of them (tests/image_ref.py), computed once per process and never modified."""
import functools
import os

import numpy as np

import image_ref
from conftest import IOR, data_path
from drt_amd import mesh_io, render, views
from oracle import diffrender_oracle as orc

EXT = orc.EXT_IOR
N_VIEWS, DISTANCE_FACTOR = 72, 1.2
TEX, SPAN = 64, 2.0
LAWS = [(2, "drop", "reference"), (6, "reflect", "reference"), (6, "reflect", "snell")]
RAY_ABS = 1e-10              # the project's exit-ray tolerance (tests/test_gpu_paths.py)
GRAZING = 0.05               # |dot(d, n)| below this: the plane hit amplifies the exit ray's error by more than 1 + 1 / 0.05 = 21
BORDER = 1e-3                # texels: a sample this close to a screen border may fall on the other side of it
SENSITIVE_CAP = 0.03         # share of pixels the image comparison may leave out
FUZZ_ORI, FUZZ_DIR = 1e-9, 1e-10          # the project's exit-ray tolerances on random shapes (tests/test_gpu_fuzz.py): origin, direction

# (name, view, height, width, supersample, channels)
SCENES = {"v5": (5, 32, 32, 2, 3), "v41": (41, 32, 32, 2, 3), "wide": (41, 24, 40, 2, 1)}


@functools.lru_cache(maxsize=None)
def hand():
    return mesh_io.read_ply(data_path("hand_vh.ply"))


@functools.lru_cache(maxsize=None)
def frame():
    return views.mesh_frame(hand().vertices)


def camera(view, height, width):
    center, extent = frame()
    return views.turntable_cameras(center, extent, N_VIEWS, width, height, distance_factor=DISTANCE_FACTOR)[view]


def texture(channels, seed=7):
    return np.random.default_rng(seed).random((TEX, TEX, channels)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    view, height, width, s, channels = SCENES[name]
    center, extent = frame()
    cam = camera(view, height, width)
    return dict(name=name, mesh=hand(), camera_M=cam, height=height, width=width, s=s, texture=texture(channels),
                screen=render.Screen.behind(cam, center, extent, TEX, TEX, span=SPAN), void=0.25, invalid=0.75)


@functools.lru_cache(maxsize=None)
def reference(name, law, fresnel):
    """image_ref.render of a scene under (max_bounces, tir, refraction); shared by the tests, left unchanged."""
    sc = scene(name)
    return image_ref.render(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], sc["s"],
                            law[0], law[1], law[2], fresnel, sc["void"], sc["invalid"], IOR, EXT)


def _scene(name):
    """A named scene, or a scene dict of the same shape as it is (tests/image_fuzz_cases.py)."""
    return name if isinstance(name, dict) else scene(name)


def sensitive(name, ref):
    """bool [H, W]: pixels with a sample whose exit ray grazes the screen (|dot(d, n^)| < GRAZING) or lands within BORDER texels of one of
    its borders -- samples that evaluate the plane at all (direct and through ones that see it).  The tops of u and v are the texture's
    own width and height, less one."""
    sc = _scene(name)
    tex_h, tex_w = np.asarray(sc["texture"]).shape[:2]
    n = np.cross(sc["screen"].eu, sc["screen"].ev)
    cos = (ref["dn"] / np.linalg.norm(n)).abs().numpy()
    looks = (ref["cls"] != image_ref.INVALID).numpy()
    seen = looks & (ref["dn"] != 0).numpy() & (ref["t"] > 0).numpy()
    u, v = ref["u"].numpy(), ref["v"].numpy()
    near = np.zeros_like(seen)
    for w, top in ((u, tex_w - 1), (v, tex_h - 1)):
        near |= (np.abs(w) < BORDER) | (np.abs(w - top) < BORDER)
    bad = (looks & (cos < GRAZING)) | (seen & near)
    return bad.reshape(sc["height"] * sc["width"], -1).any(1).reshape(sc["height"], sc["width"])


def tolerance(name, ref):
    """2^-23 + G * RAY_ABS * (1 + t_max) * 21 / pitch: an exit ray off by RAY_ABS in origin and direction moves its screen point by at most
    RAY_ABS (1 + t) (1 + 1 / GRAZING) off the grazing cut, i.e. by that many / pitch texels, and a texel step changes the bilinear
    sample by at most G, the largest difference between neighbouring texels; 2^-23 is the float32 store of a value in [0, 1].
    A scene dict (a random shape) has the exit-ray tolerances of the project's fuzz tests in place of RAY_ABS (1 + t_max): FUZZ_ORI on
    the origin and FUZZ_DIR on the direction, i.e. FUZZ_ORI + FUZZ_DIR * t_max; and, its texture not being square, the smaller of the two
    pitches |eu|, |ev| (a displacement of the screen point is that many texels along the finer axis)."""
    sc = _scene(name)
    tex = sc["texture"].astype(np.float64)
    G = max(np.abs(np.diff(tex, axis=0)).max(), np.abs(np.diff(tex, axis=1)).max())
    t = ref["t"].numpy()[ref["on"].numpy()]
    t_max = float(t.max()) if len(t) else 0.0
    if isinstance(name, dict):
        pitch = min(float(np.linalg.norm(sc["screen"].eu)), float(np.linalg.norm(sc["screen"].ev)))
        return 2.0 ** -23 + G * (FUZZ_ORI + FUZZ_DIR * t_max) * (1.0 + 1.0 / GRAZING) / pitch
    pitch = float(np.linalg.norm(sc["screen"].eu))
    return 2.0 ** -23 + G * RAY_ABS * (1.0 + t_max) * (1.0 + 1.0 / GRAZING) / pitch


if __name__ == "__main__":       # the figures the GPU test's docstring quotes: python tests/image_cases.py
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for name in SCENES:
        for law in LAWS:
            r = reference(name, law, True)
            cls = r["cls"].numpy()
            looks = cls != image_ref.INVALID
            print(name, law, "direct", int((cls == 0).sum()), "through", int((cls == 1).sum()), "invalid", int((cls == 2).sum()),
                  "off-screen", int((looks & ~r["on"].numpy()).sum()), "away", int((looks & ~((r["t"] > 0).numpy())).sum()),
                  "sensitive pixels", int(sensitive(name, r).sum()), "of", cls.size // SCENES[name][3] ** 2, "tol", tolerance(name, r))
