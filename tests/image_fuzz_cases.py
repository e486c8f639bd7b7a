"""Random cases of the image family's fuzz tests (tests/test_image_fuzz_host.py on the CPU, tests/test_gpu_image_fuzz.py on the device):
``case(seed)`` is a scene dict shaped like ``image_cases.scene`` -- a random closed shape of ``test_gpu_fuzz._shape`` (one body, two shells
or two lobes), a turntable camera far from, close to or inside it, an odd image size, 1 to 4 samples a side, a NON-SQUARE texture on a
screen that may be tilted against the camera, a non-square environment under a seeded rotation -- with its own IORs, law, Fresnel flag,
fills, weight plane, absorption and target.  Everything is deterministic from the seed.  ``CASES`` is the literal list of admitted seeds;
admission is computed from the float64 restatements alone (tests/test_image_fuzz_host.py), never from what a device returns."""
import functools
import math

import numpy as np
import torch

import image_cases
import image_loss_ref
from conftest import IOR
from drt_amd import calibrate, render, views
from test_gpu_fuzz import _shape

EXT = image_cases.EXT
BASE = 11000                 # the generator of seed k is numpy's default_rng(BASE + k)
N_VIEWS = 72
IORS_INT, IORS_EXT = (IOR, 1.1, 1.33, 2.4), (EXT, 1.0)
DISTANCES = (2.5, 1.2, 0.8, 0.3)          # 0.3: the camera is inside the object or at its rim
SIZES = ((1, 1), (1, 67), (5, 7), (17, 23), (32, 20), (9, 41), (3, 3), (7, 5))
TEXTURES = ((33, 17), (17, 33), (2, 2), (2, 37), (64, 40))          # (Th, Tw)
SPANS = (1.0, 2.0, 8.0)
ENVIRONMENTS = ((16, 32), (8, 40), (24, 20), (2, 3))                # (Eh, Ew)
MAX_SAMPLES = 10000          # every case has fewer samples than this
TARGET_FACTOR = 1.05         # the target is the restatement's own image at this multiple of ior_int

# The admitted seeds, chosen for the coverage tests/test_image_fuzz_host.py asserts.  A seed that fails admission there (sensitive share,
# texel margins, a loss of rounding alone, conditioning) is replaced by the next one that serves the same purpose and noted here with its
# figure.  Rejected: 2 (17 x 23, s = 3: 10.5 % of the pixels sensitive), 6 (14.6 %), 32 (3.6 %), 40 (5.7 %), 26 (a through sample exactly on
# a texel line: margin 0); 4, 17, 19, 39, 44, 45 (1 x 1) and 15, 27, 35 (every sample invalid): the target at 1.05 ior_int is the image
# itself, a loss of 1e-15 and less -- 97 is the 1 x 1 case; of the views, 24 (an environment read 6.0e-7 from a texel line) -- 1 took its place.
CASES = [0, 1, 8, 16, 20, 22, 24, 25, 28, 29, 33, 42, 64, 97, 110, 114]
SCREEN_CASES = [0, 1, 16, 25, 64, 97]
CAMERA_CASES = [20, 22, 24, 25, 110, 114]
ABSORB_CASES = [0, 1, 28, 33, 42, 64]
ENV_CASES = [(0, True, True), (24, True, True), (33, True, False), (114, False, True), (22, False, True), (28, False, False)]          # (seed, with_screen, reflection)
VIEWS_CASES = [0, 1, 22, 33]


def rotation(a, b):
    """Rx(a) Ry(b), world -> environment frame."""
    cx, sx, cy, sy = math.cos(a), math.sin(a), math.cos(b), math.sin(b)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def _fill(rng, channels):
    """A fill in [0, 1]: a scalar on some cases, one value per channel on others."""
    return float(rng.random()) if rng.random() < 0.5 else rng.random(channels)


def _weight(rng, height, width):
    """None, a random positive plane, or one with a block of zeros (float32 [H, W])."""
    kind = int(rng.integers(3))
    w = (0.25 + 1.5 * rng.random((height, width))).astype(np.float32)
    if kind == 0:
        return None
    if kind == 2:
        y0, x0 = int(rng.integers(height)), int(rng.integers(width))
        w[y0: y0 + max(1, height // 2), x0: x0 + max(1, width // 2)] = 0.0
    return np.ascontiguousarray(w)


def screen_for(rng, cam, center, extent, tex_h, tex_w):
    """``render.Screen.behind`` at a seeded span; on a third of the cases moved rigidly (``calibrate.screen_pose``) by a few texels and a
    tilt of a few degrees, so that eu and ev are not the camera's axes."""
    span = float(rng.choice(SPANS))
    screen = render.Screen.behind(cam, center, extent, tex_w, tex_h, span=span)
    moved = bool(rng.random() < 1.0 / 3.0)
    shift, tilt = rng.uniform(-3.0, 3.0, 3), np.radians(rng.uniform(-6.0, 6.0, 3))
    if moved:
        half = math.hypot((tex_w - 1) / 2.0, (tex_h - 1) / 2.0)
        pose = calibrate.screen_pose(screen, tex_h, tex_w, torch.tensor(np.concatenate([shift, tilt * half]))).numpy()
        screen = render.Screen(pose[0], pose[1], pose[2])
    return screen, span, moved


@functools.lru_cache(maxsize=None)
def base(seed):
    """The case without its target (which needs a trace): every draw, in a fixed order."""
    rng = np.random.default_rng(BASE + seed)
    mesh = _shape(rng)
    ior_int, ior_ext = float(rng.choice(IORS_INT)), float(rng.choice(IORS_EXT))
    center, extent = views.mesh_frame(mesh.vertices)
    distance, view = float(rng.choice(DISTANCES)), int(rng.integers(N_VIEWS))
    height, width = SIZES[int(rng.integers(len(SIZES)))]
    s, channels = int(rng.integers(1, 5)), int(rng.choice([1, 3]))
    while height * width * s * s >= MAX_SAMPLES:
        s -= 1
    cam = views.turntable_cameras(center, extent, N_VIEWS, width, height, distance_factor=distance)[view]
    tex_h, tex_w = TEXTURES[int(rng.integers(len(TEXTURES)))]
    texture3 = rng.random((tex_h, tex_w, channels)).astype(np.float32)
    flat = bool(channels == 1 and rng.random() < 0.5)              # C = 1: a [Th, Tw] texture on some cases, [Th, Tw, 1] on the others
    screen, span, moved = screen_for(rng, cam, center, extent, tex_h, tex_w)
    env_h, env_w = ENVIRONMENTS[int(rng.integers(len(ENVIRONMENTS)))]
    env = rng.random((env_h, env_w, channels)).astype(np.float32)
    angles = rng.uniform(-math.pi, math.pi, 2)
    void, invalid = _fill(rng, channels), _fill(rng, channels)
    weight = _weight(rng, height, width)
    law = image_cases.LAWS[int(rng.integers(len(image_cases.LAWS)))]
    fresnel = bool(rng.random() < 0.5)
    sigma = rng.uniform(1e-3, 8e-3, channels)
    return dict(name=f"fuzz{seed}", seed=seed, mesh=mesh, center=center, extent=extent, ior_int=ior_int, ior_ext=ior_ext, distance=distance, view=view,
                camera_M=cam, height=height, width=width, s=s, texture=np.ascontiguousarray(texture3[:, :, 0]) if flat else texture3, texture3=texture3,
                screen=screen, span=span, moved=moved, environment=env, rotation=rotation(float(angles[0]), float(angles[1])), void=void, invalid=invalid,
                weight=weight, law=law, fresnel=fresnel, sigma=sigma)


def render_args(sc):
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture3"])


def target_of(sc):
    """float32 [H, W, C]: the restatement's image of a scene at TARGET_FACTOR * ior_int (as image_loss_cases.target does at 1.55)."""
    fwd = image_loss_ref.forward(*render_args(sc), sc["s"], sc["law"], sc["fresnel"], sc["void"], sc["invalid"], TARGET_FACTOR * sc["ior_int"], sc["ior_ext"])
    return np.ascontiguousarray(fwd["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1).numpy())


@functools.lru_cache(maxsize=None)
def case(seed):
    """The scene dict of a seed, with its target; shared by the tests and left unchanged."""
    sc = dict(base(seed))
    sc["target"] = target_of(sc)
    return sc


def two_components(sc):
    """Whether the mesh is two bodies (no vertex of one is in a face of the other): ``_shape`` appends the second body's vertices."""
    F = np.asarray(sc["mesh"].faces)
    for cut in range(1, len(sc["mesh"].vertices)):
        lo = (F < cut).all(1)
        if lo.any() and not lo.all() and ((F < cut).any(1) == lo).all():
            return True
    return False


# ---- the restatements' results, computed once per process and never modified ---------------------------------------------------------------
def _law_args(sc):
    return (sc["s"], sc["law"], sc["fresnel"], sc["void"], sc["invalid"], sc["ior_int"], sc["ior_ext"])


@functools.lru_cache(maxsize=None)
def stage(seed, fresnel=None):
    """image_ref.render of a case (``fresnel``: the case's own flag, or this one -- the environment members are Fresnel-on)."""
    import image_ref
    sc = case(seed)
    return image_ref.render(*render_args(sc), sc["s"], *sc["law"], sc["fresnel"] if fresnel is None else fresnel, sc["void"], sc["invalid"], sc["ior_int"],
                            sc["ior_ext"])


def loss_of_scene(sc, **kw):
    """image_loss_ref.loss_and_grads of a scene dict with its own target and weight."""
    return image_loss_ref.loss_and_grads(*render_args(sc), sc["target"], *_law_args(sc), weight=sc["weight"], **kw)


@functools.lru_cache(maxsize=None)
def loss_reference(seed, throughput_gradient=True):
    return loss_of_scene(case(seed), throughput_gradient=throughput_gradient)


@functools.lru_cache(maxsize=None)
def screen_reference(seed, detach_direct=False):
    import image_screen_ref
    sc = case(seed)
    const = image_screen_ref.trace(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["s"], sc["law"], sc["fresnel"],
                                   sc["ior_int"], sc["ior_ext"])
    return image_screen_ref.loss_and_grads(const, image_screen_ref.rows_of(sc["screen"]), sc["texture3"], sc["target"], sc["s"], sc["void"], sc["invalid"],
                                           weight=sc["weight"], detach_direct=detach_direct)


@functools.lru_cache(maxsize=None)
def camera_reference(seed):
    import image_camera_ref
    sc = case(seed)
    return image_camera_ref.loss_and_grads(*render_args(sc), sc["target"], *_law_args(sc), weight=sc["weight"])


@functools.lru_cache(maxsize=None)
def absorb_reference(seed, length_gradient=True):
    import image_absorb_ref
    sc = case(seed)
    return image_absorb_ref.loss_and_grads(*render_args(sc), sc["target"], *_law_args(sc), sc["sigma"], weight=sc["weight"], length_gradient=length_gradient)


def env_args(sc, with_screen):
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None,
            sc["texture3"] if with_screen else None, sc["environment"], sc["rotation"])


@functools.lru_cache(maxsize=None)
def env_target(seed, with_screen, reflection):
    """float32 [H, W, C]: image_env_ref's image of the case at TARGET_FACTOR * ior_int."""
    import image_env_ref
    sc = case(seed)
    fwd = image_env_ref.loss_forward(*env_args(sc, with_screen), sc["s"], sc["law"], sc["invalid"], TARGET_FACTOR * sc["ior_int"], sc["ior_ext"], reflection)
    return np.ascontiguousarray(fwd["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1).numpy())


@functools.lru_cache(maxsize=None)
def env_image_reference(seed, with_screen, reflection):
    """image_env_ref.render_from on ``stage(seed, True)``."""
    import image_env_ref
    import image_ref
    sc = case(seed)
    refl = None
    if reflection:
        o, d = image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
        refl = image_env_ref.reflection(sc["mesh"].faces, sc["mesh"].vertices, o, d, sc["ior_int"], sc["ior_ext"])
    return image_env_ref.render_from(stage(seed, True), sc["height"], sc["width"], sc["s"], sc["screen"] if with_screen else None,
                                     sc["texture3"] if with_screen else None, sc["environment"], sc["rotation"], sc["invalid"], refl)


@functools.lru_cache(maxsize=None)
def env_loss_reference(seed, with_screen, reflection):
    import image_env_ref
    sc = case(seed)
    return image_env_ref.loss_and_grads(*env_args(sc, with_screen), env_target(seed, with_screen, reflection), sc["s"], sc["law"], sc["invalid"], sc["ior_int"],
                                        sc["ior_ext"], weight=sc["weight"], reflect=reflection)


@functools.lru_cache(maxsize=None)
def env_param_reference(seed, with_screen, reflection):
    import image_env_param_ref
    sc = case(seed)
    return image_env_param_ref.loss_and_grads(*env_args(sc, with_screen), env_target(seed, with_screen, reflection), sc["s"], sc["law"], sc["invalid"],
                                              sc["ior_int"], sc["ior_ext"], weight=sc["weight"], reflect=reflection)


# ---- the multi-view captures ---------------------------------------------------------------------------------------------------------------
VIEW_DISTANCES = (2.5, 1.2, 0.8)
VIEW_IDS = [2, 0, 2]          # out of order, with a repeat


@functools.lru_cache(maxsize=None)
def capture(seed):
    """Three views of the shape of a case: three cameras at the three VIEW_DISTANCES, each with a screen of its own (seeded span, moved on a
    third), the case's size, samples, texture, fills and law; per view a scene dict with its own target and weight, stacked for the binding."""
    sc = case(seed)
    rng = np.random.default_rng(BASE + 500000 + seed)
    tex_h, tex_w = sc["texture3"].shape[:2]
    scs = []
    for k, distance in enumerate(VIEW_DISTANCES):
        cam = views.turntable_cameras(sc["center"], sc["extent"], N_VIEWS, sc["width"], sc["height"], distance_factor=distance)[int(rng.integers(N_VIEWS))]
        screen, span, moved = screen_for(rng, cam, sc["center"], sc["extent"], tex_h, tex_w)
        one = dict(sc, name=f"fuzz{seed}/view{k}", camera_M=cam, distance=distance, screen=screen, span=span, moved=moved,
                   weight=np.ascontiguousarray((0.25 + 1.5 * rng.random((sc["height"], sc["width"]))).astype(np.float32)))
        one["target"] = target_of(one)
        scs.append(one)
    return dict(scenes=scs, cams=[s["camera_M"] for s in scs], screens=[s["screen"] for s in scs], targets=np.stack([s["target"] for s in scs]),
                weights=np.stack([s["weight"] for s in scs]))


@functools.lru_cache(maxsize=None)
def capture_references(seed):
    """The restatement's result of every view of ``capture(seed)``."""
    return [loss_of_scene(one) for one in capture(seed)["scenes"]]


@functools.lru_cache(maxsize=None)
def capture_env(seed):
    """``capture(seed)`` in front of the case's environment, reflection on: per-view targets of image_env_ref, and its results."""
    import image_env_ref
    cap = capture(seed)
    targets, refs = [], []
    for one in cap["scenes"]:
        fwd = image_env_ref.loss_forward(*env_args(one, True), one["s"], one["law"], one["invalid"], TARGET_FACTOR * one["ior_int"], one["ior_ext"], True)
        targets.append(np.ascontiguousarray(fwd["mean"].detach().to(torch.float32).view(one["height"], one["width"], -1).numpy()))
        refs.append(image_env_ref.loss_and_grads(*env_args(one, True), targets[-1], one["s"], one["law"], one["invalid"], one["ior_int"], one["ior_ext"],
                                                 weight=one["weight"], reflect=True))
    return dict(targets=np.stack(targets), refs=refs)


def summed(refs, ids=VIEW_IDS):
    """The sum over the listed views of the restatement's loss, gradients and count."""
    return {k: sum(refs[i][k] for i in ids) for k in ("loss", "grad_V", "g_int", "g_ext", "count")}
