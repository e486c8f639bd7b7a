"""Cases of the environment tests (Scene.render_image with ``environment``): the three scenes of ``image_cases.SCENES`` under its three
``LAWS``, each with its screen and with ``screen=None``, with the outer-surface reflection on and off, in front of a random float32 environment [16, 32, C] turned by Rx(0.3) Ry(0.7);
the restatement's result for each (tests/image_env_ref.py on top of ``image_cases.reference``), computed once per process and never modified."""
import functools
import math
import os

import numpy as np
import torch

import image_cases
import image_env_ref
import image_ref
from drt_amd import render

EH, EW = 16, 32
POLE = 1e-3                  # 1 - |e_y| below this: the pole amplifies an error of the direction into u without bound
SCENES, LAWS = image_cases.SCENES, image_cases.LAWS
# The error of phi = atan2(., .) in double precision, in radians, for results of magnitude up to pi (1 ulp = 2^-51): what reaches u.
# The test holds a device image against a host restatement, and each side is off the true phi by its own library's error, so the two
# differ by at most the SUM of the bounds.  Host: 1 ulp (glibc's manual, "Errors in Math Functions"; SLEEF's u10 functions in torch).
# Device: 6 ulp, the bound for atan2 in the OpenCL C specification (7.4, "Relative error as ULPs") that ROCm's device library OCML
# states it meets.  (acos, which reaches v, has 1 ulp and 4 ulp there: smaller, and v is not in the bound below.)
MATH_ABS = (1 + 6) * 2.0 ** -51


@functools.lru_cache(maxsize=None)
def environment(channels, seed=11):
    return render.Environment(np.random.default_rng(seed).random((EH, EW, channels)).astype(np.float32), image_env_ref.rotation())


@functools.lru_cache(maxsize=None)
def reflected(name):
    """image_env_ref.reflection of a scene's sample rays: the same under every law (the first interaction is), left unchanged."""
    sc = image_cases.scene(name)
    o, d = image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
    return image_env_ref.reflection(sc["mesh"].faces, sc["mesh"].vertices, o, d, image_cases.IOR, image_cases.EXT)


@functools.lru_cache(maxsize=None)
def reference(name, law, with_screen, reflection=False):
    """image_env_ref.render_from of a scene under (max_bounces, tir, refraction), Fresnel on; shared by the tests, left unchanged."""
    sc = image_cases.scene(name)
    stage = image_cases.reference(name, law, True)
    env = environment(sc["texture"].shape[2])
    return image_env_ref.render_from(stage, sc["height"], sc["width"], sc["s"], sc["screen"] if with_screen else None, sc["texture"] if with_screen else None,
                                     env.texels, env.rotation, sc["invalid"], reflected(name) if reflection else None)


def sensitive(name, law, with_screen, reflection=False, ref=None, stage=None):
    """bool [H, W]: with a screen ``image_cases.sensitive``'s pixels (a sample that grazes the screen's plane or lands near a border of it
    may change between screen and environment); pixels with a sample that goes to the environment within POLE of a pole; and, with the
    reflection, pixels with an added reflected ray that goes to the environment within POLE of a pole, sees the screen's plane within
    BORDER texels of a border, or lands on the screen with |dot(d, n^)| < GRAZING.  The tops of u and v are the texture's own width and
    height, less one.  A scene dict (tests/image_fuzz_cases.py) comes with its own ``ref`` (``image_env_ref.render_from``'s dict) and
    ``stage`` (``image_ref.render``'s)."""
    sc = image_cases._scene(name)
    ref = reference(name, law, with_screen, reflection) if ref is None else ref
    tex_h, tex_w = np.asarray(sc["texture"]).shape[:2]
    bad = (ref["src"] == image_env_ref.ENV) & (1.0 - ref["ey"].abs() < POLE)
    if reflection:
        rb, added = ref["rb"], ref["added"]
        bad = bad | (added & ~rb["on"] & (1.0 - rb["ey"].abs() < POLE))
        if with_screen:
            n = np.cross(sc["screen"].eu, sc["screen"].ev)
            cos = (rb["dn"] / np.linalg.norm(n)).abs()
            seen = (rb["dn"] != 0) & (rb["t"] > 0)
            near = torch.zeros_like(seen)
            for w, top in ((rb["su"], tex_w - 1), (rb["sv"], tex_h - 1)):
                near = near | (w.abs() < image_cases.BORDER) | ((w - top).abs() < image_cases.BORDER)
            bad = bad | (added & ((rb["on"] & (cos < image_cases.GRAZING)) | (seen & near)))
    bad = bad.numpy().reshape(sc["height"] * sc["width"], -1).any(1).reshape(sc["height"], sc["width"])
    if with_screen:
        bad = bad | image_cases.sensitive(name, image_cases.reference(name, law, True) if stage is None else stage)
    return bad


TARGET_IOR = 1.55            # the photograph: the same scene at another IOR (tests/image_loss_cases.py)
TEXEL_MARGIN = 1e-6          # texels: every environment-going ray of a loss case is at least this far from a texel line of the environment


def _loss_args(name, with_screen):
    sc = image_cases.scene(name)
    env = environment(sc["texture"].shape[2])
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None,
            sc["texture"] if with_screen else None, env.texels, env.rotation)


@functools.lru_cache(maxsize=None)
def loss_target(name, law, with_screen, reflection):
    """float32 [H, W, C]: the restatement's image of the case at TARGET_IOR."""
    sc = image_cases.scene(name)
    fwd = image_env_ref.loss_forward(*_loss_args(name, with_screen), sc["s"], law, sc["invalid"], TARGET_IOR, image_cases.EXT, reflection)
    return np.ascontiguousarray(fwd["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1).numpy())


@functools.lru_cache(maxsize=None)
def loss_reference(name, law, with_screen, reflection, weighted=False, detach=None):
    """image_env_ref.loss_and_grads of a case at conftest.IOR; its image is held to ``reference``'s, and every ray that goes to the
    environment -- exit or added reflection -- is asserted to stay TEXEL_MARGIN from the environment's texel lines and inside the clamp
    of v: a condition on the inputs (the environment's seed), not a measurement."""
    import image_loss_cases
    sc = image_cases.scene(name)
    ref = image_env_ref.loss_and_grads(*_loss_args(name, with_screen), loss_target(name, law, with_screen, reflection), sc["s"], law, sc["invalid"],
                                       image_cases.IOR, image_cases.EXT, weight=image_loss_cases.half_weight(name) if weighted else None, reflect=reflection,
                                       detach=detach)
    base = reference(name, law, with_screen, reflection)
    fwd = ref["fwd"]
    assert np.array_equal(fwd["cls"].numpy(), base["cls"].numpy())
    assert np.abs(ref["image"].astype(np.float64) - base["image"].numpy().astype(np.float64)).max() <= 2.0 ** -22
    rays = [(fwd["bg"], (fwd["cls"] == image_ref.THROUGH) & ~fwd["bg"]["on"])]
    if reflection:
        assert np.array_equal(fwd["added"].numpy(), base["added"].numpy())
        rays.append((fwd["rb"], ~fwd["rb"]["on"]))
    for bg, sel in rays:
        u, v = bg["u"].detach().numpy()[sel.numpy()], bg["v"].detach().numpy()[sel.numpy()]
        assert np.abs(u - np.rint(u)).min() >= TEXEL_MARGIN and np.abs(v - np.rint(v)).min() >= TEXEL_MARGIN
    return ref


def env_step(channels):
    """G_env: the largest difference between neighbouring texels of the environment, the seam's pair included (``channels``: of the named
    cases' environment, or a scene dict with its own ``environment``)."""
    env = (np.asarray(channels["environment"]) if isinstance(channels, dict) else environment(channels).texels).astype(np.float64)
    return max(np.abs(np.diff(env, axis=0)).max(), np.abs(np.diff(np.concatenate([env, env[:, :1]], axis=1), axis=1)).max())


def tolerance(name, law, with_screen, stage=None):
    """2^-23 + the screen's term (image_cases.tolerance without its own 2^-23; with a screen) + G_env * delta * Ew / (2 pi sin(theta_min)):
    an exit direction off by delta = RAY_ABS + MATH_ABS moves phi by at most delta / sin(theta) off the pole cut, i.e. u by that times
    Ew / (2 pi) texels, and a texel step changes the bilinear sample by at most G_env, the largest difference between neighbouring texels
    of the environment (the seam's pair included); sin(theta_min) = sqrt(1 - (1 - POLE)^2).
    This is the bound as it was set for these tests, and it takes the direction's error through phi and u only.  The same delta reaches
    theta = acos(e_y) with the same 1 / sin(theta) and v with the factor Eh / pi, which equals Ew / (2 pi) for this 16 x 32 map: a bound
    that covered both coordinates would have the environment term twice (1.1e-8 more on 1.3e-7).  The term is NOT added: the bound stays
    as set, it is the narrower of the two, and a device image that needed the v share would fail here and be looked at.
    With the reflection a colour is T B(exit) + R1 B(ro, wr) with T <= 1 - R1: the two backgrounds' errors are weighted by factors that
    sum to at most 1, so the same bound holds.
    A scene dict (tests/image_fuzz_cases.py; ``stage``: its ``image_ref.render``) has an environment of its own extents: the texel
    factor is max(Ew / 2 pi, Eh / pi), the same number for 16 x 32, and delta is image_cases.FUZZ_DIR + MATH_ABS."""
    if isinstance(name, dict):
        eh, ew = np.asarray(name["environment"]).shape[:2]
        sin_min = math.sqrt(1.0 - (1.0 - POLE) ** 2)
        tol = 2.0 ** -23 + env_step(name) * (image_cases.FUZZ_DIR + MATH_ABS) * max(ew / (2.0 * math.pi), eh / math.pi) / sin_min
        if with_screen:
            tol += image_cases.tolerance(name, stage) - 2.0 ** -23
        return tol
    sc = image_cases.scene(name)
    G = env_step(sc["texture"].shape[2])
    sin_min = math.sqrt(1.0 - (1.0 - POLE) ** 2)
    tol = 2.0 ** -23 + G * (image_cases.RAY_ABS + MATH_ABS) * EW / (2.0 * math.pi * sin_min)
    if with_screen:
        tol += image_cases.tolerance(name, image_cases.reference(name, law, True)) - 2.0 ** -23
    return tol


if __name__ == "__main__":       # the figures the GPU test's docstring quotes: python tests/image_env_cases.py
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for name in SCENES:
        for law in LAWS:
            for with_screen in (True, False):
                for reflection in (False, True):
                    r = reference(name, law, with_screen, reflection)
                    src = r["src"].numpy()
                    bad = sensitive(name, law, with_screen, reflection)
                    print(name, law, "screen" if with_screen else "no screen", "reflection" if reflection else "no reflection", "fill", int((src == 0).sum()),
                          "screen", int((src == 1).sum()), "environment", int((src == 2).sum()), "added reflections", int(r["added"].sum()) if reflection else 0,
                          "of them on the screen", int((r["added"] & r["rb"]["on"]).sum()) if reflection else 0, "sensitive pixels", int(bad.sum()), "of", bad.size,
                          "tol", tolerance(name, law, with_screen))
