"""Cases of the tests of absorbing glass in the multi-view image term (Scene.image_loss_views_fused with ``absorption``): the
views v5 and v41 of tests/image_cases.py (the hand, 32 x 32, s = 2, C = 3) under its three laws with the coefficients of
tests/image_absorb_cases.py, in front of their screens ("screen": image_absorb_ref, the target of image_loss_cases), in the room of
tests/image_env_cases.py with their screens ("room-screen") and without ("room"; both image_absorb_env_ref, the targets of image_env_cases: the
CLEAR glass at TARGET_IOR), the reflection on and off where there is a room.  The restatement's result of every case is computed once per
process and never modified; the multi-view reference is the SUM of per-view results.

Every case is checked here, with the reference alone, for the conditions the comparisons rest on: the sensitive share of its pixels (the
pole cut of image_env_cases included) stays under image_cases.SENSITIVE_CAP, and every ray that goes to the environment stays TEXEL_MARGIN
from the environment's texel lines."""
import functools

import numpy as np

import image_absorb_cases
import image_absorb_env_ref
import image_cases
import image_env_cases
import image_loss_cases
import image_ref

PAIR = ("v5", "v41")
LAWS = image_cases.LAWS
KINDS = ("screen", "room-screen", "room")
# (kind, reflection): every background the call has
BACKGROUNDS = [("screen", False), ("room-screen", False), ("room-screen", True), ("room", False), ("room", True)]
SIGMA = np.array(image_absorb_cases.SIGMA3, np.float64)
TEXEL_MARGIN = image_env_cases.TEXEL_MARGIN


def has_screen(kind):
    return kind != "room"


def has_room(kind):
    return kind != "screen"


def target(name, law, kind, reflection=False):
    """float32 [H, W, C]: the photograph of the case, clear glass at TARGET_IOR."""
    if not has_room(kind):
        return image_loss_cases.target(name, law, True)
    return image_env_cases.loss_target(name, law, has_screen(kind), reflection)


def sensitive(name, law, kind, reflection=False):
    """bool [H, W]: the pixels an image comparison leaves out."""
    if not has_room(kind):
        return image_cases.sensitive(name, image_cases.reference(name, law, True))
    return image_env_cases.sensitive(name, law, has_screen(kind), reflection)


def _room_args(name, kind):
    sc = image_cases.scene(name)
    env = image_env_cases.environment(sc["texture"].shape[2])
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"] if has_screen(kind) else None,
            sc["texture"] if has_screen(kind) else None, env.texels, env.rotation)


@functools.lru_cache(maxsize=None)
def reference(name, law, kind, reflection=False, sigma=tuple(SIGMA), length_gradient=True, sigma_sees_reflection=False):
    """dict(loss, grad_V, g_int, g_ext, g_sigma, count, image, fwd) of one view of a case at conftest.IOR, asserted to meet the module's
    conditions."""
    assert has_room(kind) or not reflection
    sc = image_cases.scene(name)
    bad = sensitive(name, law, kind, reflection)
    assert bad.mean() <= image_cases.SENSITIVE_CAP, (name, law, kind, reflection, float(bad.mean()))
    if not has_room(kind):
        assert not sigma_sees_reflection
        if sigma == tuple(SIGMA):
            return image_absorb_cases.reference(name, law, True, length_gradient=length_gradient)
        import image_absorb_ref
        return image_absorb_ref.loss_and_grads(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"],
                                               target(name, law, kind), sc["s"], law, True, sc["void"], sc["invalid"], image_cases.IOR, image_cases.EXT,
                                               np.array(sigma), length_gradient=length_gradient)
    ref = image_absorb_env_ref.loss_and_grads(*_room_args(name, kind), target(name, law, kind, reflection), sc["s"], law, sc["invalid"], image_cases.IOR,
                                              image_cases.EXT, np.array(sigma), reflect=reflection, length_gradient=length_gradient,
                                              sigma_sees_reflection=sigma_sees_reflection)
    fwd = ref["fwd"]
    base = image_env_cases.reference(name, law, has_screen(kind), reflection)
    assert np.array_equal(fwd["cls"].numpy(), base["cls"].numpy())
    rays = [(fwd["bg"], (fwd["cls"] == image_ref.THROUGH) & ~fwd["bg"]["on"])]
    if reflection:
        assert np.array_equal(fwd["added"].numpy(), base["added"].numpy())
        rays.append((fwd["rb"], ~fwd["rb"]["on"]))
    for bg, sel in rays:
        u, v = bg["u"].detach().numpy()[sel.numpy()], bg["v"].detach().numpy()[sel.numpy()]
        assert np.abs(u - np.rint(u)).min() >= TEXEL_MARGIN and np.abs(v - np.rint(v)).min() >= TEXEL_MARGIN
    return ref


def summed(order, law, kind, reflection=False, **kw):
    """The multi-view reference of the listed views: the sum of loss, grad_V, g_int, g_ext, g_sigma and count over ``order``."""
    refs = [reference(name, law, kind, reflection, **kw) for name in order]
    return {k: sum(r[k] for r in refs) for k in ("loss", "grad_V", "g_int", "g_ext", "g_sigma", "count")}


def image_tolerance(name, law, kind):
    """The bound of an image comparison off the sensitive pixels: the background's own (image_cases.tolerance with a screen alone,
    image_env_cases.tolerance in a room) plus image_absorb_cases.image_tolerance's length term -- sigma_max (max_bounces - 1) 2 RAY_ABS
    (1 + 1 / GRAZING): |d c / d L| <= sigma_max for a colour in [0, 1], whichever background it came from."""
    length = float(SIGMA.max()) * (law[0] - 1) * 2 * image_cases.RAY_ABS * (1 + 1 / image_cases.GRAZING)
    if not has_room(kind):
        return image_cases.tolerance(name, image_cases.reference(name, law, True)) + length
    return image_env_cases.tolerance(name, law, has_screen(kind)) + length


if __name__ == "__main__":       # the conditions of every case: python tests/image_views_absorb_cases.py
    for law in LAWS:
        for kind, reflection in BACKGROUNDS:
            for name in PAIR:
                r = reference(name, law, kind, reflection)
                print(name, law, kind, "reflection" if reflection else "", "sensitive share", float(sensitive(name, law, kind, reflection).mean()), "loss", r["loss"],
                      "count", r["count"], "g_sigma", r["g_sigma"])
