"""Cases of the absorbing-image tests (Scene.render_image / Scene.image_loss_fused with ``absorption``): the scenes, laws and targets of
tests/image_loss_cases.py (the target is the CLEAR glass at TARGET_IOR) evaluated at ``conftest.IOR`` with the absorption coefficients
below; the restatement's result (tests/image_absorb_ref.py) of every case, computed once per process and never modified."""
import functools

import numpy as np

import image_absorb_ref
import image_cases
import image_loss_cases
from conftest import IOR

EXT = image_cases.EXT
LAWS = image_cases.LAWS
SCENES = image_loss_cases.SCENES
SIGMA3, SIGMA1 = (0.004, 0.012, 0.03), (0.012,)      # per unit of mesh length; the hand is 115 units across: A covers most of (0, 1)


def sigma(name):
    if isinstance(name, dict):           # a scene dict carries its own coefficients (tests/image_fuzz_cases.py)
        return np.asarray(name["sigma"], np.float64)
    return np.array(SIGMA3 if image_cases.SCENES[name][4] == 3 else SIGMA1, np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, law, fresnel, weighted=False, length_gradient=True):
    """image_absorb_ref.loss_and_grads of a case at conftest.IOR and sigma(name)."""
    sc = image_cases.scene(name)
    return image_absorb_ref.loss_and_grads(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"],
                                           image_loss_cases.target(name, law, fresnel), sc["s"], law, fresnel, sc["void"], sc["invalid"], IOR, EXT,
                                           sigma(name), weight=image_loss_cases.half_weight(name) if weighted else None, length_gradient=length_gradient)


def image_tolerance(name, base, law):
    """image_cases.tolerance plus sigma_max (max_bounces - 1) 2 RAY_ABS (1 + 1 / GRAZING): an interior segment's two end points are each
    off by at most RAY_ABS (1 + 1 / GRAZING) along the ray, there are at most max_bounces - 1 interior segments, and
    |d c / d L| <= sigma_max for a colour in [0, 1].  On a scene dict (a random shape) an end point is off by the fuzz tests' origin
    tolerance image_cases.FUZZ_ORI in place of RAY_ABS."""
    if isinstance(name, dict):
        return image_cases.tolerance(name, base) + float(sigma(name).max()) * (law[0] - 1) * 2 * image_cases.FUZZ_ORI * (1 + 1 / image_cases.GRAZING)
    return image_cases.tolerance(name, base) + float(sigma(name).max()) * (law[0] - 1) * 2 * image_cases.RAY_ABS * (1 + 1 / image_cases.GRAZING)
