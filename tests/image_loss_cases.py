"""Cases of the image-loss tests (Scene.image_loss_fused): the scenes and laws of tests/image_cases.py with a target rendered by the
restatement (tests/image_loss_ref.py) at IOR 1.55 and the loss evaluated at ``conftest.IOR``; the restatement's loss and gradients of
every case, computed once per process and never modified."""
import functools

import numpy as np

import image_cases
import image_loss_ref
import image_ref
from conftest import IOR

EXT = image_cases.EXT
TARGET_IOR = 1.55
LAWS = image_cases.LAWS
SCENES = ("v5", "v41", "wide")
# through samples on the screen at conftest.IOR: (scene, law) -> count (the same with the Fresnel term on and off)
COUNTS = {("v5", LAWS[0]): 896, ("v5", LAWS[1]): 1120, ("v5", LAWS[2]): 963, ("wide", LAWS[0]): 1209, ("wide", LAWS[1]): 1227, ("wide", LAWS[2]): 1126}
TEXEL_MARGIN = 1e-6          # texels: every through sample is at least this far from any texel line or screen border
# loss: the host build's relative difference from the restatement, the largest of the 18 cases as measured (tests/test_image_loss_host.py
# prints each); asserted with a factor of ten for another summation order, and never more than 1e-10
MEASURED_LOSS_REL = 3e-15
LOSS_REL = 10 * MEASURED_LOSS_REL
assert LOSS_REL <= 1e-10
GRAD_REL, GRAD_ABS = 1e-9, 1e-5      # the project's gradient tolerance: of the largest entry, and absolute


def _render_args(sc, law, fresnel):
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"])


@functools.lru_cache(maxsize=None)
def target(name, law, fresnel):
    """float32 [H, W, C]: the restatement's image of the scene at TARGET_IOR."""
    sc = image_cases.scene(name)
    fwd = image_loss_ref.forward(*_render_args(sc, law, fresnel), sc["s"], law, fresnel, sc["void"], sc["invalid"], TARGET_IOR, EXT)
    return np.ascontiguousarray(fwd["mean"].detach().to(image_ref.torch.float32).view(sc["height"], sc["width"], -1).numpy())


def half_weight(name):
    """float32 [H, W]: zero on the left half of the image, a ramp of non-trivial weights on the right."""
    sc = image_cases.scene(name)
    w = np.tile(np.linspace(0.5, 1.5, sc["width"], dtype=np.float32), (sc["height"], 1))
    w[:, : sc["width"] // 2] = 0.0
    return np.ascontiguousarray(w)


@functools.lru_cache(maxsize=None)
def reference(name, law, fresnel, weighted=False, throughput_gradient=True):
    """image_loss_ref.loss_and_grads of a case at conftest.IOR; checked against image_ref.render (its T within 1e-15, its image within
    2^-23) and for the distance of every through sample from the texel lines."""
    sc = image_cases.scene(name)
    ref = image_loss_ref.loss_and_grads(*_render_args(sc, law, fresnel), target(name, law, fresnel), sc["s"], law, fresnel, sc["void"], sc["invalid"],
                                        IOR, EXT, weight=half_weight(name) if weighted else None, throughput_gradient=throughput_gradient)
    base = image_cases.reference(name, law, fresnel)
    fwd = ref["fwd"]
    assert np.array_equal(fwd["cls"].numpy(), base["cls"].numpy()) and np.array_equal(fwd["on"].numpy(), base["on"].numpy())
    assert float((fwd["T"].detach() - base["T"]).abs().max()) <= 1e-15
    assert np.abs(ref["image"].astype(np.float64) - base["image"].numpy().astype(np.float64)).max() <= 2.0 ** -23
    sel = (fwd["on"] & (fwd["cls"] == image_ref.THROUGH)).numpy()
    tex_h, tex_w = sc["texture"].shape[:2]
    for w, top in ((fwd["u"].detach().numpy()[sel], tex_w - 1), (fwd["v"].detach().numpy()[sel], tex_h - 1)):
        assert np.abs(w - np.rint(w)).min() >= TEXEL_MARGIN and w.min() >= TEXEL_MARGIN and (top - w).min() >= TEXEL_MARGIN
    return ref


def close(got, want):
    """The project's gradient tolerance: GRAD_REL of the largest entry of the reference and GRAD_ABS absolute."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.isfinite(got).all() and np.abs(got - want).max() <= min(GRAD_ABS, GRAD_REL * np.abs(want).max()) if np.abs(want).max() > 0
                else not got.any())
