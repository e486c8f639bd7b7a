"""Cases of the environment-parameter tests (Scene.image_loss_fused with ``env_texels_param`` / ``env_rotation_param``):
``image_env_cases``' 36 -- `v5`, `v41` and `wide` under the three laws, with and without the screen, reflection off and on, in front of its
environment (seed 11) and against its targets -- with the restatement's result for each (tests/image_env_param_ref.py), computed once per
process and never modified.

Two conditions on the inputs are asserted for every case (conditions, not measurements): every sample that reads the environment, the
DIRECT ones included, stays TEXEL_MARGIN texels from the integer lines of u and v -- v = 0 and v = Eh - 1, the edges of the clamp, are
among them -- and none lies inside the pole cut.  ``python tests/image_env_param_cases.py`` prints the margins and the counts."""
import functools
import os

import numpy as np

import image_cases
import image_env_cases
import image_env_param_ref
import image_ref

EH, EW = image_env_cases.EH, image_env_cases.EW
POLE = image_env_cases.POLE
TEXEL_MARGIN = image_env_cases.TEXEL_MARGIN
SCENES, LAWS = image_env_cases.SCENES, image_env_cases.LAWS
ENV_SEED = 11
CASES = [(n, l, w, r) for n in SCENES for l in LAWS for w in (True, False) for r in (False, True)]
CASE_IDS = [f"{n}-{l[0]}-{l[1]}-{l[2]}-{'screen' if w else 'no-screen'}-{'reflection' if r else 'no-reflection'}" for n, l, w, r in CASES]


def case_args(name, with_screen):
    sc = image_cases.scene(name)
    env = image_env_cases.environment(sc["texture"].shape[2], ENV_SEED)
    return (sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None,
            sc["texture"] if with_screen else None), env


@functools.lru_cache(maxsize=None)
def samples(name, law, with_screen, reflection):
    """image_env_param_ref.samples of a case at conftest.IOR: shared by its references, left unchanged."""
    sc = image_cases.scene(name)
    args, _ = case_args(name, with_screen)
    return image_env_param_ref.samples(*args, sc["s"], law, image_cases.IOR, image_cases.EXT, reflection)


def margins(fwd):
    """(the smallest distance of an exit / direct read from an integer line of u or v, that of a reflection's read, the smallest 1 - |e_y|
    of any read, the reads inside the clamp of v, the exit and direct reads, all reads)."""
    def of(u, v, ey, sel):
        u, v, ey = u.numpy()[sel.numpy()], v.numpy()[sel.numpy()], ey.numpy()[sel.numpy()]
        if len(u) == 0:
            return np.inf, np.inf, 0, 0
        return (min(np.abs(u - np.rint(u)).min(), np.abs(v - np.rint(v)).min()), (1.0 - np.abs(ey)).min(), int(((v < 0) | (v > EH - 1)).sum()), len(u))
    a = of(fwd["u"], fwd["v"], fwd["ey"], fwd["read"])
    b = of(fwd["ru"], fwd["rv"], fwd["rey"], fwd["r_read"]) if "ru" in fwd else (np.inf, np.inf, 0, 0)
    return a[0], b[0], min(a[1], b[1]), a[2] + b[2], a[3], a[3] + b[3]


@functools.lru_cache(maxsize=None)
def reference(name, law, with_screen, reflection, weighted=False, detach=None):
    """image_env_param_ref.loss_and_grads of a case; the two conditions on the inputs are asserted here, and the loss is held to
    ``image_env_cases.loss_reference``'s (the same law, restated twice)."""
    import image_loss_cases
    sc = image_cases.scene(name)
    args, env = case_args(name, with_screen)
    ref = image_env_param_ref.loss_and_grads(*args, env.texels, env.rotation, image_env_cases.loss_target(name, law, with_screen, reflection), sc["s"], law,
                                             sc["invalid"], image_cases.IOR, image_cases.EXT, weight=image_loss_cases.half_weight(name) if weighted else None,
                                             reflect=reflection, detach=detach, sm=samples(name, law, with_screen, reflection))
    exit_margin, refl_margin, pole, _, n_direct, n_reads = margins(ref["fwd"])
    assert exit_margin >= TEXEL_MARGIN and refl_margin >= TEXEL_MARGIN, (name, law, with_screen, reflection, exit_margin, refl_margin)
    assert pole >= POLE, (name, law, with_screen, reflection, pole)
    sm = ref["sm"]
    assert n_direct >= int(((sm["cls"] == image_ref.DIRECT) & ~sm["on"]).sum()) > 0 and (n_reads > n_direct) == reflection      # (every kind of read is there)
    base = image_env_cases.loss_reference(name, law, with_screen, reflection, weighted)
    assert abs(ref["loss"] - base["loss"]) <= 1e-13 * base["loss"]
    return ref


# ---- the rotation fit (calibrate.fit_environment) ------------------------------------------------------------------------
FIT_VIEWS, FIT_H, FIT_W, FIT_S = (5, 29, 53), 32, 32, 2
FIT_LAW = (6, "reflect", "snell")
FIT_EH, FIT_EW = 32, 64
FIT_OFFSET = (0.5, 1.5, 0.0)          # texels: a tilt of 0.5 about the frame's x axis and a yaw of 1.5
FIT_STEPS, FIT_LR = 150, 0.02
FIT_INVALID = 0.75


def smooth_environment():
    """float32 [32, 64, 3]: low-order trigonometric functions of the direction of each texel's centre (degree 1 and 2 in its components)
    -- a random map has a basin of one texel, this one's is the whole sphere."""
    theta = (np.arange(FIT_EH) + 0.5) / FIT_EH * np.pi
    phi = ((np.arange(FIT_EW) + 0.5) / FIT_EW - 0.5) * 2.0 * np.pi
    ex, ey, ez = np.sin(theta)[:, None] * np.sin(phi)[None, :], np.cos(theta)[:, None] * np.ones(FIT_EW)[None, :], -np.sin(theta)[:, None] * np.cos(phi)[None, :]
    return np.ascontiguousarray(np.stack([0.5 + 0.3 * ex + 0.15 * ey * ez, 0.5 + 0.3 * ey + 0.15 * ex * ez, 0.5 + 0.3 * ez + 0.15 * ex * ey], axis=2), dtype=np.float32)


def rotation_angle(Ra, Rb):
    """The angle of the rotation Ra Rb^T, in degrees."""
    c = (np.trace(np.asarray(Ra) @ np.asarray(Rb).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


@functools.lru_cache(maxsize=None)
def fit_case():
    """dict(cams, photos (float32, the restatement's images at the true rotation), true / start (``render.Environment``), sms (the
    restatement's samples per view)): three views of the hand, no screen, reflection on."""
    import torch
    import image_env_ref
    import image_loss_ref  # noqa: F401
    from drt_amd import calibrate, render
    mesh = image_cases.hand()
    texels = smooth_environment()
    true = render.Environment(texels, image_env_ref.rotation())
    start = render.Environment(texels, calibrate.environment_pose(true, torch.tensor(FIT_OFFSET, dtype=torch.float64)).numpy())
    cams = [image_cases.camera(v, FIT_H, FIT_W) for v in FIT_VIEWS]
    sms = [image_env_param_ref.samples(mesh.faces, mesh.vertices, cam, FIT_H, FIT_W, None, None, FIT_S, FIT_LAW, image_cases.IOR, image_cases.EXT, True) for cam in cams]
    E, R = torch.as_tensor(texels).to(torch.float64), torch.as_tensor(true.rotation)
    photos = [np.ascontiguousarray(image_env_param_ref.loss_forward(sm, E, R, FIT_S, FIT_INVALID)["mean"].to(torch.float32).view(FIT_H, FIT_W, 3).numpy()) for sm in sms]
    return dict(cams=cams, photos=photos, true=true, start=start, sms=sms)


def fit_on_the_restatement(steps=FIT_STEPS, lr=FIT_LR):
    """calibrate.fit_environment's loop over the restatement on the CPU: (the fitted rotation, the loss history)."""
    import torch
    import image_loss_ref
    from drt_amd import calibrate
    case = fit_case()
    E = torch.as_tensor(case["start"].texels).to(torch.float64)

    def loss_of(three):
        R = calibrate.environment_pose(case["start"], three)
        return sum(image_loss_ref.loss_of(image_env_param_ref.loss_forward(sm, E, R, FIT_S, FIT_INVALID)["mean"], photo) for sm, photo in zip(case["sms"], case["photos"]))
    three, history = calibrate._adam_from_zero(loss_of, steps, lr, 3)
    return calibrate.environment_pose(case["start"], three).numpy(), history


if __name__ == "__main__":       # the figures DESIGN.md 10.9 quotes: python tests/image_env_param_cases.py
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if "fit" in sys.argv[1:]:
        case = fit_case()
        R, history = fit_on_the_restatement()
        print("fit on the restatement: loss", history[0], "->", min(history), "angle to the true rotation", rotation_angle(case["start"].rotation, case["true"].rotation),
              "->", rotation_angle(R, case["true"].rotation), "degrees")
        sys.exit(0)
    for name, law, with_screen, reflection in CASES:
        r = reference(name, law, with_screen, reflection)
        m = margins(r["fwd"])
        sm = r["sm"]
        print(name, law, "screen" if with_screen else "no screen", "reflection" if reflection else "no reflection", "exit/direct margin", m[0], "reflected margin", m[1],
              "min 1 - |e_y|", m[2], "reads inside the v clamp", m[3], "direct reads", int(((sm["cls"] == image_ref.DIRECT) & ~sm["on"]).sum()), "reads", m[5],
              "loss", r["loss"], "max |g_env|", np.abs(r["g_env"]).max(), "max |g_R|", np.abs(r["g_R"]).max())
