"""CPU: the gradients of the photometric image loss w.r.t. the environment's texels and rotation (drt_amd/csrc/drt_image_env_param.h),
compiled for the host by g++ with -ffp-contract=off (tests/hostsim/image_env_param.cpp), against torch autograd of the restatement
tests/image_env_param_ref.py and against central differences of the host loss itself; and what of the Python layer needs no GPU: the new
argument checks of ``Scene.image_loss_fused``, ``calibrate.environment_pose`` and the declarations.

Tolerances: the gradients ``image_loss_cases.close`` (1e-9 of the largest entry of the reference, 1e-5 absolute) for the texel gradient
and for the nine rotation partials; central differences 1e-5 relative, the bound of the same check in tests/test_image_screen_host.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_param_cases as cases
import image_loss_cases
import image_ref
from drt_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
EH, EW = cases.EH, cases.EW
LAWS = image_cases.LAWS


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_env_param.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_env_param.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_env_param.h", "drt_image_env.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h",
                                                    "drt_shade.h", "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.env_param_view.restype = _D
    lib.env_param_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I, _I] + [_P] * 12
    return lib


@pytest.fixture(scope="module")
def hs():
    return load_hs()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def host_view_of(hs, sc, law, with_screen, reflection, sm, texels, rot, target, weight, ior_int, ior_ext, grads=True):
    """The header's loss, texel gradient [Eh, Ew, C], rotation partials [3, 3] and read statistics of a scene dict (one of image_cases, or
    one of tests/image_fuzz_cases.py with its own texture and environment extents) on ``sm``, image_env_param_ref.samples' dict."""
    mesh = sc["mesh"]
    faces, verts = np.ascontiguousarray(mesh.faces, dtype=np.int32), np.ascontiguousarray(mesh.vertices, dtype=np.float64)
    cam = np.ascontiguousarray(np.concatenate([np.asarray(sc["camera_M"][3]).reshape(-1), np.asarray(sc["camera_M"][2])[:3, :].reshape(-1)]))
    tex = np.asarray(sc["texture"], np.float32)
    tex = np.ascontiguousarray(tex[:, :, None] if tex.ndim == 2 else tex)
    C = tex.shape[2]
    texels, rot = np.ascontiguousarray(texels, dtype=np.float32), np.ascontiguousarray(rot, dtype=np.float64)
    eh, ew = texels.shape[:2]
    g_env, g_R, stats = (np.zeros((eh, ew, C)), np.zeros((3, 3)), np.zeros(5)) if grads else (None, None, None)
    seen = sm["refl"]["seen"] if reflection else torch.zeros(len(sm["cls"]), dtype=torch.bool)
    invalid = np.ascontiguousarray(np.broadcast_to(np.asarray(sc["invalid"], np.float64), (C,)))
    loss = hs.env_param_view(_p(cam), sc["height"], sc["width"], sc["s"], _p(sc["screen"].packed()) if with_screen else None, _p(tex) if with_screen else None,
                             tex.shape[0], tex.shape[1], C, _p(texels), eh, ew, _p(rot), _p(faces), _p(verts), len(faces), ior_int, ior_ext,
                             int(law[2] == "snell"), int(reflection), _p(np.ascontiguousarray(sm["cls"].numpy(), dtype=np.int32)),
                             _p(np.ascontiguousarray(sm["out_o"].numpy())), _p(np.ascontiguousarray(sm["out_d"].numpy())), _p(np.ascontiguousarray(sm["T"].numpy())),
                             _p(np.ascontiguousarray(sm["tape"][0].numpy(), dtype=np.int32)), _p(np.ascontiguousarray(seen.numpy(), dtype=np.uint8)),
                             _p(invalid), _p(np.ascontiguousarray(target)), _p(weight),
                             _p(g_env), _p(g_R), _p(stats))
    return dict(loss=loss, g_env=g_env, g_R=g_R, stats=stats)


def host_view(hs, name, law, with_screen, reflection, weighted=False, env=None, R=None, grads=True):
    """The header's loss, texel gradient [Eh, Ew, C], rotation partials [3, 3] and read statistics of a case, on the restatement's classes,
    exit rays, throughputs and occlusion verdicts; ``env`` / ``R``: other texels (float32) / another matrix (any nine numbers)."""
    sc = image_cases.scene(name)
    sm = cases.samples(name, law, with_screen, reflection)
    _, e = cases.case_args(name, with_screen)
    weight = image_loss_cases.half_weight(name) if weighted else None
    return host_view_of(hs, sc, law, with_screen, reflection, sm, e.texels if env is None else env, e.rotation if R is None else R,
                        image_env_cases.loss_target(name, law, with_screen, reflection), weight, image_cases.IOR, image_cases.EXT, grads)


# `v5` and `v41` have three channels, `wide` one
GRAD_CASES = [("wide", LAWS[1], True, True), ("wide", LAWS[2], False, True), ("v5", LAWS[2], True, True), ("v5", LAWS[0], False, False), ("v5", LAWS[1], False, True),
              ("v41", LAWS[0], True, False), ("v41", LAWS[2], False, True), ("wide", LAWS[0], True, False)]
IDS = [f"{n}-{l[0]}-{l[1]}-{l[2]}-{'screen' if w else 'no-screen'}-{'reflection' if r else 'no-reflection'}" for n, l, w, r in GRAD_CASES]


@pytest.mark.parametrize("name,law,with_screen,reflection", GRAD_CASES, ids=IDS)
def test_texel_gradient_and_rotation_partials_against_autograd(hs, name, law, with_screen, reflection):
    """Loss within LOSS_REL; texel gradient and the nine rotation partials within ``close``; texels nothing reads are exactly 0; and the sum
    of the texel gradient per channel equals sum_reads w g_c[ch], because the four bilinear weights of a read sum to 1: each read adds four
    products (one rounding each, relative 2^-53) of weights whose sum is 1 to within 3 roundings, and the two sums of up to N terms each
    round N times more, so the difference is bounded by (7 + 2 N) 2^-53 sum_reads |w g_c| -- N is the number of reads (706 to 4 700
    here).  Measured: 2e-16 to 3e-14 absolute, at most 1e-3 of that bound; the gradients differ from autograd's by 1e-15 to 4e-14."""
    got, ref = host_view(hs, name, law, with_screen, reflection), cases.reference(name, law, with_screen, reflection)
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    n_reads = int(got["stats"][4])
    bound = (7 + 2 * n_reads) * 2.0 ** -53 * got["stats"][3]
    C = got["g_env"].shape[2]
    dsum = np.abs(got["g_env"].reshape(-1, C).sum(0) - got["stats"][:C]).max()
    print(name, law, with_screen, reflection, "loss rel", rel, "reads", n_reads, "max |d g_env|", np.abs(got["g_env"] - ref["g_env"]).max(), "of", np.abs(ref["g_env"]).max(),
          "max |d g_R|", np.abs(got["g_R"] - ref["g_R"]).max(), "of", np.abs(ref["g_R"]).max(), "sum difference", dsum, "bound", bound)
    assert ref["loss"] > 0.5 and rel <= image_loss_cases.LOSS_REL
    assert image_loss_cases.close(got["g_env"], ref["g_env"]) and np.abs(ref["g_env"]).max() > 1e-3
    assert image_loss_cases.close(got["g_R"], ref["g_R"]) and np.abs(ref["g_R"]).max() > 1e-2
    assert not got["g_env"][ref["g_env"] == 0].any()
    m = cases.margins(ref["fwd"])
    assert n_reads == m[5] and dsum <= bound


def test_the_cases_have_unread_texels_reads_inside_the_clamp_and_seam_reads(hs):
    """What the checks above rely on is there: a screen leaves texels of the environment unread; the (6, reflect, snell) cases of `v41` and
    `wide` have reads with v outside [0, Eh - 1] (g_v = 0); reads across the seam (columns Ew - 1 and 0) exist."""
    ref = cases.reference("v5", LAWS[2], True, True)
    assert (ref["g_env"] == 0).all(2).sum() > 10
    for name in ("v41", "wide"):
        assert cases.margins(cases.reference(name, LAWS[2], False, True)["fwd"])[3] >= 2
    fwd = cases.reference("wide", LAWS[1], False, True)["fwd"]
    u = fwd["u"].numpy()[fwd["read"].numpy()]
    assert ((u < 0) | (u > EW - 1)).any()


@pytest.mark.parametrize("name,law,with_screen", [("wide", LAWS[1], False), ("v5", LAWS[2], True)], ids=["wide", "v5"])
def test_central_differences_of_the_host_loss(hs, name, law, with_screen):
    """Independent of the restatement, reflection on.  Rotation: central differences of the host loss with h = 1e-7 along a fixed random
    direction D (entries in [-1, 1]) of the NINE numbers -- R + h D is no rotation and is not made one; the law is called directly, the
    host build checks no orthonormality.  A step of 1e-7 moves u, v by at most Ew / (2 pi) * 3e-7 / sin(theta_min) < 4e-5 texels off the
    pole cut only in the worst case and by about 1e-6 typically; a sample that crossed a texel line would show as a difference of 1e-3 and
    more.  Texels: the three with the largest gradient among (column 0 or Ew - 1 with a read across the seam, anywhere, anywhere), with a
    step of 2^-7: the loss is quadratic in a texel, and the difference is divided by the step the float32 texels actually made.
    Measured relative differences: rotation 2.3e-10 (wide) and 1.6e-8 (v5); texels at most 3.0e-12.  Asserted: 1e-5."""
    got = host_view(hs, name, law, with_screen, True)
    _, e = cases.case_args(name, with_screen)
    D = np.random.default_rng(7).uniform(-1, 1, (3, 3))
    h = 1e-7
    fd = (host_view(hs, name, law, with_screen, True, R=e.rotation + h * D, grads=False)["loss"] -
          host_view(hs, name, law, with_screen, True, R=e.rotation - h * D, grads=False)["loss"]) / (2 * h)
    an = float((got["g_R"] * D).sum())
    print(f"{name}: along the rotation direction {an:.10e} against {fd:.10e} ({abs(an - fd) / abs(fd):.1e})")
    assert abs(an - fd) <= 1e-5 * abs(fd)
    # a texel of column 0 or Ew - 1 that a read across the seam touches: a row in which BOTH seam columns received a gradient from reads with u outside [0, Ew - 1]
    fwd = cases.reference(name, law, with_screen, True)["fwd"]
    sel = fwd["read"].numpy()
    u, v = fwd["u"].numpy()[sel], fwd["v"].numpy()[sel]
    across = (u < 0) | (u > EW - 1)
    assert across.any()
    row = int(np.floor(np.clip(v[across], 0, EH - 1)).min(initial=EH - 2))
    seam = max(((row, 0), (row, EW - 1)), key=lambda at: np.abs(got["g_env"][at]).max())
    g = np.abs(got["g_env"]).max(2)
    rest = [tuple(np.unravel_index(i, g.shape)) for i in np.argsort(g.reshape(-1))[-2:]]
    for at in [seam] + rest:
        ch = int(np.argmax(np.abs(got["g_env"][at])))
        up, dn = e.texels.copy(), e.texels.copy()
        up[at][ch] += np.float32(2.0 ** -7)
        dn[at][ch] -= np.float32(2.0 ** -7)
        step = float(up[at][ch]) - float(dn[at][ch])
        fd = (host_view(hs, name, law, with_screen, True, env=up, grads=False)["loss"] - host_view(hs, name, law, with_screen, True, env=dn, grads=False)["loss"]) / step
        an = float(got["g_env"][at][ch])
        print(f"{name}: texel {at} channel {ch} {an:.10e} against {fd:.10e} ({abs(an - fd) / abs(fd):.1e})")
        assert an != 0 and abs(an - fd) <= 1e-5 * abs(fd)


@pytest.mark.parametrize("detach", ["direct", "reflection"])
def test_a_restatement_with_reads_detached_is_another_gradient(hs, detach):
    """Negative controls: with the direct samples' reads, or the reflection's, cut out of autograd's graph the restatement's gradients fall
    outside ``close`` of the header's -- the header differentiates both."""
    name, law = "wide", LAWS[1]
    got = host_view(hs, name, law, True, True)
    ref, cut = cases.reference(name, law, True, True), cases.reference(name, law, True, True, detach=detach)
    assert cut["loss"] == ref["loss"]
    assert image_loss_cases.close(got["g_env"], ref["g_env"]) and not image_loss_cases.close(got["g_env"], cut["g_env"])
    assert image_loss_cases.close(got["g_R"], ref["g_R"]) and not image_loss_cases.close(got["g_R"], cut["g_R"])


def test_a_transposed_rotation_is_another_gradient(hs):
    """Negative control: g_R[r][c] = g_e[r] d[c], not g_e[c] d[r], and the map is looked up under R, not R^T."""
    name, law = "wide", LAWS[1]
    got, ref = host_view(hs, name, law, True, True), cases.reference(name, law, True, True)
    assert not image_loss_cases.close(got["g_R"].T, ref["g_R"])
    _, e = cases.case_args(name, True)
    wrong = host_view(hs, name, law, True, True, R=e.rotation.T)
    assert not image_loss_cases.close(wrong["g_R"], ref["g_R"]) and not image_loss_cases.close(wrong["g_env"], ref["g_env"])


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def _args():
    cam = image_cases.camera(5, 8, 8)
    return dict(camera_M=cam, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32),
                target=np.zeros((8, 8, 3), np.float32), environment=render.Environment(np.zeros((4, 8, 3), np.float32)))


_T3 = lambda *shape, **kw: torch.zeros(shape, **kw)      # noqa: E731
_EYE = torch.eye(3, dtype=torch.float64)
_MONO = dict(environment=render.Environment(np.zeros((4, 8), np.float32)), screen=None, texture=None, target=np.zeros((8, 8), np.float32))


@pytest.mark.parametrize("change,match", [
    (dict(environment=None, env_texels_param=_T3(4, 8, 3)), "env_texels_param needs an environment"),
    (dict(environment=None, env_rotation_param=_EYE), "env_rotation_param needs an environment"),
    (dict(environment=np.zeros((4, 8, 3), np.float32), env_rotation_param=_EYE), "needs an environment"),
    (dict(env_texels_param=np.zeros((4, 8, 3), np.float32)), "env_texels_param must be a float32 or float64 tensor"),
    (dict(env_texels_param=_T3(4, 8, 3, dtype=torch.float16)), "env_texels_param must be float32 or float64"),
    (dict(env_texels_param=_T3(4, 8, 3, dtype=torch.int32)), "env_texels_param must be float32 or float64"),
    (dict(env_texels_param=_T3(4, 8)), "env_texels_param must have the shape"),
    (dict(env_texels_param=_T3(8, 4, 3)), "env_texels_param must have the shape"),
    (dict(env_texels_param=_T3(4, 8, 1)), "env_texels_param must have the shape"),
    (dict(env_texels_param=torch.full((4, 8, 3), float("nan"))), "env_texels_param must be finite"),
    (dict(env_rotation_param=np.eye(3)), "env_rotation_param must be a float64 tensor"),
    (dict(env_rotation_param=torch.eye(3)), "env_rotation_param must be float64"),
    (dict(env_rotation_param=torch.eye(4, dtype=torch.float64)), r"env_rotation_param must have shape \(3, 3\)"),
    (dict(env_rotation_param=_EYE * 1.001), "env_rotation_param: .*orthonormal"),
    (dict(env_rotation_param=torch.full((3, 3), float("nan"), dtype=torch.float64)), "env_rotation_param: .*rotation"),
    (dict(_MONO, env_texels_param=_T3(4, 8, 3)), "env_texels_param must have the shape"),
    (dict(_MONO, screen=_args()["screen"], texture=_args()["texture"], env_texels_param=_T3(4, 8)), "channels"),
    (dict(env_texels_param=_T3(4, 8, 3), absorption=0.1), "absorption"),
    (dict(env_rotation_param=_EYE, screen_param=_EYE, screen=None), "screen_param"),
    (dict(env_texels_param=_T3(4, 8, 3), texture_param=_T3(4, 4, 3), texture=None), "texture_param"),
    (dict(env_rotation_param=_EYE, camera_param=(torch.eye(4, dtype=torch.float64), _EYE), camera_M=None), "camera_param"),
    (dict(env_rotation_param=_EYE, reflection=True, fresnel=False), "reflection")])
def test_image_loss_fused_names_the_bad_argument(change, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    kw = dict(_args(), **change)
    pos = [kw.pop(k) for k in ("camera_M", "height", "width", "screen", "texture", "target")]
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_fused(object(), *pos, **kw)


def test_check_image_loss_args_puts_the_params_in_the_environments_place():
    a = _args()
    R = torch.as_tensor(render.Environment.yaw(30.0))
    t = torch.rand((4, 8, 3), dtype=torch.float64, requires_grad=True)
    got = render.check_image_loss_args(a["camera_M"], 8, 8, a["screen"], a["texture"], a["target"], environment=a["environment"], env_texels_param=t,
                                       env_rotation_param=R)
    env = got["environment"]
    assert isinstance(env, render.Environment) and env is not a["environment"] and not env.texels.requires_grad and torch.equal(env.texels, t.detach())
    assert np.array_equal(env.rotation, R.numpy()) and env.packed().dtype == np.float64
    mono = render.check_image_loss_args(a["camera_M"], 8, 8, None, None, np.zeros((8, 8), np.float32), environment=_MONO["environment"],
                                        env_texels_param=torch.rand((4, 8)))
    assert tuple(mono["environment"].texels.shape) == (4, 8, 1) and mono["channels"] == 1
    same = render.check_image_loss_args(a["camera_M"], 8, 8, a["screen"], a["texture"], a["target"], environment=a["environment"])
    assert same["environment"] is a["environment"]


def test_the_multi_view_call_has_no_such_keyword():
    import inspect
    from drt_amd import diffrender
    names = inspect.signature(diffrender.Scene.image_loss_views_fused).parameters
    assert "env_texels_param" not in names and "env_rotation_param" not in names
    with pytest.raises(ValueError, match="multi-view"):
        diffrender.Scene.image_loss_views_fused(object(), None, [0], np.zeros((4, 4, 3), np.float32), environment=_args()["environment"])


# ---- the pose of the fit ---------------------------------------------------------------------------------------------------------------
def test_environment_pose():
    """Zero gives R0 (to the bit, or within one unit in the last place of an entry: expm(0) is the identity and the product rounds);
    three = (0, t, 0) is a yaw that moves u of an equator direction by t texels (towards smaller u); the result passes the 1e-12
    orthonormality check over the whole range a fit visits (|three| up to 40 texels here, far beyond it); the chain is differentiable
    (torch.autograd.gradcheck at zero and at a general point)."""
    import image_env_ref
    from drt_amd import calibrate
    R0 = image_env_ref.rotation()
    env = render.Environment(np.zeros((32, 64, 3), np.float32), R0)
    zero = calibrate.environment_pose(env, torch.zeros(3, dtype=torch.float64)).numpy()
    assert np.abs(zero - R0).max() <= np.spacing(1.0)
    flat = render.Environment(np.zeros((32, 64, 3), np.float32))
    d = torch.tensor([[math.sin(0.4), 0.0, -math.cos(0.4)], [math.sin(-2.0), 0.0, -math.cos(-2.0)]], dtype=torch.float64)
    u0, _, _ = image_env_ref.env_uv(np.eye(3), d, 32, 64)
    for t in (0.25, 1.0, -3.5):
        R = calibrate.environment_pose(flat, torch.tensor([0.0, t, 0.0], dtype=torch.float64)).numpy()
        u1, v1, _ = image_env_ref.env_uv(R, d, 32, 64)
        # 1e-9 texels: what is tested is the UNIT of the three numbers, and a fit steps by 1e-2 of it; torch documents no error bound for
        # matrix_exp, whose angle is what reaches u (acos / atan2 add UV_ULPS, 1e-14)
        assert np.abs((u0 - u1).numpy() - t).max() <= 1e-9 and np.abs(v1.numpy() - 15.5).max() <= 1e-9
    rng = np.random.default_rng(5)
    worst = 0.0
    for scale in (1e-9, 1e-3, 0.02, 0.5, 2.0, 10.0, 40.0):
        for _ in range(40):
            R = calibrate.environment_pose(env, torch.as_tensor(rng.uniform(-scale, scale, 3))).numpy()
            worst = max(worst, float(np.abs(R @ R.T - np.eye(3)).max()))
            render.Environment(env.texels, R)
    print("max |R R^T - I| over the range", worst)
    assert worst <= render.ORTHO_TOL
    f = lambda three: calibrate.environment_pose(env, three)      # noqa: E731
    assert torch.autograd.gradcheck(f, (torch.zeros(3, dtype=torch.float64, requires_grad=True),))
    assert torch.autograd.gradcheck(f, (torch.tensor([0.7, -1.5, 0.3], dtype=torch.float64, requires_grad=True),))


def test_fit_environment_refuses_what_it_sets_itself():
    from drt_amd import calibrate
    env = render.Environment(np.zeros((4, 8, 3), np.float32))
    view = [(image_cases.camera(5, 8, 8), np.zeros((8, 8, 3), np.float32))]
    for bad in ("env_rotation_param", "env_texels_param", "vertices", "absorption"):
        with pytest.raises(ValueError, match=bad):
            calibrate.fit_environment(object(), view, env, steps=1, lr=0.1, **{bad: None})
    with pytest.raises(ValueError, match="Environment"):
        calibrate.fit_environment(object(), view, np.zeros((4, 8, 3), np.float32), steps=1, lr=0.1)
    with pytest.raises(ValueError, match="views"):
        calibrate.fit_environment(object(), [], env, steps=1, lr=0.1)


# ---- the declarations --------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    assert len(_lib.SIGNATURES["drt_render_image_loss_env_param"][1]) == len(_lib.SIGNATURES["drt_render_image_loss_env"][1]) + 2
    assert _lib.SIGNATURES["drt_render_image_loss_env_param"][1][:-3] == _lib.SIGNATURES["drt_render_image_loss_env"][1][:-1]
    assert "drt_image_env_param.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss_env_param(" in header and "double* d_grad_env,\n" in header and "double* d_grad_env_rot, void* stream);" in header
    unit = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_env.hip")).read()
    assert "int drt_render_image_loss_env_param(" in unit and unit.count("return env_loss_call(") == 2          # one host body for both
    kernel = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_env_param.hip")).read()
    assert "k_image_env_param_bwd" in kernel and "block_flush<DET, 9>" in kernel and "sink_pass<DET, kImageEnvParamBatch, TEXELS>" in kernel
    source = open(os.path.join(ROOT, "drt_amd", "diffrender.py")).read()
    assert source.count("drt_render_image_loss_env_param") >= 2 and source.count("_lib.lib().drt_render_image_loss_env_param") == 1      # packed in one place
