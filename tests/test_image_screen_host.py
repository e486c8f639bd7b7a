"""CPU: the adjoint of the photometric image loss w.r.t. the screen's pose and the texture (drt_amd/csrc/drt_image_screen.h), compiled for
the host by g++ with -ffp-contract=off (tests/hostsim/image_screen.cpp), against torch autograd of the restatement
tests/image_screen_ref.py and against central differences of the host loss itself; and what of the Python layer needs no GPU: the new
argument checks of ``Scene.image_loss_fused`` and the pose chain of ``calibrate.fit_screen``.

Tolerances are those of tests/test_image_loss_host.py: the loss LOSS_REL, the gradients ``image_loss_cases.close`` (1e-9 of the largest
entry of the reference, 1e-5 absolute) for the nine screen partials and for the texture gradient, central differences 1e-5 relative."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_loss_cases as cases
import image_screen_ref as ref_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _D, _I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
LAWS = ref_mod.LAWS


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_screen.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_screen.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_screen.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h",
                                                    "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.is_view.restype = _D
    lib.is_view.argtypes = [_I, _I, _I, _P, _P, _I, _I, _I] + [_P] * 11
    return lib


@pytest.fixture(scope="module")
def hs():
    return load_hs()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


class HostView:
    """One case on the host build with the restatement's constants (classes, rays, throughputs) handed in.  ``name``: a scene of
    image_cases, or a scene dict of tests/image_fuzz_cases.py with its own IORs, fills, target and weight."""

    def __init__(self, hs, name, law, fresnel):
        own = isinstance(name, dict)
        self.hs, self.sc = hs, image_cases._scene(name)
        sc = self.sc
        const = ref_mod.trace(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["s"], law, fresnel, sc["ior_int"],
                              sc["ior_ext"]) if own else ref_mod.constants(name, law, fresnel)
        self.cls = np.ascontiguousarray(const["cls"].numpy(), np.int32)
        self.o, self.d, self.T = (np.ascontiguousarray(const[k].numpy(), np.float64) for k in ("o", "d", "T"))
        self.P = np.ascontiguousarray((ref_mod.rows_of(sc["screen"]) if own else ref_mod.pose(name)).numpy())
        tex = np.asarray(sc["texture"], np.float32)
        self.tex = np.ascontiguousarray(tex[:, :, None] if tex.ndim == 2 else tex)
        self.target = np.ascontiguousarray(sc["target"]) if own else cases.target(name, law, fresnel)
        self.weight = sc["weight"] if own else None
        C = self.tex.shape[2]
        self.void, self.invalid = (np.ascontiguousarray(np.broadcast_to(np.asarray(sc[k], np.float64), (C,))) for k in ("void", "invalid"))

    def run(self, P=None, tex=None):
        sc = self.sc
        P = self.P if P is None else np.ascontiguousarray(P, np.float64)
        tex = self.tex if tex is None else np.ascontiguousarray(tex, np.float32)
        g_screen, g_tex, count = np.zeros(9), np.zeros(tex.shape, np.float64), np.zeros(1, np.int64)
        loss = self.hs.is_view(sc["height"], sc["width"], sc["s"], _p(P.reshape(-1)), _p(tex), tex.shape[0], tex.shape[1], tex.shape[2], _p(self.cls), _p(self.o),
                               _p(self.d), _p(self.T), _p(self.void), _p(self.invalid), _p(self.target), _p(self.weight), _p(g_screen), _p(g_tex), _p(count))
        return dict(loss=loss, g_screen=g_screen.reshape(3, 3), g_texture=g_tex, count=int(count[0]))


_views = {}


def host_case(hs, name, law, fresnel):
    key = (name, law, fresnel)
    if key not in _views:
        hv = HostView(hs, name, law, fresnel)
        _views[key] = (hv, hv.run())
    return _views[key]


# ---- the view ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_screen_and_texture_gradients_match_the_restatement(hs, name, law, fresnel):
    """Also the texel-line condition, on the restatement: every gradient-carrying sample, the direct ones included, lies at least
    TEXEL_MARGIN from any texel line and any screen border (measured: at least 8.9e-5 texels over the twelve cases), and the direct samples
    are the larger part of them."""
    ref = ref_mod.reference(name, law, fresnel)
    _, got = host_case(hs, name, law, fresnel)
    assert ref["margin"] >= cases.TEXEL_MARGIN
    through_on = cases.reference(name, law, fresnel)["count"]
    assert got["count"] == ref["on"] > 2 * through_on > 0
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    print(f"{name} {law} fresnel={fresnel}: margin {ref['margin']:.2e} texels; loss {got['loss']:.12e} restatement {ref['loss']:.12e} ({rel:.1e}); "
          f"max |g_screen| {np.abs(ref['g_screen']).max():.3e} differs by {np.abs(got['g_screen'] - ref['g_screen']).max():.2e}; "
          f"max |g_texture| {np.abs(ref['g_texture']).max():.3e} differs by {np.abs(got['g_texture'] - ref['g_texture']).max():.2e}")
    assert ref["loss"] > 0 and rel <= cases.LOSS_REL
    assert abs(ref["loss"] - cases.reference(name, law, fresnel)["loss"]) <= cases.LOSS_REL * ref["loss"]      # the loss image_loss_ref states
    assert cases.close(got["g_screen"], ref["g_screen"]) and np.abs(ref["g_screen"]).min() > 0
    assert cases.close(got["g_texture"], ref["g_texture"]) and np.abs(ref["g_texture"]).max() > 0
    assert ((got["g_texture"] == 0) == (ref["g_texture"] == 0)).all()          # a texel nothing lands on has gradient exactly 0


@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_leaving_the_direct_samples_out_is_caught(hs, name, law, fresnel):
    """The negative control: the restatement with the direct samples' colours detached -- what a pass over the through list alone computes
    -- is outside the tolerance of the host build on every case, in the screen partials and in the texture gradient."""
    bad = ref_mod.reference(name, law, fresnel, detach_direct=True)
    _, got = host_case(hs, name, law, fresnel)
    assert bad["loss"] == ref_mod.reference(name, law, fresnel)["loss"]
    assert not cases.close(got["g_screen"], bad["g_screen"]) and not cases.close(got["g_texture"], bad["g_texture"])


@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_central_differences_of_the_host_loss(hs, name):
    """Independent of the restatement: (2, drop, reference), Fresnel on.  Central differences of the host loss with h = 1e-6 texels along a
    fixed random direction in the nine screen numbers (p0 in units of the pitch, the axes in units of pitch / 64; eu and ev move
    independently, the host build checks no orthogonality), and on the three texels with the largest gradient with a step of 2^-7 (the
    loss is quadratic in a texel; the difference is divided by the step the float32 texels actually made).  Measured relative
    differences: screen 1.5e-9 (v5) and 1.6e-9 (wide); texels at most 2.7e-13 (v5) and 2.2e-13 (wide).  Asserted: 1e-5, the bound
    of the same check in tests/test_image_loss_host.py."""
    hv, got = host_case(hs, name, LAWS[0], True)
    pitch = float(np.linalg.norm(hv.P[1]))
    D = np.random.default_rng(13).standard_normal((3, 3)) * np.array([[pitch], [pitch / 64], [pitch / 64]])
    h = 1e-6
    fd = (hv.run(P=hv.P + h * D)["loss"] - hv.run(P=hv.P - h * D)["loss"]) / (2 * h)
    an = float((got["g_screen"] * D).sum())
    print(f"{name}: along the screen direction {an:.10e} against {fd:.10e} ({abs(an - fd) / abs(fd):.1e})")
    assert abs(an - fd) <= 1e-5 * abs(fd)
    flat = np.argsort(np.abs(got["g_texture"]).reshape(-1))[-3:]
    for idx in flat:
        at = np.unravel_index(idx, hv.tex.shape)
        up, down = hv.tex.copy(), hv.tex.copy()
        up[at] += np.float32(2.0 ** -7)
        down[at] -= np.float32(2.0 ** -7)
        fd = (hv.run(tex=up)["loss"] - hv.run(tex=down)["loss"]) / (float(up[at]) - float(down[at]))
        # (the midpoint of the two float32 texels is the texel to 2^-25, and the loss is quadratic in it)
        an = float(got["g_texture"][at])
        print(f"{name}: texel {at} {an:.10e} against {fd:.10e} ({abs(an - fd) / abs(fd):.1e})")
        assert an != 0 and abs(an - fd) <= 1e-5 * abs(fd)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build, diffrender
    sig = _lib.SIGNATURES
    assert "drt_render_image_loss_screen" in sig and len(sig["drt_render_image_loss_screen"][1]) == 30 and len(sig["drt_render_image_loss"][1]) == 28
    assert sig["drt_render_image_loss_screen"][1][:27] == sig["drt_render_image_loss"][1][:27]          # the same arguments up to d_count
    assert "drt_image_screen.hip" in build.UNITS and "drt_image_loss.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss_screen(" in header and "int drt_render_image_loss(" in header
    api = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_api.hip")).read()
    version = re.search(r"int drt_version\(void\) \{ return (\d+); \}", api)
    assert version and int(version.group(1)) >= 11
    wave = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_wave.h")).read()
    assert "int launch_image_screen_bwd(" in wave
    assert callable(diffrender.Scene.image_loss_fused)


def _args():
    from drt_amd import render
    cam = image_cases.camera(5, 8, 8)
    return dict(camera_M=cam, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32),
                target=np.zeros((8, 8, 3), np.float32))


_EYE = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
_TEX = torch.zeros((4, 4, 3), dtype=torch.float32)


@pytest.mark.parametrize("kw,match", [
    (dict(screen_param=_EYE), "screen_param"),                                             # both forms given
    (dict(texture_param=_TEX), "texture_param"),
    (dict(screen=None), "screen"),                                                         # neither form given
    (dict(texture=None), "texture"),
    (dict(screen=None, screen_param=_EYE.numpy()), "screen_param"),                        # not a tensor
    (dict(screen=None, screen_param=_EYE.reshape(9)), "screen_param"),                     # wrong shape
    (dict(screen=None, screen_param=_EYE.to(torch.float32)), "screen_param"),              # wrong dtype
    (dict(screen=None, screen_param=_EYE * float("nan")), "screen_param"),                 # non-finite
    (dict(screen=None, screen_param=torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=torch.float64)), "screen_param"),      # a zero axis
    (dict(screen=None, screen_param=torch.tensor([[0.0, 0, 0], [1, 0, 0], [1e-9, 1, 0]], dtype=torch.float64)), "screen_param"),   # not orthogonal
    (dict(texture=None, texture_param=_TEX.numpy()), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4, 4, 2))), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4, 1, 3))), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4,))), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4, 4, 3), dtype=torch.float16)), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4, 4, 3), dtype=torch.int32)), "texture_param"),
    (dict(texture=None, texture_param=torch.full((4, 4, 3), float("inf"))), "texture_param"),
    (dict(texture=None, texture_param=torch.zeros((4, 4))), "target"),                      # one channel against a three-channel target
])
def test_image_loss_fused_names_the_bad_new_argument(kw, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    args = dict(_args(), **kw)
    pos = [args.pop(k) for k in ("camera_M", "height", "width", "screen", "texture", "target")]
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_fused(object(), *pos, **args)


def test_the_parameter_forms_are_accepted():
    from drt_amd import render
    a = _args()
    got = render.check_image_loss_args(a["camera_M"], 8, 8, None, None, a["target"], screen_param=_EYE.clone().requires_grad_(True),
                                       texture_param=torch.rand((4, 4, 3), dtype=torch.float64, requires_grad=True))
    assert np.array_equal(got["screen"], _EYE.numpy().reshape(-1)) and got["channels"] == 3
    assert tuple(got["texture"].shape) == (4, 4, 3) and not got["texture"].requires_grad
    one = render.check_image_loss_args(a["camera_M"], 8, 8, a["screen"], None, np.zeros((8, 8), np.float32), texture_param=torch.rand((5, 4)))
    assert one["channels"] == 1 and tuple(one["texture"].shape) == (5, 4, 1) and tuple(one["target"].shape) == (8, 8, 1)


# ---- calibrate.fit_screen's pose chain ---------------------------------------------------------------------------------------------------
def _a_screen():
    from drt_amd import render
    center, extent = image_cases.frame()
    return render.Screen.behind(image_cases.camera(5, 32, 32), center, extent, 48, 64)


def test_the_pose_chain_against_finite_differences():
    """screen_pose is torch from the six numbers to the nine: its Jacobian against central differences (torch.autograd.gradcheck, float64,
    its default tolerances) at zero -- where a rotation vector's closed form would divide by its length -- and at a general point; one
    unit of any of the six moves a corner by about a texel; the pose at zero is the screen itself."""
    from drt_amd import calibrate
    sc = _a_screen()
    for six in (torch.zeros(6, dtype=torch.float64), torch.tensor([0.3, -0.2, 0.1, 0.4, 0.5, -0.6], dtype=torch.float64)):
        six = six.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: calibrate.screen_pose(sc, 64, 48, x), (six,))
    at_zero = calibrate.screen_pose(sc, 64, 48, torch.zeros(6, dtype=torch.float64)).numpy()
    assert np.abs(at_zero - np.stack([sc.p0, sc.eu, sc.ev])).max() <= 1e-12 * np.abs(sc.p0).max()
    pitch = np.linalg.norm(sc.eu)
    for k in range(6):
        rows = calibrate.screen_pose(sc, 64, 48, torch.eye(6, dtype=torch.float64)[k]).numpy()
        moved = max(np.linalg.norm((rows[0] + a * 47 * rows[1] + b * 63 * rows[2]) - (sc.p0 + a * 47 * sc.eu + b * 63 * sc.ev)) for a in (0, 1) for b in (0, 1))
        assert 0.3 * pitch <= moved <= 1.5 * pitch, (k, moved / pitch)


def test_a_fitted_pose_keeps_the_pitch_and_passes_the_screens_check():
    """fit_pose on a loss that pulls the pose towards a rigidly moved copy: the rows it ends at build a Screen (orthogonal to 1e-12), with
    the pitch of the start, and the loss falls."""
    from drt_amd import calibrate, render
    sc = _a_screen()
    goal = calibrate.screen_pose(sc, 64, 48, torch.tensor([0.8, -0.5, 0.3, 0.6, -0.4, 0.9], dtype=torch.float64))
    scale = float(np.linalg.norm(sc.eu))
    six, history = calibrate.fit_pose(lambda rows: (((rows - goal) / scale) ** 2).sum(), sc, 64, 48, 60, 0.05)
    rows = calibrate.screen_pose(sc, 64, 48, six).numpy()
    fitted = render.Screen(rows[0], rows[1], rows[2])
    assert len(history) == 60 and min(history) < 0.05 * history[0]
    for a, b in ((fitted.eu, sc.eu), (fitted.ev, sc.ev)):
        assert abs(np.linalg.norm(a) - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    assert abs(fitted.eu @ fitted.ev) <= 1e-12 * np.linalg.norm(fitted.eu) * np.linalg.norm(fitted.ev)
    with pytest.raises(ValueError, match="steps"):
        calibrate.fit_pose(lambda rows: rows.sum(), sc, 64, 48, 0, 0.05)
    with pytest.raises(ValueError, match="views"):
        calibrate.fit_screen(object(), [], sc, np.zeros((64, 48, 3), np.float32), steps=1, lr=0.1)
