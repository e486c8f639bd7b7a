"""CPU: the adjoint of the photometric image loss w.r.t. the camera's 21 numbers (drt_amd/csrc/drt_image_camera.h), compiled for the host
by g++ with -ffp-contract=off (tests/hostsim/image_camera.cpp), against torch autograd of the restatement tests/image_camera_ref.py and
against central differences of the host loss itself; and what of the Python layer needs no GPU: the new argument checks of
``Scene.image_loss_fused``, the declarations of the entry point, and ``calibrate.camera_pose``.

Tolerances are those of tests/test_image_loss_host.py: the loss LOSS_REL; the gradients ``image_loss_cases.close`` (1e-9 of the largest
entry of the reference, 1e-5 absolute) for each of the three groups rinv[:, :3], rinv[:, 3] and kinv on its own -- the groups differ by
orders of magnitude, and one tolerance over all 21 would hide the small ones --; central differences 1e-5 relative."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_camera_ref as ref_mod
import image_loss_cases as cases
import image_loss_ref
from conftest import IOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _D, _I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
EXT = cases.EXT
LAWS = ref_mod.LAWS
CONTROLS = ("detach_direct", "detach_origin", "detach_T")


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_camera.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_camera.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_camera.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h",
                                                    "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.ic_view.restype = _D
    lib.ic_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _D, _D, _I, _I] + [_P] * 10
    return lib


@pytest.fixture(scope="module")
def hs():
    return load_hs()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _cam21(camera_M):
    return np.ascontiguousarray(np.concatenate([np.asarray(camera_M[3], np.float64).reshape(-1), np.asarray(camera_M[2], np.float64)[:3, :].reshape(-1)]))


class HostView:
    """One case on the host build with the classes and the tape of the restatement's trace at the fixture's camera held fixed.  ``name``:
    a scene of image_cases, or a scene dict of tests/image_fuzz_cases.py with its own IORs, fills, target and weight."""

    def __init__(self, hs, name, law, fresnel):
        own = isinstance(name, dict)
        self.hs, self.sc, self.law, self.fresnel = hs, image_cases._scene(name), law, fresnel
        sc = self.sc
        self.ior_int, self.ior_ext = (sc["ior_int"], sc["ior_ext"]) if own else (IOR, EXT)
        self.F = np.ascontiguousarray(sc["mesh"].faces, np.int32)
        self.V = np.ascontiguousarray(sc["mesh"].vertices, np.float64)
        o, d = image_loss_ref.image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
        aux = image_loss_ref.snell_ref.trace(sc["mesh"].faces, torch.tensor(self.V), o, d, self.ior_int, self.ior_ext, *law)
        hit, valid = aux["tape"][0] >= 0, aux["valid"]
        self.cls = np.ascontiguousarray(torch.where(hit, torch.where(valid, 1, 2), 0).numpy(), np.int32)
        self.tape = np.ascontiguousarray(aux["tape"].numpy(), np.int32)
        self.hits = np.ascontiguousarray(aux["hits"].numpy(), np.uint8)
        self.cam21 = _cam21(sc["camera_M"])
        self.target = np.ascontiguousarray(sc["target"]) if own else cases.target(name, law, fresnel)
        self.weight = sc["weight"] if own else None
        tex = np.asarray(sc["texture"], np.float32)
        self.tex = np.ascontiguousarray(tex[:, :, None] if tex.ndim == 2 else tex)
        C = self.tex.shape[2]
        self.void, self.invalid = (np.ascontiguousarray(np.broadcast_to(np.asarray(sc[k], np.float64), (C,))) for k in ("void", "invalid"))

    def run(self, cam21=None):
        sc = self.sc
        cam21 = self.cam21 if cam21 is None else np.ascontiguousarray(cam21, np.float64)
        g_cam, count, through = np.zeros(21), np.zeros(1, np.int64), np.zeros(1, np.int64)
        loss = self.hs.ic_view(_p(cam21), sc["height"], sc["width"], sc["s"], _p(sc["screen"].packed()), _p(self.tex), self.tex.shape[0], self.tex.shape[1],
                               self.tex.shape[2], _p(self.F), _p(self.V), self.ior_int, self.ior_ext, int(self.law[2] == "snell"), int(self.fresnel), _p(self.cls),
                               _p(self.tape), _p(self.hits), _p(self.void), _p(self.invalid), _p(self.target), _p(self.weight), _p(g_cam), _p(count), _p(through))
        return dict(loss=loss, g_kinv=g_cam[:9].reshape(3, 3), g_rinv=g_cam[9:].reshape(3, 4), count=int(count[0]), through=int(through[0]))


_views = {}


def host_case(hs, name, law, fresnel):
    key = (name, law, fresnel)
    if key not in _views:
        hv = HostView(hs, name, law, fresnel)
        _views[key] = (hv, hv.run())
    return _views[key]


def _group_report(got, ref):
    want, have = ref_mod.groups(ref["g_rinv"], ref["g_kinv"]), ref_mod.groups(got["g_rinv"], got["g_kinv"])
    return {k: (float(np.abs(want[k]).max()), float(np.abs(have[k] - want[k]).max()), cases.close(have[k], want[k])) for k in want}


# ---- the view ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_camera_gradient_matches_the_restatement(hs, name, law, fresnel):
    """Also the texel-line condition, on the restatement at the fixtures' own camera: every gradient-carrying sample, the direct ones
    included, lies at least TEXEL_MARGIN from any texel line and any screen border (10.4 measured 8.9e-5 texels there), and the direct
    samples are the larger part of them.  Measured over the twelve cases: the smallest margin 8.86e-5 texels; the loss within 3.0e-15
    relative; rinv[:, :3] (largest entries 26.7 .. 226) within 1.4e-12, rinv[:, 3] (0.0765 .. 0.829) within 3.4e-15, kinv (818 .. 3724)
    within 2.4e-11 absolute -- each some 1e-14 of its group's largest entry."""
    ref = ref_mod.reference(name, law, fresnel)
    _, got = host_case(hs, name, law, fresnel)
    assert ref["margin"] >= cases.TEXEL_MARGIN
    through_on = cases.reference(name, law, fresnel)["count"]
    assert got["loss"] >= 0, "the two kernels' on-screen verdicts differ"
    assert got["through"] == ref["through_on"] == through_on
    assert got["count"] == ref["on"] > 2 * through_on > 0
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    report = _group_report(got, ref)
    print(f"{name} {law} fresnel={fresnel}: margin {ref['margin']:.2e} texels; loss {got['loss']:.12e} restatement {ref['loss']:.12e} ({rel:.1e}); "
          + "; ".join(f"max |{k}| {m:.3e} differs by {d:.2e}" for k, (m, d, _) in report.items()))
    assert ref["loss"] > 0 and rel <= cases.LOSS_REL
    assert abs(ref["loss"] - cases.reference(name, law, fresnel)["loss"]) <= cases.LOSS_REL * ref["loss"]      # the loss image_loss_ref states
    for k, (largest, _, ok) in report.items():
        assert largest > 0 and ok, k


@pytest.mark.parametrize("control", CONTROLS)
@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_the_negative_controls_are_caught(hs, name, law, fresnel, control):
    """The restatement with the direct samples detached, with the ray origin detached, or with the throughput detached is outside the
    tolerance of the host build in at least one group: on all twelve cases for the first two, on the six Fresnel-on cases for the
    third (with the Fresnel term off T is the constant 1 and the control is the law itself, which is asserted instead)."""
    bad = ref_mod.reference(name, law, fresnel, control)
    _, got = host_case(hs, name, law, fresnel)
    assert bad["loss"] == ref_mod.reference(name, law, fresnel)["loss"]
    report = _group_report(got, bad)
    print(f"{name} {law} fresnel={fresnel} {control}: " + "; ".join(f"{k} off by {d:.2e} of {m:.2e} ({'inside' if ok else 'outside'})" for k, (m, d, ok) in report.items()))
    if control == "detach_T" and not fresnel:
        assert all(ok for _, _, ok in report.values())
    else:
        assert not all(ok for _, _, ok in report.values()), f"{control} is inside the tolerance on {name} {law} fresnel={fresnel}"


@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_central_differences_of_the_host_loss(hs, name):
    """Independent of the restatement: (2, drop, reference), Fresnel on, classes and tape held (they carry no gradient, and the recompute
    is smooth on fixed faces).  Central differences of the host loss with h = 1e-6 along a fixed random direction of the 21 numbers,
    scaled per group so that each moves the image by about a pixel: rinv[:, :3] by 1 / f (an angle of a pixel), rinv[:, 3] by z / f (the
    object's depth over the focal length) and kinv by 1 / (f max(H, W)) (its first two columns are multiplied by the pixel coordinates).
    Measured relative differences: 1.5e-9 (v5) and 4.9e-10 (wide).  Asserted: 1e-5, the bound of the same check in
    tests/test_image_loss_host.py."""
    hv, got = host_case(hs, name, LAWS[0], True)
    sc = hv.sc
    f = float(np.asarray(sc["camera_M"][1])[0, 0])
    rinv = np.asarray(sc["camera_M"][2], np.float64)
    z = float((image_cases.frame()[0] - rinv[:3, 3]) @ rinv[:3, 2])
    rng = np.random.default_rng(17)
    D_k = rng.standard_normal((3, 3)) / (f * max(sc["height"], sc["width"]))
    D_r = rng.standard_normal((3, 4)) * np.array([1 / f, 1 / f, 1 / f, z / f])
    D = np.concatenate([D_k.reshape(-1), D_r.reshape(-1)])
    h = 1e-6
    fd = (hv.run(hv.cam21 + h * D)["loss"] - hv.run(hv.cam21 - h * D)["loss"]) / (2 * h)
    an = float((got["g_kinv"] * D_k).sum() + (got["g_rinv"] * D_r).sum())
    print(f"{name}: along the camera direction {an:.10e} against {fd:.10e} ({abs(an - fd) / abs(fd):.1e})")
    assert an != 0 and abs(an - fd) <= 1e-5 * abs(fd)


# ---- calibrate.camera_pose -------------------------------------------------------------------------------------------------------------------
def test_camera_pose_at_zero_and_its_units():
    """Zero gives the input camera to 1e-15.  One unit of each of the six numbers moves a projected point by 1 pixel within 5 %: the
    object's centre for the two sideways translations and the two tilts; a point one extent to the centre's side for the translation
    along and the rotation about the view axis, which leave the image of a centre on that axis where it is (asserted: it moves by less
    than 0.05 pixels)."""
    from drt_amd import calibrate
    cam = image_cases.camera(5, 32, 32)
    centre, extent = image_cases.frame()
    rinv, kinv = calibrate.camera_pose(cam, torch.zeros(6, dtype=torch.float64), centre, extent)
    assert rinv.shape == (4, 4) and kinv.shape == (3, 3)
    assert np.abs(rinv.numpy() - np.asarray(cam[2])).max() <= 1e-15 * np.abs(np.asarray(cam[2])).max() and np.array_equal(kinv.numpy(), np.asarray(cam[3]))
    side = centre + extent * np.asarray(cam[2])[:3, 0]
    for k in range(6):
        r, kk = (m.numpy() for m in calibrate.camera_pose(cam, torch.eye(6, dtype=torch.float64)[k], centre, extent))
        moved = (np.linalg.inv(r), cam[1], r, kk)
        at_centre = np.linalg.norm(ref_mod.project(moved, centre) - ref_mod.project(cam, centre))
        at_side = np.linalg.norm(ref_mod.project(moved, side) - ref_mod.project(cam, side))
        print(f"six[{k}]: the centre's image moves by {at_centre:.4f} pixels, the side point's by {at_side:.4f}")
        if k in (2, 5):
            assert at_centre < 0.05 and abs(at_side - 1.0) <= 0.05, (k, at_centre, at_side)
        else:
            assert abs(at_centre - 1.0) <= 0.05, (k, at_centre)
    six = torch.tensor([0.3, -0.2, 0.1, 0.4, 0.5, -0.6], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: calibrate.camera_pose(cam, x, centre, extent)[0][:3], (six,))
    with pytest.raises(ValueError, match="steps"):
        calibrate.fit_pose(lambda rows: rows.sum(), None, 4, 4, 0, 0.05)          # (the shared loop's checks, reached through fit_screen's optimiser)


def test_the_restatement_fit_replays_its_recorded_first_steps():
    """image_camera_ref.CPU_FIT records the fit of the displaced camera on the restatement (150 steps, re-traced every step).
    Here its first ten steps are run again and give the recorded losses to 1e-6 relative (Adam's first steps are lr * sign(g) and do not
    amplify last bits); the recorded start error is the case's."""
    rec = ref_mod.CPU_FIT
    case = ref_mod.fit_case()
    assert abs(ref_mod.pose_error(case["start"], case["true"], case["centre"], case["extent"]) - rec["start_error"]) <= 1e-9
    _, history = ref_mod.fit_on_the_restatement(steps=10)
    print("first ten losses:", " ".join(f"{v:.9e}" for v in history))
    assert np.abs(np.array(history) - np.array(rec["first"])).max() <= 1e-6 * rec["first"][0]
    assert rec["best"] < rec["first"][0] and rec["error"] < rec["start_error"]


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build, diffrender
    sig = _lib.SIGNATURES
    assert "drt_render_image_loss_camera" in sig and len(sig["drt_render_image_loss_camera"][1]) == 31
    assert sig["drt_render_image_loss_camera"][1][:29] == sig["drt_render_image_loss_screen"][1][:29]      # the same arguments up to d_grad_texture
    assert "drt_image_camera.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss_camera(" in header
    exports = open(os.path.join(ROOT, "drt_amd", "csrc", "exports.map")).read()
    assert "drt_*" in exports or "drt_render_image_loss_camera" in exports
    api = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_api.hip")).read()
    version = re.search(r"int drt_version\(void\) \{ return (\d+); \}", api)
    assert version and int(version.group(1)) >= 12
    wave = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_wave.h")).read()
    assert "int launch_image_camera_bwd(" in wave and "int launch_image_loss_bwd_camera(" in wave
    assert callable(diffrender._UnitSeedTerm.apply)


def _args():
    from drt_amd import render
    return dict(camera_M=None, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32),
                target=np.zeros((8, 8, 3), np.float32))


_R4, _K3 = torch.eye(4, dtype=torch.float64), torch.eye(3, dtype=torch.float64)


@pytest.mark.parametrize("kw,match", [
    (dict(camera_M=image_cases.camera(5, 8, 8), camera_param=(_R4, _K3)), "camera_param is given"),      # both forms given
    (dict(), "camera_M is None"),                                                                         # neither form given
    (dict(camera_param=_R4), "camera_param must be the pair"),                                            # not a pair
    (dict(camera_param=(_R4, _K3, _K3)), "camera_param must be the pair"),
    (dict(camera_param=(_R4.numpy(), _K3)), "Rinv must be a float64 tensor"),                             # not a tensor
    (dict(camera_param=(_R4, _K3.numpy())), "Kinv must be a float64 tensor"),
    (dict(camera_param=(_R4[:, :3], _K3)), "Rinv must have shape"),                                       # wrong shape
    (dict(camera_param=(_R4, _R4)), "Kinv must have shape"),
    (dict(camera_param=(_R4.to(torch.float32), _K3)), "Rinv must be float64"),                            # wrong dtype
    (dict(camera_param=(_R4, _K3.to(torch.float32))), "Kinv must be float64"),
    (dict(camera_param=(_R4 * float("nan"), _K3)), "Rinv must be finite"),                                # non-finite
    (dict(camera_param=(_R4[:3], _K3 * float("inf"))), "Kinv must be finite"),
])
def test_image_loss_fused_names_the_bad_camera_argument(kw, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    args = dict(_args(), **kw)
    pos = [args.pop(k) for k in ("camera_M", "height", "width", "screen", "texture", "target")]
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_fused(object(), *pos, **args)


def test_the_camera_forms_are_accepted():
    from drt_amd import render
    cam = image_cases.camera(5, 8, 8)
    a = _args()
    plain = render.check_image_loss_args(cam, 8, 8, a["screen"], a["texture"], a["target"])
    Rinv, Kinv = ref_mod.camera_tensors(cam)
    for R in (Rinv.clone().requires_grad_(True), Rinv[:3].clone().requires_grad_(True)):
        got = render.check_image_loss_args(None, 8, 8, a["screen"], a["texture"], a["target"], camera_param=(R, Kinv.clone().requires_grad_(True)))
        assert np.array_equal(got["camera"], plain["camera"]) and got["camera"].shape == (21,)
