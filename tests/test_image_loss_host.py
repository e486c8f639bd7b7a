"""CPU: the photometric loss of the refracted image and its adjoint (drt_amd/csrc/drt_image_loss.h), compiled for the host by g++ with
-ffp-contract=off (tests/hostsim/image_loss.cpp), against torch autograd of the restatement tests/image_loss_ref.py, against central
differences of the host loss itself, and the Python layer's checks that need no GPU.

Loss: the host build's relative difference from the restatement over the 18 cases (3 scenes x 3 laws x Fresnel on / off) was measured
as at most 3e-15 (image_loss_cases.MEASURED_LOSS_REL; the two sum the pixel terms in a different order and take different square roots); the tests assert
ten times that, LOSS_REL, which is far below the 1e-10 the figure may never exceed.  Gradients: the project's tolerance, 1e-9 of
the largest entry of the reference and 1e-5 absolute, for the vertex gradient and the two IOR partials."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_loss_cases as cases
import image_loss_ref
from conftest import IOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
EXT = cases.EXT
LOSS_REL = cases.LOSS_REL


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_loss.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_loss.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h", "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.il_fresnel_backward.argtypes = [_P, _P, _P, _P, _I64, _P, _P, _P]
    lib.il_view.restype = _D
    lib.il_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _D, _D, _I, _I] + [_P] * 12
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
    return np.ascontiguousarray(np.concatenate([np.asarray(camera_M[3]).reshape(-1), np.asarray(camera_M[2])[:3, :].reshape(-1)]))


class HostView:
    """One case on the host build with the classes and the tape of the restatement's forward at conftest.IOR held fixed.  ``name``: a
    scene of image_cases, or a scene dict of tests/image_fuzz_cases.py with its own IORs, fills, target and weight."""

    def __init__(self, hs, name, law, fresnel, weighted=False):
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
        self.target = np.ascontiguousarray(sc["target"]) if own else cases.target(name, law, fresnel)
        self.weight = sc["weight"] if own else cases.half_weight(name) if weighted else None
        tex = np.asarray(sc["texture"], np.float32)
        self.tex = np.ascontiguousarray(tex[:, :, None] if tex.ndim == 2 else tex)
        C = self.tex.shape[2]
        self.void, self.invalid = (np.ascontiguousarray(np.broadcast_to(np.asarray(sc[k], np.float64), (C,))) for k in ("void", "invalid"))

    def run(self, V=None, ior_int=None, ior_ext=None, want_image=False):
        sc, V = self.sc, self.V if V is None else np.ascontiguousarray(V)
        ior_int, ior_ext = self.ior_int if ior_int is None else ior_int, self.ior_ext if ior_ext is None else ior_ext
        grad, g_ior, count = np.zeros_like(V), np.zeros(2), np.zeros(1, np.int64)
        image = np.empty((sc["height"], sc["width"], self.tex.shape[2]), np.float32) if want_image else None
        loss = self.hs.il_view(_p(_cam21(sc["camera_M"])), sc["height"], sc["width"], sc["s"], _p(sc["screen"].packed()), _p(self.tex), self.tex.shape[0],
                               self.tex.shape[1], self.tex.shape[2], _p(self.F), _p(V), ior_int, ior_ext, int(self.law[2] == "snell"), int(self.fresnel),
                               _p(self.cls), _p(self.tape), _p(self.hits), _p(self.void), _p(self.invalid), _p(self.target), _p(self.weight), _p(grad),
                               _p(g_ior), _p(count), _p(image), None)
        return dict(loss=loss, grad_V=grad, g_int=g_ior[0], g_ext=g_ior[1], count=int(count[0]), image=image)


_views = {}


def host_case(hs, name, law, fresnel, weighted=False):
    key = (name, law, fresnel, weighted)
    if key not in _views:
        hv = HostView(hs, name, law, fresnel, weighted)
        _views[key] = (hv, hv.run(want_image=True))
    return _views[key]


# ---- fresnel_R_backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta_i,eta_t", [(1.00029, 1.4723), (1.4723, 1.00029), (1.0, 1.5), (1.5, 1.0)])
def test_fresnel_backward_matches_autograd(hs, eta_i, eta_t):
    """ci in {1, 0.5, 0.05} and the clamp edges: ci = 1 (1 - ci^2 = 0: the guarded root), ci = 0 from the thinner side (1 - ci^2 = 1: the closed upper
    bound passes the gradient; from the denser side R is 0 / 0 there and a mirrored bounce never evaluates it), ci just above 1 (below the lower bound: nothing passes), and, from the denser side, both sides of the critical
    angle (beyond it cos_t is the constant 0).  1e-12 relative to the largest partial of a row, or to the seed where that is
    larger (a mirrored row's partials are the residue of cancelling terms of the seed's size): some thirty roundings of such terms."""
    crit = np.sqrt(max(1.0 - (eta_t / eta_i) ** 2, 0.0))           # ci at the critical angle (0 from the thinner side)
    ci = np.array([1.0, 0.5, 0.05, 0.0 if eta_i < eta_t else 0.9, 1.0 + 1e-9, crit + 1e-3, max(crit - 1e-3, 1e-3), 0.999999])
    n = len(ci)
    ei, et, gR = np.full(n, eta_i), np.full(n, eta_t), np.linspace(0.5, 2.0, n)
    got = [np.empty(n) for _ in range(3)]
    hs.il_fresnel_backward(_p(ci), _p(ei), _p(et), _p(gR), n, *(_p(g) for g in got))
    t = [torch.tensor(a, requires_grad=True) for a in (ci, ei, et)]
    want = torch.autograd.grad((image_loss_ref.fresnel_R(*t) * torch.tensor(gR)).sum(), t)
    want = [w.numpy() for w in want]
    scale = np.max(np.abs(want), axis=0)
    for g, w in zip(got, want):
        assert np.isfinite(g).all() and np.isfinite(w).all()
        assert (np.abs(g - w) <= 1e-12 * np.maximum(scale, gR)).all(), (g, w)
    assert np.abs(got[0][3]) > 0 and np.abs(got[0][5]) > 0          # refracting rows: R depends on ci


# ---- the view ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", cases.LAWS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_loss_and_gradients_match_the_restatement(hs, name, law, fresnel):
    ref = cases.reference(name, law, fresnel)
    hv, got = host_case(hs, name, law, fresnel)
    if (name, law) in cases.COUNTS:
        assert ref["count"] == cases.COUNTS[(name, law)]
    assert got["count"] == ref["count"] > 0
    assert np.abs(got["image"].astype(np.float64) - ref["image"].astype(np.float64)).max() <= 2.0 ** -23
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    print(f"{name} {law} fresnel={fresnel}: loss {got['loss']:.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; "
          f"g_int {got['g_int']:.9e} / {ref['g_int']:.9e}, g_ext {got['g_ext']:.9e} / {ref['g_ext']:.9e}, "
          f"max |grad_V| {np.abs(ref['grad_V']).max():.3e} differs by {np.abs(got['grad_V'] - ref['grad_V']).max():.2e}")
    assert ref["loss"] > 0 and rel <= LOSS_REL
    assert cases.close(got["grad_V"], ref["grad_V"]) and np.abs(ref["grad_V"]).max() > 0
    assert cases.close(got["g_int"], ref["g_int"]) and cases.close(got["g_ext"], ref["g_ext"])
    assert ref["g_int"] != 0 and ref["g_ext"] != 0


@pytest.mark.parametrize("law", cases.LAWS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_dropping_the_throughput_term_is_caught(hs, name, law):
    """The negative control: the restatement with T detached -- what an adjoint that leaves the Fresnel factor out computes -- is outside
    the tolerance of the host build on every Fresnel-on case, in the vertex gradient and in both IOR partials."""
    bad = cases.reference(name, law, True, throughput_gradient=False)
    _, got = host_case(hs, name, law, True)
    assert bad["loss"] == cases.reference(name, law, True)["loss"]
    assert not cases.close(got["grad_V"], bad["grad_V"])
    assert not cases.close(got["g_int"], bad["g_int"]) and not cases.close(got["g_ext"], bad["g_ext"])


@pytest.mark.parametrize("name", ["v5", "wide"])
def test_a_zero_weight_removes_exactly_those_pixels(hs, name):
    law = cases.LAWS[0]
    ref = cases.reference(name, law, True, weighted=True)
    _, got = host_case(hs, name, law, True, weighted=True)
    assert abs(got["loss"] - ref["loss"]) <= LOSS_REL * ref["loss"] and 0 < ref["loss"] < cases.reference(name, law, True)["loss"] * 1.5
    assert cases.close(got["grad_V"], ref["grad_V"]) and cases.close(got["g_int"], ref["g_int"]) and cases.close(got["g_ext"], ref["g_ext"])


@pytest.mark.parametrize("name", ["v5", "wide"])
def test_central_differences_of_the_host_loss(hs, name):
    """Independent of the restatement: (2, drop, reference), Fresnel on; central differences of the host loss (classes and tape fixed)
    with h = 1e-6 along a fixed random vertex direction and in ior_int agree with the gradient to 1e-5 relative."""
    hv, got = host_case(hs, name, cases.LAWS[0], True)
    h = 1e-6
    D = np.random.default_rng(11).standard_normal(hv.V.shape)
    fd_v = (hv.run(V=hv.V + h * D)["loss"] - hv.run(V=hv.V - h * D)["loss"]) / (2 * h)
    fd_i = (hv.run(ior_int=IOR + h)["loss"] - hv.run(ior_int=IOR - h)["loss"]) / (2 * h)
    an_v = float((got["grad_V"] * D).sum())
    print(f"{name}: along the vertex direction {an_v:.10e} against {fd_v:.10e} ({abs(an_v - fd_v) / abs(fd_v):.1e}); "
          f"d / d ior_int {got['g_int']:.10e} against {fd_i:.10e} ({abs(got['g_int'] - fd_i) / abs(fd_i):.1e})")
    assert abs(an_v - fd_v) <= 1e-5 * abs(fd_v) and abs(got["g_int"] - fd_i) <= 1e-5 * abs(fd_i)


def test_the_target_itself_gives_a_loss_of_rounding_only(hs):
    """Against its own float32 image a pixel's residual is the rounding of that store: at most 2^-24 of a value below 2, so the loss is at
    most H W C 2^-46."""
    hv, got = host_case(hs, "v5", cases.LAWS[0], True)
    saved = hv.target
    try:
        hv.target = np.ascontiguousarray(got["image"])
        again = hv.run()
    finally:
        hv.target = saved
    assert 0.0 <= again["loss"] <= got["image"].size * 2.0 ** -46


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def _args():
    from drt_amd import render
    cam = image_cases.camera(5, 8, 8)
    return dict(camera_M=cam, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32),
                target=np.zeros((8, 8, 3), np.float32))


@pytest.mark.parametrize("key,value", [("camera_M", None), ("height", 0), ("width", -1), ("supersample", 5), ("max_bounces", 1), ("max_bounces", 4.0),
                                       ("tir", "mirror"), ("refraction", "exact"), ("fresnel", 1), ("screen", (0, 1, 2)),
                                       ("texture", np.zeros((4, 4, 2), np.float32)), ("void", [0.0, 1.0]), ("invalid", "red"), ("max_samples", 0),
                                       ("target", None), ("target", np.zeros((8, 8), np.float32)), ("target", np.zeros((8, 7, 3), np.float32)),
                                       ("target", np.zeros((8, 8, 3), np.float64)), ("target", np.zeros((8, 8, 3), np.int32)),
                                       ("target", np.full((8, 8, 3), np.nan, np.float32)),
                                       ("weight", np.zeros((8, 8, 1), np.float32)), ("weight", np.zeros((7, 8), np.float32)),
                                       ("weight", np.zeros((8, 8), np.uint8)), ("weight", np.full((8, 8), np.inf, np.float32)),
                                       ("ior_int", "glass"), ("ior_int", float("nan")), ("ior_int", torch.ones(2)), ("ior_ext", 0.0),
                                       ("vertices", 1), ("want_image", "yes")])
def test_image_loss_fused_names_the_bad_argument(key, value):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    kw = dict(_args(), **{key: value})
    pos = [kw.pop(k) for k in ("camera_M", "height", "width", "screen", "texture", "target")]
    with pytest.raises(ValueError, match=key):
        diffrender.Scene.image_loss_fused(object(), *pos, **kw)


def test_targets_of_every_accepted_form():
    from drt_amd import render
    a = _args()
    one = dict(a, texture=np.zeros((4, 4), np.float32))
    for kw, tgt in ((a, np.zeros((8, 8, 3), np.float32)), (one, np.zeros((8, 8), np.float32)), (one, np.zeros((8, 8, 1), np.float32))):
        got = render.check_image_loss_args(kw["camera_M"], 8, 8, kw["screen"], kw["texture"], tgt)
        assert got["target"].shape == (8, 8, got["channels"]) and got["target"].dtype == np.float32 and got["weight"] is None
    b = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(8, 8, 3)
    got = render.check_image_loss_args(a["camera_M"], 8, 8, a["screen"], a["texture"], b, weight=np.ones((8, 8), np.float32), ior_int=1.5,
                                       ior_ext=torch.tensor(1.0, dtype=torch.float64))
    assert np.array_equal(got["target"], b.astype(np.float32) / np.float32(255.0)) and got["weight"].shape == (8, 8)
    assert got["ior"] == (1.5, None)          # a number is checked and returned; a tensor's value is read by the caller


def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    assert "drt_render_image_loss" in _lib.SIGNATURES and len(_lib.SIGNATURES["drt_render_image_loss"][1]) == 28
    assert "drt_image_loss.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss(" in header
    api = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_api.hip")).read()
    version = re.search(r"int drt_version\(void\) \{ return (\d+); \}", api)
    assert version and int(version.group(1)) >= 9
    from drt_amd import diffrender
    assert callable(diffrender.Scene.image_loss_fused)
