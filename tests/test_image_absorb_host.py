"""CPU: the absorbing refracted image, its photometric loss and the adjoint (drt_amd/csrc/drt_image_absorb.h), compiled for the host by
g++ with -ffp-contract=off (tests/hostsim/image_absorb.cpp), against the restatement tests/image_absorb_ref.py and torch autograd of it,
against central differences of the host loss itself, against the clear-glass host functions at sigma = 0, and the Python layer's checks
that need no GPU.

Tolerances.  The interior length L: 0 -- the header's t is bounce_forward's; the restatement takes the value of L from the same
operations in the same order in numpy (image_absorb_ref.length_values: moller_trumbore's t along the recorded tape, with correctly
rounded roots in the path between the interactions), summed in interaction order.  A = exp(-(sigma L)): 4 * 2^-52 relative, two exp implementations each within one unit in
the last place.  The image: 2^-23, the float32 store of a value in [0, 1].  The loss: image_loss_cases.LOSS_REL.  Every gradient -- the
vertices, both IORs, sigma --: image_loss_cases.close, 1e-9 of the largest entry of the reference and 1e-5 absolute."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_absorb_cases as cases
import image_absorb_ref
import image_cases
import image_loss_cases
import image_ref
import test_image_loss_host as clear
from conftest import IOR
from oracle.diffrender_oracle import moller_trumbore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
EXT = cases.EXT
_p, _cam21 = clear._p, clear._cam21
close = image_loss_cases.close


def _build(stem, headers):
    src = os.path.join(ROOT, "tests", "hostsim", stem + ".cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, f"lib{stem}.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in headers]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)


_HEADERS = ("drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h", "drt_traverse.h", "drt_common.h")


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    lib = _build("image_absorb", ("drt_image_absorb.h",) + _HEADERS)
    lib.ia_t_backward.argtypes = [_P, _P, _P, _D, _D, _I, _P, _I64] + [_P] * 7
    lib.ia_view.restype = _D
    lib.ia_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _D, _D, _I, _I] + [_P] * 16
    return lib


@pytest.fixture(scope="module")
def hs():
    return load_hs()


@pytest.fixture(scope="module")
def hs_clear():
    lib = _build("image_loss", _HEADERS)
    lib.il_view.restype = _D
    lib.il_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _D, _D, _I, _I] + [_P] * 12
    return lib


class HostView(clear.HostView):
    """One case on the host build of the absorbing law, with the classes and the tape of the restatement's forward held fixed."""

    def __init__(self, hs, name, law, fresnel, weighted=False):
        super().__init__(hs, name, law, fresnel, weighted)
        self.sigma = cases.sigma(name)

    def run(self, V=None, ior_int=None, ior_ext=None, sigma=None, want_image=False):
        sc, V = self.sc, self.V if V is None else np.ascontiguousarray(V)
        ior_int, ior_ext = self.ior_int if ior_int is None else ior_int, self.ior_ext if ior_ext is None else ior_ext
        sigma = np.ascontiguousarray(self.sigma if sigma is None else sigma, np.float64)
        C, n = self.tex.shape[2], len(self.cls)
        grad, g_ior, g_sigma, count = np.zeros_like(V), np.zeros(2), np.zeros(C), np.zeros(1, np.int64)
        image = np.empty((sc["height"], sc["width"], C), np.float32) if want_image else None
        length = np.empty((sc["height"], sc["width"]), np.float32) if want_image else None
        L, A = (np.empty(n), np.empty((n, C))) if want_image else (None, None)
        loss = self.hs.ia_view(_p(_cam21(sc["camera_M"])), sc["height"], sc["width"], sc["s"], _p(sc["screen"].packed()), _p(self.tex), self.tex.shape[0],
                               self.tex.shape[1], C, _p(self.F), _p(V), ior_int, ior_ext, int(self.law[2] == "snell"), int(self.fresnel),
                               _p(self.cls), _p(self.tape), _p(self.hits), _p(self.void), _p(self.invalid), _p(sigma), _p(self.target), _p(self.weight),
                               _p(grad), _p(g_ior), _p(g_sigma), _p(count), _p(image), _p(length), _p(L), _p(A))
        return dict(loss=loss, grad_V=grad, g_int=g_ior[0], g_ext=g_ior[1], g_sigma=g_sigma, count=int(count[0]), image=image, length=length, L=L, A=A)


_views = {}


def host_case(hs, name, law, fresnel, weighted=False):
    key = (name, law, fresnel, weighted)
    if key not in _views:
        hv = HostView(hs, name, law, fresnel, weighted)
        _views[key] = (hv, hv.run(want_image=True))
    return _views[key]


# ---- bounce_t_backward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snell", [0, 1])
def test_t_backward_matches_autograd_and_both_laws_fill_t_and_sg(hs, snell):
    """Random triangles and rays that meet them from either side.  t and sg of law_forward<SNELL> are bounce_forward's bits and
    moller_trumbore's t; the adjoint of t agrees with autograd within 1e-12 of the largest partial of a row (some twenty roundings)."""
    rng = np.random.default_rng(3 + snell)
    n = 64
    tri = rng.standard_normal((n, 3, 3))
    bary = rng.dirichlet([1.0, 1.0, 1.0], n)
    point = (bary[:, :, None] * tri).sum(1)
    o = point + rng.standard_normal((n, 3)) * 2.0
    d = point - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    g_t = rng.uniform(0.5, 2.0, n)
    o, d, tri = (np.ascontiguousarray(a) for a in (o, d, tri))
    t, sg, t0, sg0 = (np.empty(n) for _ in range(4))
    gv, g_o, g_d = np.empty((n, 3, 3)), np.empty((n, 3)), np.empty((n, 3))
    hs.ia_t_backward(_p(o), _p(d), _p(tri), EXT, IOR, snell, _p(g_t), n, _p(t), _p(sg), _p(t0), _p(sg0), _p(gv), _p(g_o), _p(g_d))
    assert np.array_equal(t, t0) and np.array_equal(sg, sg0)
    to, td, tt = (torch.tensor(a, requires_grad=True) for a in (o, d, tri))
    _, _, ref_t, ref_n = moller_trumbore(to, td, tt)
    assert np.array_equal(t, ref_t.detach().numpy())
    inside = ~((-td * ref_n).sum(1).clamp(-1, 1) > 0).numpy()
    assert np.array_equal(sg < 0, inside) and 0 < inside.sum() < n
    want = torch.autograd.grad((ref_t * torch.tensor(g_t)).sum(), (tt, to, td))
    scale = np.maximum(np.abs(want[0].numpy()).reshape(n, -1).max(1), 1.0)
    for got, w in zip((gv, g_o, g_d), want):
        w = w.numpy()
        assert np.isfinite(got).all() and (np.abs(got - w).reshape(n, -1).max(1) <= 1e-12 * scale).all()
    assert np.abs(g_o).max() > 0 and np.abs(g_d).max() > 0


# ---- the view ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", cases.LAWS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_law_loss_and_gradients_match_the_restatement(hs, name, law, fresnel):
    ref = cases.reference(name, law, fresnel)
    fwd = ref["fwd"]
    hv, got = host_case(hs, name, law, fresnel)
    sc = hv.sc
    through = (fwd["cls"] == image_ref.THROUGH).numpy()
    L_ref, A_ref = fwd["L"].detach().numpy(), fwd["A"].detach().numpy()
    assert through.sum() > 0 and np.array_equal(got["L"][through], L_ref[through])
    assert (L_ref[through] > 0).all() and not got["L"][~through].any()
    a_rel = np.abs(got["A"][through] / A_ref[through] - 1).max()
    assert a_rel <= 4 * 2.0 ** -52
    assert 0 < A_ref[through].min() and A_ref[through].max() < 1
    if A_ref.shape[1] == 3:          # the three coefficients together cover most of (0, 1)
        assert A_ref[through].min() < 0.25 and A_ref[through].max() > 0.75
    assert np.abs(got["image"].astype(np.float64) - ref["image"].astype(np.float64)).max() <= 2.0 ** -23
    assert np.array_equal(got["length"], image_absorb_ref.length_plane(fwd, sc["height"], sc["width"], sc["s"]).numpy())
    if (name, law) in image_loss_cases.COUNTS:
        assert ref["count"] == image_loss_cases.COUNTS[(name, law)]
    assert got["count"] == ref["count"] > 0
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    print(f"{name} {law} fresnel={fresnel}: loss {got['loss']:.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; A off by {a_rel:.2e}; "
          f"g_int {got['g_int']:.9e} / {ref['g_int']:.9e}, g_ext {got['g_ext']:.9e} / {ref['g_ext']:.9e}, g_sigma {got['g_sigma']} / {ref['g_sigma']}, "
          f"max |grad_V| {np.abs(ref['grad_V']).max():.3e} differs by {np.abs(got['grad_V'] - ref['grad_V']).max():.2e}")
    assert ref["loss"] > 0 and rel <= image_loss_cases.LOSS_REL
    assert close(got["grad_V"], ref["grad_V"]) and np.abs(ref["grad_V"]).max() > 0
    assert close(got["g_int"], ref["g_int"]) and close(got["g_ext"], ref["g_ext"]) and ref["g_int"] != 0 and ref["g_ext"] != 0
    assert close(got["g_sigma"], ref["g_sigma"]) and ref["g_sigma"].all()


@pytest.mark.parametrize("law", cases.LAWS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_dropping_the_length_term_is_caught(hs, name, law):
    """The negative control: the restatement with L detached -- what an adjoint without bounce_t_backward computes -- has the same loss and
    the same sigma partials, and a vertex gradient outside the tolerance of the host build."""
    good, bad = cases.reference(name, law, True), cases.reference(name, law, True, length_gradient=False)
    _, got = host_case(hs, name, law, True)
    assert bad["loss"] == good["loss"] and close(bad["g_sigma"], good["g_sigma"])
    assert not close(got["grad_V"], bad["grad_V"])


@pytest.mark.parametrize("name", ["v5", "wide"])
def test_a_zero_weight_removes_exactly_those_pixels(hs, name):
    law = cases.LAWS[1]
    ref = cases.reference(name, law, True, weighted=True)
    _, got = host_case(hs, name, law, True, weighted=True)
    assert abs(got["loss"] - ref["loss"]) <= image_loss_cases.LOSS_REL * ref["loss"]
    assert close(got["grad_V"], ref["grad_V"]) and close(got["g_int"], ref["g_int"]) and close(got["g_ext"], ref["g_ext"])
    assert close(got["g_sigma"], ref["g_sigma"])


@pytest.mark.parametrize("name", ["v5", "wide"])
def test_central_differences_of_the_host_loss(hs, name):
    """Independent of the restatement: (6, reflect, snell), Fresnel on; central differences of the host loss (classes and tape fixed) in
    every sigma_ch with h = 1e-6 -- the loss is smooth in sigma, its third derivative times h^2 is far below the bound -- and along a fixed
    random vertex direction agree with the gradient to 1e-5 relative."""
    hv, got = host_case(hs, name, cases.LAWS[2], True)
    h = 1e-6
    for ch in range(len(hv.sigma)):
        e = np.zeros_like(hv.sigma)
        e[ch] = h
        fd = (hv.run(sigma=hv.sigma + e)["loss"] - hv.run(sigma=hv.sigma - e)["loss"]) / (2 * h)
        print(f"{name}: d / d sigma[{ch}] {got['g_sigma'][ch]:.10e} against {fd:.10e} ({abs(got['g_sigma'][ch] - fd) / abs(fd):.1e})")
        assert abs(got["g_sigma"][ch] - fd) <= 1e-5 * abs(fd)
    D = np.random.default_rng(11).standard_normal(hv.V.shape)
    fd_v = (hv.run(V=hv.V + h * D)["loss"] - hv.run(V=hv.V - h * D)["loss"]) / (2 * h)
    an_v = float((got["grad_V"] * D).sum())
    print(f"{name}: along the vertex direction {an_v:.10e} against {fd_v:.10e} ({abs(an_v - fd_v) / abs(fd_v):.1e})")
    assert abs(an_v - fd_v) <= 1e-5 * abs(fd_v)


@pytest.mark.parametrize("fresnel", [True, False])
@pytest.mark.parametrize("law", cases.LAWS)
@pytest.mark.parametrize("name", ["v5", "wide"])
def test_sigma_zero_gives_the_bits_of_the_clear_glass(hs, hs_clear, name, law, fresnel):
    hv, _ = host_case(hs, name, law, fresnel)
    got = hv.run(sigma=np.zeros_like(hv.sigma), want_image=True)
    want = clear.HostView(hs_clear, name, law, fresnel).run(want_image=True)
    assert got["loss"] == want["loss"] and got["count"] == want["count"] and np.array_equal(got["image"], want["image"])
    assert np.array_equal(got["grad_V"], want["grad_V"]) and got["g_int"] == want["g_int"] and got["g_ext"] == want["g_ext"]
    assert (got["A"] == 1.0).all() and got["g_sigma"].all()          # the sigma partials do not vanish at 0


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
_BAD = [-0.1, float("nan"), float("inf"), [0.1, 0.2], [0.1, 0.2, 0.3, 0.4], "thick", True, torch.zeros(3, dtype=torch.float32),
        torch.zeros(2, dtype=torch.float64), torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64), [0.1, float("nan"), 0.3]]


@pytest.mark.parametrize("value", _BAD)
def test_render_image_names_a_bad_absorption(value):
    from drt_amd import diffrender
    a = clear._args()
    with pytest.raises(ValueError, match="absorption"):
        diffrender.Scene.render_image(object(), a["camera_M"], 8, 8, a["screen"], a["texture"], absorption=value)


@pytest.mark.parametrize("value", _BAD)
def test_image_loss_fused_names_a_bad_absorption(value):
    from drt_amd import diffrender
    a = clear._args()
    with pytest.raises(ValueError, match="absorption"):
        diffrender.Scene.image_loss_fused(object(), a["camera_M"], 8, 8, a["screen"], a["texture"], a["target"], absorption=value)


@pytest.mark.parametrize("other", ["screen_param", "texture_param", "camera_param"])
def test_absorption_goes_with_no_other_parameter_gradient(other):
    from drt_amd import diffrender
    a = clear._args()
    cam = a["camera_M"]
    kw = dict(absorption=0.01)
    pos = [cam, 8, 8, a["screen"], a["texture"], a["target"]]
    if other == "screen_param":
        kw[other], pos[3] = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float64), None
    elif other == "texture_param":
        kw[other], pos[4] = torch.zeros((4, 4, 3)), None
    else:
        kw[other], pos[0] = (torch.tensor(np.asarray(cam[2])), torch.tensor(np.asarray(cam[3]))), None
    with pytest.raises(ValueError, match=f"absorption cannot be combined with {other}"):
        diffrender.Scene.image_loss_fused(object(), *pos, **kw)


def test_absorption_of_every_accepted_form():
    from drt_amd import render
    a = clear._args()
    pos = (a["camera_M"], 8, 8, a["screen"], a["texture"])
    assert render.check_render_args(*pos)["absorption"] is None
    for value in (0.02, np.float32(0.5), 0, [0.02], [0.0, 0.1, 0.2], np.array([0.0, 0.1, 0.2]), torch.tensor([0.0, 0.1, 0.2], dtype=torch.float64)):
        got = render.check_render_args(*pos, absorption=value)["absorption"]
        assert got.dtype == np.float64 and got.shape == (3,) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, np.broadcast_to(np.asarray(value, np.float64).reshape(-1), (3,)))
    one = render.check_image_loss_args(a["camera_M"], 8, 8, a["screen"], np.zeros((4, 4), np.float32), np.zeros((8, 8), np.float32), absorption=0.3)
    assert np.array_equal(one["absorption"], [0.3])


def test_fit_absorption_names_its_bad_arguments():
    from drt_amd import calibrate
    a = clear._args()
    views = [(a["camera_M"], a["target"])]
    for kw, match in ((dict(steps=0, lr=0.1), "steps"), (dict(steps=3, lr=0.0), "lr"), (dict(steps=3, lr=0.1, absorption=0.1), "absorption"),
                      (dict(steps=3, lr=0.1, vertices=True), "vertices")):
        with pytest.raises(ValueError, match=match):
            calibrate.fit_absorption(object(), views, a["screen"], a["texture"], **kw)
    with pytest.raises(ValueError, match="views"):
        calibrate.fit_absorption(object(), [], a["screen"], a["texture"], steps=3, lr=0.1)


def test_entry_points_are_declared_everywhere():
    from drt_amd import _lib, build, diffrender
    plain, loss = _lib.SIGNATURES["drt_render_image"][1], _lib.SIGNATURES["drt_render_image_loss"][1]
    assert len(_lib.SIGNATURES["drt_render_image_absorb"][1]) == len(plain) + 2
    assert len(_lib.SIGNATURES["drt_render_image_loss_absorb"][1]) == len(loss) + 2
    assert "drt_image_absorb.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    exports = open(os.path.join(ROOT, "drt_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^}]*?)local:", exports, re.S).group(1).replace(";", " ").split()
    for name in ("drt_render_image_absorb", "drt_render_image_loss_absorb"):
        assert f"int {name}(" in header and any(fnmatch.fnmatchcase(name, p) for p in patterns)          # (the map exports drt_*)
    api = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_api.hip")).read()
    assert re.search(r"int drt_version\(void\) \{ return 13; \}", api)          # callers probe for the symbols instead
    assert callable(diffrender.enqueue_image_absorb_term)
