"""CPU: absorbing glass in the image term of several views, in front of their screens, of one environment, or of both
(drt_render_image_loss_views_absorb).  Nothing is new per sample: the law is drt_image_absorb.h's, the environment's
drt_image_env.h's and the mapping drt_image_views.h's, so the host checks are about their product, compiled for the host by g++ with
-ffp-contract=off (tests/hostsim/image_views_absorb.cpp, which restates the kernels' few lines and does not compile them):

  * the interior length, the attenuation and the transmitted colour formed through the table row of a sample's band row, for every sample
    of the bands at which the mapping can go wrong, against those of the single-view functions, bit for bit;
  * the host loss, vertex gradient, IOR partials and sigma partials of two views in one pass against the SUM of the restatement
    (tests/image_views_absorb_cases.py; tolerances image_loss_cases.LOSS_REL and .close, the count exact) under the three laws and the five
    backgrounds;
  * the length's adjoint through an environment-going sample against autograd, the sigma partials against central differences, two
    negative controls, sigma = 0 against the clear functions;
  * every argument check that needs no GPU, the declarations, and the native call each ``absorption`` makes."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import image_absorb_env_ref
import image_cases
import image_env_cases
import image_loss_cases as cases
import image_ref
import image_views_absorb_cases as vac
from conftest import IOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
EXT = image_cases.EXT
EH, EW = image_env_cases.EH, image_env_cases.EW
PAIR = vac.PAIR
LAWS = image_cases.LAWS
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
BG_IDS = [k + ("-reflection" if r else "") for k, r in vac.BACKGROUNDS]
WHO = "drt_render_image_loss_views_absorb"


def load_hv():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_views_absorb.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_views_absorb.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_views.h", "drt_image_env.h", "drt_image_absorb.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h",
                                                    "drt_path.h", "drt_shade.h", "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.iva_band.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I] + [_P] * 9
    lib.iva_view.argtypes = [_P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I] + [_P] * 9
    lib.iva_views_loss.restype = _D
    lib.iva_views_loss.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I, _I] + [_P] * 14
    lib.iva_env_adjoint.restype = _D
    lib.iva_env_adjoint.argtypes = [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I] + [_P] * 8
    return lib


@pytest.fixture(scope="module")
def hv():
    return load_hv()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _cam21(camera_M):
    return np.ascontiguousarray(np.concatenate([np.asarray(camera_M[3], np.float64).reshape(-1), np.asarray(camera_M[2], np.float64)[:3, :].reshape(-1)]))


def _mesh():
    mesh = image_cases.hand()
    return np.ascontiguousarray(mesh.faces, dtype=np.int32), np.ascontiguousarray(mesh.vertices, dtype=np.float64)


def _path(name, law):
    """dict(cls int32 [n], tape int32 [K, n], hits / seen uint8 [n]) of a view: the restatement's (the path does not know its background)."""
    fwd = vac.reference(name, law, "room", True)["fwd"]
    return dict(cls=np.ascontiguousarray(fwd["cls"].numpy(), dtype=np.int32), tape=np.ascontiguousarray(fwd["tape"].numpy(), dtype=np.int32),
                hits=np.ascontiguousarray(fwd["hits"].numpy(), dtype=np.uint8), seen=np.ascontiguousarray(fwd["seen"].numpy(), dtype=np.uint8))


def _background_args(kind, C=3):
    """(tex, th, tw, C, env texels, Eh, Ew, rotation) as the host functions take them."""
    env = image_env_cases.environment(C)
    tex = image_cases.scene("v5")["texture"] if vac.has_screen(kind) else None
    return (_p(tex), image_cases.TEX, image_cases.TEX, C, _p(env.texels) if vac.has_room(kind) else None, EH, EW,
            _p(np.ascontiguousarray(env.rotation)) if vac.has_room(kind) else None)


# ---- the table rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["screen", "room-screen"])
def test_length_attenuation_and_colour_through_the_table_row_have_the_bits_of_the_single_view(hv, kind):
    """v5 then v41 in the table, listed [1, 0]; the band (27, 36) straddles the view border, rows 31, 32 and 63 are its two sides and the
    last row."""
    law = LAWS[2]
    faces, verts = _mesh()
    H = W = 32
    s, s2, C = 2, 4, 3
    scs = [image_cases.scene(name) for name in PAIR]
    paths = [_path(name, law) for name in PAIR]
    void, invalid = np.full(C, scs[0]["void"]), np.full(C, scs[0]["invalid"])
    bg = _background_args(kind)
    single = []
    for sc, p in zip(scs, paths):
        n = H * W * s2
        out = dict(L=np.zeros(n), A=np.zeros((n, C)), col=np.zeros((n, C)))
        hv.iva_view(_p(_cam21(sc["camera_M"])), _p(np.ascontiguousarray(sc["screen"].packed())), H, W, s, *bg, _p(faces), _p(verts), len(faces), IOR, EXT, 1,
                    _p(p["cls"]), _p(p["tape"]), _p(p["hits"]), _p(vac.SIGMA), _p(void), _p(invalid), _p(out["L"]), _p(out["A"]), _p(out["col"]))
        single.append(out)
    cams21 = np.ascontiguousarray(np.stack([_cam21(sc["camera_M"]) for sc in scs]))
    screens9 = np.ascontiguousarray(np.stack([sc["screen"].packed() for sc in scs]))
    ids = [1, 0]
    ids_c = np.ascontiguousarray(ids, np.int32)
    n_inside = 0
    for r0, r1 in [(27, 36), (31, 32), (32, 33), (63, 64)]:
        n = (r1 - r0) * W * s2
        i = np.arange(n)
        pix = i // s2
        r = r0 + pix // W
        view, inside = np.asarray(ids)[r // H], ((r % H) * W + pix % W) * s2 + i % s2          # the sample's view and its index within that view
        gather = lambda key: np.ascontiguousarray(np.stack([p[key] for p in paths])[view, inside])      # noqa: E731
        tape = np.ascontiguousarray(np.stack([p["tape"] for p in paths])[view, :, inside].T)
        L, A, col = np.zeros(n), np.zeros((n, C)), np.zeros((n, C))
        hv.iva_band(_p(cams21), _p(screens9), 2, _p(ids_c), 2, H, W, s, r0, r1, *bg, _p(faces), _p(verts), len(faces), IOR, EXT, 1, _p(gather("cls")), _p(tape),
                    _p(gather("hits")), _p(vac.SIGMA), _p(void), _p(invalid), _p(L), _p(A), _p(col))
        for got, key in ((L, "L"), (A, "A"), (col, "col")):
            want = np.ascontiguousarray(np.stack([sv[key] for sv in single])[view, inside])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (key, r0, r1)
        n_inside += int((L > 0).sum())
        assert ((A < 1) == (L > 0)[:, None]).all()
    assert n_inside > 200


# ---- loss and gradients ---------------------------------------------------------------------------------------------------------------------
def _views_loss(hv, law, kind, reflection, order=("v41", "v5"), sigma=vac.SIGMA, want_images=False, clear=False):
    """dict(loss, grad_V, g_int, g_ext, g_sigma, count, images) of the host pass over the listed views; the table holds v5 then v41."""
    sc = image_cases.scene("v5")
    H, W, s, C = sc["height"], sc["width"], sc["s"], 3
    faces, verts = _mesh()
    cams = np.ascontiguousarray(np.stack([_cam21(image_cases.scene(name)["camera_M"]) for name in PAIR]))
    screens = np.ascontiguousarray(np.stack([image_cases.scene(name)["screen"].packed() for name in PAIR]))
    targets = np.ascontiguousarray(np.stack([vac.target(name, law, kind, reflection) for name in PAIR]))
    ids = np.ascontiguousarray([PAIR.index(name) for name in order], np.int32)
    paths = [_path(name, law) for name in order]
    cat = lambda key: np.ascontiguousarray(np.concatenate([p[key] for p in paths]))      # noqa: E731
    tape = np.ascontiguousarray(np.concatenate([p["tape"] for p in paths], axis=1))
    grad, g_ior, g_sigma, count = np.zeros_like(verts), np.zeros(2), np.zeros(C), np.zeros(1, np.int64)
    images = np.zeros((2, H, W, C), np.float32) if want_images else None
    sigma = None if clear else np.ascontiguousarray(sigma, dtype=np.float64)
    loss = hv.iva_views_loss(_p(cams), _p(screens), 2, _p(ids), len(order), H, W, s, *_background_args(kind), _p(faces), _p(verts), len(faces), IOR, EXT,
                             int(law[2] == "snell"), int(reflection), _p(cat("cls")), _p(tape), _p(cat("hits")), _p(cat("seen")), _p(sigma), _p(np.full(C, float(sc["void"]))),
                             _p(np.full(C, float(sc["invalid"]))), _p(targets), None, _p(grad), _p(g_ior), _p(g_sigma), _p(count), _p(images))
    return dict(loss=loss, grad_V=grad, g_int=g_ior[0], g_ext=g_ior[1], g_sigma=g_sigma, count=int(count[0]), images=images)


@pytest.mark.parametrize("kind,reflection", vac.BACKGROUNDS, ids=BG_IDS)
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_two_views_in_one_pass_give_the_sum_of_the_restatement(hv, law, kind, reflection):
    """The table holds v5 then v41; the call lists them as [v41, v5], so that neither slot reads its own row by accident."""
    order = ("v41", "v5")
    got = _views_loss(hv, law, kind, reflection, order, want_images=True)
    want = vac.summed(order, law, kind, reflection)
    rel = abs(got["loss"] - want["loss"]) / want["loss"]
    print(f"{law} {kind} reflection={reflection}: loss {got['loss']:.12e} against {want['loss']:.12e} ({rel:.2e}); count {got['count']}; max |d grad_V| "
          f"{np.abs(got['grad_V'] - want['grad_V']).max():.2e} of {np.abs(want['grad_V']).max():.3e}; g_sigma {got['g_sigma']} differs by "
          f"{np.abs(got['g_sigma'] - want['g_sigma']).max():.2e}")
    assert rel <= cases.LOSS_REL and got["count"] == want["count"] > 0
    assert cases.close(got["grad_V"], want["grad_V"]) and cases.close(got["g_int"], want["g_int"]) and cases.close(got["g_ext"], want["g_ext"])
    assert cases.close(got["g_sigma"], want["g_sigma"])
    assert not cases.close(got["grad_V"], vac.reference(order[0], law, kind, reflection)["grad_V"])          # (one view alone is outside the tolerance)
    for slot, name in enumerate(PAIR):                                                                    # the images sit at their views' places
        assert np.abs(got["images"][slot].astype(np.float64) - vac.reference(name, law, kind, reflection)["image"]).max() <= 2.0 ** -22


def test_the_length_adjoint_through_an_environment_going_sample_against_autograd(hv):
    """No screen: every through sample goes to the environment.  The adjoint of sum_samples sum_ch g_c[ch] (A T E)[ch] under fixed seeds,
    per sample by image_env_sample_backward<.., LENGTH> -- which hands g_L to bounce_t_backward at every interaction inside the object --,
    against autograd of the restatement's transmitted colours; with L detached the restatement is outside the tolerance."""
    law, name = LAWS[2], "v5"
    sc = image_cases.scene(name)
    faces, verts = _mesh()
    p = _path(name, law)
    env = image_env_cases.environment(3)
    g_c = np.array([0.7, -1.1, 0.4])
    sel = np.ascontiguousarray(p["cls"] == image_ref.THROUGH, dtype=np.uint8)
    grad, g_ior = np.zeros_like(verts), np.zeros(2)
    total = hv.iva_env_adjoint(_p(_cam21(sc["camera_M"])), sc["height"], sc["width"], sc["s"], 3, _p(env.texels), EH, EW, _p(np.ascontiguousarray(env.rotation)), _p(faces),
                               _p(verts), len(faces), IOR, EXT, 1, _p(p["cls"]), _p(p["tape"]), _p(p["hits"]), _p(sel), _p(vac.SIGMA), _p(g_c), _p(grad), _p(g_ior))

    def autograd(detach_L):
        V = torch.tensor(verts, requires_grad=True)
        ii, ie = torch.tensor(IOR, dtype=torch.float64, requires_grad=True), torch.tensor(EXT, dtype=torch.float64, requires_grad=True)
        fwd = image_absorb_env_ref.forward(faces, V, sc["camera_M"], sc["height"], sc["width"], None, None, env.texels, env.rotation, sc["s"], law, sc["invalid"], ii, ie,
                                           vac.SIGMA, detach_L=detach_L)
        f = (fwd["trans"][torch.as_tensor(sel.astype(bool))] * torch.as_tensor(g_c)).sum()
        return (float(f.detach()),) + tuple(g.numpy() for g in torch.autograd.grad(f, (V, ii, ie)))

    f, gV, gi, ge = autograd(False)
    print(f"sum {total:.12e} / {f:.12e}; max |grad_V| {np.abs(gV).max():.3e} differs by {np.abs(grad - gV).max():.2e}; g_int {g_ior[0]:.9e} / {float(gi):.9e}")
    assert int(sel.sum()) > 1000 and abs(total - f) <= 1e-12 * abs(f)
    assert cases.close(grad, gV) and cases.close(g_ior[0], gi) and cases.close(g_ior[1], ge)
    assert not cases.close(grad, autograd(True)[1])


@pytest.mark.parametrize("kind", ["room-screen", "room"])
def test_sigma_partials_against_central_differences_with_the_reflection(hv, kind):
    """(loss(sigma + h e_ch) - loss(sigma - h e_ch)) / 2h of the host pass against its own partial.  h = 1e-6: the truncation is
    h^2 / 6 times the third derivative, at most L_max^2 times the first; six interactions inside a hand 115 units across keep L below
    some 350 units, so L^2 <= 1.2e5 and the truncation is at most 2e-8 of the partial; the rounding of a loss of some 100 is
    100 * 2^-52 / h = 2e-8 against partials of a thousand.  Asserted at 1e-6 of the partial."""
    law, h = LAWS[2], 1e-6
    base = _views_loss(hv, law, kind, True)
    for ch in range(3):
        e = np.zeros(3)
        e[ch] = h
        fd = (_views_loss(hv, law, kind, True, sigma=vac.SIGMA + e)["loss"] - _views_loss(hv, law, kind, True, sigma=vac.SIGMA - e)["loss"]) / (2 * h)
        print(f"{kind} d loss / d sigma[{ch}]: {base['g_sigma'][ch]:.9e}, central difference {fd:.9e}")
        assert abs(base["g_sigma"][ch]) > 100 and abs(fd - base["g_sigma"][ch]) <= 1e-6 * abs(base["g_sigma"][ch])


@pytest.mark.parametrize("kind", ["room-screen", "room"])
def test_two_restatements_that_are_not_the_law_fall_outside_the_tolerance(hv, kind):
    """A sigma partial that takes the reflected light along (what multiplying the walk's c[] by L AFTER the reflection was added would
    give), and an adjoint with the interior length detached."""
    law = LAWS[2]
    got = _views_loss(hv, law, kind, True)
    leaked = vac.summed(("v41", "v5"), law, kind, True, sigma_sees_reflection=True)
    assert cases.close(got["grad_V"], leaked["grad_V"]) and not cases.close(got["g_sigma"], leaked["g_sigma"])
    flat = vac.summed(("v41", "v5"), law, kind, True, length_gradient=False)
    assert abs(flat["loss"] - got["loss"]) <= cases.LOSS_REL * got["loss"] and cases.close(got["g_sigma"], flat["g_sigma"])
    assert not cases.close(got["grad_V"], flat["grad_V"]) and not cases.close(got["g_int"], flat["g_int"])


@pytest.mark.parametrize("kind,reflection", vac.BACKGROUNDS, ids=BG_IDS)
def test_sigma_zero_is_the_clear_pass_and_its_sigma_partial_is_not_zero(hv, kind, reflection):
    """A = exp(-(0 L)) = 1 exactly and g_L = 0: loss, gradients and count are those of the clear functions, value for value (a zero may
    differ in sign: x + -0 keeps x)."""
    law = LAWS[2]
    zero = _views_loss(hv, law, kind, reflection, sigma=np.zeros(3))
    clear = _views_loss(hv, law, kind, reflection, clear=True)
    assert zero["loss"] == clear["loss"] > 0 and zero["count"] == clear["count"] > 0
    assert np.array_equal(zero["grad_V"], clear["grad_V"]) and zero["g_int"] == clear["g_int"] and zero["g_ext"] == clear["g_ext"] and clear["grad_V"].any()
    want = vac.summed(("v41", "v5"), law, kind, reflection, sigma=(0.0, 0.0, 0.0))["g_sigma"]
    assert np.abs(zero["g_sigma"]).min() > 0 and cases.close(zero["g_sigma"], want) and not clear["g_sigma"].any()


# ---- the argument checks -------------------------------------------------------------------------------------------------------------------
def _bind_args(n=4, H=8, W=6, C=3):
    from drt_amd import render
    cams = [image_cases.camera(5 + k, H, W) for k in range(n)]
    screens = [render.Screen([0, 0, k], [1, 0, 0], [0, 1, 0]) for k in range(n)]
    return dict(cameras=cams, height=H, width=W, screens=screens, targets=np.zeros((n, H, W, C), np.float32), environment=image_env_cases.environment(C))


def _fake_binding(**kw):
    """A binding with everything the argument checks read and no device table behind it."""
    from drt_amd import render
    b = render.ImageViews.__new__(render.ImageViews)
    b.args = render.check_image_views_args(**dict(_bind_args(), **kw))
    b.n, b.height, b.width, b.channels, b._h, b._mesh, b.scene = 4, 8, 6, 3, None, None, None
    return b


TEX = np.zeros((4, 4, 3), np.float32)


@pytest.mark.parametrize("bind,kw,match", [
    ({}, {"absorption": -0.1}, "absorption must be"),
    ({}, {"absorption": (0.1, 0.2)}, "absorption must be"),
    ({}, {"absorption": float("nan")}, "absorption must be"),
    ({}, {"absorption": torch.zeros(3, dtype=torch.float32)}, "absorption must be.*float32"),
    ({"environment": None}, {"absorption": True}, "absorption must be"),
    ({}, {"absorption": 0.1, "want_images": 1}, "want_images must be"),
    ({}, {"want_images": True}, "want_images=True needs absorption"),
    ({"environment": None}, {"absorption": 0.1, "reflection": True}, "multi-view"),
    ({}, {"absorption": 0.1, "reflection": True, "fresnel": False}, "fresnel"),
])
def test_image_loss_views_fused_names_the_bad_argument(bind, kw, match):
    """Raised in render.check_image_views_law, before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_views_fused(object(), _fake_binding(**bind), [0, 1], TEX, **kw)


def test_the_accepted_calls_reach_the_scene_check():
    """Absorption goes with a binding's environment here -- with and without screens, with the reflection --, and in every form."""
    from drt_amd import diffrender, render
    for bind, texture, kw in (({}, TEX, {"absorption": 0.02, "reflection": True}), ({"screens": None}, None, {"absorption": (0.1, 0.2, 0.3), "want_images": True}),
                              ({"environment": None}, TEX, {"absorption": torch.tensor([0.1, 0.0, 0.3], dtype=torch.float64)}), ({}, TEX, {"absorption": 0.0})):
        with pytest.raises(ValueError, match="another scene"):
            diffrender.Scene.image_loss_views_fused(object(), _fake_binding(**bind), [0, 1], texture, **kw)
    a = render.check_image_views_law(_fake_binding(), [3, 0, 3], TEX, reflection=True, absorption=0.25, want_images=True)
    assert np.array_equal(a["absorption"], [0.25] * 3) and a["absorption"].dtype == np.float64 and a["want_images"] is True and a["environment"] is not None
    a = render.check_image_views_law(_fake_binding(), [3, 0, 3], TEX)
    assert a["absorption"] is None and a["want_images"] is False


def test_the_single_view_refusals_stay():
    from drt_amd import render
    sc = image_cases.scene("v5")
    with pytest.raises(ValueError, match="absorption"):
        render.check_render_args(sc["camera_M"], 8, 8, sc["screen"], sc["texture"], absorption=0.1, environment=image_env_cases.environment(3))


def test_the_absorption_state_makes_fit_absorptions_update():
    from drt_amd import optim
    fixed = optim.AbsorptionState((0.1, 0.2, 0.3), 3)
    assert not fixed.fitted and fixed.lr == 0.0 and np.array_equal(fixed.sigma, [0.1, 0.2, 0.3]) and fixed.sigma.dtype == np.float64
    assert np.array_equal(optim.AbsorptionState(None, 3, 0.01).sigma, np.zeros(3)) and np.array_equal(optim.AbsorptionState(0.5, 1).sigma, [0.5])
    state = optim.AbsorptionState(None, 3, 0.01)
    held = state.sigma                                       # (the array the packed call's pointer is taken from stays the same object)
    ref = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=0.01)
    rng = np.random.default_rng(3)
    for k in range(5):
        g = -np.abs(rng.standard_normal(3)) - 0.1
        g[2] = 1.0 - g[2]                                    # a partial that pushes below zero: the projection holds it at 0
        ref.grad = torch.as_tensor(g.copy())
        opt.step()
        with torch.no_grad():
            ref.clamp_(min=0.0)
        assert state.update(g) is held and np.array_equal(held, ref.detach().numpy()) and state.steps == k + 1
    assert held[2] == 0.0 and (held >= 0).all() and held[:2].max() > 0
    for bad in (-0.1, float("nan"), True, "0.1"):
        with pytest.raises(ValueError, match="absorption_lr"):
            optim.AbsorptionState(None, 3, bad)
    with pytest.raises(ValueError, match="absorption must be"):
        optim.AbsorptionState((0.1, 0.2), 3)


def test_the_photo_loop_and_the_capture_take_the_keywords():
    from drt_amd import captured_data, diffrender, optim
    for fn, names in ((optim.PhotoIteration.__init__, ("absorption", "absorption_lr")), (optim.optimize_photometric, ("absorption", "absorption_lr")),
                      (captured_data.SyntheticPhotoData.__init__, ("absorption",)), (diffrender.Scene.image_loss_views_fused, ("absorption", "want_images")),
                      (diffrender.enqueue_image_views_term, ("absorption", "grad_sigma_ptr", "images_ptr"))):
        p = inspect.signature(fn).parameters
        assert all(n in p for n in names)
        assert p["absorption"].default is None
    assert inspect.signature(optim.PhotoIteration.__init__).parameters["absorption_lr"].default == 0.0
    assert inspect.signature(diffrender.Scene.image_loss_views_fused).parameters["want_images"].default is False
    assert "image_loss_views_fused(absorption=" in captured_data.SyntheticPhotoData.__doc__ and "want_images=True" in captured_data.SyntheticPhotoData.__doc__


def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    sig = _lib.SIGNATURES[WHO][1]
    assert len(sig) == 34 and sig[:25] == _lib.SIGNATURES["drt_render_image_loss_views"][1][:25]
    assert sig[25:27] == _lib.SIGNATURES["drt_render_image_loss_absorb"][1][27:29] and sig[27:32] == _lib.SIGNATURES["drt_render_image_loss_views_env"][1][25:30]
    assert len(_lib.SIGNATURES["drt_render_image_loss_views"][1]) == 26 and len(_lib.SIGNATURES["drt_render_image_loss_views_env"][1]) == 31
    assert "drt_image_views_absorb.hip" in build.UNITS
    assert f"int {WHO}(" in open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    unit = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_views_absorb.hip")).read()
    code = "\n".join(line for line in unit.splitlines() if not line.lstrip().startswith("//"))
    assert f"int {WHO}(" in code and "image_start_views" in code and "k_image_start" not in code and "ImageOneView" not in code
    assert "absorb_sigma_check" in code and "env_args_check" in code and "grow_doubles" in code and "reflection_pass" not in code        # (env_loss_run's)
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, WHO)
    assert getattr(lib, WHO)(*([None] * 4), 2, 0, 8, 1, 1.5, 1.0, 2, 0, 1, None, 4, 4, 3, *([None] * 11), 4, 8, None, 0, None, None) != 0
    assert lib.drt_last_error()


# ---- which native call an ``absorption`` makes ----------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        def call(*args):
            self.calls.append((fn, args))
            return 0
        return call


class _Ptr:
    def __init__(self, p, shape=()):
        self.p, self.shape = p, shape

    def data_ptr(self):
        return self.p


def _enqueue(monkeypatch, binding, texture, **kw):
    from drt_amd import _lib, diffrender
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(diffrender, "_stream", lambda: 77)
    scene = type("S", (), {"optix_mesh": type("M", (), {"_h": 11})()})()
    void, invalid = np.zeros(3), np.ones(3)
    diffrender.enqueue_image_views_term(scene, _Ptr(21), binding, [1, 0], texture, (6, "reflect", "snell"), 2, True, void, invalid, (1.5, 1.0), 31, 32, 33, 34,
                                        bands=[(0, 5), (5, 16)], **kw)
    return rec.calls, void, invalid


ROT = np.ascontiguousarray(np.eye(3).reshape(-1))
HEAD = (2, 5, 16, 2, 1.5, 1.0, 6, 3, 1)


def _bindings():
    plain = type("B", (), {"_h": 41, "height": 8, "targets": _Ptr(51), "weights": None})()
    room = type("B", (), {"_h": 41, "height": 8, "targets": _Ptr(51), "weights": _Ptr(52), "env": _Ptr(71, (16, 32, 3)), "env_rot": ROT})()
    return plain, room


def test_absorption_none_makes_the_calls_of_before(monkeypatch):
    plain, room = _bindings()
    calls, void, invalid = _enqueue(monkeypatch, plain, _Ptr(61, (4, 5, 3)), absorption=None, grad_sigma_ptr=None, images_ptr=None)
    assert [c[0] for c in calls] == ["drt_render_image_loss_views"] * 2
    assert len(calls[1][1]) == 26 and calls[1][1][4:] == HEAD + (61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, None, 31, 32, 33, 34, 77)
    calls, void, invalid = _enqueue(monkeypatch, room, _Ptr(61, (4, 5, 3)), reflection=True, absorption=None)
    assert [c[0] for c in calls] == ["drt_render_image_loss_views_env"] * 2
    assert len(calls[1][1]) == 31 and calls[1][1][4:] == HEAD + (61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, 52, 31, 32, 33, 34, 71, 16, 32,
                                                                ROT.ctypes.data, 1, 77)


def test_an_absorption_makes_the_new_call(monkeypatch):
    plain, room = _bindings()
    sigma = np.array([0.1, 0.2, 0.3])
    calls, void, invalid = _enqueue(monkeypatch, room, _Ptr(61, (4, 5, 3)), reflection=True, absorption=sigma, grad_sigma_ptr=35, images_ptr=36)
    assert [c[0] for c in calls] == [WHO] * 2 and list(calls[0][1][3]) == [1, 0] and calls[0][1][:3] == (11, 21, 41) and calls[0][1][5:7] == (0, 5)
    assert len(calls[1][1]) == 34 and calls[1][1][4:] == HEAD + (61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, 52, 31, 32, 33, 34, sigma.ctypes.data, 35,
                                                                71, 16, 32, ROT.ctypes.data, 1, 36, 77)
    calls, void, invalid = _enqueue(monkeypatch, plain, _Ptr(61, (4, 5, 3)), absorption=sigma)          # screens only: no environment, no reflection
    assert [c[0] for c in calls] == [WHO] * 2
    assert calls[1][1][4:] == HEAD + (61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, None, 31, 32, 33, 34, sigma.ctypes.data, None, None, 0, 0, None, 0, None, 77)
    calls, _, _ = _enqueue(monkeypatch, room, None, absorption=sigma)                                   # the room without screens
    assert calls[0][1][13:17] == (None, 0, 0, 3) and calls[0][1][27:32] == (71, 16, 32, ROT.ctypes.data, 0)
