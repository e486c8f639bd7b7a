"""GPU: absorbing glass -- Scene.render_image and Scene.image_loss_fused with ``absorption`` (drt_render_image_absorb,
drt_render_image_loss_absorb; drt_amd/csrc/drt_image_absorb.hip) -- against the float64 restatement tests/image_absorb_ref.py and torch
autograd of it, on the small views of tests/image_cases.py at sigma = (0.004, 0.012, 0.03) / (0.012,) (tests/image_absorb_cases.py).

Tolerances.  The image, off the sensitive pixels of image_cases (mask and cap as they are: absorption moves no exit ray):
image_cases.tolerance plus sigma_max (max_bounces - 1) 2 RAY_ABS (1 + 1 / GRAZING) for the end points of the interior segments
(image_absorb_cases.image_tolerance), about a thousand times below the float32 store.  The loss: image_loss_cases.LOSS_REL; the four
gradients: image_loss_cases.close; the count: exact.  sigma = 0: the bits of the clear call in deterministic mode.  The fit's achieved
error is printed and recorded in DESIGN.md 10.7 as a measurement; the assertions are those of the issue: the loss falls and every
coefficient ends nearer the truth than it began."""
import numpy as np
import pytest
import torch

import image_absorb_cases as cases
import image_absorb_ref
import image_cases
import image_loss_cases
from conftest import IOR
from drt_amd import _lib, calibrate, det, diffrender as Render, render, views

pytestmark = pytest.mark.gpu
EXT = cases.EXT
LAWS = cases.LAWS
LOSS_REL = image_loss_cases.LOSS_REL
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
BAND_REL = 1e-12             # float64 mode: bands against the single band (another order of the same atomics)
close = image_loss_cases.close


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR)
    Render.intIOR, Render.extIOR = IOR, EXT
    yield
    Render.intIOR, Render.extIOR = saved


@pytest.fixture
def deterministic():
    was = det.enable(True)
    yield
    det.enable(was)


def _fresh():
    scene = Render.Scene(image_cases.hand(), 0)
    scene.update_verticex(torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True))
    return scene


@pytest.fixture(scope="module")
def hand_scene():
    return _fresh()


def _law_kw(sc, law, fresnel=True):
    return dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=fresnel, void=sc["void"], invalid=sc["invalid"])


def _call(scene, name, law=LAWS[0], fresnel=True, sigma="case", grads=True, scale=None, **kw):
    """dict(loss, grad_V, g_int, g_ext, g_sigma, count[, image]) of one call on a scene of image_cases; sigma None: the clear call."""
    sc = image_cases.scene(name)
    args = _law_kw(sc, law, fresnel)
    args.update(kw)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
    sg = None
    if sigma is not None:
        sg = torch.tensor(cases.sigma(name) if isinstance(sigma, str) else np.broadcast_to(np.asarray(sigma, np.float64), cases.sigma(name).shape).copy(),
                          dtype=torch.float64, requires_grad=True)
        args["absorption"] = sg
    out = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], image_loss_cases.target(name, law, fresnel),
                                 ior_int=ii, ior_ext=ie, **args)
    loss, image = out if args.get("want_image") else (out, None)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), image=image, grad_V=None, g_sigma=None)
    if grads:
        wrt = ([scene.vertices] if args.get("vertices", True) else []) + [ii, ie] + ([sg] if sg is not None else [])
        g = [t.clone() for t in torch.autograd.grad(loss if scale is None else loss * scale, wrt)]
        if args.get("vertices", True):
            res["grad_V"] = g.pop(0)
        res["g_int"], res["g_ext"] = g[0], g[1]
        if sg is not None:
            res["g_sigma"] = g[2]
            assert g[2].device.type == "cpu" and g[2].shape == sg.shape and g[2].dtype == torch.float64
    return res


def _check_against(got, ref):
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; g_int {float(got['g_int']):.9e} / {ref['g_int']:.9e}, "
          f"g_ext {float(got['g_ext']):.9e} / {ref['g_ext']:.9e}, g_sigma {got['g_sigma'].numpy()} / {ref['g_sigma']}, max |grad_V| "
          f"{np.abs(ref['grad_V']).max():.3e} differs by {np.abs(got['grad_V'].cpu().numpy() - ref['grad_V']).max():.2e}; count {got['count']} / {ref['count']}")
    assert got["count"] == ref["count"]
    assert rel <= LOSS_REL
    assert close(got["grad_V"].cpu().numpy(), ref["grad_V"])
    assert close(float(got["g_int"]), ref["g_int"]) and close(float(got["g_ext"]), ref["g_ext"])
    assert close(got["g_sigma"].numpy(), ref["g_sigma"])


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_image_against_the_restatement(hand_scene, name, law, fresnel):
    sc = image_cases.scene(name)
    fwd = cases.reference(name, law, fresnel)["fwd"]
    base = image_cases.reference(name, law, fresnel)
    want = fwd["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1)
    image, hit, through, length = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], want_planes=True,
                                                          absorption=cases.sigma(name), **_law_kw(sc, law, fresnel))
    assert image.dtype == length.dtype == torch.float32 and image.shape == want.shape and length.shape == image.shape[:2]
    assert torch.equal(hit.cpu(), base["hit"]) and torch.equal(through.cpu(), base["through"])
    bad = image_cases.sensitive(name, base)
    tol = cases.image_tolerance(name, base, law)
    diff = (image.cpu().double() - want.double()).abs().amax(2).numpy()
    want_len = image_absorb_ref.length_plane(fwd, sc["height"], sc["width"], sc["s"])
    len_diff = (length.cpu().double() - want_len.double()).abs().max()
    print(name, law, "fresnel" if fresnel else "geometry", "sensitive pixels", int(bad.sum()), "of", bad.size, "tol", tol, "max diff", diff[~bad].max(),
          "length plane differs by", float(len_diff), "of", float(want_len.max()))
    assert bad.mean() <= image_cases.SENSITIVE_CAP
    assert np.isfinite(diff).all() and diff[~bad].max() <= tol
    assert float((image.cpu().double() - base["image"].double()).abs().max()) > 0.05          # the glass IS darker than the clear one
    # the plane: the float32 store of a length (half a unit in the last place of the largest), whose segments' end points are off by
    # RAY_ABS (1 + 1 / GRAZING) each -- 2e-8 for five segments, taken as 1e-7
    assert want_len.max() > 10 and len_diff <= 2.0 ** -24 * float(want_len.max()) + 1e-7
    assert not length.cpu()[through.cpu() == 0].any()


@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_loss_and_all_four_gradients_against_the_restatement(hand_scene, name, law, fresnel):
    ref = cases.reference(name, law, fresnel)
    got = _call(hand_scene, name, law, fresnel)
    if (name, law) in image_loss_cases.COUNTS:
        assert got["count"] == image_loss_cases.COUNTS[(name, law)]
    _check_against(got, ref)


# ------------------------------------------------------------------------------------------------------------------------- sigma = 0
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_sigma_zero_gives_the_bits_of_the_clear_calls(hand_scene, deterministic, law):
    for name in ("v5", "wide"):
        sc = image_cases.scene(name)
        pos = (sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"])
        clear_image = hand_scene.render_image(*pos, **_law_kw(sc, law))
        assert torch.equal(hand_scene.render_image(*pos, absorption=0.0, **_law_kw(sc, law)), clear_image)
        clear, zero = _call(hand_scene, name, law, sigma=None, want_image=True), _call(hand_scene, name, law, sigma=0.0, want_image=True)
        assert clear["count"] == zero["count"] > 0 and torch.equal(zero["image"], clear_image)
        for k in ("loss", "grad_V", "g_int", "g_ext", "image"):
            assert torch.equal(clear[k], zero[k]), k
        assert zero["g_sigma"].all()


def test_sigma_zero_agrees_with_the_clear_call_in_float64_mode(hand_scene):
    assert not det.on()
    clear, zero = _call(hand_scene, "v41", LAWS[2], sigma=None), _call(hand_scene, "v41", LAWS[2], sigma=0.0)
    assert clear["count"] == zero["count"] and abs(float(clear["loss"]) - float(zero["loss"])) <= LOSS_REL * float(clear["loss"])
    assert close(zero["grad_V"].cpu().numpy(), clear["grad_V"].cpu().numpy())
    assert close(float(zero["g_int"]), float(clear["g_int"])) and close(float(zero["g_ext"]), float(clear["g_ext"]))


# ------------------------------------------------------------------------------------------------------------------ bands, repeats, modes
def _small_view(scene, height=7, width=5, s=3, channels=1, **kw):
    """A view of the hand against a random target: (loss, grad_V, g_int, g_ext, g_sigma) and the image with want_image."""
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, height, width)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    target = np.random.default_rng(3).random((height, width, channels), dtype=np.float32)[:, :, 0 if channels == 1 else slice(None)]
    ii = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
    sg = torch.tensor((cases.SIGMA1 if channels == 1 else cases.SIGMA3), dtype=torch.float64, device="cuda", requires_grad=True)
    out = scene.image_loss_fused(cam, height, width, screen, image_cases.texture(channels), np.ascontiguousarray(target), ior_int=ii, ior_ext=ie, supersample=s,
                                 max_bounces=6, tir="reflect", refraction="snell", void=0.25, invalid=0.75, absorption=sg, **kw)
    loss, image = (out[0], (out[1],)) if kw.get("want_image") else (out, ())
    return (loss.detach().clone(),) + tuple(g.clone() for g in torch.autograd.grad(loss, [scene.vertices, ii, ie, sg])) + image


def _banded(scene):
    """7 x 5 at s = 3 whole and in single rows of 45 samples; 32 x 32 at s = 2 (C = 3) whole and in bands of nine rows, the last of five."""
    assert render.plan_bands(7, 5, 3, 45) == [(y, y + 1) for y in range(7)]
    yield _small_view(scene), _small_view(scene, max_samples=45)
    yield _small_view(scene, 32, 32, 2, 3), _small_view(scene, 32, 32, 2, 3, max_samples=9 * 128 + 5)


def test_bands_give_the_bits_of_the_single_band_in_deterministic_mode(hand_scene, deterministic):
    for whole, banded in _banded(hand_scene):
        assert float(whole[0]) > 0 and whole[1].abs().max() > 0 and whole[2] != 0 and whole[4].all()
        for a, b in zip(whole, banded):
            assert torch.equal(a, b)


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    assert not det.on()
    for whole, banded in _banded(hand_scene):
        for a, b in zip(whole, banded):
            assert (a - b).abs().max() <= BAND_REL * a.abs().max()


def test_two_deterministic_runs_give_the_same_bits(hand_scene, deterministic):
    a = _call(hand_scene, "v41", LAWS[2])
    b = _call(hand_scene, "v41", LAWS[2])
    for k in ("loss", "grad_V", "g_int", "g_ext", "g_sigma"):
        assert torch.equal(a[k], b[k])
    _check_against(a, cases.reference("v41", LAWS[2], True))


def test_without_vertices_the_loss_the_ior_and_the_sigma_partials_are_the_same(hand_scene, deterministic):
    full = _call(hand_scene, "wide", LAWS[1])
    fixed = _call(hand_scene, "wide", LAWS[1], vertices=False)
    assert fixed["grad_V"] is None and fixed["count"] == full["count"]
    for k in ("loss", "g_int", "g_ext", "g_sigma"):
        assert torch.equal(full[k], fixed[k])
    assert full["g_sigma"].all()


def test_backward_scales_the_gradients(hand_scene, deterministic):
    one = _call(hand_scene, "v5", LAWS[0])
    three = _call(hand_scene, "v5", LAWS[0], scale=3.0)
    for k in ("grad_V", "g_int", "g_ext", "g_sigma"):
        assert torch.equal(three[k], one[k] * 3.0)


def test_a_scene_without_faces_gives_the_direct_loss_and_a_zero_sigma_gradient(deterministic):
    scene = _fresh()
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    got = _call(scene, "v5", LAWS[2])
    clear = _call(scene, "v5", LAWS[2], sigma=None)
    assert float(got["loss"]) > 0 and torch.equal(got["loss"], clear["loss"])          # every sample is direct: L = 0, A = 1
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0 and not got["g_sigma"].any()


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    scene = _fresh()
    V = scene.vertices
    sc = image_cases.scene("v5")
    tex, tgt = torch.as_tensor(sc["texture"]).cuda(), torch.as_tensor(image_loss_cases.target("v5", LAWS[1], True)).cuda()
    kw = dict(supersample=sc["s"], max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"], absorption=cases.SIGMA3)

    def step():
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, **kw)
        return loss.detach(), torch.autograd.grad(loss, V)[0]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and eager[1].abs().max() > 0
    for a, b in zip(eager, static):
        assert torch.equal(a, b)
    # a workspace that would have to grow inside a capture is refused with a message
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="eagerly before capturing"):
        with torch.cuda.graph(g2):
            scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, **dict(kw, supersample=4))
    torch.cuda.synchronize()


def test_growth_of_the_lengths_alone_inside_a_capture_is_refused(deterministic):
    """A clear call has sized everything but the lengths: the absorbing call of the same size must still refuse to allocate them."""
    scene = _fresh()
    sc = image_cases.scene("v5")
    tex, tgt = torch.as_tensor(sc["texture"]).cuda(), torch.as_tensor(image_loss_cases.target("v5", LAWS[1], True)).cuda()
    kw = dict(supersample=sc["s"], max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"])
    scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="eagerly before capturing"):
        with torch.cuda.graph(g):
            scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, absorption=0.01, **kw)
    torch.cuda.synchronize()


def test_the_workspace_is_shared_with_the_clear_loss_and_the_path_loss(deterministic):
    """On one scene: the absorbing loss, the clear loss, the one-pass path loss (which shares the lists, the rows and the tape) and the
    absorbing loss again, at sizes that grow and shrink -- every result is that of the same call on a scene built for it alone."""
    center, _ = image_cases.frame()
    cam = image_cases.camera(5, 24, 20)
    o, d = (t.cuda() for t in views.generate_ray(24, 20, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((24 * 20, 3)) * 40.0 + np.asarray(center) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(24 * 20) > 0.1, device="cuda")

    def paths(scene):
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    def clear(scene):
        r = _call(scene, "v5", LAWS[2], sigma=None)
        return r["loss"], r["grad_V"], r["g_int"], r["g_ext"]

    steps = [lambda sc: _small_view(sc, 16, 16, 2, 3, want_image=True), clear, paths, lambda sc: _small_view(sc, 24, 20, 1, 3, want_image=True),
             lambda sc: _small_view(sc, 16, 16, 2, 3, want_image=True)]
    scene = _fresh()
    got = [step(scene) for step in steps]
    assert float(got[0][0]) > 0 and got[0][1].any() and got[0][4].all() and float(got[2][0]) > 0 and got[2][1].any()
    for step, mine in zip(steps, got):
        alone = step(_fresh())
        assert len(alone) == len(mine)
        for a, b in zip(alone, mine):
            assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_outputs_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_absorb") and hasattr(lib, "drt_render_image_loss_absorb")
    sc = image_cases.scene("v5")
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, 16, 16)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    a = render.check_image_loss_args(cam, 16, 16, screen, sc["texture"], np.zeros((16, 16, 3), np.float32), supersample=2)
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    loss = torch.zeros((), dtype=torch.float64, device="cuda")
    grad, ior, gsig = torch.zeros_like(V), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    image = torch.full((16, 16, 3), 7.0, dtype=torch.float32, device="cuda")
    length = torch.full((16, 16), 7.0, dtype=torch.float32, device="cuda")
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    good = np.array(cases.SIGMA3)
    base = dict(height=16, y0=0, y1=16, s=2, max_bounces=4, channels=3, target=tgt.data_ptr(), sigma=good)
    stream = torch.cuda.current_stream().cuda_stream

    def call_loss(**kw):
        p = dict(base, **kw)
        return lib.drt_render_image_loss_absorb(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, p["height"], 16, p["y0"], p["y1"], p["s"], IOR, EXT,
                                                p["max_bounces"], 3, 1, a["screen"].ctypes.data, tex.data_ptr(), tex.shape[0], tex.shape[1], p["channels"],
                                                a["void"].ctypes.data, a["invalid"].ctypes.data, p["target"], None, loss.data_ptr(), grad.data_ptr(),
                                                ior.data_ptr(), image.data_ptr(), count.data_ptr(), None if p["sigma"] is None else p["sigma"].ctypes.data,
                                                gsig.data_ptr(), stream)

    def call_image(**kw):
        p = dict(base, **kw)
        return lib.drt_render_image_absorb(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, p["height"], 16, p["y0"], p["y1"], p["s"], IOR, EXT,
                                           p["max_bounces"], 3, 1, a["screen"].ctypes.data, tex.data_ptr(), tex.shape[0], tex.shape[1], p["channels"],
                                           a["void"].ctypes.data, a["invalid"].ctypes.data, image.data_ptr(), None, None,
                                           None if p["sigma"] is None else p["sigma"].ctypes.data, length.data_ptr(), stream)

    was = det.enable(False)
    try:
        bad_sigmas = [None, np.array([0.1, -1e-300, 0.1]), np.array([np.nan, 0.1, 0.1]), np.array([0.1, 0.1, np.inf])]
        for kw in [dict(s=0), dict(channels=2), dict(max_bounces=9), dict(y0=5, y1=5), dict(height=0, y1=0)] + [dict(sigma=sg) for sg in bad_sigmas]:
            for call in (call_loss, call_image):
                assert call(**kw) == -1, kw                        # DRT_E_INVALID
                assert lib.drt_last_error()
        assert call_loss(target=None) == -1
        assert call_loss(sigma=bad_sigmas[1]) == -1 and b"sigma[1]" in lib.drt_last_error()          # the entry is named
        assert call_image(sigma=bad_sigmas[3]) == -1 and b"sigma[2]" in lib.drt_last_error()
        torch.cuda.synchronize()
        assert float(loss) == 0 and not grad.any() and not ior.any() and not gsig.any() and (image == 7).all() and (length == 7).all() and int(count) == 0
        assert call_image(y0=3, y1=9) == 0                         # the good calls write their band, and add into their targets
        torch.cuda.synchronize()
        assert (image[:3] == 7).all() and (image[9:] == 7).all() and (image[3:9] != 7).all() and (length[:3] == 7).all() and (length[3:9] != 7).all()
        rendered = image.clone()
        assert call_loss(y0=3, y1=9) == 0
        torch.cuda.synchronize()
        assert float(loss) > 0 and grad.any() and ior.all() and gsig.all() and int(count) > 0 and torch.equal(image, rendered)
        first = (loss.clone(), grad.clone(), ior.clone(), gsig.clone(), count.clone())
        assert call_loss(y0=3, y1=9) == 0                          # ... and a second one adds again
        torch.cuda.synchronize()
        assert int(count) == 2 * int(first[4]) and float(loss) == pytest.approx(2 * float(first[0]), rel=1e-12)
        for now, once in ((grad, first[1]), (ior, first[2]), (gsig, first[3])):
            assert (now - 2 * once).abs().max() <= 1e-12 * once.abs().max()
    finally:
        det.enable(was)


# ------------------------------------------------------------------------------------------------------------------------------ a fit
def test_fit_absorption_moves_every_coefficient_towards_the_truth(hand_scene):
    """The target is v5 rendered at SIGMA3 with the mesh and the IOR fixed; Adam from 0.  Asserted: the loss ends below its start and
    every coefficient ends nearer the truth than it began.  The achieved error is printed (DESIGN.md 10.7 records it)."""
    sc = image_cases.scene("v5")
    law = LAWS[2]
    kw = _law_kw(sc, law)
    truth = np.array(cases.SIGMA3)
    photo = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], absorption=truth, **kw)
    sigma, history = calibrate.fit_absorption(hand_scene, [(sc["camera_M"], photo)], sc["screen"], sc["texture"], steps=60, lr=0.001, **kw)
    print("fit_absorption: loss", history[0], "->", min(history), "sigma", sigma, "truth", truth, "relative error", np.abs(sigma - truth) / truth)
    assert len(history) == 60 and min(history) < history[0] and history[-1] < history[0]
    assert (sigma >= 0).all() and (np.abs(sigma - truth) < np.abs(0.0 - truth)).all()
