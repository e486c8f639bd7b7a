"""GPU: Scene.image_loss_fused -- the photometric loss of the refracted image with its vertex and IOR gradients (drt_render_image_loss,
drt_amd/csrc/drt_image_loss.hip) -- against torch autograd of the float64 restatement tests/image_loss_ref.py on the small views of
data/hand_vh.ply of tests/image_cases.py (targets rendered at IOR 1.55, evaluated at conftest.IOR: tests/image_loss_cases.py).

Tolerances are those of tests/test_image_loss_host.py, where they are derived: the loss LOSS_REL (ten times the measured difference of the
host build, 3e-14, far below 1e-10), the gradients the project's 1e-9 of the largest entry and 1e-5 absolute.  The number of samples that
carry a gradient is exact."""
import numpy as np
import pytest
import torch

import image_cases
import image_loss_cases as cases
import image_loss_ref
from conftest import IOR
from drt_amd import _lib, det, diffrender as Render, render, views

pytestmark = pytest.mark.gpu
EXT = cases.EXT
LAWS = cases.LAWS
LOSS_REL = cases.LOSS_REL
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
BAND_REL = 1e-12             # float64 mode: bands against the single band (another order of the same atomics)


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


@pytest.fixture(scope="module")
def hand_scene():
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene


def _call(scene, name, law=LAWS[0], fresnel=True, target=None, ior=True, grads=True, scale=None, **kw):
    """dict(loss, grad_V, g_int, g_ext, count[, image]) of one call on a scene of image_cases, as host values."""
    sc = image_cases.scene(name)
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=fresnel, void=sc["void"], invalid=sc["invalid"])
    args.update(kw)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True) if ior else None
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True) if ior else None
    out = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target(name, law, fresnel) if target is None else target,
                                 ior_int=ii, ior_ext=ie, **args)
    loss, image = out if args.get("want_image") else (out, None)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), image=image)
    if grads:
        wrt = [scene.vertices] if args.get("vertices", True) else []
        wrt += [ii, ie] if ior else []
        g = list(torch.autograd.grad(loss if scale is None else loss * scale, wrt))
        res["grad_V"] = g.pop(0).clone() if args.get("vertices", True) else None
        if ior:
            res["g_int"], res["g_ext"] = g[0].clone(), g[1].clone()
            assert g[0].device.type == "cpu" and g[1].device.type == "cuda" and g[0].shape == g[1].shape == ()
    return res


def _check_against(got, ref):
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; g_int {float(got['g_int']):.9e} / {ref['g_int']:.9e}, "
          f"g_ext {float(got['g_ext']):.9e} / {ref['g_ext']:.9e}, max |grad_V| {np.abs(ref['grad_V']).max():.3e} differs by "
          f"{np.abs(got['grad_V'].cpu().numpy() - ref['grad_V']).max():.2e}; count {got['count']} / {ref['count']}")
    assert got["count"] == ref["count"]
    assert rel <= LOSS_REL
    assert cases.close(got["grad_V"].cpu().numpy(), ref["grad_V"])
    assert cases.close(float(got["g_int"]), ref["g_int"]) and cases.close(float(got["g_ext"]), ref["g_ext"])


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_loss_and_gradients_against_the_restatement(hand_scene, name, law, fresnel):
    ref = cases.reference(name, law, fresnel)
    got = _call(hand_scene, name, law, fresnel)
    if (name, law) in cases.COUNTS:
        assert got["count"] == cases.COUNTS[(name, law)]
    _check_against(got, ref)


@pytest.mark.parametrize("name", ["v5", "wide"])
def test_a_zero_weight_removes_exactly_those_pixels(hand_scene, name):
    ref = cases.reference(name, LAWS[0], True, weighted=True)
    w = cases.half_weight(name)
    got = _call(hand_scene, name, weight=w)
    _check_against(got, ref)                                   # (the count is of samples, weighted or not)
    again = _call(hand_scene, name, weight=torch.as_tensor(w).cuda())
    assert abs(float(again["loss"]) - float(got["loss"])) <= BAND_REL * float(got["loss"])


def test_want_image_gives_the_bits_of_render_image(hand_scene):
    for name, law in (("v5", LAWS[2]), ("wide", LAWS[1])):
        sc = image_cases.scene(name)
        got = _call(hand_scene, name, law, grads=False, want_image=True, max_samples=9 * sc["width"] * sc["s"] ** 2)
        image = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], supersample=sc["s"], max_bounces=law[0], tir=law[1],
                                        refraction=law[2], void=sc["void"], invalid=sc["invalid"])
        assert got["image"].dtype == torch.float32 and torch.equal(got["image"], image)


def test_the_calls_own_image_as_target_gives_a_loss_of_rounding_only(hand_scene):
    """A pixel's residual is then the rounding of its float32 store, at most 2^-24 of a value below 2: loss <= H W C 2^-46."""
    first = _call(hand_scene, "v5", LAWS[2], grads=False, want_image=True)
    again = _call(hand_scene, "v5", LAWS[2], target=first["image"], grads=False)
    assert 0.0 <= float(again["loss"]) <= first["image"].numel() * 2.0 ** -46
    as_bytes = _call(hand_scene, "v5", LAWS[2], target=torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda"), grads=False)
    zeros = _call(hand_scene, "v5", LAWS[2], target=np.zeros((32, 32, 3), np.float32), grads=False)
    assert float(as_bytes["loss"]) == pytest.approx(float(zeros["loss"]), rel=BAND_REL) and float(zeros["loss"]) > 1


# ------------------------------------------------------------------------------------------------------------------ bands, repeats, modes
def _small_view(scene, height, width, s, channels, **kw):
    """A view of the hand against a random target: (loss, grad_V, g_int, g_ext) on the device, and the image behind them with want_image."""
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, height, width)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    target = np.random.default_rng(3).random((height, width, channels), dtype=np.float32)[:, :, 0 if channels == 1 else slice(None)]
    ii = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
    out = scene.image_loss_fused(cam, height, width, screen, image_cases.texture(channels), np.ascontiguousarray(target), ior_int=ii, ior_ext=ie, supersample=s, max_bounces=6,
                                 tir="reflect", refraction="snell", void=0.25, invalid=0.75, **kw)
    loss, image = (out[0], (out[1],)) if kw.get("want_image") else (out, ())
    return (loss.detach().clone(),) + tuple(g.clone() for g in torch.autograd.grad(loss, [scene.vertices, ii, ie])) + image


def _banded_cases(scene):
    """(whole, banded) result pairs: 32 x 32 at s = 2 in bands of nine rows (four bands, the last of 5 rows = 640 samples), 7 x 5 at s = 3
    (C = 1, a [H, W] target) in bands of two rows (the last a single row of 45 samples), 9 x 40 at s = 1 in single rows of 40 samples, each over the cap."""
    assert render.plan_bands(32, 32, 2, 9 * 128 + 5) == [(0, 9), (9, 18), (18, 27), (27, 32)] and (5 * 128) % 256 != 0
    assert len(render.plan_bands(7, 5, 3, 100)) == 4 and len(render.plan_bands(9, 40, 1, 39)) == 9
    for height, width, s, channels, cap in ((32, 32, 2, 3, 9 * 128 + 5), (7, 5, 3, 1, 100), (9, 40, 1, 1, 39)):
        yield _small_view(scene, height, width, s, channels), _small_view(scene, height, width, s, channels, max_samples=cap)


def test_bands_give_the_bits_of_the_single_band_in_deterministic_mode(hand_scene, deterministic):
    for whole, banded in _banded_cases(hand_scene):
        assert float(whole[0]) > 0 and whole[1].abs().max() > 0 and whole[2] != 0
        for a, b in zip(whole, banded):
            assert torch.equal(a, b)


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    assert not det.on()
    for whole, banded in _banded_cases(hand_scene):
        for a, b in zip(whole, banded):
            assert (a - b).abs().max() <= BAND_REL * a.abs().max()


def test_two_deterministic_runs_give_the_same_bits(hand_scene, deterministic):
    a = _call(hand_scene, "v41", LAWS[2])
    b = _call(hand_scene, "v41", LAWS[2])
    for k in ("loss", "grad_V", "g_int", "g_ext"):
        assert torch.equal(a[k], b[k])
    _check_against(a, cases.reference("v41", LAWS[2], True))


def test_without_vertices_the_loss_and_the_ior_partials_are_the_same(hand_scene, deterministic):
    full = _call(hand_scene, "wide", LAWS[1])
    fixed = _call(hand_scene, "wide", LAWS[1], vertices=False)
    assert fixed["grad_V"] is None and fixed["count"] == full["count"]
    for k in ("loss", "g_int", "g_ext"):
        assert torch.equal(full[k], fixed[k])
    sc = image_cases.scene("wide")
    loss = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("wide", LAWS[1], True), vertices=False,
                                       supersample=sc["s"], max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"])
    assert not loss.requires_grad and torch.equal(loss, full["loss"])          # float IORs from the module, a fixed mesh: nothing to differentiate


def test_backward_scales_the_gradients(hand_scene, deterministic):
    one = _call(hand_scene, "v5", LAWS[0])
    three = _call(hand_scene, "v5", LAWS[0], scale=3.0)
    for k in ("grad_V", "g_int", "g_ext"):
        assert torch.equal(three[k], one[k] * 3.0)


def test_a_scene_without_faces_gives_the_loss_of_the_direct_image_and_zero_gradients():
    sc = image_cases.scene("v5")
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    got = _call(scene, "v5", LAWS[2])
    fwd = image_loss_ref.forward(np.zeros((0, 3), np.int64), np.zeros((0, 3)), sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], sc["s"],
                                 LAWS[2], True, sc["void"], sc["invalid"], IOR, EXT)
    want = float(image_loss_ref.loss_of(fwd["mean"], cases.target("v5", LAWS[2], True)))
    assert want > 0 and abs(float(got["loss"]) - want) <= LOSS_REL * want
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    sc = image_cases.scene("v5")
    tex, tgt = torch.as_tensor(sc["texture"]).cuda(), torch.as_tensor(cases.target("v5", LAWS[1], True)).cuda()

    def step():
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, supersample=sc["s"], max_bounces=6, tir="reflect",
                                      void=sc["void"], invalid=sc["invalid"])
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
            scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, supersample=4, void=sc["void"], invalid=sc["invalid"])
    torch.cuda.synchronize()


def test_calls_of_growing_and_shrinking_size_on_one_scene_give_the_bits_of_a_fresh_scene(deterministic):
    """render_image and image_loss_fused grow one workspace (ray lists, parked rows and tape, throughputs; the loss also its pixel seeds):
    render_image sizes it for 1 024 samples of 256 pixels; the loss of 480 samples finds all of that large enough and allocates only its
    seeds, for 480 pixels; then the first size again, as an image and as a loss whose seeds are now more than it needs.  Every result is
    that of the same call on a scene built for it alone, and the one-pass path call, which shares the lists, the rows and the tape the loss
    has just written, is not disturbed."""
    mesh = image_cases.hand()
    center, extent = image_cases.frame()

    def fresh():
        scene = Render.Scene(mesh, 0)
        scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True))
        return scene

    def image(scene, height, width, s):
        cam = image_cases.camera(5, height, width)
        screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
        return scene.render_image(cam, height, width, screen, image_cases.texture(3), supersample=s, max_bounces=6, tir="reflect", refraction="snell", void=0.25,
                                  invalid=0.75, want_planes=True)

    cam = image_cases.camera(5, 24, 20)
    o, d = (t.cuda() for t in views.generate_ray(24, 20, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((24 * 20, 3)) * 40.0 + np.asarray(center) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(24 * 20) > 0.1, device="cuda")

    def paths(scene):
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    steps = [lambda sc: image(sc, 16, 16, 2),
             lambda sc: _small_view(sc, 24, 20, 1, 3, want_image=True),
             paths,
             lambda sc: image(sc, 16, 16, 2),
             lambda sc: _small_view(sc, 16, 16, 2, 3, want_image=True)]
    scene = fresh()
    got = [step(scene) for step in steps]
    assert got[0][1].max() > 0 and got[0][2].max() > 0                                    # the object is in the picture and light gets through it
    assert float(got[1][0]) > 0 and got[1][1].any() and got[1][2] != 0 and float(got[2][0]) > 0 and got[2][1].any()
    for step, mine in zip(steps, got):
        alone = step(fresh())
        assert len(alone) == len(mine)
        for a, b in zip(alone, mine):
            assert torch.equal(a, b)
    assert torch.equal(got[4][4], got[3][0])                                             # (and want_image is render_image at that size too)


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_outputs_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() >= 9
    sc = image_cases.scene("v5")
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, 16, 16)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    a = render.check_image_loss_args(cam, 16, 16, screen, sc["texture"], np.zeros((16, 16, 3), np.float32), supersample=2)
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    loss = torch.zeros((), dtype=torch.float64, device="cuda")
    grad, ior = torch.zeros_like(V), torch.zeros(2, dtype=torch.float64, device="cuda")
    image = torch.full((16, 16, 3), 7.0, dtype=torch.float32, device="cuda")
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    base = dict(height=16, width=16, y0=0, y1=16, s=2, max_bounces=4, law_flags=3, fresnel=1, channels=3, tex_h=tex.shape[0], target=tgt.data_ptr(),
                loss=loss.data_ptr())

    def call(**kw):
        p = dict(base, **kw)
        return lib.drt_render_image_loss(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, p["height"], p["width"], p["y0"], p["y1"], p["s"], IOR, EXT,
                                         p["max_bounces"], p["law_flags"], p["fresnel"], a["screen"].ctypes.data, tex.data_ptr(), p["tex_h"], tex.shape[1], p["channels"],
                                         a["void"].ctypes.data, a["invalid"].ctypes.data, p["target"], None, p["loss"], grad.data_ptr(), ior.data_ptr(),
                                         image.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)

    was = det.enable(False)
    try:
        for kw in (dict(s=0), dict(s=5), dict(channels=2), dict(tex_h=1), dict(max_bounces=1), dict(max_bounces=9), dict(law_flags=4), dict(fresnel=2),
                   dict(y0=5, y1=5), dict(y0=0, y1=17), dict(height=0, y1=0), dict(target=None), dict(loss=None)):
            assert call(**kw) == -1, kw                        # DRT_E_INVALID
            assert lib.drt_last_error()
        torch.cuda.synchronize()
        assert float(loss) == 0 and not grad.any() and not ior.any() and (image == 7).all() and int(count) == 0
        assert call(y0=3, y1=9) == 0                           # the good call adds into its targets and writes its band of the image
        torch.cuda.synchronize()
        assert float(loss) > 0 and grad.any() and ior.all() and int(count) > 0 and (image[:3] == 7).all() and (image[9:] == 7).all() and (image[3:9] != 7).all()
        first = (loss.clone(), grad.clone(), ior.clone(), count.clone())
        assert call(y0=3, y1=9) == 0                           # ... and a second one adds again
        torch.cuda.synchronize()
        assert int(count) == 2 * int(first[3]) and float(loss) == pytest.approx(2 * float(first[0]), rel=1e-12)
        assert (grad - 2 * first[1]).abs().max() <= 1e-12 * first[1].abs().max() and (ior - 2 * first[2]).abs().max() <= 1e-12 * first[2].abs().max()
    finally:
        det.enable(was)
