"""GPU: the camera gradient of Scene.image_loss_fused (camera_param; drt_render_image_loss_camera, drt_amd/csrc/drt_image_camera.hip)
against torch autograd of the float64 restatement tests/image_camera_ref.py, on the scenes `v5` and `wide` of tests/image_cases.py with
the targets of tests/image_loss_cases.py.

Tolerances are those of tests/test_image_camera_host.py: the loss LOSS_REL; the 21 partials in the three groups rinv[:, :3], rinv[:, 3]
and kinv, each with ``image_loss_cases.close`` (1e-9 of the group's largest entry, 1e-5 absolute).  In deterministic mode bands, runs and
a graph replay give the same bits.  The count the device returns is ``last_image_count``, the through samples that carried a gradient
(the entry point has no slot for the direct ones; the host test counts both)."""
import numpy as np
import pytest
import torch

import image_cases
import image_camera_ref as ref_mod
import image_loss_cases as cases
import image_ref
import image_screen_ref
from conftest import IOR
from drt_amd import _lib, calibrate, det, diffrender as Render, render

pytestmark = pytest.mark.gpu
EXT = cases.EXT
LAWS = ref_mod.LAWS
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


def _scene(faces=True):
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    if not faces:
        scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    return scene


@pytest.fixture(scope="module")
def hand_scene():
    return _scene()


def _call(scene, sc, target, law=LAWS[0], fresnel=True, camera=True, rows=4, ends=False, only_camera=False, **kw):
    """One call on a scene dict of image_cases (or one shaped like it), on the device.  ``camera``: the camera goes in as camera_param --
    Rinv a host tensor of ``rows`` rows, Kinv a device tensor -- and its gradient is taken; ``ends``: screen and texture go in as
    screen_param / texture_param too; ``only_camera``: vertices=False and plain IOR floats, so that nothing else is asked for."""
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=fresnel, void=sc["void"], invalid=sc["invalid"])
    args.update(kw)
    wrt, names = [], []
    if only_camera:
        args.update(vertices=False, ior_int=IOR, ior_ext=EXT)
    else:
        ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
        ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
        args.update(ior_int=ii, ior_ext=ie)
        wrt, names = [scene.vertices, ii, ie], ["grad_V", "g_int", "g_ext"]
    screen, texture, camera_M = sc["screen"], sc["texture"], sc["camera_M"]
    if ends:
        P = image_screen_ref.rows_of(screen).requires_grad_(True)
        T = torch.tensor(texture, dtype=torch.float64, device="cuda", requires_grad=True)
        args.update(screen_param=P, texture_param=T)
        wrt, names = wrt + [P, T], names + ["g_screen", "g_texture"]
        screen, texture = None, None
    if camera:
        Rinv, Kinv = ref_mod.camera_tensors(camera_M)
        Rinv, Kinv = Rinv[:rows].clone().requires_grad_(True), Kinv.cuda().requires_grad_(True)
        args.update(camera_param=(Rinv, Kinv))
        wrt, names = wrt + [Rinv, Kinv], names + ["g_rinv", "g_kinv"]
        camera_M = None
    loss = scene.image_loss_fused(camera_M, sc["height"], sc["width"], screen, texture, target, **args)
    g = [x.clone() for x in torch.autograd.grad(loss, wrt)]
    res = dict(zip(names, g), loss=loss.detach().clone(), count=int(scene.last_image_count))
    if camera:
        assert res["g_rinv"].device.type == "cpu" and res["g_rinv"].shape == (rows, 4) and res["g_rinv"].dtype == torch.float64
        assert res["g_kinv"].device.type == "cuda" and res["g_kinv"].shape == (3, 3) and res["g_kinv"].dtype == torch.float64
        if rows == 4:
            assert not res["g_rinv"][3].any()
    return res


def _case(scene, name, law=LAWS[0], fresnel=True, **kw):
    return _call(scene, image_cases.scene(name), cases.target(name, law, fresnel), law, fresnel, **kw)


def _check_against(got, ref):
    want = ref_mod.groups(ref["g_rinv"], ref["g_kinv"])
    have = ref_mod.groups(got["g_rinv"].numpy(), got["g_kinv"].cpu().numpy())
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} ({rel:.1e}); "
          + "; ".join(f"max |{k}| {np.abs(want[k]).max():.3e} differs by {np.abs(have[k] - want[k]).max():.2e}" for k in want))
    assert rel <= cases.LOSS_REL
    for k in want:
        assert np.abs(want[k]).max() > 0 and cases.close(have[k], want[k]), k


_OLD = ("loss", "grad_V", "g_int", "g_ext")
_ENDS = ("g_screen", "g_texture")
_CAM = ("g_rinv", "g_kinv")


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_camera_gradient_against_the_restatement(hand_scene, name, law, fresnel):
    """... with the screen, the texture, the vertices and both IORs differentiated in the same call; their gradients and the count are
    those of the call without camera_param (float64 mode: ``close``)."""
    ref = ref_mod.reference(name, law, fresnel)
    got = _case(hand_scene, name, law, fresnel, ends=True)
    _check_against(got, ref)
    assert got["count"] == ref["through_on"] == cases.reference(name, law, fresnel)["count"]
    plain = _case(hand_scene, name, law, fresnel, ends=True, camera=False)
    assert plain["count"] == got["count"]
    for k in _OLD[1:] + _ENDS:
        assert cases.close(got[k].cpu().numpy(), plain[k].cpu().numpy()), k
    assert abs(float(got["loss"]) - float(plain["loss"])) <= BAND_REL * float(plain["loss"])


@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_the_other_gradients_keep_their_bits_in_deterministic_mode(hand_scene, deterministic, name):
    got, plain = _case(hand_scene, name, LAWS[2], ends=True), _case(hand_scene, name, LAWS[2], ends=True, camera=False)
    for k in _OLD + _ENDS:
        assert torch.equal(got[k], plain[k]), k
    _check_against(got, ref_mod.reference(name, LAWS[2], True))


def test_without_the_keyword_the_call_is_the_parents(hand_scene, deterministic, monkeypatch):
    """The method's route without camera_param is the "plain" / "screen" term, as before; and the camera entry point with a null camera
    accumulator -- the "camera" term with nothing of the camera to track -- gives those routes' bits."""
    sc = image_cases.scene("v5")
    a = render.check_image_loss_args(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("v5", LAWS[1], True),
                                     supersample=sc["s"], max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"])
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")
    lib, entries = _lib.lib(), []
    for name in ("drt_render_image_loss", "drt_render_image_loss_screen", "drt_render_image_loss_camera"):
        monkeypatch.setattr(lib, name, lambda *args, name=name, fn=getattr(lib, name): entries.append(name) or fn(*args))
    for ends in (False, True):
        got = []
        del entries[:]
        old = "screen" if ends else "plain"
        for entry, extra in ((old, (None, None) if ends else ()), ("camera", (None, None, None, None))):
            ii = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
            T = torch.as_tensor(a["texture"], dtype=torch.float64, device="cuda").requires_grad_(True)
            if ends:
                extra = (None, T) + extra[2:]
            term = Render._image_term(hand_scene, a, (IOR, EXT), tex, tgt, None, entry)
            loss = Render._UnitSeedTerm.apply(term, hand_scene.vertices, ii, None, *extra)
            wrt = [hand_scene.vertices, ii] + ([T] if ends else [])
            got.append((loss.detach().clone(), term.count.clone()) + tuple(g.clone() for g in torch.autograd.grad(loss, wrt)))
        assert list(dict.fromkeys(entries)) == ["drt_render_image_loss" + ("_screen" if ends else ""), "drt_render_image_loss_camera"]      # two different native entry points
        assert float(got[0][0]) > 0 and got[0][2].any() and got[0][3] != 0
        for x, y in zip(*got):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ bands, repeats, modes
def _banded(scene, name, rows):
    """(single band, bands of ``rows`` image rows)."""
    sc = image_cases.scene(name)
    cap = rows * sc["width"] * sc["s"] ** 2 + 5
    n_bands = len(render.plan_bands(sc["height"], sc["width"], sc["s"], cap))
    return _case(scene, name, LAWS[2], ends=True), _case(scene, name, LAWS[2], ends=True, max_samples=cap), n_bands


def test_bands_give_the_bits_of_the_single_band_in_deterministic_mode(hand_scene, deterministic):
    """`v5`, 1024 pixels: three bands of at most 11 rows (352 pixels: a partial block of the 256-thread pixel kernels) and four of 8 rows
    (256 pixels); and a second run of the single band."""
    whole, three, n3 = _banded(hand_scene, "v5", 11)
    _, four, n4 = _banded(hand_scene, "v5", 8)
    again = _case(hand_scene, "v5", LAWS[2], ends=True)
    assert (n3, n4) == (3, 4)
    for k in _OLD + _ENDS + _CAM:
        assert torch.equal(whole[k], three[k]) and torch.equal(whole[k], four[k]) and torch.equal(whole[k], again[k]), k
    assert whole["count"] == three["count"] == four["count"]


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    assert not det.on()
    for rows in (11, 8):
        whole, banded, _ = _banded(hand_scene, "v5", rows)
        for k in _OLD + _ENDS + _CAM:
            assert (whole[k] - banded[k]).abs().max() <= BAND_REL * whole[k].abs().max(), k
        _check_against(banded, ref_mod.reference("v5", LAWS[2], True))


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    """camera_param is read to the host once per call and a host tensor's gradient leaves the device -- neither can be captured, which is
    screen_param's rule -- so the captured step is the autograd Function itself with the camera's values in the checked
    arguments and device tensors standing for Rinv and Kinv: the three entry-point kernels, the 21 partials and their split into the two
    shapes are all inside the graph."""
    scene = _scene()
    sc = image_cases.scene("v5")
    Rinv, Kinv = (m.cuda().requires_grad_(True) for m in ref_mod.camera_tensors(sc["camera_M"]))
    a = render.check_image_loss_args(None, sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("v5", LAWS[1], True), supersample=sc["s"],
                                     max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"], camera_param=(Rinv, Kinv))
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")

    def step():
        term = Render._image_term(scene, a, (IOR, EXT), tex, tgt, None, "camera")
        loss = Render._UnitSeedTerm.apply(term, scene.vertices, None, None, None, None, Rinv, Kinv)
        return (loss.detach(),) + torch.autograd.grad(loss, [scene.vertices, Rinv, Kinv])

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and all(t.abs().max() > 0 for t in eager[1:])
    for x, y in zip(eager, static):
        assert torch.equal(x, y)
    ref = ref_mod.reference("v5", LAWS[1], True)
    _check_against(dict(loss=static[0], g_rinv=static[2].cpu()[:3], g_kinv=static[3]), ref)


def test_the_first_growth_of_the_seed_buffer_under_capture_is_refused(deterministic):
    """A scene whose every other buffer has its size from an eager call WITHOUT camera_param: the first camera call is the first to
    need the camera-ray seeds, and inside a stream capture it is refused with the message of the pixel seeds; after one eager camera
    call the same capture goes through (the replay test above)."""
    scene = _scene()
    sc = image_cases.scene("v5")
    Rinv, Kinv = (m.cuda().requires_grad_(True) for m in ref_mod.camera_tensors(sc["camera_M"]))
    a = render.check_image_loss_args(None, sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("v5", LAWS[1], True), supersample=sc["s"],
                                     max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"], camera_param=(Rinv, Kinv))
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")

    def step(camera):
        term = Render._image_term(scene, a, (IOR, EXT), tex, tgt, None, "camera")
        return Render._UnitSeedTerm.apply(term, scene.vertices, None, None, None, None, *((Rinv, Kinv) if camera else (None, None)))

    plain = step(False).detach().clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="camera-ray seeds and cannot run inside a stream capture"):
        with torch.cuda.graph(g):
            step(True)
    torch.cuda.synchronize()
    assert torch.equal(step(True).detach(), plain)


# -------------------------------------------------------------------------------------------------------------------------- supersampling
def _small(s):
    """The `v5` camera at 8 x 12 with s x s samples per pixel: a scene dict like image_cases.scene's, its target (the restatement's image
    at TARGET_IOR) and the restatement at conftest.IOR."""
    centre, extent = image_cases.frame()
    cam = image_cases.camera(5, 8, 12)
    sc = dict(mesh=image_cases.hand(), camera_M=cam, height=8, width=12, s=s, texture=image_cases.texture(3),
              screen=render.Screen.behind(cam, centre, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN), void=0.25, invalid=0.75)
    Rinv, Kinv = ref_mod.camera_tensors(cam)
    fwd = ref_mod.forward(sc["mesh"].faces, sc["mesh"].vertices, Rinv, Kinv, 8, 12, sc["screen"], sc["texture"], s, LAWS[2], True, sc["void"], sc["invalid"],
                          cases.TARGET_IOR, EXT)
    target = np.ascontiguousarray(fwd["mean"].to(torch.float32).view(8, 12, 3).numpy())
    ref = ref_mod.loss_and_grads(sc["mesh"].faces, sc["mesh"].vertices, cam, 8, 12, sc["screen"], sc["texture"], target, s, LAWS[2], True, sc["void"], sc["invalid"])
    return sc, target, ref


@pytest.mark.parametrize("s", [1, 3, 4])
def test_supersampling(hand_scene, s):
    """8 x 12 pixels of the `v5` camera under (6, reflect, snell) with Fresnel: through samples on the screen at s = 1, 3, 4 were counted
    on the CPU before the size was fixed: 29, 237 and 420 of 96, 864 and 1536 samples, beside 37, 377 and 712 direct ones."""
    sc, target, ref = _small(s)
    assert ref["through_on"] > 0 and ref["on"] > ref["through_on"] and ref["margin"] >= cases.TEXEL_MARGIN
    got = _call(hand_scene, sc, target, LAWS[2], True)
    _check_against(got, ref)
    assert got["count"] == ref["through_on"]


# ----------------------------------------------------------------------------------------------------------------------- special inputs
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_an_empty_mesh_every_sample_direct(name):
    sc = image_cases.scene(name)
    target = cases.target(name, LAWS[2], True)
    ref = ref_mod.loss_and_grads(np.zeros((0, 3), np.int64), np.zeros((0, 3)), sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target,
                                 sc["s"], LAWS[2], True, sc["void"], sc["invalid"])
    assert ref["through_on"] == 0 and ref["on"] > 0 and ref["margin"] >= cases.TEXEL_MARGIN
    got = _case(_scene(faces=False), name, LAWS[2])
    _check_against(got, ref)
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def test_a_half_visible_screen(hand_scene):
    """The screen moved by 24 texels along its x: part of the image looks past it.  Off-screen and invalid samples contribute nothing."""
    sc = dict(image_cases.scene("v5"))
    r = image_screen_ref.shifted(sc["screen"], 24.25, 0.0).numpy()
    sc["screen"] = render.Screen(r[0], r[1], r[2])
    target = cases.target("v5", LAWS[1], True)
    ref = ref_mod.loss_and_grads(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, sc["s"],
                                 LAWS[1], True, sc["void"], sc["invalid"])
    looking = int((ref["fwd"]["cls"] != image_ref.INVALID).sum())
    assert 0.3 * looking < ref["on"] < 0.8 * looking and ref["margin"] >= cases.TEXEL_MARGIN
    got = _call(hand_scene, sc, target, LAWS[1], True)
    _check_against(got, ref)
    assert got["count"] == ref["through_on"] and 0 < ref["through_on"] < cases.reference("v5", LAWS[1], True)["count"]


def test_only_the_camera_gradient_and_both_shapes_of_rinv(hand_scene, deterministic):
    """vertices=False and plain IOR floats: only the camera gradient is asked for, and it has the bits of the full call's; a [3, 4] Rinv
    gives the values of the [4, 4] one."""
    full = _case(hand_scene, "wide", LAWS[2], ends=True)
    only = _case(hand_scene, "wide", LAWS[2], only_camera=True)
    three = _case(hand_scene, "wide", LAWS[2], only_camera=True, rows=3)
    assert only["count"] == full["count"] > 0 and torch.equal(only["loss"], full["loss"])
    for k in _CAM:
        assert torch.equal(only[k], full[k]), k
    assert torch.equal(three["g_rinv"], only["g_rinv"][:3]) and torch.equal(three["g_kinv"], only["g_kinv"])
    _check_against(only, ref_mod.reference("wide", LAWS[2], True))


# ---------------------------------------------------------------------------------------------------------------------------------- fit
def test_fit_camera_recovers_a_displaced_camera(hand_scene):
    """The hand from view 5 at 32 x 32, s = 2, (6, reflect, snell) with Fresnel, image_screen_ref's smooth 64 x 64 three-channel texture,
    the photograph rendered by the restatement at the true camera; the start is off by a quarter of a pixel sideways and 0.15 degrees
    about the view axis (half of the displacement first planned: from that one the restatement's own fit does not converge, see
    image_camera_ref.FIT_SIDEWAYS_PIXELS).  image_camera_ref.CPU_FIT records the same fit -- calibrate's Adam loop, 150 steps of 0.02 pixels -- over the restatement on
    the CPU, re-traced at every step.  Asserted here: half of the CPU's improvement in decades, for the loss and for the pose error (the
    projected displacement of the object's centre and of a point one extent to its side); the same arithmetic in another summation
    order, the margin is for the optimiser's sensitivity to last bits."""
    case, rec = ref_mod.fit_case(), ref_mod.CPU_FIT
    start_err = ref_mod.pose_error(case["start"], case["true"], case["centre"], case["extent"])
    assert abs(start_err - rec["start_error"]) <= 1e-9
    fitted, history = calibrate.fit_camera(hand_scene, case["start"], torch.as_tensor(case["photo"]).cuda(), case["screen"], case["texture"],
                                           steps=ref_mod.FIT_STEPS, lr=ref_mod.FIT_LR, supersample=ref_mod.FIT_S, max_bounces=ref_mod.FIT_LAW[0],
                                           tir=ref_mod.FIT_LAW[1], refraction=ref_mod.FIT_LAW[2], void=case["void"], invalid=case["invalid"], ior_int=IOR,
                                           ior_ext=EXT)
    err = ref_mod.pose_error(fitted, case["true"], case["centre"], case["extent"])
    print(f"loss {history[0]:.6e} -> {min(history):.6e}; pose error {start_err:.4f} -> {err:.5f} pixels")
    assert len(history) == ref_mod.FIT_STEPS and abs(history[0] - rec["first"][0]) <= 1e-6 * rec["first"][0]
    loss_decades = np.log10(rec["first"][0] / rec["best"])
    error_decades = np.log10(rec["start_error"] / rec["error"])
    assert loss_decades > 0 and error_decades > 0
    assert min(history) <= rec["first"][0] * 10 ** (-0.5 * loss_decades) and err <= rec["start_error"] * 10 ** (-0.5 * error_decades)
    assert len(fitted) == 4 and np.array_equal(fitted[3], np.asarray(case["true"][3]))
