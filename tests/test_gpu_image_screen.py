"""GPU: the screen-pose and texture gradients of Scene.image_loss_fused (screen_param / texture_param; drt_render_image_loss_screen,
drt_amd/csrc/drt_image_screen.hip) against torch autograd of the float64 restatement tests/image_screen_ref.py, on the scenes `v5` and
`wide` of tests/image_cases.py with the targets of tests/image_loss_cases.py.

Tolerances are those of tests/test_image_screen_host.py: the loss LOSS_REL, every gradient ``image_loss_cases.close`` (1e-9 of the largest
entry of the reference, 1e-5 absolute).  In deterministic mode bands, runs and a graph replay give the same bits."""
import numpy as np
import pytest
import torch

import image_cases
import image_loss_cases as cases
import image_ref
import image_screen_ref as ref_mod
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


def _call(scene, name, law=LAWS[0], fresnel=True, rows=None, texture=None, target=None, params=True, tex_dtype=torch.float64, **kw):
    """dict(loss, grad_V, g_int, g_ext, count[, g_screen, g_texture]) of one call on a scene of image_cases, on the device.  ``params``:
    the screen and the texture go in as screen_param (a host tensor) / texture_param (a device tensor) and their gradients are taken."""
    sc = image_cases.scene(name)
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=fresnel, void=sc["void"], invalid=sc["invalid"])
    args.update(kw)
    rows = ref_mod.pose(name) if rows is None else rows
    texture = sc["texture"] if texture is None else texture
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
    wrt = [scene.vertices, ii, ie]
    if params:
        P = rows.clone().requires_grad_(True)
        T = torch.tensor(texture, dtype=tex_dtype, device="cuda", requires_grad=True)
        args.update(screen_param=P, texture_param=T)
        wrt += [P, T]
        screen, texture = None, None
    else:
        r = rows.numpy()
        screen = render.Screen(r[0], r[1], r[2])
    loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], screen, texture, cases.target(name, law, fresnel) if target is None else target,
                                  ior_int=ii, ior_ext=ie, **args)
    g = [x.clone() for x in torch.autograd.grad(loss, wrt)]
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), grad_V=g[0], g_int=g[1], g_ext=g[2])
    if params:
        assert g[3].device.type == "cpu" and g[3].shape == (3, 3) and g[3].dtype == torch.float64
        assert g[4].device.type == "cuda" and g[4].shape == T.shape and g[4].dtype == tex_dtype
        res.update(g_screen=g[3], g_texture=g[4])
    return res


def _check_against(got, ref):
    gs, gt = got["g_screen"].numpy(), got["g_texture"].cpu().numpy().reshape(ref["g_texture"].shape)
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} ({rel:.1e}); max |g_screen| {np.abs(ref['g_screen']).max():.3e} differs by "
          f"{np.abs(gs - ref['g_screen']).max():.2e}; max |g_texture| {np.abs(ref['g_texture']).max():.3e} differs by {np.abs(gt - ref['g_texture']).max():.2e}")
    assert rel <= cases.LOSS_REL
    assert cases.close(gs, ref["g_screen"]) and np.abs(ref["g_screen"]).max() > 0
    assert cases.close(gt, ref["g_texture"]) and np.abs(ref["g_texture"]).max() > 0
    assert ((gt == 0) == (ref["g_texture"] == 0)).all()              # a texel nothing lands on has gradient exactly 0


_OLD = ("loss", "grad_V", "g_int", "g_ext")


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_gradients_against_the_restatement(hand_scene, name, law, fresnel):
    """... and the vertex gradient, the IOR partials and the count of the same call are those of a call without the new keywords."""
    ref = ref_mod.reference(name, law, fresnel)
    got = _call(hand_scene, name, law, fresnel)
    _check_against(got, ref)
    plain = _call(hand_scene, name, law, fresnel, params=False)
    assert got["count"] == plain["count"] == cases.reference(name, law, fresnel)["count"]
    for k in _OLD[1:]:
        assert cases.close(got[k].cpu().numpy(), plain[k].cpu().numpy())
    assert abs(float(got["loss"]) - float(plain["loss"])) <= BAND_REL * float(plain["loss"])


@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_the_old_gradients_keep_their_bits_in_deterministic_mode(hand_scene, deterministic, name):
    got, plain = _call(hand_scene, name, LAWS[2]), _call(hand_scene, name, LAWS[2], params=False)
    for k in _OLD:
        assert torch.equal(got[k], plain[k])
    _check_against(got, ref_mod.reference(name, LAWS[2], True))


def test_without_the_keywords_the_call_is_todays(hand_scene, deterministic, monkeypatch):
    """The method's route without the keywords is the "plain" term / drt_render_image_loss, as before; and the screen entry point with both
    accumulators null -- the "screen" term with nothing to track -- gives that route's bits."""
    sc = image_cases.scene("v5")
    a = render.check_image_loss_args(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("v5", LAWS[1], True),
                                     supersample=sc["s"], max_bounces=6, tir="reflect", void=sc["void"], invalid=sc["invalid"])
    tex, tgt = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(a["target"], device="cuda")
    got, entries = [], []
    lib = _lib.lib()
    for name in ("drt_render_image_loss", "drt_render_image_loss_screen"):
        monkeypatch.setattr(lib, name, lambda *args, name=name, fn=getattr(lib, name): entries.append(name) or fn(*args))
    for entry, extra in (("plain", ()), ("screen", (None, None))):
        ii = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
        term = Render._image_term(hand_scene, a, (IOR, EXT), tex, tgt, None, entry)
        loss = Render._UnitSeedTerm.apply(term, hand_scene.vertices, ii, None, *extra)
        got.append((loss.detach().clone(), term.count.clone()) + tuple(g.clone() for g in torch.autograd.grad(loss, [hand_scene.vertices, ii])))
    assert list(dict.fromkeys(entries)) == ["drt_render_image_loss", "drt_render_image_loss_screen"]          # two different native entry points
    assert float(got[0][0]) > 0 and got[0][2].any() and got[0][3] != 0
    for x, y in zip(*got):
        assert torch.equal(x, y)


def test_a_float32_texture_receives_a_float32_gradient(hand_scene, deterministic):
    wide, narrow = _call(hand_scene, "wide"), _call(hand_scene, "wide", tex_dtype=torch.float32)
    assert torch.equal(narrow["g_texture"], wide["g_texture"].to(torch.float32)) and torch.equal(narrow["g_screen"], wide["g_screen"])
    flat = _call(hand_scene, "wide", texture=image_cases.scene("wide")["texture"][:, :, 0])          # [Th, Tw]: the gradient has that shape
    assert flat["g_texture"].shape == (image_cases.TEX, image_cases.TEX) and torch.equal(flat["g_texture"], wide["g_texture"][:, :, 0])


# ------------------------------------------------------------------------------------------------------------------ bands, repeats, modes
def _banded(scene, name):
    sc = image_cases.scene(name)
    cap = 9 * sc["width"] * sc["s"] ** 2 + 5
    assert len(render.plan_bands(sc["height"], sc["width"], sc["s"], cap)) >= 3
    return _call(scene, name, LAWS[2]), _call(scene, name, LAWS[2], max_samples=cap)


@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_bands_give_the_bits_of_the_single_band_in_deterministic_mode(hand_scene, deterministic, name):
    whole, banded = _banded(hand_scene, name)
    again = _call(hand_scene, name, LAWS[2])
    for k in _OLD + ("g_screen", "g_texture"):
        assert torch.equal(whole[k], banded[k]) and torch.equal(whole[k], again[k])
    assert whole["count"] == banded["count"]


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    assert not det.on()
    whole, banded = _banded(hand_scene, "v5")
    for k in _OLD + ("g_screen", "g_texture"):
        assert (whole[k] - banded[k]).abs().max() <= BAND_REL * whole[k].abs().max()
    _check_against(banded, ref_mod.reference("v5", LAWS[2], True))


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    """Plain IOR floats and a plain Screen: a gradient of screen_param leaves the device for the host tensor it belongs to, which a
    capture cannot hold, so the captured call takes the texture and the vertex gradients."""
    scene = _scene()
    sc = image_cases.scene("v5")
    tex = torch.tensor(sc["texture"], device="cuda", requires_grad=True)
    tgt = torch.as_tensor(cases.target("v5", LAWS[1], True)).cuda()

    def step():
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], None, tgt, supersample=sc["s"], max_bounces=6, tir="reflect",
                                      void=sc["void"], invalid=sc["invalid"], texture_param=tex)
        return (loss.detach(),) + torch.autograd.grad(loss, [scene.vertices, tex])

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and eager[1].abs().max() > 0 and eager[2].abs().max() > 0
    for a, b in zip(eager, static):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------------- contention
def _four_texels():
    """`v5` in front of a 2 x 2 texture that spans the whole view: every on-screen sample adds to the same four texels."""
    sc = image_cases.scene("v5")
    center, extent = image_cases.frame()
    screen = render.Screen.behind(sc["camera_M"], center, extent, 2, 2, span=8.0)
    tex = np.array([[[0.1, 0.5, 0.9], [0.8, 0.2, 0.4]], [[0.3, 0.7, 0.6], [0.9, 0.1, 0.2]]], np.float32)
    ref = ref_mod.loss_and_grads(ref_mod.constants("v5", LAWS[1], True), ref_mod.rows_of(screen), tex, cases.target("v5", LAWS[1], True), sc["s"], sc["void"],
                                 sc["invalid"])
    n_looking = int((ref_mod.constants("v5", LAWS[1], True)["cls"] != image_ref.INVALID).sum())
    # (all but the few through samples whose exit ray points away from the plane; none near a border)
    assert 0.95 * n_looking < ref["on"] <= n_looking and n_looking > 4000 and ref["margin"] >= cases.TEXEL_MARGIN
    return ref_mod.rows_of(screen), tex, ref


def test_every_sample_on_the_same_four_texels_in_float64_mode(hand_scene):
    rows, tex, ref = _four_texels()
    _check_against(_call(hand_scene, "v5", LAWS[1], rows=rows, texture=tex), ref)


def test_every_sample_on_the_same_four_texels_in_deterministic_mode(hand_scene, deterministic):
    """Within the tolerance of the restatement, and the same bits from two runs and from other block counts (four bands)."""
    rows, tex, ref = _four_texels()
    runs = [_call(hand_scene, "v5", LAWS[1], rows=rows, texture=tex, **kw) for kw in ({}, {}, dict(max_samples=9 * 128 + 5))]
    _check_against(runs[0], ref)
    for other in runs[1:]:
        for k in _OLD + ("g_screen", "g_texture"):
            assert torch.equal(runs[0][k], other[k])


# --------------------------------------------------------------------------------------------------- direct samples only, half a screen
@pytest.mark.parametrize("name", ref_mod.SCENES)
def test_an_empty_mesh_still_gives_the_screen_and_texture_gradients(name):
    sc = image_cases.scene(name)
    const = ref_mod.trace(np.zeros((0, 3), np.int64), np.zeros((0, 3)), sc["camera_M"], sc["height"], sc["width"], sc["s"], LAWS[2], True)
    rows = ref_mod.shifted(sc["screen"], 24.25, 0.0)              # (moved along its x, so that some texels are out of every sample's sight)
    ref = ref_mod.loss_and_grads(const, rows, sc["texture"], cases.target(name, LAWS[2], True), sc["s"], sc["void"], sc["invalid"])
    assert ref["margin"] >= cases.TEXEL_MARGIN and (ref["g_texture"] == 0).any() and 0 < ref["on"] < len(const["cls"])
    got = _call(_scene(faces=False), name, LAWS[2], rows=rows)
    _check_against(got, ref)                                      # (a texel nothing lands on has gradient exactly 0: checked there)
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def test_a_half_visible_screen(hand_scene):
    """The screen moved by 24 texels along its x: part of the image looks past it.  Off-screen and invalid samples contribute nothing, and
    last_image_count is still the number of through samples on the screen."""
    sc = image_cases.scene("v5")
    rows = ref_mod.shifted(sc["screen"], 24.25, 0.0)
    const = ref_mod.constants("v5", LAWS[1], True)
    ref = ref_mod.loss_and_grads(const, rows, sc["texture"], cases.target("v5", LAWS[1], True), sc["s"], sc["void"], sc["invalid"])
    looking = int((const["cls"] != image_ref.INVALID).sum())
    assert 0.3 * looking < ref["on"] < 0.8 * looking and ref["margin"] >= cases.TEXEL_MARGIN
    got = _call(hand_scene, "v5", LAWS[1], rows=rows)
    _check_against(got, ref)
    through_on = int((ref["fwd"]["on"] & (const["cls"] == image_ref.THROUGH)).sum())
    assert got["count"] == through_on and 0 < through_on < cases.reference("v5", LAWS[1], True)["count"]


# ---------------------------------------------------------------------------------------------------------------------------------- fit
def test_fit_screen_recovers_a_misplaced_screen(hand_scene):
    """Three views of the hand (3, 5, 7 of 72) at 32 x 32, s = 2, (6, reflect, snell) with Fresnel, one screen behind view 5 with the
    smooth texture of image_screen_ref, photographs rendered by the restatement at the true pose; the start is off by half a texel pitch
    along eu and by 0.5 degrees about the normal through the centre (corner error 0.823 pitches).  The same fit -- calibrate.fit_pose, 150
    Adam steps of 0.02 texels -- over the restatement's screen stage on the CPU (image_screen_ref.fit_on_the_restatement; exit rays are
    constants of a fixed mesh) took the loss from 5.1478 to 6.94e-6 (5.87 decades) and the corner error to 0.00913 pitches (1.95
    decades).  Asserted here: half of each in decades -- the loss below 5.1478 * 10^-2.93 = 6.0e-3 and the corner error below
    0.823 * 10^-0.98 = 0.087 pitches; the same arithmetic in another summation order, the margin is for the optimiser's sensitivity
    to last bits."""
    case = ref_mod.fit_case()
    start_err = ref_mod.corner_error(case["start"], case["true"], ref_mod.FIT_TEX, ref_mod.FIT_TEX)
    assert abs(start_err - 0.823) < 1e-3
    views = [(cam, torch.as_tensor(photo).cuda()) for cam, photo in zip(case["cams"], case["photos"])]
    fitted, history = calibrate.fit_screen(hand_scene, views, case["start"], case["texture"], steps=ref_mod.FIT_STEPS, lr=ref_mod.FIT_LR,
                                           supersample=ref_mod.FIT_S, max_bounces=ref_mod.FIT_LAW[0], tir=ref_mod.FIT_LAW[1], refraction=ref_mod.FIT_LAW[2],
                                           void=case["void"], invalid=case["invalid"], ior_int=IOR, ior_ext=EXT)
    err = ref_mod.corner_error(fitted, case["true"], ref_mod.FIT_TEX, ref_mod.FIT_TEX)
    print(f"loss {history[0]:.6e} -> {min(history):.6e}; corner error {start_err:.4f} -> {err:.5f} pitches")
    assert abs(history[0] - 5.1478) < 1e-3 and len(history) == ref_mod.FIT_STEPS
    assert min(history) <= 5.1478 * 10 ** -2.93 and err <= 0.823 * 10 ** -0.98
    assert isinstance(fitted, render.Screen)
