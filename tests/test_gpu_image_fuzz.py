"""GPU: the image family -- Scene.render_image, Scene.image_loss_fused with every gradient it has, Scene.bind_image_views and
Scene.image_loss_views_fused (drt_amd/csrc/drt_image*.hip) -- against the float64 restatements on the random cases of
tests/image_fuzz_cases.py: random closed shapes of one or two bodies, cameras far from, close to and inside them, IOR 1.1 to 2.4, images
from 1 x 1 to 32 x 20 at 1 to 4 samples a side, NON-SQUARE textures on screens that may be tilted against the camera, non-square
environments under seeded rotations, scalar and per-channel fills, weight planes with zeros.  Every case is admitted by the restatements
alone, and the host builds of the headers are held to the same restatements with the same tolerances, in tests/test_image_fuzz_host.py.

Tolerances are the project's: planes and counts exact; the image within image_cases.tolerance (absorption: image_absorb_cases.image_tolerance,
environment: image_env_cases.tolerance) off the sensitive pixels, whose share is at most 3 %; the loss 1e-10 relative (the ceiling
image_loss_cases states, and what the ray-loss fuzz of tests/test_gpu_fuzz.py uses; exactly zero for a zero reference); every gradient
``image_loss_cases.close``, 1e-9 of the reference's largest entry and at most 1e-5.

Measured on an MI355X (each test prints its figures before it asserts): every image has the restatement's float32 bits on
every pixel; the loss differs by at most 7.5e-15 relative; the vertex gradient by 2.0e-13 of its largest entry, the screen pose by
4.6e-15, the texture by 1.4e-14, the camera groups by 1.9e-14, the environment's texels by 7.6e-14 and its rotation by 6.3e-14."""
import numpy as np
import pytest
import torch

import image_absorb_cases
import image_camera_ref
import image_cases
import image_env_cases
import image_fuzz_cases as fz
import image_loss_cases
import image_screen_ref
from drt_amd import det, diffrender as Render, render

pytestmark = pytest.mark.gpu
close = image_loss_cases.close
LOSS_REL = 1e-10
ENV_IDS = [f"{seed}-{'screen' if ws else 'no-screen'}-{'reflection' if rf else 'no-reflection'}" for seed, ws, rf in fz.ENV_CASES]
BANDED = [0, 8, 24, 28]          # image heights 5, 7, 9 and 17: bands of 2, 3, 4 and 4 rows leave a last band of a single row


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR)
    yield
    Render.intIOR, Render.extIOR = saved


_scenes = {}


def _scene(seed):
    """The Scene of a case's mesh (built once per seed), with the module's IORs set to the case's."""
    sc = fz.case(seed)
    Render.intIOR, Render.extIOR = sc["ior_int"], sc["ior_ext"]
    if seed not in _scenes:
        assert len(sc["mesh"].faces) <= 1600
        scene = Render.Scene(sc["mesh"], 0)
        scene.update_verticex(torch.tensor(sc["mesh"].vertices, dtype=torch.float64, device="cuda", requires_grad=True))
        _scenes[seed] = scene
    return _scenes[seed]


def _law_kw(sc, fresnel=True):
    kw = dict(supersample=sc["s"], max_bounces=sc["law"][0], tir=sc["law"][1], refraction=sc["law"][2], void=sc["void"], invalid=sc["invalid"])
    if fresnel:
        kw["fresnel"] = sc["fresnel"]
    return kw


def _iors(sc):
    return (torch.tensor(sc["ior_int"], dtype=torch.float64, requires_grad=True), torch.tensor(sc["ior_ext"], dtype=torch.float64, device="cuda", requires_grad=True))


def _loss_close(got, want):
    return got == 0.0 if want == 0.0 else abs(got - want) <= LOSS_REL * abs(want)


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def _check_image(what, image, want, bad, tol):
    diff = (image.cpu().double() - torch.as_tensor(np.asarray(want)).double()).abs().amax(2).numpy()
    print(f"{what}: sensitive pixels {int(bad.sum())} of {bad.size}, tolerance {tol:.3e}, largest difference {diff[~bad].max() if (~bad).any() else 0.0:.3e}, on the "
          f"sensitive pixels {diff[bad].max() if bad.any() else 0.0:.3e}")
    assert image.dtype == torch.float32 and tuple(image.shape) == tuple(np.asarray(want).shape)
    assert bad.mean() <= image_cases.SENSITIVE_CAP
    assert np.isfinite(diff).all() and (not (~bad).any() or diff[~bad].max() <= tol)


def _check_loss_and_grads(what, got, ref):
    gV = got["grad_V"].cpu().numpy()
    print(f"{what}: loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} relative difference {_rel(float(got['loss']), ref['loss']):.2e}; g_int "
          f"{float(got['g_int']):.9e} / {ref['g_int']:.9e}, g_ext {float(got['g_ext']):.9e} / {ref['g_ext']:.9e}, max |grad_V| {np.abs(ref['grad_V']).max():.3e} differs by "
          f"{np.abs(gV - ref['grad_V']).max():.2e}; count {got['count']} / {ref['count']}")
    assert got["count"] == ref["count"]
    assert _loss_close(float(got["loss"]), ref["loss"])
    assert close(gV, ref["grad_V"]) and close(float(got["g_int"]), ref["g_int"]) and close(float(got["g_ext"]), ref["g_ext"])
    if ref["count"] == 0:
        assert np.isfinite(gV).all() and not gV.any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def _loss_call(scene, sc, target, screen="case", texture="case", camera="case", extra=(), fresnel=True, **kw):
    """One image_loss_fused call on a case: dict(loss, grad_V, g_int, g_ext, count, image, extra: the gradients of ``extra``)."""
    ii, ie = _iors(sc)
    out = scene.image_loss_fused(sc["camera_M"] if camera == "case" else camera, sc["height"], sc["width"], sc["screen"] if screen == "case" else screen,
                                 sc["texture"] if texture == "case" else texture, target, weight=sc["weight"], ior_int=ii, ior_ext=ie, **_law_kw(sc, fresnel), **kw)
    loss, image = out if kw.get("want_image") else (out, None)
    count = int(scene.last_image_count)
    g = [t.clone() for t in torch.autograd.grad(loss, [scene.vertices, ii, ie] + list(extra))]
    return dict(loss=loss.detach().clone(), grad_V=g[0], g_int=g[1], g_ext=g[2], count=count, image=image, extra=g[3:])


# ---- a. render_image -------------------------------------------------------------------------------------------------------------------------
def _render(scene, sc, **kw):
    return scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], want_planes=True, **_law_kw(sc), **kw)


@pytest.mark.parametrize("seed", fz.CASES)
def test_render_image_against_the_restatement(seed):
    sc, st, scene = fz.case(seed), fz.stage(seed), _scene(seed)
    image, hit, through = _render(scene, sc)
    print(f"seed {seed}: planes differ on {int((hit.cpu() != st['hit']).sum())} and {int((through.cpu() != st['through']).sum())} pixels")
    assert torch.equal(hit.cpu(), st["hit"]) and torch.equal(through.cpu(), st["through"])          # exact, every pixel
    _check_image(f"seed {seed}", image, st["image"], image_cases.sensitive(sc, st), image_cases.tolerance(sc, st))
    for a, b in zip((image, hit, through), _render(scene, sc)):
        assert torch.equal(a, b)
    if seed in BANDED:
        rows = {5: 2, 7: 3, 9: 4, 17: 4}[sc["height"]]
        cap = rows * sc["width"] * sc["s"] ** 2
        bands = render.plan_bands(sc["height"], sc["width"], sc["s"], cap)
        assert len(bands) > 1 and bands[-1][1] - bands[-1][0] == 1
        for a, b in zip((image, hit, through), _render(scene, sc, max_samples=cap)):
            assert torch.equal(a, b)


def test_the_banded_cases_are_cases():
    assert set(BANDED) <= set(fz.CASES) and sorted(fz.case(seed)["height"] for seed in BANDED) == [5, 7, 9, 17]


# ---- b. image_loss_fused ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.CASES)
def test_loss_and_gradients_against_the_restatement(seed):
    sc, ref, scene = fz.case(seed), fz.loss_reference(seed), _scene(seed)
    got = _loss_call(scene, sc, sc["target"], want_image=True)
    _check_loss_and_grads(f"seed {seed}", got, ref)
    assert torch.equal(got["image"], _render(scene, sc)[0])
    flat = _loss_call(scene, sc, np.ascontiguousarray(sc["target"][:, :, 0])) if sc["texture3"].shape[2] == 1 else None          # C = 1: a [H, W] target
    was = det.enable(True)
    try:
        one, two = _loss_call(scene, sc, sc["target"]), _loss_call(scene, sc, sc["target"])
    finally:
        det.enable(was)
    for k in ("loss", "grad_V", "g_int", "g_ext"):
        assert torch.equal(one[k], two[k])
    _check_loss_and_grads(f"seed {seed}, deterministic", one, ref)
    if flat is not None:
        _check_loss_and_grads(f"seed {seed}, [H, W] target", flat, ref)


# ---- c. screen pose and texture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.SCREEN_CASES)
def test_screen_pose_and_texture_gradients_against_the_restatement(seed):
    sc, ref, scene = fz.case(seed), fz.screen_reference(seed), _scene(seed)
    P = image_screen_ref.rows_of(sc["screen"]).requires_grad_(True)
    T = torch.tensor(sc["texture3"], dtype=torch.float64, device="cuda", requires_grad=True)
    got = _loss_call(scene, sc, sc["target"], screen=None, texture=None, extra=(P, T), screen_param=P, texture_param=T)
    gs, gt = got["extra"][0].numpy(), got["extra"][1].cpu().numpy()
    print(f"seed {seed}: loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} ({_rel(float(got['loss']), ref['loss']):.1e}); max |g_screen| "
          f"{np.abs(ref['g_screen']).max():.3e} differs by {np.abs(gs - ref['g_screen']).max():.2e}; max |g_texture| {np.abs(ref['g_texture']).max():.3e} differs by "
          f"{np.abs(gt - ref['g_texture']).max():.2e}")
    assert gs.shape == (3, 3) and gt.shape == ref["g_texture"].shape == sc["texture3"].shape
    assert _loss_close(float(got["loss"]), ref["loss"])
    assert close(gs, ref["g_screen"]) and np.abs(ref["g_screen"]).max() > 0
    assert close(gt, ref["g_texture"]) and np.abs(ref["g_texture"]).max() > 0
    assert ((gt == 0) == (ref["g_texture"] == 0)).all()          # a texel nothing lands on has gradient exactly 0
    _check_loss_and_grads(f"seed {seed}", got, fz.loss_reference(seed))


# ---- d. camera ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.CAMERA_CASES)
def test_camera_gradient_against_the_restatement(seed):
    sc, ref, scene = fz.case(seed), fz.camera_reference(seed), _scene(seed)
    Rinv, Kinv = image_camera_ref.camera_tensors(sc["camera_M"])
    Rinv, Kinv = Rinv.clone().requires_grad_(True), Kinv.cuda().requires_grad_(True)
    got = _loss_call(scene, sc, sc["target"], camera=None, extra=(Rinv, Kinv), camera_param=(Rinv, Kinv))
    want = image_camera_ref.groups(ref["g_rinv"], ref["g_kinv"])
    have = image_camera_ref.groups(got["extra"][0].numpy(), got["extra"][1].cpu().numpy())
    print(f"seed {seed}: loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} ({_rel(float(got['loss']), ref['loss']):.1e}); "
          + "; ".join(f"max |{k}| {np.abs(want[k]).max():.3e} differs by {np.abs(have[k] - want[k]).max():.2e}" for k in want))
    assert _loss_close(float(got["loss"]), ref["loss"]) and got["count"] == ref["through_on"]
    assert not got["extra"][0][3].any()
    for k in want:
        assert np.abs(want[k]).max() > 0 and close(have[k], want[k]), k
    _check_loss_and_grads(f"seed {seed}", got, fz.loss_reference(seed))


# ---- e. absorption -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.ABSORB_CASES)
def test_absorption_against_the_restatement(seed):
    sc, st, ref, scene = fz.case(seed), fz.stage(seed), fz.absorb_reference(seed), _scene(seed)
    image, hit, through, length = _render(scene, sc, absorption=sc["sigma"])
    want = ref["fwd"]["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1)
    assert torch.equal(hit.cpu(), st["hit"]) and torch.equal(through.cpu(), st["through"]) and length.shape == hit.shape
    _check_image(f"seed {seed}", image, want, image_cases.sensitive(sc, st), image_absorb_cases.image_tolerance(sc, st, sc["law"]))
    assert not length.cpu()[through.cpu() == 0].any() and float((want.double() - st["image"].double()).abs().max()) > 0          # the glass IS darker
    sg = torch.tensor(sc["sigma"], dtype=torch.float64, requires_grad=True)
    got = _loss_call(scene, sc, sc["target"], extra=(sg,), absorption=sg)
    _check_loss_and_grads(f"seed {seed}", got, ref)
    g_sigma = got["extra"][0].numpy()
    print(f"seed {seed}: g_sigma {g_sigma} / {ref['g_sigma']}")
    assert g_sigma.shape == sc["sigma"].shape and close(g_sigma, ref["g_sigma"]) and np.abs(ref["g_sigma"]).max() > 0


# ---- f. environment ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,with_screen,reflection", fz.ENV_CASES, ids=ENV_IDS)
def test_environment_against_the_restatement(seed, with_screen, reflection):
    sc, scene = fz.case(seed), _scene(seed)
    st, img = fz.stage(seed, True), fz.env_image_reference(seed, with_screen, reflection)
    ref, par = fz.env_loss_reference(seed, with_screen, reflection), fz.env_param_reference(seed, with_screen, reflection)
    env = render.Environment(sc["environment"], sc["rotation"])
    ends = dict(screen="case" if with_screen else None, texture="case" if with_screen else None)
    planes = scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None, sc["texture"] if with_screen else None,
                                want_planes=True, environment=env, reflection=reflection, **_law_kw(sc, fresnel=False))
    image, hit, through = planes[:3]
    assert torch.equal(hit.cpu(), st["hit"]) and torch.equal(through.cpu(), st["through"])
    if reflection:
        assert torch.equal(planes[3].cpu(), img["reflect"])
    _check_image(f"seed {seed}", image, img["image"], image_env_cases.sensitive(sc, sc["law"], with_screen, reflection, ref=img, stage=st),
                 image_env_cases.tolerance(sc, sc["law"], with_screen, stage=st))
    target = fz.env_target(seed, with_screen, reflection)
    got = _loss_call(scene, sc, target, fresnel=False, environment=env, reflection=reflection, **ends)
    _check_loss_and_grads(f"seed {seed}", got, ref)
    E = torch.as_tensor(sc["environment"]).to(device="cuda", dtype=torch.float64).requires_grad_(True)
    R = torch.tensor(sc["rotation"], dtype=torch.float64, requires_grad=True)
    got = _loss_call(scene, sc, target, fresnel=False, extra=(E, R), environment=env, reflection=reflection, env_texels_param=E, env_rotation_param=R, **ends)
    g_env, g_R = got["extra"][0].cpu().numpy(), got["extra"][1].numpy()
    print(f"seed {seed}: max |g_env| {np.abs(par['g_env']).max():.3e} differs by {np.abs(g_env - par['g_env']).max():.2e}; max |g_R| {np.abs(par['g_R']).max():.3e} "
          f"differs by {np.abs(g_R - par['g_R']).max():.2e}")
    assert _loss_close(float(got["loss"]), par["loss"])
    assert g_env.shape == sc["environment"].shape and close(g_env, par["g_env"]) and close(g_R, par["g_R"])
    assert np.abs(par["g_env"]).max() > 0 and np.abs(par["g_R"]).max() > 0 and not g_env[par["g_env"] == 0].any()
    _check_loss_and_grads(f"seed {seed}, with the parameters", got, ref)


# ---- g. views ----------------------------------------------------------------------------------------------------------------------------------
def _views_call(scene, sc, binding, texture, fresnel=True, **kw):
    ii, ie = _iors(sc)
    loss = scene.image_loss_views_fused(binding, fz.VIEW_IDS, texture, ior_int=ii, ior_ext=ie, **_law_kw(sc, fresnel), **kw)
    count = int(scene.last_image_count)
    g = [t.clone() for t in torch.autograd.grad(loss, [scene.vertices, ii, ie])]
    return dict(loss=loss.detach().clone(), grad_V=g[0], g_int=g[1], g_ext=g[2].cpu(), count=count)


@pytest.mark.parametrize("seed", fz.VIEWS_CASES)
def test_views_listed_out_of_order_with_a_repeat_against_the_summed_restatement(seed):
    """Three cameras at three distance factors with three screens in one binding, listed [2, 0, 2]; then below one view's sample count per
    band; then in front of the case's environment with the reflection."""
    sc, cap, scene = fz.case(seed), fz.capture(seed), _scene(seed)
    want = fz.summed(fz.capture_references(seed))
    binding = scene.bind_image_views(cap["cams"], sc["height"], sc["width"], cap["screens"], cap["targets"], cap["weights"])
    got = _views_call(scene, sc, binding, sc["texture"])
    _check_loss_and_grads(f"seed {seed} views {fz.VIEW_IDS}", got, want)
    assert want["count"] > 0 and not close(got["grad_V"].cpu().numpy(), fz.capture_references(seed)[2]["grad_V"])          # (one view alone is outside)
    per_view = sc["height"] * sc["width"] * sc["s"] ** 2
    cap_samples = max(1, (per_view * 2) // 3)
    assert len(render.plan_bands(len(fz.VIEW_IDS) * sc["height"], sc["width"], sc["s"], cap_samples)) > len(fz.VIEW_IDS) or sc["height"] == 1
    _check_loss_and_grads(f"seed {seed} views {fz.VIEW_IDS}, at most {cap_samples} samples a band", _views_call(scene, sc, binding, sc["texture"], max_samples=cap_samples),
                          want)
    room = fz.capture_env(seed)
    env = render.Environment(sc["environment"], sc["rotation"])
    binding = scene.bind_image_views(cap["cams"], sc["height"], sc["width"], cap["screens"], room["targets"], cap["weights"], environment=env)
    got = _views_call(scene, sc, binding, sc["texture"], fresnel=False, reflection=True)
    _check_loss_and_grads(f"seed {seed} views {fz.VIEW_IDS}, environment and reflection", got, fz.summed(room["refs"]))
