"""GPU: Scene.render_image with ``environment`` -- the refracted image in front of a screen and a lat-long environment map, or of the
environment alone (drt_render_image_env, drt_amd/csrc/drt_image_env.hip) -- against the float64 restatement tests/image_env_ref.py on
the scenes, laws and environment of tests/image_env_cases.py.

What must be exact: the ``hit``, ``through`` and ``reflect`` planes, on every pixel, as in tests/test_gpu_image.py (the paths do not know
what they will look at; the reflected rays are the restatement's bit for bit -- tests/test_image_env_host.py -- and the occlusion query
runs under the shared tracer contract).

The image: at most tol = 2^-23 + the screen's term of image_cases.tolerance + G_env (1e-10 + 7 * 2^-51) Ew / (2 pi sin(theta_min))
(image_env_cases.tolerance): 1.30e-7 without a screen (G_env = 0.996, Ew = 32, sin(theta_min) = 0.0447: 1.19e-7 + 1.1e-8), 3.3e-7 with
one.  Pixels left out of the image comparison: with a screen image_cases.sensitive's (a sample there may change between screen and
environment); with or without one, pixels with an environment-going sample within 1e-3 of a pole (1 - |e_y|).  Measured on the CPU with
the restatement, in the order v5, v41 (of 1 024), wide (of 960), each under the three laws:
    with a screen     1, 7, 10;  0, 13, 14;  0, 16, 13    (tests/test_gpu_image.py's figures: no sample is inside the pole cut)
    without a screen  0, 0, 0;   0, 0, 0;    0, 0, 0
The outer-surface reflection adds the rules of image_env_cases.sensitive for the reflected rays (pole, screen border, grazing landing;
913 to 1 410 reflections are added per case, 16 to 51 of them land on the screen) and changes none of these counts.  Their share is
asserted to stay below 3 % for every case."""
import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_ref
import image_ref
from conftest import IOR
from drt_amd import _lib, det, diffrender as Render, render

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAWS = image_cases.LAWS
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
SCREEN_IDS = ["screen", "no-screen"]


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR)
    Render.intIOR, Render.extIOR = IOR, EXT
    yield
    Render.intIOR, Render.extIOR = saved


@pytest.fixture(scope="module")
def hand_scene():
    return Render.Scene(image_cases.hand(), 0)


def _render(scene, name, law, with_screen=True, environment="case", **kw):
    sc = image_cases.scene(name)
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=True, void=sc["void"], invalid=sc["invalid"], want_planes=True,
                environment=image_env_cases.environment(sc["texture"].shape[2]) if isinstance(environment, str) else environment)
    args.update(kw)
    return scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None, sc["texture"] if with_screen else None, **args)


def _check_against(name, law, with_screen, got, reflection=False):
    image, hit, through, reflect = got
    sc = image_cases.scene(name)
    ref = image_env_cases.reference(name, law, with_screen, reflection)
    assert image.dtype == hit.dtype == through.dtype == torch.float32 and image.is_cuda
    assert image.shape == ref["image"].shape == (sc["height"], sc["width"], sc["texture"].shape[2]) and hit.shape == through.shape == image.shape[:2]
    bad = image_env_cases.sensitive(name, law, with_screen, reflection)
    tol = image_env_cases.tolerance(name, law, with_screen)
    want_reflect = ref["reflect"] if reflection else torch.zeros_like(ref["hit"])
    diff = (image.cpu().double() - ref["image"].double()).abs().amax(2).numpy()
    print(name, law, "screen" if with_screen else "no screen", "reflection" if reflection else "no reflection", "reflect plane differs on",
          int((reflect.cpu() != want_reflect).sum()), "sensitive pixels", int(bad.sum()), "of", bad.size, "tol", tol, "max diff", diff[~bad].max(),
          "max diff on sensitive pixels", diff[bad].max() if bad.any() else 0.0, "planes differ on", int((hit.cpu() != ref["hit"]).sum()),
          int((through.cpu() != ref["through"]).sum()))
    assert torch.equal(hit.cpu(), ref["hit"]) and torch.equal(through.cpu(), ref["through"])          # exact, every pixel
    assert reflect.dtype == torch.float32 and torch.equal(reflect.cpu(), want_reflect)
    assert bad.mean() <= image_cases.SENSITIVE_CAP
    assert np.isfinite(diff).all() and diff[~bad].max() <= tol


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("reflection", [False, True], ids=["no-reflection", "reflection"])
@pytest.mark.parametrize("with_screen", [True, False], ids=SCREEN_IDS)
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", list(image_cases.SCENES))
def test_image_and_planes_against_the_restatement(hand_scene, name, law, with_screen, reflection):
    _check_against(name, law, with_screen, _render(hand_scene, name, law, with_screen, reflection=reflection), reflection)
    ref = image_env_cases.reference(name, law, with_screen, reflection)
    src = ref["src"].numpy()
    if reflection:          # occluded reflections, reflections of invalid samples and reflections that land on the screen are all in the picture
        refl = image_env_cases.reflected(name)
        assert ref["added"].sum() > 900 and (refl["qual"] & ~refl["seen"]).sum() > 5 and (refl["seen"] & ~ref["added"]).sum() > 5
        assert (ref["added"] & ref["rb"]["on"]).any() == with_screen
        plain = image_env_cases.reference(name, law, with_screen, False)
        assert (ref["image"] >= plain["image"]).all() and ((ref["image"] > plain["image"]).any(2) == (ref["reflect"] > 0)).all()
    # every source is in the picture; with an environment nothing is `void`
    assert (src == image_env_ref.FILL).sum() > 20 and (src == image_env_ref.ENV).sum() > 500 and ((src == image_env_ref.SCREEN).sum() > 500) == with_screen


def test_the_environment_replaces_void_and_nothing_else(hand_scene):
    """Against the call of before on the same scene: the planes are its bits; a pixel whose samples all land on the screen or are invalid
    keeps its bits; a pixel with a sample beside the screen does not show the void fill any more."""
    name, law = "v41", LAWS[2]
    sc = image_cases.scene(name)
    plain = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], supersample=sc["s"], max_bounces=law[0], tir=law[1],
                                    refraction=law[2], void=sc["void"], invalid=sc["invalid"], want_planes=True)
    env = _render(hand_scene, name, law)
    assert torch.equal(plain[1], env[1]) and torch.equal(plain[2], env[2])
    src = image_env_cases.reference(name, law, True)["src"].view(sc["height"], sc["width"], -1)
    bad = torch.as_tensor(image_env_cases.sensitive(name, law, True))
    kept = (src != image_env_ref.ENV).all(2) & ~bad
    gone = (src == image_env_ref.ENV).all(2) & ~bad
    assert kept.sum() > 100 and gone.sum() > 100
    assert torch.equal(plain[0].cpu()[kept], env[0].cpu()[kept])
    assert (plain[0].cpu()[gone] == sc["void"]).all() and (env[0].cpu()[gone] != sc["void"]).any(1).all()


def test_without_the_keyword_the_old_entry_point_runs_and_gives_its_bits(hand_scene, monkeypatch):
    name, law = "v5", LAWS[1]
    sc = image_cases.scene(name)
    kw = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"], want_planes=True)
    before = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], **kw)
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, fn):
            if fn.startswith("drt_render_image"):
                called.append(fn)
            return getattr(lib, fn)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    none = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], environment=None, **kw)
    assert called == ["drt_render_image"]
    _render(hand_scene, name, law)
    assert called == ["drt_render_image", "drt_render_image_env"]
    for a, b in zip(before, none):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- bands, repeats, modes
def _small_view(scene, height, width, s, with_screen, **kw):
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, height, width)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    return scene.render_image(cam, height, width, screen if with_screen else None, image_cases.texture(3) if with_screen else None, supersample=s, max_bounces=6,
                              tir="reflect", refraction="snell", void=0.25, invalid=0.75, want_planes=True, environment=image_env_cases.environment(3),
                              reflection=True, **kw)


@pytest.mark.parametrize("with_screen", [True, False], ids=SCREEN_IDS)
def test_bands_give_the_bits_of_the_whole_image(hand_scene, with_screen):
    """7 x 5 pixels at s = 3 in single rows, and 32 x 32 at s = 2 in bands of nine rows (the last of five)."""
    for height, width, s, cap, n_bands in ((7, 5, 3, 5 * 9, 7), (32, 32, 2, 9 * 32 * 4 + 3, 4)):
        assert len(render.plan_bands(height, width, s, cap)) == n_bands
        whole = _small_view(hand_scene, height, width, s, with_screen)
        banded = _small_view(hand_scene, height, width, s, with_screen, max_samples=cap)
        for a, b in zip(whole, banded):
            assert torch.equal(a, b)
        assert whole[1].max() == 1 and 0 < whole[2].mean() < whole[1].mean() < 1 and 0 < whole[3].mean() < whole[2].mean()


@pytest.mark.parametrize("reflection", [False, True], ids=["no-reflection", "reflection"])
def test_two_runs_and_the_deterministic_mode_give_the_same_bits(hand_scene, reflection):
    a = _render(hand_scene, "v41", LAWS[2], reflection=reflection)
    b = _render(hand_scene, "v41", LAWS[2], reflection=reflection)
    was = det.enable(True)
    try:
        c = _render(hand_scene, "v41", LAWS[2], reflection=reflection)
    finally:
        det.enable(was)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    only = _render(hand_scene, "v41", LAWS[2], want_planes=False, reflection=reflection)
    assert isinstance(only, torch.Tensor) and torch.equal(only, a[0])
    on_device = render.Environment(torch.as_tensor(image_env_cases.environment(3).texels).cuda(), image_env_ref.rotation())
    assert torch.equal(_render(hand_scene, "v41", LAWS[2], environment=on_device, reflection=reflection)[0], a[0])


def test_the_rotation_turns_the_picture(hand_scene):
    """A constant environment gives the throughput whatever the rotation: 1 on a direct pixel, T on a through one; a random one gives
    another picture under another rotation, with the same planes."""
    sc = image_cases.scene("v5")
    ones = np.ones((4, 8, 3), np.float32)
    a = _render(hand_scene, "v5", LAWS[0], False, render.Environment(ones, render.Environment.yaw(20.0)))
    b = _render(hand_scene, "v5", LAWS[0], False, render.Environment(ones, image_env_ref.rotation()))
    assert torch.equal(a[0], b[0])
    direct = a[1] == 0
    assert direct.sum() > 400 and (a[0][direct] == 1).all()
    only = a[2] == 1
    assert only.sum() > 50 and (a[0][only] > 0).all() and (a[0][only] < 1).any() and (a[0] <= 1).all()
    env = image_env_cases.environment(3)
    c = _render(hand_scene, "v5", LAWS[0], False, render.Environment(env.texels, render.Environment.yaw(20.0)))
    d = _render(hand_scene, "v5", LAWS[0], False, env)
    assert not torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    assert sc["s"] == 2


# --------------------------------------------------------------------------------------------------------------------- other paths
def test_a_scene_without_triangles_gives_a_pure_environment_image():
    sc = image_cases.scene("v5")
    scene = Render.Scene(image_cases.hand(), 0)
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    image, hit, through, reflect = _render(scene, "v5", LAWS[2], False, reflection=True)
    assert not reflect.any()                               # no surface, no reflection
    env = image_env_cases.environment(3)
    o, d = image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
    ref = image_ref.pixel_mean(image_env_ref.lookup(env.texels, env.rotation, d), sc["s"]).view(sc["height"], sc["width"], 3)
    assert not hit.any() and not through.any()
    assert (image.cpu().double() - ref.double()).abs().max() <= image_env_cases.tolerance("v5", LAWS[2], False)
    assert ref.std() > 0.01


def test_a_captured_call_replays_with_the_same_bits(hand_scene):
    sc = image_cases.scene("v5")
    env = image_env_cases.environment(3)
    dev = render.Environment(torch.as_tensor(env.texels).cuda(), env.rotation)      # on the device already: the capture sees no host copy
    tex = torch.as_tensor(sc["texture"]).cuda()
    kw = dict(supersample=sc["s"], max_bounces=6, tir="reflect", refraction="snell", void=sc["void"], invalid=sc["invalid"], want_planes=True, environment=dev,
              reflection=True)
    eager = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, **kw)
    for t in held:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, held):
        assert torch.equal(a, b)


def test_a_workspace_that_would_grow_under_capture_is_refused():
    """The environment call grows nothing of its own: the refusal is the forward wavefront's, with this entry point's name."""
    scene = Render.Scene(image_cases.hand(), 0)
    env = image_env_cases.environment(3)
    dev = render.Environment(torch.as_tensor(env.texels).cuda(), env.rotation)
    _render(scene, "v5", LAWS[0], False, dev, supersample=1)      # the workspace now holds 32 x 32 samples
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="drt_render_image_env.*eagerly before capturing"):
        with torch.cuda.graph(g):
            _render(scene, "v5", LAWS[0], False, dev)             # four times as many
    torch.cuda.synchronize()
    _check_against("v5", LAWS[0], False, _render(scene, "v5", LAWS[0], False))


def test_other_calls_on_the_scene_keep_their_bits():
    """The workspace is shared with the call of before and with the loss: each gives the same bits before and after an environment call."""
    mesh = image_cases.hand()
    hand_scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    hand_scene.update_verticex(V)
    sc = image_cases.scene("v5")
    law = LAWS[2]
    kw = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"])
    target = torch.as_tensor(image_cases.reference("v5", law, True)["image"]).cuda()
    was = det.enable(True)
    try:
        def others():
            img = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], **kw)
            loss = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target * 0.5, **kw)
            g, = torch.autograd.grad(loss, V)
            return [img, loss.detach().clone(), g.clone()]

        before = others()
        env = _render(hand_scene, "v5", law, reflection=True)
        after = others()
    finally:
        det.enable(was)
    assert before[1].item() > 0 and before[2].any()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    _check_against("v5", law, True, env, True)


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_output_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_env")
    sc = image_cases.scene("v5")
    envo = image_env_cases.environment(3)
    a = render.check_render_args(sc["camera_M"], 16, 16, sc["screen"], sc["texture"], 2, environment=envo)
    tex = torch.as_tensor(a["texture"], device="cuda")
    env = torch.as_tensor(envo.texels, device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    image = torch.full((16, 16, 3), 7.0, dtype=torch.float32, device="cuda")
    planes = [torch.full((16, 16), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    base = dict(y0=0, y1=16, s=2, fresnel=1, screen=a["screen"].ctypes.data, tex=tex.data_ptr(), channels=3, env=env.data_ptr(), env_h=env.shape[0],
                env_w=env.shape[1], rot=envo.packed(), reflection=1)

    def call(**kw):
        p = dict(base, **kw)
        rot = None if p["rot"] is None else np.ascontiguousarray(p["rot"], dtype=np.float64)
        return lib.drt_render_image_env(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, 16, 16, p["y0"], p["y1"], p["s"], IOR, EXT, 4, 3, p["fresnel"],
                                        p["screen"], p["tex"], tex.shape[0], tex.shape[1], p["channels"], a["void"].ctypes.data, a["invalid"].ctypes.data,
                                        image.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(), p["env"], p["env_h"], p["env_w"],
                                        None if rot is None else rot.ctypes.data, p["reflection"], planes[2].data_ptr(), torch.cuda.current_stream().cuda_stream)

    skew = envo.packed().copy()
    skew[0:3] += 1e-9 * skew[3:6]
    bad = [(dict(env=None), "d_env"), (dict(env=None, screen=None, tex=None), "d_env"), (dict(env_h=1), "env_h"), (dict(env_w=1), "env_w"), (dict(rot=None), "env_rot9"), (dict(rot=skew), "env_rot9"),
           (dict(rot=np.zeros(9)), "env_rot9"), (dict(reflection=2), "reflection"), (dict(reflection=-1), "reflection"), (dict(reflection=1, fresnel=0), "fresnel"),
           (dict(screen=None), "screen9"),
           (dict(tex=None), "d_texture"), (dict(s=5), "supersample"), (dict(channels=2), "channels"), (dict(y0=9, y1=3), "band")]
    for kw, word in bad:
        assert call(**kw) == -1, kw                        # DRT_E_INVALID
        assert word in lib.drt_last_error().decode(), (kw, lib.drt_last_error())
    torch.cuda.synchronize()
    assert (image == 7).all() and all((p == 7).all() for p in planes)
    # the good call writes its band and nothing else; without a screen the texture's sides are not read
    assert call(y0=3, y1=9) == 0
    torch.cuda.synchronize()
    assert (image[:3] == 7).all() and (image[9:] == 7).all() and (image[3:9] != 7).all() and (planes[0][3:9] <= 1).all() and (planes[1][:3] == 7).all()
    assert (planes[2][3:9] <= 1).all() and (planes[2][3:9] > 0).any() and (planes[2][:3] == 7).all() and (planes[2][9:] == 7).all()
    with_screen = image.clone()
    assert call(y0=3, y1=9, reflection=0) == 0
    torch.cuda.synchronize()
    assert (planes[2][3:9] == 0).all() and (planes[2][:3] == 7).all() and (image[3:9] <= with_screen[3:9]).all() and not torch.equal(image, with_screen)
    assert call(screen=None, tex=None) == 0
    torch.cuda.synchronize()
    assert (image != 7).all() and not torch.equal(image[3:9], with_screen[3:9])
