"""GPU: Scene.image_loss_fused with ``environment`` / ``reflection`` -- the photometric loss of the image in front of an environment map,
with its vertex and IOR gradients (drt_render_image_loss_env, drt_amd/csrc/drt_image_env.hip) -- against the restatement
tests/image_env_ref.py (autograd) on the cases of tests/image_env_cases.py: the three scenes under the three laws, with and without a
screen, with and without the outer-surface reflection, target rendered by the restatement at IOR 1.55.

Tolerances are tests/image_loss_cases.py's: the loss within LOSS_REL (3e-14), gradients within ``close`` (1e-9 of the largest entry, at
most 1e-5); the count (every through sample) exact.  tests/test_image_env_host.py holds the header to the same restatement on the host
(measured there: loss 5e-16 to 4e-15 relative, gradients 5e-14 to 5e-13 absolute)."""
import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_loss_cases
from conftest import IOR
from drt_amd import _lib, det, diffrender as Render, render, views

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAWS = image_cases.LAWS
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]


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


def _scene():
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene


@pytest.fixture(scope="module")
def hand_scene():
    return _scene()


def _call(scene, name, law, with_screen=True, reflection=True, ior=True, scale=None, target=None, **kw):
    """dict(loss, grad_V, g_int, g_ext, count[, image]) of one call on a case of image_env_cases."""
    sc = image_cases.scene(name)
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"],
                environment=image_env_cases.environment(sc["texture"].shape[2]), reflection=reflection)
    args.update(kw)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True) if ior else None
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True) if ior else None
    out = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None, sc["texture"] if with_screen else None,
                                 image_env_cases.loss_target(name, law, with_screen, reflection) if target is None else target, ior_int=ii, ior_ext=ie, **args)
    loss, image = out if args.get("want_image") else (out, None)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), image=image)
    wrt = ([scene.vertices] if args.get("vertices", True) else []) + ([ii, ie] if ior else [])
    g = list(torch.autograd.grad(loss if scale is None else loss * scale, wrt))
    res["grad_V"] = g.pop(0).clone() if args.get("vertices", True) else None
    if ior:
        res["g_int"], res["g_ext"] = g[0].clone(), g[1].clone()
    return res


def _check_against(got, ref):
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; g_int {float(got['g_int']):.9e} / {ref['g_int']:.9e}, "
          f"g_ext {float(got['g_ext']):.9e} / {ref['g_ext']:.9e}, max |grad_V| {np.abs(ref['grad_V']).max():.3e} differs by "
          f"{np.abs(got['grad_V'].cpu().numpy() - ref['grad_V']).max():.2e}; count {got['count']} / {ref['count']}")
    assert got["count"] == ref["count"]
    assert rel <= image_loss_cases.LOSS_REL
    assert image_loss_cases.close(got["grad_V"].cpu().numpy(), ref["grad_V"])
    assert image_loss_cases.close(float(got["g_int"]), ref["g_int"]) and image_loss_cases.close(float(got["g_ext"]), ref["g_ext"])


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("reflection", [False, True], ids=["no-reflection", "reflection"])
@pytest.mark.parametrize("with_screen", [True, False], ids=["screen", "no-screen"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", list(image_cases.SCENES))
def test_loss_gradients_and_count_against_the_restatement(hand_scene, name, law, with_screen, reflection):
    ref = image_env_cases.loss_reference(name, law, with_screen, reflection)
    assert ref["loss"] > 0.5 and ref["count"] > 900 and np.abs(ref["grad_V"]).max() > 0.5
    _check_against(_call(hand_scene, name, law, with_screen, reflection), ref)


def test_a_weight_plane_and_the_image_of_render_image(hand_scene):
    name, law = "wide", LAWS[2]
    sc = image_cases.scene(name)
    w = image_loss_cases.half_weight(name)
    got = _call(hand_scene, name, law, weight=w, want_image=True)
    _check_against(got, image_env_cases.loss_reference(name, law, True, True, weighted=True))
    assert not got["grad_V"].cpu().numpy()[np.abs(image_env_cases.loss_reference(name, law, True, True, weighted=True)["grad_V"]).sum(1) == 0].any()
    image = hand_scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], supersample=sc["s"], max_bounces=law[0], tir=law[1],
                                    refraction=law[2], void=sc["void"], invalid=sc["invalid"], environment=image_env_cases.environment(1), reflection=True)
    assert torch.equal(got["image"], image)


# --------------------------------------------------------------------------------------------------------- bands, repeats, modes
def _small(scene, height, width, s, **kw):
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, height, width)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    target = np.random.default_rng(3).random((height, width, 3)).astype(np.float32)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    loss = scene.image_loss_fused(cam, height, width, screen, image_cases.texture(3), target, ior_int=ii, supersample=s, max_bounces=6, tir="reflect",
                                  refraction="snell", void=0.25, invalid=0.75, environment=image_env_cases.environment(3), reflection=True, **kw)
    gV, gi = torch.autograd.grad(loss, [scene.vertices, ii])
    return [loss.detach().clone(), gV.clone(), gi.clone(), scene.last_image_count.clone()]


def test_bands_and_repeats_give_the_same_bits_in_deterministic_mode(hand_scene, deterministic):
    """7 x 5 pixels at s = 3 in single rows, 32 x 32 at s = 2 in bands of nine rows; two runs."""
    for height, width, s, cap, n_bands in ((7, 5, 3, 5 * 9, 7), (32, 32, 2, 9 * 32 * 4 + 3, 4)):
        assert len(render.plan_bands(height, width, s, cap)) == n_bands
        whole, again, banded = _small(hand_scene, height, width, s), _small(hand_scene, height, width, s), _small(hand_scene, height, width, s, max_samples=cap)
        assert float(whole[0]) > 0 and whole[1].abs().max() > 0 and int(whole[3]) > 0
        for a, b, c in zip(whole, again, banded):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    whole, banded = _small(hand_scene, 32, 32, 2), _small(hand_scene, 32, 32, 2, max_samples=9 * 32 * 4 + 3)
    assert abs(float(whole[0]) - float(banded[0])) <= 1e-12 * float(whole[0]) and int(whole[3]) == int(banded[3])
    assert image_loss_cases.close(banded[1].cpu().numpy(), whole[1].cpu().numpy()) and image_loss_cases.close(float(banded[2]), float(whole[2]))


def test_without_vertices_and_with_a_scaled_backward(hand_scene, deterministic):
    name, law = "v5", LAWS[2]
    full = _call(hand_scene, name, law)
    fixed = _call(hand_scene, name, law, vertices=False)
    assert fixed["grad_V"] is None and torch.equal(fixed["loss"], full["loss"]) and fixed["count"] == full["count"]
    assert torch.equal(fixed["g_int"], full["g_int"]) and torch.equal(fixed["g_ext"], full["g_ext"])
    scaled = _call(hand_scene, name, law, scale=-2.5)
    assert torch.equal(scaled["grad_V"], full["grad_V"] * -2.5) and torch.equal(scaled["g_int"], full["g_int"] * -2.5)
    assert torch.equal(scaled["g_ext"], full["g_ext"] * -2.5)


def test_a_scene_without_faces_gives_the_loss_of_the_environment_image_and_zero_gradients():
    scene = _scene()
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    sc = image_cases.scene("v5")
    env = image_env_cases.environment(3)
    image = scene.render_image(sc["camera_M"], sc["height"], sc["width"], None, None, supersample=sc["s"], environment=env)
    target = np.zeros((sc["height"], sc["width"], 3), np.float32)
    got = _call(scene, "v5", LAWS[2], False, True, target=target)
    want = float((image.double() ** 2).sum())
    assert abs(float(got["loss"]) - want) <= 1e-6 * want and got["count"] == 0
    assert not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    scene = _scene()
    V = scene.vertices
    sc = image_cases.scene("v5")
    law = LAWS[1]
    envo = image_env_cases.environment(3)
    env = render.Environment(torch.as_tensor(envo.texels).cuda(), envo.rotation)
    tex, tgt = torch.as_tensor(sc["texture"]).cuda(), torch.as_tensor(image_env_cases.loss_target("v5", law, True, True)).cuda()

    def step(**kw):
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, **dict(dict(supersample=sc["s"], max_bounces=6,
                                      tir="reflect", void=sc["void"], invalid=sc["invalid"], environment=env, reflection=True), **kw))
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
    # the call grows no buffer of its own: a workspace that would have to grow inside a capture is refused by the forward wavefront, by name
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="drt_render_image_loss_env.*eagerly before capturing"):
        with torch.cuda.graph(g2):
            step(supersample=4)
    torch.cuda.synchronize()


def test_other_calls_on_the_scene_keep_their_bits(deterministic):
    """The workspace is shared with the clear loss and with paths_ray_loss_fused: each gives the same bits before and after an environment
    loss with its reflection pass."""
    scene = _scene()
    V = scene.vertices
    sc = image_cases.scene("v5")
    law = LAWS[2]
    kw = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"])
    cam = image_cases.camera(5, 48, 48)
    o, d = (t.cuda() for t in views.generate_ray(48, 48, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((48 * 48, 3)) * 40.0 + np.asarray(image_cases.frame()[0]) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(48 * 48) > 0.1, device="cuda")
    target = image_loss_cases.target("v5", law, True)

    def others():
        a = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, **kw)
        b = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        return [a.detach().clone(), torch.autograd.grad(a, V)[0].clone(), b.detach().clone(), torch.autograd.grad(b, V)[0].clone()]

    before = others()
    got = _call(scene, "v5", law)
    after = others()
    assert float(before[0]) > 0 and before[1].any() and float(before[2]) > 0 and before[3].any()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    _check_against(got, image_env_cases.loss_reference("v5", law, True, True))


def test_without_the_keywords_the_old_entry_point_runs_and_gives_its_bits(hand_scene, monkeypatch, deterministic):
    """(Deterministic accumulation, so that two runs of the old entry point can be compared bit for bit.)"""
    sc = image_cases.scene("v5")
    law = LAWS[1]
    kw = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"])
    target = image_loss_cases.target("v5", law, True)
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, fn):
            if fn.startswith("drt_render_image"):
                called.append(fn)
            return getattr(lib, fn)

    before = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, **kw).detach().clone()
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    none = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, environment=None, reflection=False, **kw)
    assert called == ["drt_render_image_loss"] and torch.equal(none.detach(), before)
    hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, environment=image_env_cases.environment(3), **kw)
    assert called == ["drt_render_image_loss", "drt_render_image_loss_env"]


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_outputs_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_loss_env")
    sc = image_cases.scene("v5")
    envo = image_env_cases.environment(3)
    a = render.check_render_args(sc["camera_M"], 16, 16, sc["screen"], sc["texture"], 2, environment=envo)
    tex, env = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(envo.texels, device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    target = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
    loss, gV, gi = (torch.full(shape, 7.0, dtype=torch.float64, device="cuda") for shape in ((), V.shape, (2,)))
    count = torch.full((), 7, dtype=torch.int64, device="cuda")
    base = dict(y0=0, y1=16, s=2, fresnel=1, screen=a["screen"].ctypes.data, tex=tex.data_ptr(), channels=3, env=env.data_ptr(), env_h=env.shape[0],
                env_w=env.shape[1], rot=envo.packed(), reflection=1, target=target.data_ptr(), loss=loss.data_ptr())

    def call(**kw):
        p = dict(base, **kw)
        rot = None if p["rot"] is None else np.ascontiguousarray(p["rot"], dtype=np.float64)
        return lib.drt_render_image_loss_env(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, 16, 16, p["y0"], p["y1"], p["s"], IOR, EXT, 4, 3,
                                             p["fresnel"], p["screen"], p["tex"], tex.shape[0], tex.shape[1], p["channels"], a["void"].ctypes.data,
                                             a["invalid"].ctypes.data, p["target"], None, p["loss"], gV.data_ptr(), gi.data_ptr(), None, count.data_ptr(), p["env"],
                                             p["env_h"], p["env_w"], None if rot is None else rot.ctypes.data, p["reflection"], torch.cuda.current_stream().cuda_stream)

    skew = envo.packed().copy()
    skew[0:3] += 1e-9 * skew[3:6]
    bad = [(dict(env=None), "d_env"), (dict(env=None, screen=None, tex=None), "d_env"), (dict(env_h=1), "env_h"), (dict(rot=None), "env_rot9"), (dict(rot=skew), "env_rot9"),
           (dict(reflection=2), "reflection"), (dict(reflection=1, fresnel=0), "fresnel"), (dict(screen=None), "screen9"), (dict(tex=None), "d_texture"),
           (dict(target=None), "d_target"), (dict(loss=None), "d_loss"), (dict(s=5), "supersample"), (dict(channels=2), "channels"), (dict(y0=9, y1=3), "band")]
    for kw, word in bad:
        assert call(**kw) == -1, kw                        # DRT_E_INVALID
        assert word in lib.drt_last_error().decode(), (kw, lib.drt_last_error())
    torch.cuda.synchronize()
    assert float(loss) == 7 and (gV == 7).all() and (gi == 7).all() and int(count) == 7
    assert call(y0=3, y1=9) == 0 and call(y0=3, y1=9, screen=None, tex=None) == 0
    torch.cuda.synchronize()
    assert float(loss) > 7 and (gV != 7).any() and (gi != 7).all() and int(count) > 7
