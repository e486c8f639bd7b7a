"""GPU: Scene.image_loss_views_fused on a binding with an environment -- the photometric image term of several views in front of ONE
environment map, with the optional outer-surface reflection, as one forward wavefront, one reflection pass and one adjoint pass
(drt_render_image_loss_views_env, drt_amd/csrc/drt_image_views_env.hip).  The law is nothing new: the result is the SUM
over the listed views of what drt_render_image_loss_env gives for each, so the call is checked

  * against the SUM of the restatement's results of the views v5 and v41 (tests/image_env_cases.loss_reference) under the three laws, with
    and without a screen, with and without the reflection, with the tolerances of tests/image_loss_cases.py: the loss LOSS_REL, the
    gradients ``close``, the count exact; one view alone is outside ``close``;
  * against the single-view call through the C ABI into the SAME accumulators, reflection on: bit for bit in deterministic mode,
    BAND_REL = 1e-12 in float64 mode (as tests/test_gpu_image_views.py) -- this is where a reflected ray formed with the row of the tall
    image instead of the row of its view would show: every view but the first of a list would reflect off the wrong pixel's ray;
  * band by band against the unbanded call, with a band that straddles the view border and with single-row bands."""
import ctypes

import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_loss_cases as cases
from conftest import IOR
from drt_amd import _lib, det, diffrender as Render, render, views

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAWS = image_cases.LAWS
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
LOSS_REL = cases.LOSS_REL
BAND_REL = 1e-12
PAIR = ("v5", "v41")


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


def _pair_capture(law, with_screen=True, reflection=True):
    """The views v5 and v41 (32 x 32, s = 2, C = 3, each with its own Screen.behind, or without screens) in the room of
    image_env_cases, as a capture of two views, ids 0 and 1; the targets are the restatement's images at IOR 1.55."""
    scs = [image_cases.scene(name) for name in PAIR]
    return dict(cams=[sc["camera_M"] for sc in scs], screens=[sc["screen"] for sc in scs] if with_screen else None, H=32, W=32, s=2,
                tex=scs[0]["texture"] if with_screen else None, env=image_env_cases.environment(3),
                targets=np.stack([image_env_cases.loss_target(name, law, with_screen, reflection) for name in PAIR]), weights=None, void=scs[0]["void"],
                invalid=scs[0]["invalid"])


def _small_capture():
    """Three views of 7 x 5 at s = 3 with one channel, random targets and a weight plane with zeros in it."""
    center, extent = image_cases.frame()
    cams = [image_cases.camera(v, 7, 5) for v in (5, 23, 41)]
    rng = np.random.default_rng(17)
    weights = rng.random((3, 7, 5), dtype=np.float32) + 0.5
    weights[:, :, 0] = 0.0
    return dict(cams=cams, screens=[render.Screen.behind(c, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN) for c in cams], H=7, W=5, s=3,
                tex=image_cases.texture(1), env=image_env_cases.environment(1), targets=rng.random((3, 7, 5), dtype=np.float32), weights=weights, void=0.25,
                invalid=0.75)


def _bind(scene, cap):
    return scene.bind_image_views(cap["cams"], cap["H"], cap["W"], cap["screens"], cap["targets"], cap["weights"], environment=cap["env"])


def _call(scene, binding, cap, ids, law=LAWS[0], reflection=True, ior=True, scale=None, **kw):
    """dict(loss, grad_V, g_int, g_ext, count) of one image_loss_views_fused call, on the device."""
    args = dict(supersample=cap["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=cap["void"], invalid=cap["invalid"], reflection=reflection)
    args.update(kw)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True) if ior else None
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True) if ior else None
    loss = scene.image_loss_views_fused(binding, ids, cap["tex"], ior_int=ii, ior_ext=ie, **args)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), grad_V=None)
    wrt = ([scene.vertices] if args.get("vertices", True) else []) + ([ii, ie] if ior else [])
    g = list(torch.autograd.grad(loss if scale is None else loss * scale, wrt))
    if args.get("vertices", True):
        res["grad_V"] = g.pop(0).clone()
    if ior:
        res["g_int"], res["g_ext"] = g[0].clone(), g[1].clone().cpu()
    return res


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("reflection", [False, True], ids=["no-reflection", "reflection"])
@pytest.mark.parametrize("with_screen", [True, False], ids=["screen", "no-screen"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_two_views_in_one_call_against_the_sum_of_the_restatement(hand_scene, law, with_screen, reflection):
    cap = _pair_capture(law, with_screen, reflection)
    got = _call(hand_scene, _bind(hand_scene, cap), cap, [0, 1], law, reflection)
    refs = [image_env_cases.loss_reference(name, law, with_screen, reflection) for name in PAIR]
    want = {k: sum(r[k] for r in refs) for k in ("loss", "grad_V", "g_int", "g_ext", "count")}
    rel = abs(float(got["loss"]) - want["loss"]) / want["loss"]
    print(f"loss {float(got['loss']):.12e} summed restatement {want['loss']:.12e} relative difference {rel:.2e}; g_int {float(got['g_int']):.9e} / "
          f"{want['g_int']:.9e}, g_ext {float(got['g_ext']):.9e} / {want['g_ext']:.9e}, max |grad_V| {np.abs(want['grad_V']).max():.3e} differs by "
          f"{np.abs(got['grad_V'].cpu().numpy() - want['grad_V']).max():.2e}; count {got['count']} / {want['count']}")
    assert got["count"] == want["count"] > 0
    assert rel <= LOSS_REL
    assert cases.close(got["grad_V"].cpu().numpy(), want["grad_V"])
    assert cases.close(float(got["g_int"]), want["g_int"]) and cases.close(float(got["g_ext"]), want["g_ext"])
    assert not cases.close(got["grad_V"].cpu().numpy(), refs[0]["grad_V"])                # (one view alone is outside the tolerance)


# ------------------------------------------------------------------------------------------------ against the single-view call, C ABI
class _Acc:
    """One set of accumulators of the current mode: loss, vertex gradient, IOR partials (det.scalar / det.acc) and the count."""

    def __init__(self, V):
        self.loss, self.grad, self.ior = det.scalar(V.device), det.acc(V), det.acc(torch.empty(2, dtype=torch.float64, device=V.device))
        self.count = torch.zeros((), dtype=torch.int64, device=V.device)

    def raw(self):
        return [t.clone() for t in (self.loss, self.grad, self.ior, self.count)]

    def values(self, V):
        return [det.value(self.loss).clone(), det.value(self.grad, V).clone(), det.value(self.ior, torch.empty(2, dtype=torch.float64)).clone()]


class _Abi:
    """A capture on the device with the two calls of the C ABI on it, reflection on."""

    def __init__(self, scene, cap, law):
        self.scene, self.cap, self.law = scene, cap, law
        self.binding = b = _bind(scene, cap)
        self.V = scene.vertices.detach().contiguous()
        self.tex = None if cap["tex"] is None else torch.as_tensor(render.check_texture(cap["tex"]), device="cuda").contiguous()
        C = b.channels
        self.void, self.invalid = np.full(C, float(cap["void"])), np.full(C, float(cap["invalid"]))
        self.flags = int(law[1] == "reflect") | (2 if law[2] == "snell" else 0)
        self.cam21 = [np.ascontiguousarray(b.args["cameras"][k]) for k in range(b.n)]
        self.scr9 = [np.ascontiguousarray(b.args["screens"][k]) for k in range(b.n)]
        self.tex_args = (None, 0, 0, C) if self.tex is None else (self.tex.data_ptr(), self.tex.shape[0], self.tex.shape[1], C)
        self.env_args = (b.env.data_ptr(), b.env.shape[0], b.env.shape[1], b.env_rot.ctypes.data)

    def single(self, view, acc):
        cap, b = self.cap, self.binding
        rc = _lib.lib().drt_render_image_loss_env(self.scene.optix_mesh._h, self.V.data_ptr(), self.cam21[view].ctypes.data, cap["H"], cap["W"], 0, cap["H"], cap["s"], IOR,
                                                  EXT, self.law[0], self.flags, 1, None if self.tex is None else self.scr9[view].ctypes.data, *self.tex_args,
                                                  self.void.ctypes.data, self.invalid.ctypes.data, b.targets[view].data_ptr(),
                                                  None if b.weights is None else b.weights[view].data_ptr(), acc.loss.data_ptr(), acc.grad.data_ptr(), acc.ior.data_ptr(),
                                                  None, acc.count.data_ptr(), *self.env_args, 1, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.lib().drt_last_error()

    def views(self, ids, acc, **kw):
        cap, b = self.cap, self.binding
        p = dict(binding=b._h, ids=ids, k=len(ids), r0=0, r1=len(ids) * cap["H"], s=cap["s"], targets=b.targets.data_ptr(), loss=acc.loss.data_ptr(), fresnel=1,
                 tex=self.tex_args, env=self.env_args[0], env_h=self.env_args[1], rot=self.env_args[3], reflection=1)
        p.update(kw)
        arr = (ctypes.c_int * max(1, len(p["ids"])))(*p["ids"])
        return _lib.lib().drt_render_image_loss_views_env(self.scene.optix_mesh._h, self.V.data_ptr(), p["binding"], arr, p["k"], p["r0"], p["r1"], p["s"], IOR, EXT,
                                                          self.law[0], self.flags, p["fresnel"], *p["tex"], self.void.ctypes.data, self.invalid.ctypes.data, p["targets"],
                                                          _lib.ptr(b.weights), p["loss"], acc.grad.data_ptr(), acc.ior.data_ptr(), acc.count.data_ptr(), p["env"],
                                                          p["env_h"], self.env_args[2], p["rot"], p["reflection"], torch.cuda.current_stream().cuda_stream)


def _exact_cases(scene):
    """(abi, ids): [0, 1], [1, 0], [0, 0] (a repeat: twice one view), k = 1, the pair without screens, and three small weighted views."""
    pair = _Abi(scene, _pair_capture(LAWS[2]), LAWS[2])
    bare = _Abi(scene, _pair_capture(LAWS[1], with_screen=False), LAWS[1])
    small = _Abi(scene, _small_capture(), LAWS[1])
    return [(pair, [0, 1]), (pair, [1, 0]), (pair, [0, 0]), (pair, [1]), (bare, [1, 0]), (small, [2, 0, 1])]


def _both(abi, ids):
    one, many = _Acc(abi.V), _Acc(abi.V)
    for v in ids:
        abi.single(v, one)
    assert abi.views(ids, many) == 0, _lib.lib().drt_last_error()
    torch.cuda.synchronize()
    return one, many


def test_one_call_gives_the_bits_of_the_single_view_calls_in_deterministic_mode(hand_scene, deterministic):
    for abi, ids in _exact_cases(hand_scene):
        one, many = _both(abi, ids)
        assert int(one.count) > 0 and one.values(abi.V)[1].abs().max() > 0 and float(one.values(abi.V)[0]) > 0
        for a, b in zip(one.raw(), many.raw()):
            assert a.dtype == b.dtype and torch.equal(a, b), ids
    abi = _exact_cases(hand_scene)[0][0]
    twice, once = _both(abi, [0, 0])[1], _both(abi, [0])[1]
    assert int(twice.count) == 2 * int(once.count) and torch.equal(twice.values(abi.V)[1], 2 * once.values(abi.V)[1])


def test_one_call_agrees_with_the_single_view_calls_in_float64_mode(hand_scene):
    assert not det.on()
    for abi, ids in _exact_cases(hand_scene):
        one, many = _both(abi, ids)
        assert int(one.count) == int(many.count) > 0
        for a, b in zip(one.raw()[:3], many.raw()[:3]):
            assert a.dtype == torch.float64 and (a - b).abs().max() <= BAND_REL * a.abs().max(), ids


# ------------------------------------------------------------------------------------------------------------------ bands, other modes
def _banded_cases(scene):
    """(whole, banded) results: the pair in bands of nine rows -- (27, 36) straddles the border between the two views -- and the three
    small views, one of them twice, in single rows."""
    assert (27, 36) in render.plan_bands(64, 32, 2, 9 * 128 + 5) and render.plan_bands(28, 5, 3, 45) == [(r, r + 1) for r in range(28)]
    pair, small = _pair_capture(LAWS[2]), _small_capture()
    for cap, ids, law, cap_samples in ((pair, [0, 1], LAWS[2], 9 * 128 + 5), (small, [1, 1, 2, 0], LAWS[1], 45)):
        b = _bind(scene, cap)
        yield _call(scene, b, cap, ids, law), _call(scene, b, cap, ids, law, max_samples=cap_samples)


def test_bands_give_the_bits_of_the_unbanded_call_in_deterministic_mode(hand_scene, deterministic):
    for whole, banded in _banded_cases(hand_scene):
        assert float(whole["loss"]) > 0 and whole["grad_V"].abs().max() > 0 and whole["count"] == banded["count"] > 0
        for k in ("loss", "grad_V", "g_int", "g_ext"):
            assert torch.equal(whole[k], banded[k])


def test_bands_agree_with_the_unbanded_call_in_float64_mode(hand_scene):
    assert not det.on()
    for whole, banded in _banded_cases(hand_scene):
        assert whole["count"] == banded["count"]
        for k in ("loss", "grad_V", "g_int", "g_ext"):
            assert (whole[k] - banded[k]).abs().max() <= BAND_REL * whole[k].abs().max()


def test_without_vertices_and_with_a_scaled_backward(hand_scene, deterministic):
    cap = _pair_capture(LAWS[1])
    b = _bind(hand_scene, cap)
    full, fixed = _call(hand_scene, b, cap, [1, 0], LAWS[1]), _call(hand_scene, b, cap, [1, 0], LAWS[1], vertices=False)
    assert fixed["grad_V"] is None and fixed["count"] == full["count"] > 0
    for k in ("loss", "g_int", "g_ext"):
        assert torch.equal(full[k], fixed[k])
    scaled = _call(hand_scene, b, cap, [1, 0], LAWS[1], scale=-2.5)
    for k in ("grad_V", "g_int", "g_ext"):
        assert full[k].abs().max() > 0 and torch.equal(scaled[k], full[k] * -2.5)


def test_a_scene_without_faces_gives_the_summed_loss_of_the_environment_images_and_zero_gradients():
    scene = _fresh()
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    cap = _pair_capture(LAWS[2], with_screen=False)
    cap["targets"] = np.zeros_like(cap["targets"])
    got = _call(scene, _bind(scene, cap), cap, [0, 1], LAWS[2])
    want = 0.0
    for cam in cap["cams"]:
        image = scene.render_image(cam, 32, 32, None, None, supersample=2, environment=cap["env"])
        want += float((image.double() ** 2).sum())
    assert want > 0 and abs(float(got["loss"]) - want) <= 1e-6 * want
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0


def test_a_captured_replay_gives_the_eager_bits(deterministic):
    scene = _fresh()
    V = scene.vertices
    cap = _pair_capture(LAWS[1])
    cap["env"] = render.Environment(torch.as_tensor(cap["env"].texels).cuda(), cap["env"].rotation)
    b = _bind(scene, cap)
    tex = torch.as_tensor(cap["tex"]).cuda()

    def step(ids=(0, 1), s=2):
        loss = scene.image_loss_views_fused(b, list(ids), tex, supersample=s, max_bounces=6, tir="reflect", void=cap["void"], invalid=cap["invalid"], reflection=True)
        return loss.detach(), torch.autograd.grad(loss, V)[0]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and eager[1].abs().max() > 0
    for x, y in zip(eager, static):
        assert torch.equal(x, y)
    g2 = torch.cuda.CUDAGraph()                    # a workspace that would have to grow inside a capture is refused, by the new entry point's name
    with pytest.raises(_lib.DrtError, match="drt_render_image_loss_views_env.*eagerly before capturing"):
        with torch.cuda.graph(g2):
            step(ids=(0, 1, 1, 0), s=4)
    torch.cuda.synchronize()


def test_calls_that_share_the_workspace_give_the_bits_of_fresh_scenes(deterministic):
    """A single-view environment call, an environment views call, a clear views call, paths_ray_loss_fused and an environment views call
    again on ONE scene: ray lists, parked rows, tape, state bytes, the two spare counter words and the pixel seeds are shared, every
    result is that of the same call on a scene built for it alone."""
    pair, small = _pair_capture(LAWS[2]), _small_capture()
    center, _ = image_cases.frame()
    cam = image_cases.camera(5, 24, 20)
    o, d = (t.cuda() for t in views.generate_ray(24, 20, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((24 * 20, 3)) * 40.0 + np.asarray(center) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(24 * 20) > 0.1, device="cuda")

    def single(scene):
        sc = image_cases.scene("wide")
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], image_env_cases.loss_target("wide", LAWS[2], True, True),
                                      supersample=sc["s"], max_bounces=6, tir="reflect", refraction="snell", void=sc["void"], invalid=sc["invalid"],
                                      environment=image_env_cases.environment(1), reflection=True)
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    def many(cap, ids, law):
        def run(scene):
            got = _call(scene, _bind(scene, cap), cap, ids, law)
            return got["loss"], got["grad_V"], got["g_int"], got["g_ext"]
        return run

    def clear(scene):
        b = scene.bind_image_views(pair["cams"], 32, 32, pair["screens"], pair["targets"])
        loss = scene.image_loss_views_fused(b, [1, 0], pair["tex"], supersample=2, max_bounces=6, tir="reflect", refraction="snell", void=pair["void"],
                                            invalid=pair["invalid"])
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    def paths(scene):
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    steps = [single, many(small, [2, 1, 0], LAWS[1]), clear, paths, many(pair, [1, 0], LAWS[2]), many(small, [0], LAWS[1])]
    scene = _fresh()
    got = [step(scene) for step in steps]
    for step, mine in zip(steps, got):
        alone = step(_fresh())
        assert float(mine[0]) > 0 and mine[1].any() and len(alone) == len(mine)
        for x, y in zip(alone, mine):
            assert torch.equal(x, y)


def test_a_binding_without_an_environment_makes_the_call_of_before(hand_scene, monkeypatch, deterministic):
    cap = _pair_capture(LAWS[1])
    b = hand_scene.bind_image_views(cap["cams"], 32, 32, cap["screens"], cap["targets"])
    kw = dict(supersample=2, max_bounces=6, tir="reflect", void=cap["void"], invalid=cap["invalid"])
    before = hand_scene.image_loss_views_fused(b, [0, 1], cap["tex"], **kw).detach().clone()
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, fn):
            if fn.startswith("drt_render_image"):
                called.append(fn)
            return getattr(lib, fn)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    again = hand_scene.image_loss_views_fused(b, [0, 1], cap["tex"], reflection=False, **kw)
    assert called == ["drt_render_image_loss_views"] and torch.equal(again.detach(), before)
    hand_scene.image_loss_views_fused(_bind(hand_scene, cap), [0, 1], cap["tex"], **kw)
    assert called == ["drt_render_image_loss_views", "drt_render_image_loss_views_env"]


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_outputs_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_loss_views_env")
    was = det.enable(False)
    try:
        abi = _Abi(hand_scene, _pair_capture(LAWS[2]), LAWS[2])
        other = _bind(_fresh(), abi.cap)
        acc = _Acc(abi.V)
        skew = abi.binding.env_rot.copy()
        skew[0:3] += 1e-9 * skew[3:6]
        bad = [(dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(ids=[0, 2]), "view_ids"), (dict(ids=[-1, 0]), "view_ids"), (dict(r0=5, r1=5), "band"),
               (dict(r0=9, r1=3), "band"), (dict(r1=65), "band"), (dict(r0=-1), "band"), (dict(binding=None), "views"), (dict(binding=other._h), "another scene"),
               (dict(targets=None), "d_targets"), (dict(loss=None), "d_loss"), (dict(s=0), "supersample"), (dict(s=5), "supersample"), (dict(env=None), "d_env"),
               (dict(env=None, tex=(None, 0, 0, 3)), "d_env"), (dict(env_h=1), "env_h"), (dict(rot=None), "env_rot9"), (dict(rot=skew.ctypes.data), "env_rot9"),
               (dict(reflection=2), "reflection"), (dict(reflection=1, fresnel=0), "fresnel"), (dict(tex=(abi.tex_args[0], 4, 4, 2)), "channels")]
        for kw, word in bad:
            assert abi.views(kw.pop("ids", [0, 1]), acc, **kw) == -1, kw             # DRT_E_INVALID
            assert word in lib.drt_last_error().decode(), (kw, lib.drt_last_error())
        torch.cuda.synchronize()
        assert float(acc.loss) == 0 and not acc.grad.any() and not acc.ior.any() and int(acc.count) == 0
        assert abi.views([0, 1], acc, r0=20, r1=41) == 0                              # the good call adds into its targets
        torch.cuda.synchronize()
        first = acc.raw()
        assert float(acc.loss) > 0 and acc.grad.any() and acc.ior.all() and int(acc.count) > 0
        assert abi.views([0, 1], acc, r0=20, r1=41, tex=(None, 0, 0, 3)) == 0         # ... and one without the screen adds again
        torch.cuda.synchronize()
        assert int(acc.count) == 2 * int(first[3]) and float(acc.loss) > float(first[0])
    finally:
        det.enable(was)
