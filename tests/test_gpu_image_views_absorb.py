"""GPU: Scene.image_loss_views_fused with ``absorption`` -- absorbing glass in the photometric image term of several views, in front of their
screens, of one environment, or of both, with the optional outer-surface reflection (drt_render_image_loss_views_absorb,
drt_amd/csrc/drt_image_views_absorb.hip).  Nothing is new per sample; the product is, so the call is checked

  * against the SUM of the restatement's results of the views v5 and v41 (tests/image_views_absorb_cases.py) under the three laws and the five
    backgrounds, with the tolerances of tests/image_loss_cases.py: the loss LOSS_REL, the vertex, IOR and sigma gradients ``close``, the
    count exact -- the sigma partial is where light reflected off the outer surface, which never entered the object, could leak in;
  * with screens, against drt_render_image_loss_absorb view by view into the SAME accumulators through the C ABI: bit for bit in
    deterministic mode, BAND_REL = 1e-12 in float64 mode;
  * with sigma = 0, against drt_render_image_loss_views and drt_render_image_loss_views_env, bit for bit in deterministic mode -- while
    the sigma partial is NOT zero there and is the restatement's;
  * the images of ``want_images`` against render_image(absorption=) with screens, against the restatement's image in the room;
  * bands, the other modes, graph capture, the shared workspace and the C ABI's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import image_absorb_cases
import image_cases
import image_env_cases
import image_loss_cases as cases
import image_views_absorb_cases as vac
from conftest import IOR
from drt_amd import _lib, det, diffrender as Render, render, views

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAWS = image_cases.LAWS
LAW_IDS = [f"{k}-{t}-{r}" for k, t, r in LAWS]
LOSS_REL = cases.LOSS_REL
BAND_REL = 1e-12
PAIR = vac.PAIR
WHO = "drt_render_image_loss_views_absorb"
SIGMA3, SIGMA1 = image_absorb_cases.SIGMA3, image_absorb_cases.SIGMA1


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


def _pair_capture(law, kind="screen", reflection=False):
    """The views v5 and v41 (32 x 32, s = 2, C = 3) as a capture of two views, ids 0 and 1, in front of their screens, in the room of
    image_env_cases, or both; the targets are the restatement's images of clear glass at IOR 1.55."""
    scs = [image_cases.scene(name) for name in PAIR]
    return dict(cams=[sc["camera_M"] for sc in scs], screens=[sc["screen"] for sc in scs] if vac.has_screen(kind) else None, H=32, W=32, s=2,
                tex=scs[0]["texture"] if vac.has_screen(kind) else None, env=image_env_cases.environment(3) if vac.has_room(kind) else None,
                targets=np.stack([vac.target(name, law, kind, reflection) for name in PAIR]), weights=None, void=scs[0]["void"], invalid=scs[0]["invalid"],
                sigma=SIGMA3)


def _small_capture(room=False):
    """Four views of 7 x 5 at s = 3 with one channel, random targets and a weight plane with zeros in it; the tests list [2, 0, 3]."""
    center, extent = image_cases.frame()
    cams = [image_cases.camera(v, 7, 5) for v in (5, 17, 29, 41)]
    rng = np.random.default_rng(17)
    weights = rng.random((4, 7, 5), dtype=np.float32) + 0.5
    weights[:, :, 0] = 0.0
    return dict(cams=cams, screens=[render.Screen.behind(c, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN) for c in cams], H=7, W=5, s=3,
                tex=image_cases.texture(1), env=image_env_cases.environment(1) if room else None, targets=rng.random((4, 7, 5), dtype=np.float32), weights=weights,
                void=0.25, invalid=0.75, sigma=SIGMA1)


def _bind(scene, cap):
    more = {} if cap["env"] is None else {"environment": cap["env"]}
    return scene.bind_image_views(cap["cams"], cap["H"], cap["W"], cap["screens"], cap["targets"], cap["weights"], **more)


def _call(scene, binding, cap, ids, law=LAWS[0], reflection=False, ior=True, scale=None, sigma="cap", **kw):
    """dict(loss, grad_V, g_int, g_ext, g_sigma, count) of one image_loss_views_fused call, on the device."""
    args = dict(supersample=cap["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=cap["void"], invalid=cap["invalid"], reflection=reflection)
    args.update(kw)
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True) if ior else None
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True) if ior else None
    sg = None if sigma is None else torch.tensor(cap["sigma"] if isinstance(sigma, str) else sigma, dtype=torch.float64, requires_grad=True)
    out = scene.image_loss_views_fused(binding, ids, cap["tex"], ior_int=ii, ior_ext=ie, absorption=sg, **args)
    loss, images = out if isinstance(out, tuple) else (out, None)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), grad_V=None, images=images)
    wrt = ([scene.vertices] if args.get("vertices", True) else []) + ([ii, ie] if ior else []) + ([sg] if sg is not None else [])
    g = list(torch.autograd.grad(loss if scale is None else loss * scale, wrt))
    if args.get("vertices", True):
        res["grad_V"] = g.pop(0).clone()
    if ior:
        res["g_int"], res["g_ext"] = g.pop(0).clone(), g.pop(0).clone().cpu()
    if sg is not None:
        res["g_sigma"] = g.pop(0).clone()
    return res


KEYS = ("loss", "grad_V", "g_int", "g_ext", "g_sigma")


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("kind,reflection", vac.BACKGROUNDS, ids=[k + ("-reflection" if r else "") for k, r in vac.BACKGROUNDS])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_two_views_in_one_call_against_the_sum_of_the_restatement(hand_scene, law, kind, reflection):
    cap = _pair_capture(law, kind, reflection)
    got = _call(hand_scene, _bind(hand_scene, cap), cap, [0, 1], law, reflection)
    want = vac.summed(PAIR, law, kind, reflection)
    rel = abs(float(got["loss"]) - want["loss"]) / want["loss"]
    gs = got["g_sigma"].numpy()
    print(f"{law} {kind} reflection={reflection}: loss {float(got['loss']):.12e} summed restatement {want['loss']:.12e} relative difference {rel:.2e}; "
          f"g_int {float(got['g_int']):.9e} / {want['g_int']:.9e}, g_ext {float(got['g_ext']):.9e} / {want['g_ext']:.9e}, max |grad_V| "
          f"{np.abs(want['grad_V']).max():.3e} differs by {np.abs(got['grad_V'].cpu().numpy() - want['grad_V']).max():.2e}; g_sigma {gs} differs by "
          f"{np.abs(gs - want['g_sigma']).max():.2e}; count {got['count']} / {want['count']}")
    assert got["count"] == want["count"] > 0
    assert rel <= LOSS_REL
    assert cases.close(got["grad_V"].cpu().numpy(), want["grad_V"])
    assert cases.close(float(got["g_int"]), want["g_int"]) and cases.close(float(got["g_ext"]), want["g_ext"])
    assert cases.close(gs, want["g_sigma"])
    assert not cases.close(got["grad_V"].cpu().numpy(), vac.reference(PAIR[0], law, kind, reflection)["grad_V"])      # (one view alone is outside the tolerance)
    if reflection:                                       # (... and so is a sigma partial that takes the reflected light along)
        assert not cases.close(gs, vac.summed(PAIR, law, kind, True, sigma_sees_reflection=True)["g_sigma"])


# -------------------------------------------------------------------------------------------------------- against the other calls, C ABI
class _Acc:
    """One set of accumulators of the current mode: loss, vertex gradient, IOR partials, sigma partials (det.scalar / det.acc), the count."""

    def __init__(self, V, C):
        self.loss, self.grad, self.ior = det.scalar(V.device), det.acc(V), det.acc(torch.empty(2, dtype=torch.float64, device=V.device))
        self.sigma = det.acc(torch.empty(C, dtype=torch.float64, device=V.device))
        self.count = torch.zeros((), dtype=torch.int64, device=V.device)
        self.C = C

    def raw(self, sigma=True):
        return [t.clone() for t in (self.loss, self.grad, self.ior, self.count) + ((self.sigma,) if sigma else ())]

    def sigma_value(self):
        return det.value(self.sigma, torch.empty(self.C, dtype=torch.float64)).clone().cpu().numpy()


class _Abi:
    """A capture on the device with the calls of the C ABI on it."""

    def __init__(self, scene, cap, law):
        self.scene, self.cap, self.law = scene, cap, law
        self.binding = b = _bind(scene, cap)
        self.V = scene.vertices.detach().contiguous()
        self.tex = None if cap["tex"] is None else torch.as_tensor(render.check_texture(cap["tex"]), device="cuda").contiguous()
        self.C = C = b.channels
        self.void, self.invalid = np.full(C, float(cap["void"])), np.full(C, float(cap["invalid"]))
        self.flags = int(law[1] == "reflect") | (2 if law[2] == "snell" else 0)
        self.cam21 = [np.ascontiguousarray(b.args["cameras"][k]) for k in range(b.n)]
        self.scr9 = [np.ascontiguousarray(b.args["screens"][k]) for k in range(b.n)]
        self.tex_args = (None, 0, 0, C) if self.tex is None else (self.tex.data_ptr(), self.tex.shape[0], self.tex.shape[1], C)
        self.env_args = (None, 0, 0, None) if cap["env"] is None else (b.env.data_ptr(), b.env.shape[0], b.env.shape[1], b.env_rot.ctypes.data)
        self.sigma = np.ascontiguousarray(cap["sigma"], dtype=np.float64)
        self.stream = torch.cuda.current_stream().cuda_stream

    def single_absorb(self, view, acc):
        cap, b = self.cap, self.binding
        rc = _lib.lib().drt_render_image_loss_absorb(self.scene.optix_mesh._h, self.V.data_ptr(), self.cam21[view].ctypes.data, cap["H"], cap["W"], 0, cap["H"], cap["s"],
                                                     IOR, EXT, self.law[0], self.flags, 1, self.scr9[view].ctypes.data, *self.tex_args, self.void.ctypes.data,
                                                     self.invalid.ctypes.data, b.targets[view].data_ptr(), None if b.weights is None else b.weights[view].data_ptr(),
                                                     acc.loss.data_ptr(), acc.grad.data_ptr(), acc.ior.data_ptr(), None, acc.count.data_ptr(), self.sigma.ctypes.data,
                                                     acc.sigma.data_ptr(), self.stream)
        assert rc == 0, _lib.lib().drt_last_error()

    def _head(self, p, arr):
        return (self.scene.optix_mesh._h, self.V.data_ptr(), p["binding"], arr, p["k"], p["r0"], p["r1"], p["s"], IOR, EXT, self.law[0], self.flags, p["fresnel"], *p["tex"],
                self.void.ctypes.data, self.invalid.ctypes.data, p["targets"], _lib.ptr(self.binding.weights), p["loss"])

    def _params(self, ids, acc, kw):
        cap, b = self.cap, self.binding
        p = dict(binding=b._h, ids=ids, k=len(ids), r0=0, r1=len(ids) * cap["H"], s=cap["s"], targets=b.targets.data_ptr(), loss=acc.loss.data_ptr(), fresnel=1,
                 tex=self.tex_args, env=self.env_args[0], env_h=self.env_args[1], rot=self.env_args[3], reflection=0, sigma=self.sigma, grad_sigma=acc.sigma.data_ptr(),
                 images=None)
        p.update(kw)
        return p, (ctypes.c_int * max(1, len(p["ids"])))(*p["ids"])

    def absorb(self, ids, acc, **kw):
        p, arr = self._params(ids, acc, kw)
        return _lib.lib().drt_render_image_loss_views_absorb(*self._head(p, arr), acc.grad.data_ptr(), acc.ior.data_ptr(), acc.count.data_ptr(),
                                                             None if p["sigma"] is None else p["sigma"].ctypes.data, p["grad_sigma"], p["env"], p["env_h"],
                                                             self.env_args[2], p["rot"], p["reflection"], p["images"], self.stream)

    def clear(self, ids, acc, **kw):
        p, arr = self._params(ids, acc, kw)
        if self.cap["env"] is None:
            return _lib.lib().drt_render_image_loss_views(*self._head(p, arr), acc.grad.data_ptr(), acc.ior.data_ptr(), acc.count.data_ptr(), self.stream)
        return _lib.lib().drt_render_image_loss_views_env(*self._head(p, arr), acc.grad.data_ptr(), acc.ior.data_ptr(), acc.count.data_ptr(), p["env"], p["env_h"],
                                                          self.env_args[2], p["rot"], p["reflection"], self.stream)


def _exact_cases(scene):
    """(abi, ids), with screens: [0, 1], [1, 0], [0, 0] (a repeat: twice one view), k = 1, and the three weighted 7 x 5 views [2, 0, 3]."""
    pair = _Abi(scene, _pair_capture(LAWS[2]), LAWS[2])
    small = _Abi(scene, _small_capture(), LAWS[1])
    return [(pair, [0, 1]), (pair, [1, 0]), (pair, [0, 0]), (pair, [1]), (small, [2, 0, 3])]


def _both(abi, ids):
    one, many = _Acc(abi.V, abi.C), _Acc(abi.V, abi.C)
    for v in ids:
        abi.single_absorb(v, one)
    assert abi.absorb(ids, many) == 0, _lib.lib().drt_last_error()
    torch.cuda.synchronize()
    return one, many


def test_one_call_gives_the_bits_of_the_single_view_absorbing_calls_in_deterministic_mode(hand_scene, deterministic):
    for abi, ids in _exact_cases(hand_scene):
        one, many = _both(abi, ids)
        assert int(one.count) > 0 and one.grad.any() and one.sigma_value().all()
        for a, b in zip(one.raw(), many.raw()):
            assert a.dtype == b.dtype and torch.equal(a, b), ids


def test_one_call_agrees_with_the_single_view_absorbing_calls_in_float64_mode(hand_scene):
    assert not det.on()
    for abi, ids in _exact_cases(hand_scene):
        one, many = _both(abi, ids)
        assert int(one.count) == int(many.count) > 0
        for a, b in zip(one.raw()[:3] + one.raw()[4:], many.raw()[:3] + many.raw()[4:]):
            assert a.dtype == torch.float64 and (a - b).abs().max() <= BAND_REL * a.abs().max(), ids


@pytest.mark.parametrize("kind,reflection", vac.BACKGROUNDS, ids=[k + ("-reflection" if r else "") for k, r in vac.BACKGROUNDS])
def test_sigma_zero_gives_the_bits_of_the_clear_calls_and_a_sigma_partial_that_is_not_zero(hand_scene, deterministic, kind, reflection):
    law = LAWS[2]
    cap = dict(_pair_capture(law, kind, reflection), sigma=(0.0, 0.0, 0.0))
    abi = _Abi(hand_scene, cap, law)
    clear, absorbing = _Acc(abi.V, 3), _Acc(abi.V, 3)
    assert abi.clear([1, 0], clear, reflection=int(reflection)) == 0, _lib.lib().drt_last_error()
    assert abi.absorb([1, 0], absorbing, reflection=int(reflection)) == 0, _lib.lib().drt_last_error()
    torch.cuda.synchronize()
    assert int(clear.count) > 0 and clear.grad.any() and clear.ior.any()
    for a, b in zip(clear.raw(sigma=False), absorbing.raw(sigma=False)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    want = vac.summed(PAIR, law, kind, reflection, sigma=(0.0, 0.0, 0.0))["g_sigma"]
    got = absorbing.sigma_value()
    print(f"{kind} reflection={reflection}: d loss / d sigma at sigma = 0: {got} restatement {want}")
    assert np.abs(want).min() > 0 and cases.close(got, want)


# ---------------------------------------------------------------------------------------------------------------------------- the images
def test_images_with_screens_are_those_of_render_image(hand_scene):
    law = LAWS[2]
    cap = _pair_capture(law)
    got = _call(hand_scene, _bind(hand_scene, cap), cap, [1, 0, 1], law, want_images=True)["images"]
    assert got.shape == (3, 32, 32, 3) and got.dtype == torch.float32 and torch.equal(got[0], got[2])
    for slot, name in ((0, "v41"), (1, "v5")):
        sc = image_cases.scene(name)
        want = hand_scene.render_image(sc["camera_M"], 32, 32, sc["screen"], sc["texture"], supersample=2, max_bounces=law[0], tir=law[1], refraction=law[2],
                                       void=sc["void"], invalid=sc["invalid"], absorption=SIGMA3)
        keep = ~vac.sensitive(name, law, "screen")
        diff = (got[slot].double() - want.double()).abs().cpu().numpy()[keep].max()
        tol = image_absorb_cases.image_tolerance(name, image_cases.reference(name, law, True), law)
        print(f"{name}: max image difference from render_image(absorption=) {diff:.2e} (bound {tol:.2e})")
        assert diff <= tol and float(want.max()) > 0


@pytest.mark.parametrize("kind", ["room-screen", "room"])
def test_images_in_the_room_are_the_restatements(hand_scene, kind):
    law = LAWS[2]
    cap = _pair_capture(law, kind, True)
    got = _call(hand_scene, _bind(hand_scene, cap), cap, [0, 1], law, True, want_images=True)["images"]
    for slot, name in enumerate(PAIR):
        want = vac.reference(name, law, kind, True)["image"]
        keep = ~vac.sensitive(name, law, kind, True)
        diff = np.abs(got[slot].double().cpu().numpy() - want.astype(np.float64))[keep].max()
        tol = vac.image_tolerance(name, law, kind)
        print(f"{name} {kind}: max image difference from the restatement {diff:.2e} (bound {tol:.2e})")
        assert diff <= tol


# ------------------------------------------------------------------------------------------------------------------ bands, other modes
def _banded_cases(scene):
    """(whole, banded) results: the pair in the room with reflection in bands of nine rows -- (27, 36) straddles the border between the two
    views -- and the small views with screens, one of them twice, in single rows."""
    assert (27, 36) in render.plan_bands(64, 32, 2, 9 * 128 + 5) and render.plan_bands(28, 5, 3, 45) == [(r, r + 1) for r in range(28)]
    pair, small = _pair_capture(LAWS[2], "room-screen", True), _small_capture()
    for cap, ids, law, cap_samples, refl in ((pair, [0, 1], LAWS[2], 9 * 128 + 5, True), (small, [1, 1, 2, 0], LAWS[1], 45, False)):
        b = _bind(scene, cap)
        yield _call(scene, b, cap, ids, law, refl), _call(scene, b, cap, ids, law, refl, max_samples=cap_samples)


def test_bands_give_the_bits_of_the_unbanded_call_in_deterministic_mode(hand_scene, deterministic):
    for whole, banded in _banded_cases(hand_scene):
        assert float(whole["loss"]) > 0 and whole["grad_V"].abs().max() > 0 and whole["count"] == banded["count"] > 0
        for k in KEYS:
            assert torch.equal(whole[k], banded[k]), k


def test_bands_agree_with_the_unbanded_call_in_float64_mode(hand_scene):
    assert not det.on()
    for whole, banded in _banded_cases(hand_scene):
        assert whole["count"] == banded["count"]
        for k in KEYS:
            assert (whole[k] - banded[k]).abs().max() <= BAND_REL * whole[k].abs().max(), k


def test_banded_images_are_the_unbanded_ones(hand_scene):
    cap = _pair_capture(LAWS[2], "room-screen", True)
    b = _bind(hand_scene, cap)
    whole = _call(hand_scene, b, cap, [0, 1], LAWS[2], True, want_images=True)["images"]
    banded = _call(hand_scene, b, cap, [0, 1], LAWS[2], True, want_images=True, max_samples=9 * 128 + 5)["images"]
    assert whole.abs().max() > 0 and torch.equal(whole, banded)


def test_without_vertices_with_a_scaled_backward_and_a_tensor_absorption(hand_scene, deterministic):
    cap = _pair_capture(LAWS[1], "room-screen", True)
    b = _bind(hand_scene, cap)
    full, fixed = _call(hand_scene, b, cap, [1, 0], LAWS[1], True), _call(hand_scene, b, cap, [1, 0], LAWS[1], True, vertices=False)
    assert fixed["grad_V"] is None and fixed["count"] == full["count"] > 0
    for k in ("loss", "g_int", "g_ext", "g_sigma"):
        assert torch.equal(full[k], fixed[k])
    scaled = _call(hand_scene, b, cap, [1, 0], LAWS[1], True, scale=-2.5)
    for k in ("grad_V", "g_int", "g_ext", "g_sigma"):
        assert full[k].abs().max() > 0 and torch.equal(scaled[k], full[k] * -2.5)
    # a tensor absorption receives its .grad through backward(); plain numbers give the same loss and no sigma accumulator
    sg = torch.tensor(SIGMA3, dtype=torch.float64, device="cuda", requires_grad=True)
    kw = dict(supersample=2, max_bounces=6, tir="reflect", void=cap["void"], invalid=cap["invalid"], reflection=True)
    loss = hand_scene.image_loss_views_fused(b, [1, 0], cap["tex"], absorption=sg, vertices=False, **kw)
    loss.backward()
    assert sg.grad is not None and sg.grad.device == sg.device and torch.equal(sg.grad.cpu(), full["g_sigma"])
    plain = hand_scene.image_loss_views_fused(b, [1, 0], cap["tex"], absorption=SIGMA3, vertices=False, **kw)
    assert torch.equal(plain.detach(), loss.detach()) and torch.equal(loss.detach(), full["loss"])


def test_a_scene_without_faces_has_direct_samples_only():
    scene = _fresh()
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    cap = _pair_capture(LAWS[2], "room")
    cap["targets"] = np.zeros_like(cap["targets"])
    got = _call(scene, _bind(scene, cap), cap, [0, 1], LAWS[2], want_images=True)
    want = 0.0
    for slot, cam in enumerate(cap["cams"]):
        image = scene.render_image(cam, 32, 32, None, None, supersample=2, environment=cap["env"])
        assert torch.equal(image, got["images"][slot])                   # L = 0, A = 1: the clear image's bits
        want += float((image.double() ** 2).sum())
    assert want > 0 and abs(float(got["loss"]) - want) <= 1e-6 * want
    assert got["count"] == 0 and not got["grad_V"].any() and float(got["g_int"]) == 0 and float(got["g_ext"]) == 0 and not got["g_sigma"].any()


def test_two_deterministic_runs_are_identical(deterministic):
    cap = _pair_capture(LAWS[2], "room-screen", True)
    runs = []
    for _ in range(2):
        scene = _fresh()
        runs.append(_call(scene, _bind(scene, cap), cap, [0, 1], LAWS[2], True))
    for k in KEYS:
        assert runs[0][k].abs().max() > 0 and torch.equal(runs[0][k], runs[1][k])


# ---------------------------------------------------------------------------------------------------------------- capture and workspace
def test_a_captured_replay_gives_the_eager_bits_and_growth_inside_a_capture_is_refused(deterministic):
    scene = _fresh()
    V = scene.vertices
    cap = _pair_capture(LAWS[1], "room-screen", True)
    cap["env"] = render.Environment(torch.as_tensor(cap["env"].texels).cuda(), cap["env"].rotation)
    b = _bind(scene, cap)
    tex = torch.as_tensor(cap["tex"]).cuda()

    def step(ids=(0, 1), s=2, absorption=SIGMA3):
        loss = scene.image_loss_views_fused(b, list(ids), tex, supersample=s, max_bounces=6, tir="reflect", void=cap["void"], invalid=cap["invalid"], reflection=True,
                                            absorption=absorption)
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
    with pytest.raises(_lib.DrtError, match=WHO + ".*eagerly before capturing"):
        with torch.cuda.graph(g2):
            step(ids=(0, 1, 1), s=3)
    torch.cuda.synchronize()
    step(ids=(0, 1, 1), s=3, absorption=None)      # a clear call sizes everything but the lengths: their growth alone is refused too
    torch.cuda.synchronize()
    g3 = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match=WHO + ".*interior lengths.*eagerly before capturing"):
        with torch.cuda.graph(g3):
            step(ids=(0, 1, 1), s=3)
    torch.cuda.synchronize()


def test_calls_that_share_the_workspace_give_the_bits_of_fresh_scenes(deterministic):
    """An absorbing views call in the room, a single-view absorbing call, a clear views-env call, paths_ray_loss_fused and absorbing views
    calls again on ONE scene: ray lists, parked rows, lengths, tape, state bytes, the spare counter words and the pixel seeds are shared,
    every result is that of the same call on a scene built for it alone."""
    pair, small = _pair_capture(LAWS[2], "room-screen", True), _small_capture()
    center, _ = image_cases.frame()
    cam = image_cases.camera(5, 24, 20)
    o, d = (t.cuda() for t in views.generate_ray(24, 20, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((24 * 20, 3)) * 40.0 + np.asarray(center) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(24 * 20) > 0.1, device="cuda")

    def single(scene):
        sc = image_cases.scene("wide")
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], cases.target("wide", LAWS[2], True),
                                      supersample=sc["s"], max_bounces=6, tir="reflect", refraction="snell", void=sc["void"], invalid=sc["invalid"], absorption=SIGMA1)
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    def many(cap, ids, law, refl):
        def run(scene):
            got = _call(scene, _bind(scene, cap), cap, ids, law, refl)
            return tuple(got[k] for k in KEYS)
        return run

    def clear(scene):
        b = _bind(scene, pair)
        loss = scene.image_loss_views_fused(b, [1, 0], pair["tex"], supersample=2, max_bounces=6, tir="reflect", refraction="snell", void=pair["void"],
                                            invalid=pair["invalid"], reflection=True)
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    def paths(scene):
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        return loss.detach().clone(), torch.autograd.grad(loss, scene.vertices)[0].clone()

    steps = [many(small, [2, 0, 3], LAWS[1], False), single, clear, paths, many(pair, [1, 0], LAWS[2], True), many(small, [0], LAWS[1], False)]
    scene = _fresh()
    got = [step(scene) for step in steps]
    for step, mine in zip(steps, got):
        alone = step(_fresh())
        assert float(mine[0]) > 0 and mine[1].any() and len(alone) == len(mine)
        for x, y in zip(alone, mine):
            assert torch.equal(x, y)


def test_absorption_none_makes_the_calls_of_before(hand_scene, monkeypatch, deterministic):
    cap = _pair_capture(LAWS[1], "room-screen")
    plain = hand_scene.bind_image_views(cap["cams"], 32, 32, cap["screens"], cap["targets"])
    room = _bind(hand_scene, cap)
    kw = dict(supersample=2, max_bounces=6, tir="reflect", void=cap["void"], invalid=cap["invalid"])
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, fn):
            if fn.startswith("drt_render_image"):
                called.append(fn)
            return getattr(lib, fn)

    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    hand_scene.image_loss_views_fused(plain, [0, 1], cap["tex"], absorption=None, **kw)
    hand_scene.image_loss_views_fused(room, [0, 1], cap["tex"], absorption=None, **kw)
    hand_scene.image_loss_views_fused(plain, [0, 1], cap["tex"], absorption=0.0, **kw)
    hand_scene.image_loss_views_fused(room, [0, 1], cap["tex"], absorption=SIGMA3, **kw)
    assert called == ["drt_render_image_loss_views", "drt_render_image_loss_views_env", WHO, WHO]


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_outputs_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, WHO)
    was = det.enable(False)
    try:
        abi = _Abi(hand_scene, _pair_capture(LAWS[2], "room-screen", True), LAWS[2])
        bare = _Abi(hand_scene, _pair_capture(LAWS[2]), LAWS[2])
        other = _bind(_fresh(), abi.cap)
        acc = _Acc(abi.V, 3)
        images = torch.full((2, 32, 32, 3), 7.0, dtype=torch.float32, device="cuda")
        skew = abi.binding.env_rot.copy()
        skew[0:3] += 1e-9 * skew[3:6]
        bad_sigma = [np.array([0.1, -1e-300, 0.1]), np.array([np.nan, 0.1, 0.1]), np.array([0.1, 0.1, np.inf])]
        bad = [(dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(ids=[0, 2]), "view_ids"), (dict(ids=[-1, 0]), "view_ids"), (dict(r0=5, r1=5), "band"),
               (dict(r0=9, r1=3), "band"), (dict(r1=65), "band"), (dict(r0=-1), "band"), (dict(binding=None), "views"), (dict(binding=other._h), "another scene"),
               (dict(targets=None), "d_targets"), (dict(loss=None), "d_loss"), (dict(s=0), "supersample"), (dict(s=5), "supersample"),
               (dict(tex=(abi.tex_args[0], 4, 4, 2)), "channels"), (dict(sigma=None), "sigma"), (dict(sigma=bad_sigma[0]), "sigma[1]"),
               (dict(sigma=bad_sigma[1]), "sigma[0]"), (dict(sigma=bad_sigma[2]), "sigma[2]"), (dict(env_h=1), "env_h"), (dict(rot=None), "env_rot9"),
               (dict(rot=skew.ctypes.data), "env_rot9"), (dict(reflection=2), "reflection"), (dict(reflection=1, fresnel=0), "fresnel"),
               (dict(env=None, reflection=1), "reflection"), (dict(env=None, tex=(None, 64, 64, 3)), "d_texture"),
               # the order: the views call's checks win over sigma's, sigma's over the environment's
               (dict(s=0, sigma=bad_sigma[0], env_h=1), "supersample"), (dict(sigma=bad_sigma[0], env_h=1), "sigma[1]")]
        for kw, word in bad:
            assert abi.absorb(kw.pop("ids", [0, 1]), acc, images=images.data_ptr(), **kw) == -1, kw             # DRT_E_INVALID
            assert word in lib.drt_last_error().decode(), (kw, lib.drt_last_error())
        assert bare.absorb([0, 1], acc, reflection=1) == -1 and "reflection" in lib.drt_last_error().decode()
        torch.cuda.synchronize()
        assert float(acc.loss) == 0 and not acc.grad.any() and not acc.ior.any() and not acc.sigma.any() and int(acc.count) == 0 and (images == 7).all()
        assert abi.absorb([0, 1], acc, r0=20, r1=41, reflection=1, images=images.data_ptr()) == 0          # the good call adds into its targets
        torch.cuda.synchronize()
        first = acc.raw()
        assert float(acc.loss) > 0 and acc.grad.any() and acc.ior.all() and acc.sigma.all() and int(acc.count) > 0
        assert (images[0, :20] == 7).all() and (images[0, 20:] != 7).all() and (images[1, :9] != 7).all() and (images[1, 9:] == 7).all()
        assert abi.absorb([0, 1], acc, r0=20, r1=41, tex=(None, 0, 0, 3)) == 0         # ... one without the screen adds again
        assert abi.absorb([0, 1], acc, r0=20, r1=41, env=None, grad_sigma=None) == 0   # ... and so does one without the room, and without sigma partials
        torch.cuda.synchronize()
        assert int(acc.count) > 2 * int(first[3]) and float(acc.loss) > float(first[0])
    finally:
        det.enable(was)
