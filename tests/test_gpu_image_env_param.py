"""GPU: Scene.image_loss_fused with ``env_texels_param`` / ``env_rotation_param`` -- the gradients of the photometric loss w.r.t. the
environment's texels and rotation (drt_render_image_loss_env_param, drt_amd/csrc/drt_image_env_param.hip) -- against the
restatement tests/image_env_param_ref.py (autograd) on the 36 cases of tests/image_env_param_cases.py.

Tolerances are tests/image_loss_cases.py's: the loss within LOSS_REL (3e-14), gradients within ``close`` (1e-9 of the largest entry, at
most 1e-5).  tests/test_image_env_param_host.py holds the header to the same restatement on the host (measured there: gradients 1e-15 to
4e-14 absolute)."""
import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_param_cases as cases
import image_env_param_ref
import image_loss_cases
from conftest import IOR
from drt_amd import _lib, calibrate, det, diffrender as Render, render

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAWS = image_cases.LAWS
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


def _scene():
    scene = Render.Scene(image_cases.hand(), 0)
    V = torch.tensor(image_cases.hand().vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene


@pytest.fixture(scope="module")
def hand_scene():
    return _scene()


def _call(scene, name, law, with_screen=True, reflection=True, texels="float64", rotation="cpu", scale=None, env=None, target=None, **kw):
    """dict(loss, grad_V, g_int, g_ext, count, image, g_env, g_R) of one call on a case.  ``texels``: None (no env_texels_param),
    "float32" / "float64" (a device tensor of that dtype that requires grad), "fixed" (given, requires no grad); ``rotation``: None, "cpu" /
    "cuda" (a float64 tensor there that requires grad), "fixed"."""
    sc = image_cases.scene(name)
    env = image_env_cases.environment(sc["texture"].shape[2]) if env is None else env
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"], environment=env, reflection=reflection)
    args.update(kw)
    tp = rp = None
    if texels is not None:
        tp = torch.as_tensor(env.texels).to(device="cuda", dtype=torch.float64 if texels == "float64" else torch.float32).clone().requires_grad_(texels != "fixed")
        args["env_texels_param"] = tp
    if rotation is not None:
        rp = torch.tensor(env.rotation, dtype=torch.float64, device="cuda" if rotation == "cuda" else "cpu", requires_grad=rotation != "fixed")
        args["env_rotation_param"] = rp
    ii = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    ie = torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
    out = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"] if with_screen else None, sc["texture"] if with_screen else None,
                                 image_env_cases.loss_target(name, law, with_screen, reflection) if target is None else target, ior_int=ii, ior_ext=ie, **args)
    loss, image = out if args.get("want_image") else (out, None)
    res = dict(loss=loss.detach().clone(), count=int(scene.last_image_count), image=image, g_env=None, g_R=None)
    wrt = [scene.vertices, ii, ie] + [p for p in (tp, rp) if p is not None and p.requires_grad]
    g = list(torch.autograd.grad(loss if scale is None else loss * scale, wrt))
    res["grad_V"], res["g_int"], res["g_ext"] = g[0].clone(), g[1].clone(), g[2].clone()
    g = g[3:]
    if tp is not None and tp.requires_grad:
        res["g_env"] = g.pop(0)
        assert res["g_env"].dtype == tp.dtype and res["g_env"].shape == tp.shape and res["g_env"].device == tp.device
    if rp is not None and rp.requires_grad:
        res["g_R"] = g.pop(0)
        assert res["g_R"].dtype == torch.float64 and res["g_R"].shape == (3, 3) and res["g_R"].device == rp.device
    return res


def _same_others(a, b, exact):
    if exact:
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad_V"], b["grad_V"]) and torch.equal(a["g_int"], b["g_int"]) and torch.equal(a["g_ext"], b["g_ext"])
        assert a["image"] is None or torch.equal(a["image"], b["image"])
    else:
        assert abs(float(a["loss"]) - float(b["loss"])) <= image_loss_cases.LOSS_REL * float(b["loss"])
        assert close(a["grad_V"].cpu().numpy(), b["grad_V"].cpu().numpy()) and close(float(a["g_int"]), float(b["g_int"])) and close(float(a["g_ext"]), float(b["g_ext"]))
        assert a["image"] is None or torch.equal(a["image"], b["image"])
    assert a["count"] == b["count"]


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name,law,with_screen,reflection", cases.CASES, ids=cases.CASE_IDS)
def test_texel_and_rotation_gradients_against_the_restatement(hand_scene, name, law, with_screen, reflection):
    """The loss within LOSS_REL, the texel gradient (a float64 param here) and the nine rotation partials within ``close`` of the
    restatement; vertex gradient, IOR partials, count and image those of the call without the keywords: within ``close`` under float64
    atomics, the same bits in deterministic mode."""
    ref = cases.reference(name, law, with_screen, reflection)
    got = _call(hand_scene, name, law, with_screen, reflection, texels="float64", want_image=True)
    plain = _call(hand_scene, name, law, with_screen, reflection, texels=None, rotation=None, want_image=True)
    rel = abs(float(got["loss"]) - ref["loss"]) / ref["loss"]
    g_env, g_R = got["g_env"].cpu().numpy(), got["g_R"].numpy()
    print(f"loss {float(got['loss']):.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; max |g_env| {np.abs(ref['g_env']).max():.3e} differs by "
          f"{np.abs(g_env - ref['g_env']).max():.2e}; max |g_R| {np.abs(ref['g_R']).max():.3e} differs by {np.abs(g_R - ref['g_R']).max():.2e}")
    assert rel <= image_loss_cases.LOSS_REL
    assert close(g_env, ref["g_env"]) and close(g_R, ref["g_R"])
    assert not g_env[ref["g_env"] == 0].any()
    _same_others(got, plain, exact=False)
    was = det.enable(True)
    try:
        got_d = _call(hand_scene, name, law, with_screen, reflection, texels="float64", want_image=True)
        plain_d = _call(hand_scene, name, law, with_screen, reflection, texels=None, rotation=None, want_image=True)
    finally:
        det.enable(was)
    _same_others(got_d, plain_d, exact=True)
    assert close(got_d["g_env"].cpu().numpy(), ref["g_env"]) and close(got_d["g_R"].numpy(), ref["g_R"])


# --------------------------------------------------------------------------------------------------------- repeats, bands, capture
def _bits(r):
    return [r["loss"], r["grad_V"], r["g_int"], r["g_ext"], r["g_env"], r["g_R"]]


def test_two_runs_and_band_cuts_give_the_same_bits_in_deterministic_mode(hand_scene, deterministic):
    """`v5` (32 x 32, s = 2) under (6, reflect, snell) with screen and reflection: whole, again, in three bands and in four."""
    name, law = "v5", LAWS[2]
    assert len(render.plan_bands(32, 32, 2, 11 * 32 * 4)) == 3 and len(render.plan_bands(32, 32, 2, 8 * 32 * 4)) == 4
    whole, again = _call(hand_scene, name, law), _call(hand_scene, name, law)
    three, four = _call(hand_scene, name, law, max_samples=11 * 32 * 4), _call(hand_scene, name, law, max_samples=8 * 32 * 4)
    assert whole["g_env"].abs().max() > 0 and whole["g_R"].abs().max() > 0
    for other in (again, three, four):
        for a, b in zip(_bits(whole), _bits(other)):
            assert torch.equal(a, b)
        assert other["count"] == whole["count"]


def test_bands_agree_with_the_single_band_in_float64_mode(hand_scene):
    name, law = "v5", LAWS[2]
    whole, banded = _call(hand_scene, name, law), _call(hand_scene, name, law, max_samples=11 * 32 * 4)
    assert close(banded["g_env"].cpu().numpy(), whole["g_env"].cpu().numpy()) and close(banded["g_R"].numpy(), whole["g_R"].numpy())


def test_a_captured_replay_with_a_texel_param_gives_the_eager_bits(deterministic):
    scene = _scene()
    sc = image_cases.scene("v5")
    law = LAWS[1]
    envo = image_env_cases.environment(3)
    env = render.Environment(torch.as_tensor(envo.texels).cuda(), envo.rotation)
    tp = torch.as_tensor(envo.texels).cuda().clone().requires_grad_(True)
    tex, tgt = torch.as_tensor(sc["texture"]).cuda(), torch.as_tensor(image_env_cases.loss_target("v5", law, True, True)).cuda()

    def step():
        loss = scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], tex, tgt, supersample=sc["s"], max_bounces=6, tir="reflect",
                                      void=sc["void"], invalid=sc["invalid"], environment=env, reflection=True, env_texels_param=tp)
        return (loss.detach(),) + torch.autograd.grad(loss, [scene.vertices, tp])

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0]) > 0 and eager[1].abs().max() > 0 and eager[2].abs().max() > 0 and eager[2].dtype == torch.float32
    for a, b in zip(eager, static):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------- a 2 x 2 environment
def _tiny(scene, **kw):
    """`v41` without a screen in front of a 2 x 2 three-channel environment: every one of the thousands of reads lands on the same four
    texels, and every column pair is read across the seam (xa, xb is (0, 1) or (1, 0))."""
    env = render.Environment(np.random.default_rng(3).random((2, 2, 3)).astype(np.float32), image_env_cases.environment(3).rotation)
    return env, _call(scene, "v41", LAWS[2], False, True, env=env, target=image_env_cases.loss_target("v41", LAWS[2], False, True), **kw)


def test_a_two_by_two_environment_holds_close_in_both_modes_and_repeats_bit_for_bit(hand_scene):
    sc = image_cases.scene("v41")
    env, got = _tiny(hand_scene)
    args, _ = cases.case_args("v41", False)
    ref = image_env_param_ref.loss_and_grads(*args, env.texels, env.rotation, image_env_cases.loss_target("v41", LAWS[2], False, True), sc["s"], LAWS[2],
                                             sc["invalid"], IOR, EXT, reflect=True, sm=cases.samples("v41", LAWS[2], False, True))
    u = ref["fwd"]["u"].numpy()[ref["fwd"]["read"].numpy()]
    assert len(u) > 4000 and ((u < 0) | (u > 1)).sum() > 500 and (ref["g_env"] != 0).all()
    m = cases.margins(ref["fwd"])          # (the conditions of the cases module, for this map: no read on a texel line or at a pole)
    assert m[0] >= cases.TEXEL_MARGIN and m[1] >= cases.TEXEL_MARGIN and m[2] >= cases.POLE
    assert close(got["g_env"].cpu().numpy(), ref["g_env"]) and close(got["g_R"].numpy(), ref["g_R"])
    was = det.enable(True)
    try:
        whole, again, banded = _tiny(hand_scene)[1], _tiny(hand_scene)[1], _tiny(hand_scene, max_samples=11 * 32 * 4)[1]
    finally:
        det.enable(was)
    assert close(whole["g_env"].cpu().numpy(), ref["g_env"]) and close(whole["g_R"].numpy(), ref["g_R"])
    for other in (again, banded):
        for a, b in zip(_bits(whole), _bits(other)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ the other routes
def test_a_scene_without_faces_has_direct_samples_only():
    scene = _scene()
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    sc = image_cases.scene("v5")
    env = image_env_cases.environment(3)
    target = np.random.default_rng(2).random((sc["height"], sc["width"], 3)).astype(np.float32)
    for with_screen in (True, False):
        got = _call(scene, "v5", LAWS[2], with_screen, True, target=target)
        ref = image_env_param_ref.loss_and_grads(np.zeros((0, 3), np.int64), image_cases.hand().vertices, sc["camera_M"], sc["height"], sc["width"],
                                                 sc["screen"] if with_screen else None, sc["texture"] if with_screen else None, env.texels, env.rotation, target,
                                                 sc["s"], LAWS[2], sc["invalid"], IOR, EXT, reflect=True)
        assert got["count"] == 0 and not got["grad_V"].any() and abs(float(got["loss"]) - ref["loss"]) <= image_loss_cases.LOSS_REL * ref["loss"]
        assert np.abs(ref["g_R"]).max() > 0 and close(got["g_env"].cpu().numpy(), ref["g_env"]) and close(got["g_R"].numpy(), ref["g_R"])


def test_only_one_param_requires_grad_and_the_dtypes_and_shapes_come_back(hand_scene, deterministic):
    """Each gradient alone has the bits it has beside the other (deterministic mode); a float32 texel param receives a float32 gradient:
    the float64 one's, rounded; a rotation on the device receives its gradient there."""
    name, law = "v5", LAWS[2]
    both = _call(hand_scene, name, law, texels="float64", rotation="cuda")
    only_t = _call(hand_scene, name, law, texels="float64", rotation="fixed")
    only_r = _call(hand_scene, name, law, texels="fixed", rotation="cpu")
    no_r = _call(hand_scene, name, law, texels="float32", rotation=None)
    no_t = _call(hand_scene, name, law, texels=None, rotation="cpu")
    assert only_t["g_R"] is None and only_r["g_env"] is None and both["g_R"].device.type == "cuda"
    assert torch.equal(only_t["g_env"], both["g_env"]) and torch.equal(only_r["g_R"], both["g_R"].cpu()) and torch.equal(no_t["g_R"], both["g_R"].cpu())
    assert no_r["g_env"].dtype == torch.float32 and torch.equal(no_r["g_env"], both["g_env"].to(torch.float32))
    for other in (only_t, only_r, no_r, no_t):
        _same_others(other, both, exact=True)


def test_a_one_channel_param_without_its_last_axis(hand_scene):
    name, law = "wide", LAWS[1]
    sc = image_cases.scene(name)
    env = image_env_cases.environment(1)
    ref = cases.reference(name, law, True, True)
    tp = torch.as_tensor(env.texels[:, :, 0]).cuda().clone().requires_grad_(True)
    loss = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], image_env_cases.loss_target(name, law, True, True),
                                       supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"], environment=env,
                                       reflection=True, env_texels_param=tp, ior_int=IOR, ior_ext=EXT)
    g, = torch.autograd.grad(loss, tp)
    assert g.shape == (cases.EH, cases.EW) and g.dtype == torch.float32
    want = ref["g_env"][:, :, 0]
    assert np.abs(g.cpu().numpy().astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-9 * np.abs(want).max()      # (the float32 store)


def test_a_scaled_backward(hand_scene, deterministic):
    name, law = "v5", LAWS[2]
    full, scaled = _call(hand_scene, name, law, texels="float64"), _call(hand_scene, name, law, texels="float64", scale=-2.5)
    assert torch.equal(scaled["g_env"], full["g_env"] * -2.5) and torch.equal(scaled["g_R"], full["g_R"] * -2.5) and torch.equal(scaled["grad_V"], full["grad_V"] * -2.5)


def test_without_the_keywords_the_old_entry_point_runs_with_its_arguments(hand_scene, monkeypatch, deterministic):
    sc = image_cases.scene("v5")
    law = LAWS[1]
    kw = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], void=sc["void"], invalid=sc["invalid"], environment=image_env_cases.environment(3),
              reflection=True)
    target = image_env_cases.loss_target("v5", law, True, True)
    lib = _lib.lib()
    called = []

    class Spy:
        def __getattr__(self, fn):
            real = getattr(lib, fn)
            if not fn.startswith("drt_render_image"):
                return real

            def spy(*a):
                called.append((fn, len(a)))
                return real(*a)
            return spy

    before = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, **kw).detach().clone()
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    none = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, env_texels_param=None, env_rotation_param=None, **kw)
    n_old = len(_lib.SIGNATURES["drt_render_image_loss_env"][1])
    assert called == [("drt_render_image_loss_env", n_old)] and torch.equal(none.detach(), before)
    fixed = hand_scene.image_loss_fused(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target,
                                        env_rotation_param=torch.as_tensor(image_env_cases.environment(3).rotation), **kw)
    assert called[1:] == [("drt_render_image_loss_env_param", n_old + 2)] and torch.equal(fixed.detach(), before)


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_null_pointers_are_the_old_entry_and_refusals_leave_the_outputs_untouched(hand_scene, deterministic):
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_loss_env_param")
    sc = image_cases.scene("v5")
    envo = image_env_cases.environment(3)
    a = render.check_render_args(sc["camera_M"], 16, 16, sc["screen"], sc["texture"], 2, environment=envo)
    tex, env = torch.as_tensor(a["texture"], device="cuda"), torch.as_tensor(envo.texels, device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    target = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
    n_env = env.numel()

    def outputs(fill):
        o = dict(loss=det.scalar("cuda"), gV=det.acc(V), gi=det.acc(torch.empty(2, dtype=torch.float64, device="cuda")),
                 ge=det.acc(torch.empty((n_env + 2) // 3 * 3, dtype=torch.float64, device="cuda")), gr=det.acc(torch.empty(9, dtype=torch.float64, device="cuda")),
                 count=torch.zeros((), dtype=torch.int64, device="cuda"))
        for t in o.values():
            t.fill_(fill)
        return o

    def call(o, fn="drt_render_image_loss_env_param", **kw):
        p = dict(dict(y0=3, y1=9, env_h=env.shape[0], env_w=env.shape[1], rot=envo.packed(), reflection=1, fresnel=1, ge=o["ge"].data_ptr(), gr=o["gr"].data_ptr(),
                      env=env.data_ptr()), **kw)
        rot = None if p["rot"] is None else np.ascontiguousarray(p["rot"], dtype=np.float64)
        extra = () if fn == "drt_render_image_loss_env" else (p["ge"], p["gr"])
        return getattr(lib, fn)(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, 16, 16, p["y0"], p["y1"], 2, IOR, EXT, 4, 3, p["fresnel"],
                                a["screen"].ctypes.data, tex.data_ptr(), tex.shape[0], tex.shape[1], 3, a["void"].ctypes.data, a["invalid"].ctypes.data,
                                target.data_ptr(), None, o["loss"].data_ptr(), o["gV"].data_ptr(), o["gi"].data_ptr(), None, o["count"].data_ptr(), p["env"], p["env_h"],
                                p["env_w"], None if rot is None else rot.ctypes.data, p["reflection"], *extra, torch.cuda.current_stream().cuda_stream)

    old, new = outputs(0), outputs(0)
    assert call(old, "drt_render_image_loss_env") == 0 and call(new, ge=None, gr=None) == 0
    torch.cuda.synchronize()
    for k in ("loss", "gV", "gi", "count"):
        assert torch.equal(old[k], new[k]), k
    assert old["gV"].any() and not new["ge"].any() and not new["gr"].any()
    full = outputs(0)
    assert call(full) == 0
    torch.cuda.synchronize()
    assert full["ge"].any() and full["gr"].any() and torch.equal(full["gV"], old["gV"]) and torch.equal(full["loss"], old["loss"])
    # refusals: DRT_E_INVALID, the argument named, nothing written
    skew = envo.packed().copy()
    skew[0:3] += 1e-9 * skew[3:6]
    kept = outputs(7)
    bad = [(dict(env=None), "d_env"), (dict(env_h=1), "env_h"), (dict(rot=None), "env_rot9"), (dict(rot=skew), "env_rot9"), (dict(reflection=2), "reflection"),
           (dict(reflection=1, fresnel=0), "fresnel"), (dict(y0=9, y1=3), "band"), (dict(env_h=1 << 16, env_w=1 << 15), "d_grad_env")]
    for kw, word in bad:
        assert call(kept, **kw) == -1, kw
        assert word in lib.drt_last_error().decode(), (kw, lib.drt_last_error())
    torch.cuda.synchronize()
    for k, t in kept.items():
        assert (t == 7).all(), k


# ----------------------------------------------------------------------------------------------------------------------------- the fit
FIT_RESTATEMENT = dict(loss0=5.049773, loss1=1.5415e-3, angle0=8.8939, angle1=0.18892)      # python tests/image_env_param_cases.py fit


def test_fit_environment_recovers_a_turned_environment(hand_scene):
    """Three views of the hand (5, 29, 53 of 72) at 32 x 32, s = 2, (6, reflect, snell) with Fresnel and the outer-surface reflection, no
    screen, in front of the smooth 32 x 64 three-channel environment of image_env_param_cases; photographs rendered by the restatement at
    the true rotation; the start is off by a yaw of 1.5 texels and a tilt of 0.5 (8.894 degrees).  The same fit -- 150 Adam steps of
    0.02 texels over ``calibrate.environment_pose`` -- on the restatement on the CPU (image_env_param_cases.fit_on_the_restatement; the
    rays are constants of a fixed mesh) took the loss from 5.0498 to 1.54e-3 (3.52 decades) and the angle to the true rotation to 0.189
    degrees (1.67 decades).  Asserted here: half of each in decades -- the loss below 5.0498 * 10^-1.76 = 8.8e-2 and the angle below
    8.894 * 10^-0.84 = 1.30 degrees; the same arithmetic in another summation order, the margin is for the optimiser's sensitivity to last
    bits."""
    case = cases.fit_case()
    angle0 = cases.rotation_angle(case["start"].rotation, case["true"].rotation)
    views = [(cam, torch.as_tensor(photo).cuda()) for cam, photo in zip(case["cams"], case["photos"])]
    fitted, history = calibrate.fit_environment(hand_scene, views, case["start"], steps=cases.FIT_STEPS, lr=cases.FIT_LR, reflection=True, supersample=cases.FIT_S,
                                                max_bounces=cases.FIT_LAW[0], tir=cases.FIT_LAW[1], refraction=cases.FIT_LAW[2], invalid=cases.FIT_INVALID,
                                                ior_int=IOR, ior_ext=EXT)
    angle1 = cases.rotation_angle(fitted.rotation, case["true"].rotation)
    print(f"loss {history[0]:.6e} -> {min(history):.6e}; angle to the true rotation {angle0:.4f} -> {angle1:.5f} degrees")
    r = FIT_RESTATEMENT
    assert abs(history[0] - r["loss0"]) <= 1e-6 * r["loss0"] and abs(angle0 - r["angle0"]) < 1e-3 and len(history) == cases.FIT_STEPS
    assert min(history) <= r["loss0"] * (r["loss1"] / r["loss0"]) ** 0.5 and angle1 <= r["angle0"] * (r["angle1"] / r["angle0"]) ** 0.5
    assert isinstance(fitted, render.Environment) and fitted.texels is case["start"].texels
