"""CPU: the image term of several views in front of one environment (drt_render_image_loss_views_env).  The law is
drt_image_env.h's and the mapping drt_image_views.h's, so the host checks are about their product, compiled for the host by g++ with
-ffp-contract=off (tests/hostsim/image_views_env.cpp):

  * the camera ray and (ro, wr, R1) that the reflection list forms through the table row of a sample's band row, for every sample of the
    bands at which the mapping can go wrong, against those of the single-view call, bit for bit.  The hostsim file restates the kernel's
    few lines (image_views_row, image_sample_ray with the row within the view, image_reflect_first); it does not compile the kernel, so
    this holds the mapping and the law through a table row -- the kernel's own choice of v.y over r is held by the GPU comparisons with
    the single-view call (tests/test_gpu_image_views_env.py), whose lists have a second slot;
  * the host loss and gradients of two views in one pass against the SUM of image_env_cases.loss_reference of the two (tolerances
    image_loss_cases.LOSS_REL and .close, the count exact), under the three laws, with and without screens, with and without reflection;
  * every argument check that needs no GPU (the library's own argument errors need a built scene: tests/test_gpu_image_views_env.py),
    the two pinned refusals, the declarations, and the native call a binding without an environment makes."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_ref
import image_loss_cases as cases
import image_ref
from conftest import IOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
EXT = image_cases.EXT
EH, EW = image_env_cases.EH, image_env_cases.EW
PAIR = ("v5", "v41")


def load_hv():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_views_env.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_views_env.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_views.h", "drt_image_env.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h",
                                                    "drt_shade.h", "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.ive_reflect_band.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _D, _D, _I] + [_P] * 6
    lib.ive_reflect_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _D, _D, _I] + [_P] * 6
    lib.ive_views_loss.restype = _D
    lib.ive_views_loss.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _D, _D, _I, _I] + [_P] * 10
    return lib


@pytest.fixture(scope="module")
def hv():
    return load_hv()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _cam21(camera_M):
    return np.ascontiguousarray(np.concatenate([np.asarray(camera_M[3], np.float64).reshape(-1), np.asarray(camera_M[2], np.float64)[:3, :].reshape(-1)]))


def _mesh():
    mesh = image_cases.hand()
    return np.ascontiguousarray(mesh.faces, dtype=np.int32), np.ascontiguousarray(mesh.vertices, dtype=np.float64)


# ---- the reflection rays across bands -------------------------------------------------------------------------------------------------------
def _first_faces(cam, H, W, s):
    """int32 [H W s^2]: the face of every sample's first interaction (the restatement's tracer), -1 without one."""
    faces, verts = _mesh()
    o, d = image_ref.sample_rays(cam[3], cam[2], H, W, s)
    return np.ascontiguousarray(image_env_ref.reflection(faces, verts, o, d, IOR, EXT)["face"].numpy(), dtype=np.int32)


def _single_view(hv, cam, H, W, s, first, snell):
    faces, verts = _mesh()
    n = H * W * s * s
    out = dict(ray=np.zeros((2, n, 3)), qual=np.zeros(n, np.uint8), ro=np.zeros((n, 3)), wr=np.zeros((n, 3)), R1=np.zeros(n))
    hv.ive_reflect_view(_p(_cam21(cam)), H, W, s, _p(faces), _p(verts), len(faces), EXT, IOR, snell, _p(first), _p(out["ray"]), _p(out["qual"]), _p(out["ro"]),
                        _p(out["wr"]), _p(out["R1"]))
    return out


# (table cameras, ids, H, W, s, bands)
def _band_cases():
    pair = [image_cases.scene(name)["camera_M"] for name in PAIR]
    small = [image_cases.camera(v, 7, 5) for v in (5, 17, 29, 41)]
    return {"the straddling band and single rows of two 32-row views": (pair, [0, 1], 32, 32, 2, [(27, 36), (31, 32), (32, 33), (63, 64)]),
            "a border inside a wave": (small, [2, 0, 3], 7, 5, 3, [(0, 21)])}


@pytest.mark.parametrize("snell", [0, 1], ids=["reference", "snell"])
@pytest.mark.parametrize("case", sorted(_band_cases()))
def test_reflection_rays_through_the_table_row_have_the_bits_of_the_single_view_call(hv, case, snell):
    cams, ids, H, W, s, bands = _band_cases()[case]
    faces, verts = _mesh()
    s2 = s * s
    first = [_first_faces(c, H, W, s) for c in cams]
    single = [_single_view(hv, c, H, W, s, f, snell) for c, f in zip(cams, first)]
    cams21 = np.ascontiguousarray(np.stack([_cam21(c) for c in cams]))
    screens9 = np.ascontiguousarray(np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (len(cams), 1)))
    ids_c = np.ascontiguousarray(ids, np.int32)
    n_qual = 0
    for r0, r1 in bands:
        n = (r1 - r0) * W * s2
        i = np.arange(n)
        pix = i // s2
        r = r0 + pix // W
        view, inside = np.asarray(ids)[r // H], ((r % H) * W + pix % W) * s2 + i % s2          # the sample's view and its index within that view
        ff = np.ascontiguousarray(np.stack(first)[view, inside])
        ray, qual, ro, wr, R1 = np.zeros((2, n, 3)), np.zeros(n, np.uint8), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        hv.ive_reflect_band(_p(cams21), _p(screens9), len(cams), _p(ids_c), len(ids), H, W, s, r0, r1, _p(faces), _p(verts), len(faces), EXT, IOR, snell, _p(ff),
                            _p(ray), _p(qual), _p(ro), _p(wr), _p(R1))
        want = {k: np.stack([sv[k] for sv in single]) for k in ("qual", "ro", "wr", "R1")}
        want_ray = np.stack([sv["ray"] for sv in single])                                        # [view, 2, n_view, 3]
        assert np.array_equal(ray.view(np.uint64), np.ascontiguousarray(want_ray[view, :, inside].transpose(1, 0, 2)).view(np.uint64))
        assert np.array_equal(qual, want["qual"][view, inside])
        for got, k in ((ro, "ro"), (wr, "wr"), (R1, "R1")):
            assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want[k][view, inside]).view(np.uint64)), (k, r0, r1)
        n_qual += int(qual.sum())
    assert n_qual > 50


# ---- loss and gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflection", [False, True], ids=["no-reflection", "reflection"])
@pytest.mark.parametrize("with_screen", [True, False], ids=["screen", "no-screen"])
@pytest.mark.parametrize("law", image_cases.LAWS, ids=[f"{k}-{t}-{r}" for k, t, r in image_cases.LAWS])
def test_two_views_in_one_pass_give_the_sum_of_the_restatement(hv, law, with_screen, reflection):
    """The table holds v5 then v41; the call lists them as [v41, v5], so that neither slot reads its own row by accident."""
    order = ("v41", "v5")
    refs = {name: image_env_cases.loss_reference(name, law, with_screen, reflection) for name in PAIR}
    sc = image_cases.scene("v5")
    H, W, s, C = sc["height"], sc["width"], sc["s"], sc["texture"].shape[2]
    env = image_env_cases.environment(C)
    faces, verts = _mesh()
    cams = np.ascontiguousarray(np.stack([_cam21(image_cases.scene(name)["camera_M"]) for name in PAIR]))
    screens = np.ascontiguousarray(np.stack([image_cases.scene(name)["screen"].packed() for name in PAIR]))
    targets = np.ascontiguousarray(np.stack([image_env_cases.loss_target(name, law, with_screen, reflection) for name in PAIR]))
    ids = np.ascontiguousarray([PAIR.index(name) for name in order], np.int32)
    fwd = [refs[name]["fwd"] for name in order]
    cls = np.ascontiguousarray(np.concatenate([f["cls"].numpy() for f in fwd]), dtype=np.int32)
    hits = np.ascontiguousarray(np.concatenate([f["hits"].numpy() for f in fwd]), dtype=np.uint8)
    seen = np.ascontiguousarray(np.concatenate([f["seen"].numpy() for f in fwd]), dtype=np.uint8)
    K = max(f["tape"].shape[0] for f in fwd)
    tape = np.ascontiguousarray(np.concatenate([np.pad(f["tape"].numpy(), ((0, K - f["tape"].shape[0]), (0, 0)), constant_values=-1) for f in fwd], axis=1),
                                dtype=np.int32)
    grad, g_ior, count = np.zeros_like(verts), np.zeros(2), np.zeros(1, np.int64)
    loss = hv.ive_views_loss(_p(cams), _p(screens), 2, _p(ids), 2, H, W, s, _p(sc["texture"]) if with_screen else None, image_cases.TEX, image_cases.TEX, C,
                             _p(env.texels), EH, EW, _p(np.ascontiguousarray(env.rotation)), _p(faces), _p(verts), len(faces), IOR, EXT, int(law[2] == "snell"),
                             int(reflection), _p(cls), _p(tape), _p(hits), _p(seen), _p(np.full(C, float(sc["invalid"]))), _p(targets), None, _p(grad), _p(g_ior),
                             _p(count))
    want = {k: sum(refs[name][k] for name in order) for k in ("loss", "grad_V", "g_int", "g_ext", "count")}
    rel = abs(loss - want["loss"]) / want["loss"]
    print(f"{law} screen={with_screen} reflection={reflection}: loss {loss:.12e} against {want['loss']:.12e} ({rel:.2e}); count {int(count[0])}; "
          f"max |d grad_V| {np.abs(grad - want['grad_V']).max():.2e} of {np.abs(want['grad_V']).max():.3e}")
    assert rel <= cases.LOSS_REL and int(count[0]) == want["count"] > 0
    assert cases.close(grad, want["grad_V"]) and cases.close(g_ior[0], want["g_int"]) and cases.close(g_ior[1], want["g_ext"])
    assert not cases.close(grad, refs[order[0]]["grad_V"])                                      # (one view alone is outside the tolerance)


# ---- the argument checks -------------------------------------------------------------------------------------------------------------------
def _bind_args(n=4, H=8, W=6, C=3):
    from drt_amd import render
    cams = [image_cases.camera(5 + k, H, W) for k in range(n)]
    screens = [render.Screen([0, 0, k], [1, 0, 0], [0, 1, 0]) for k in range(n)]
    return dict(cameras=cams, height=H, width=W, screens=screens, targets=np.zeros((n, H, W, C), np.float32), environment=image_env_cases.environment(C))


def test_bind_arguments_of_every_accepted_form():
    from drt_amd import render
    a = _bind_args()
    got = render.check_image_views_args(**a)
    assert got["environment"] is a["environment"] and got["has_screens"] and np.array_equal(got["screens"][3], a["screens"][3].packed())
    bare = render.check_image_views_args(**dict(a, screens=None))
    assert not bare["has_screens"] and bare["screens"].shape == (4, 9) and np.array_equal(bare["screens"][2], render.NO_SCREEN_ROW)
    assert render.Screen(*np.asarray(render.NO_SCREEN_ROW).reshape(3, 3)).packed().shape == (9,)          # the placeholder passes Screen's own checks
    plain = render.check_image_views_args(**{k: v for k, v in a.items() if k != "environment"})
    assert plain["environment"] is None and plain["has_screens"]
    mono = render.check_image_views_args(**dict(a, targets=np.zeros((4, 8, 6), np.float32), environment=image_env_cases.environment(1)))
    assert mono["channels"] == 1


@pytest.mark.parametrize("name,change,match", [
    ("no screens and no environment", lambda a: dict(a, screens=None, environment=None), "screens is None"),
    ("an environment that is none", lambda a: dict(a, environment=np.zeros((4, 8, 3), np.float32)), "environment must be"),
    ("a one-channel environment for three-channel targets", lambda a: dict(a, environment=image_env_cases.environment(1)), "environment has 1 channels"),
    ("the same without screens", lambda a: dict(a, screens=None, environment=image_env_cases.environment(1)), "environment has 1 channels"),
    ("fewer screens than cameras", lambda a: dict(a, screens=a["screens"][:3]), "screens"),
])
def test_bind_image_views_names_the_bad_argument(name, change, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.bind_image_views(object(), **change(_bind_args()))


def _fake_binding(**kw):
    """A binding with everything the argument checks read and no device table behind it."""
    from drt_amd import render
    b = render.ImageViews.__new__(render.ImageViews)
    b.args = render.check_image_views_args(**dict(_bind_args(), **kw))
    b.n, b.height, b.width, b.channels, b._h, b._mesh, b.scene = 4, 8, 6, 3, None, None, None
    return b


@pytest.mark.parametrize("bind,texture,kw,match", [
    ({}, None, {}, "texture is None"),
    ({"screens": None}, np.zeros((4, 4, 3), np.float32), {}, "texture must be None"),
    ({}, np.zeros((4, 4, 3), np.float32), {"reflection": True, "fresnel": False}, "fresnel"),
    ({}, np.zeros((4, 4, 3), np.float32), {"reflection": 1}, "reflection"),
    ({}, np.zeros((4, 4), np.float32), {}, "channels"),
    ({"screens": None}, None, {"supersample": 5}, "supersample"),
    ({"environment": None}, np.zeros((4, 4, 3), np.float32), {"reflection": True}, "multi-view"),
    ({}, np.zeros((4, 4, 3), np.float32), {"environment": image_env_cases.environment(3)}, "multi-view.*bind_image_views"),
])
def test_image_loss_views_fused_names_the_bad_argument(bind, texture, kw, match):
    from drt_amd import diffrender
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_views_fused(object(), _fake_binding(**bind), [0, 1], texture, **kw)


def test_the_accepted_calls_reach_the_scene_check():
    """With everything in order the next check is the binding's scene: the call is accepted as far as the host can tell."""
    from drt_amd import diffrender, render
    for bind, texture, kw in (({}, np.zeros((4, 4, 3), np.float32), {"reflection": True}), ({"screens": None}, None, {"reflection": True}),
                              ({"screens": None}, None, {})):
        with pytest.raises(ValueError, match="another scene"):
            diffrender.Scene.image_loss_views_fused(object(), _fake_binding(**bind), [0, 1], texture, **kw)
    a = render.check_image_views_law(_fake_binding(screens=None), [3, 0, 3], None, supersample=2, max_samples=6 * 4 * 5, reflection=True)
    assert a["texture"] is None and a["screen"] is None and a["reflection"] and a["environment"] is not None and a["channels"] == 3
    assert a["ids"] == [3, 0, 3] and a["bands"] == render.plan_bands(24, 6, 2, 6 * 4 * 5)


def test_the_two_pinned_refusals():
    """``environment=`` on the call and ``reflection=True`` without a binding's environment raise before the binding's type is looked at."""
    from drt_amd import diffrender
    tex = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(ValueError, match=r"multi-view.*bind_image_views\(\.\.\., environment=\)"):
        diffrender.Scene.image_loss_views_fused(object(), None, [0], tex, environment=image_env_cases.environment(3))
    for binding in (None, object(), _fake_binding(environment=None)):
        with pytest.raises(ValueError, match="multi-view"):
            diffrender.Scene.image_loss_views_fused(object(), binding, [0], tex, reflection=True)
    names = inspect.signature(diffrender.Scene.image_loss_views_fused).parameters
    assert "env_texels_param" not in names and "env_rotation_param" not in names and "reflection" in names


def test_the_photo_loop_and_the_capture_take_the_keywords():
    from drt_amd import captured_data, optim, render
    for fn, names in ((optim.PhotoIteration.__init__, ("reflection",)), (optim.optimize_photometric, ("reflection",)),
                      (captured_data.PhotoData.__init__, ("environment",)), (captured_data.SyntheticPhotoData.__init__, ("environment", "reflection", "screen"))):
        p = inspect.signature(fn).parameters
        assert all(n in p for n in names)
    assert inspect.signature(optim.PhotoIteration.__init__).parameters["reflection"].default is False
    assert inspect.signature(captured_data.SyntheticPhotoData.__init__).parameters["screen"].default is True
    cams = [image_cases.camera(5 + k, 8, 6) for k in range(2)]
    data = captured_data.PhotoData(cams, None, None, np.zeros((2, 8, 6, 3), np.float32), np.zeros((2, 8, 6)), 6, 8, device="cpu",
                                   environment=image_env_cases.environment(3))
    assert data.screens is None and data.texture is None and isinstance(data.environment, render.Environment)
    with pytest.raises(ValueError, match="screen=False needs an environment"):
        captured_data.SyntheticPhotoData(None, None, None, 6, 8, None, screen=False)


def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    sig = _lib.SIGNATURES["drt_render_image_loss_views_env"][1]
    assert len(sig) == 31 and sig[:25] == _lib.SIGNATURES["drt_render_image_loss_views"][1][:25]
    assert sig[25:30] == _lib.SIGNATURES["drt_render_image_loss_env"][1][27:32] and len(_lib.SIGNATURES["drt_render_image_loss_views"][1]) == 26
    assert "drt_image_views_env.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss_views_env(" in header
    unit = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_views_env.hip")).read()
    code = "\n".join(line for line in unit.splitlines() if not line.lstrip().startswith("//"))
    assert "int drt_render_image_loss_views_env(" in code and "image_start_views" in code and "k_image_start" not in code        # no second copy of the start kernel
    shared = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_env_loss.h")).read()
    assert "k_image_reflect_list(PathCtx c, VIEW view" in shared and "k_image_reflect_bwd(PathCtx c, VIEW view" in shared
    for other in ("drt_image_env.hip", "drt_image_views.hip"):                                    # each kernel is stated once
        text = open(os.path.join(ROOT, "drt_amd", "csrc", other)).read()
        assert "void __launch_bounds__(kPathBlock) k_image_reflect_list" not in text and "k_image_reflect_bwd(PathCtx" not in text
    lib = _lib.lib()
    assert lib.drt_version() == 13 and hasattr(lib, "drt_render_image_loss_views_env")
    assert lib.drt_render_image_loss_views_env(*([None] * 4), 2, 0, 8, 1, 1.5, 1.0, 2, 0, 1, None, 4, 4, 3, *([None] * 9), 4, 8, None, 0, None) != 0
    assert lib.drt_last_error()


# ---- which native call a binding makes ------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        def call(*args):
            self.calls.append((fn, args))
            return 0
        return call


class _Ptr:
    def __init__(self, p, shape=()):
        self.p, self.shape = p, shape

    def data_ptr(self):
        return self.p


def _enqueue(monkeypatch, binding, texture, **kw):
    from drt_amd import _lib, diffrender
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(diffrender, "_stream", lambda: 77)
    scene = type("S", (), {"optix_mesh": type("M", (), {"_h": 11})()})()
    void, invalid = np.zeros(3), np.ones(3)
    diffrender.enqueue_image_views_term(scene, _Ptr(21), binding, [1, 0], texture, (6, "reflect", "snell"), 2, True, void, invalid, (1.5, 1.0), 31, 32, 33, 34,
                                        bands=[(0, 5), (5, 16)], **kw)
    return rec.calls, void, invalid


def test_a_binding_without_an_environment_makes_the_call_of_before(monkeypatch):
    b = type("B", (), {"_h": 41, "height": 8, "targets": _Ptr(51), "weights": None})()
    calls, void, invalid = _enqueue(monkeypatch, b, _Ptr(61, (4, 5, 3)))
    assert [c[0] for c in calls] == ["drt_render_image_loss_views"] * 2
    for (fn, args), (r0, r1) in zip(calls, [(0, 5), (5, 16)]):
        assert len(args) == 26 and list(args[3]) == [1, 0]
        assert args[:3] == (11, 21, 41) and args[4:] == (2, r0, r1, 2, 1.5, 1.0, 6, 3, 1, 61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, None, 31, 32, 33, 34, 77)
    with_none = type("B", (), {"_h": 41, "height": 8, "targets": _Ptr(51), "weights": None, "env": None, "env_rot": None})()
    again, _, _ = _enqueue(monkeypatch, with_none, _Ptr(61, (4, 5, 3)), reflection=False)
    assert [(fn, a[:3], a[4:14]) for fn, a in again] == [(fn, a[:3], a[4:14]) for fn, a in calls] and all(len(a) == 26 for _, a in again)


def test_a_binding_with_an_environment_makes_the_new_call(monkeypatch):
    rot = np.ascontiguousarray(np.eye(3).reshape(-1))
    b = type("B", (), {"_h": 41, "height": 8, "targets": _Ptr(51), "weights": _Ptr(52), "env": _Ptr(71, (16, 32, 3)), "env_rot": rot})()
    calls, void, invalid = _enqueue(monkeypatch, b, _Ptr(61, (4, 5, 3)), reflection=True)
    assert [c[0] for c in calls] == ["drt_render_image_loss_views_env"] * 2
    args = calls[1][1]
    assert len(args) == 31 and args[4:] == (2, 5, 16, 2, 1.5, 1.0, 6, 3, 1, 61, 4, 5, 3, void.ctypes.data, invalid.ctypes.data, 51, 52, 31, 32, 33, 34, 71, 16, 32,
                                            rot.ctypes.data, 1, 77)
    calls, _, _ = _enqueue(monkeypatch, b, None)
    assert calls[0][1][13:17] == (None, 0, 0, 3) and calls[0][1][29] == 0
