"""CPU: the image term of several views in one call (drt_amd/csrc/drt_image_views.h).  The mapping of a band of the tall
image to (view, x, y, sample) and the table-row lookup, compiled for the host by g++ with -ffp-contract=off
(tests/hostsim/image_views.cpp), against a few lines of Python for every sample of the bands at which it can go wrong; the camera ray
through a table row against the ray through the by-value camera, bit for bit; the host loss and gradients of two views in one pass
against the SUM of the restatement's results of the two views (image_loss_cases.reference, tolerances image_loss_cases.LOSS_REL and
.close); and every argument check that needs no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_loss_cases as cases
from conftest import IOR
from test_image_loss_host import HostView, _cam21

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
EXT = cases.EXT


def load_hv():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_views.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_views.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_views.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h",
                                                    "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.iv_map.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I] + [_P] * 7
    lib.iv_rays.argtypes = [_P, _P, _I, _I, _I, _I, _I, _P, _P]
    lib.iv_views_loss.restype = _D
    lib.iv_views_loss.argtypes = [_P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _D, _D, _I, _I] + [_P] * 10
    return lib


@pytest.fixture(scope="module")
def hv():
    return load_hv()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _table(n_views, seed=3):
    """cameras [n, 21] whose rinv[3] (the camera's x position) is 100 + view, and screens [n, 9]."""
    rng = np.random.default_rng(seed)
    cams = rng.standard_normal((n_views, 21))
    cams[:, 9 + 3] = 100.0 + np.arange(n_views)
    return np.ascontiguousarray(cams), np.ascontiguousarray(rng.standard_normal((n_views, 9)))


# (n_views, ids, H, W, s, bands)
MAPPINGS = {
    "border inside a wave": (4, [2, 0, 3], 7, 5, 3, [(0, 21)]),
    "bands of nine rows": (3, [1, 2], 32, 32, 2, [(0, 9), (9, 18), (18, 27), (27, 36), (36, 45), (45, 54), (54, 63), (63, 64)]),
    "single rows": (3, [1, 2], 32, 32, 2, [(31, 32), (32, 33), (63, 64)]),
    "a repeated id": (2, [1, 1, 0, 1], 7, 5, 3, [(0, 28), (5, 16)]),
    "sixteen views": (16, list(range(15, -1, -1)), 3, 4, 1, [(0, 48)]),
}


@pytest.mark.parametrize("case", sorted(MAPPINGS))
def test_every_sample_of_a_band_maps_to_its_view_row_and_pixel(hv, case):
    n_views, ids, H, W, s, bands = MAPPINGS[case]
    cams, screens = _table(n_views)
    ids_c = np.ascontiguousarray(ids, np.int32)
    assert hv.iv_row_bytes() == 240
    for r0, r1 in bands:
        n = (r1 - r0) * W * s * s
        x, y, j, slot, view = (np.full(n, -9, np.int32) for _ in range(5))
        mark, at = np.zeros(n), np.zeros((n, 2), np.int64)
        hv.iv_map(_p(cams), _p(screens), n_views, _p(ids_c), len(ids), H, W, s, r0, r1, _p(x), _p(y), _p(j), _p(slot), _p(view), _p(mark), _p(at))
        i = np.arange(n)
        pix = i // (s * s)
        r = r0 + pix // W
        want_view = np.asarray(ids)[r // H]
        assert np.array_equal(j, i % (s * s)) and np.array_equal(x, pix % W)
        assert np.array_equal(slot, r // H) and np.array_equal(y, r % H) and np.array_equal(view, want_view)
        assert np.array_equal(mark, 100.0 + want_view)                                   # the table row the id selects
        assert np.array_equal(at[:, 0], (want_view * H + r % H) * W + pix % W) and np.array_equal(at[:, 1], pix)
    if case == "bands of nine rows":
        assert (27, 36) in bands and 27 < H < 36                                         # this band straddles the view border


def test_the_ray_through_a_table_row_has_the_bits_of_the_by_value_camera(hv):
    cams = np.ascontiguousarray(np.stack([_cam21(image_cases.scene(name)["camera_M"]) for name in ("v5", "v41")]))
    screens = np.ascontiguousarray(np.stack([image_cases.scene(name)["screen"].packed() for name in ("v5", "v41")]))
    H, W, s = 7, 5, 3
    n = H * W * s * s
    for view in (0, 1):
        a, b = np.zeros((2, n, 3)), np.ones((2, n, 3))
        hv.iv_rays(_p(cams), _p(screens), 2, view, H, W, s, _p(a), _p(b))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.abs(np.linalg.norm(a[1], axis=1) - 1.0).max() < 1e-15
    assert not np.array_equal(a[0], np.zeros_like(a[0]))


@pytest.mark.parametrize("order", [("v5", "v41"), ("v41", "v5")])
@pytest.mark.parametrize("law", cases.LAWS)
def test_two_views_in_one_pass_give_the_sum_of_the_restatement(hv, law, order):
    """Fresnel on; the table holds v5 then v41, the call lists them in `order`."""
    table = ("v5", "v41")
    views = {name: HostView(None, name, law, True) for name in table}
    refs = [cases.reference(name, law, True) for name in order]
    sc = image_cases.scene("v5")
    H, W, s = sc["height"], sc["width"], sc["s"]
    cams = np.ascontiguousarray(np.stack([_cam21(image_cases.scene(name)["camera_M"]) for name in table]))
    screens = np.ascontiguousarray(np.stack([image_cases.scene(name)["screen"].packed() for name in table]))
    targets = np.ascontiguousarray(np.stack([views[name].target for name in table]))
    ids = np.ascontiguousarray([table.index(name) for name in order], np.int32)
    cls = np.ascontiguousarray(np.concatenate([views[name].cls for name in order]))
    hits = np.ascontiguousarray(np.concatenate([views[name].hits for name in order]))
    K = max(views[name].tape.shape[0] for name in order)
    tape = np.ascontiguousarray(np.concatenate([np.pad(views[name].tape, ((0, K - views[name].tape.shape[0]), (0, 0)), constant_values=-1) for name in order], axis=1))
    one = views["v5"]
    grad, g_ior, count = np.zeros_like(one.V), np.zeros(2), np.zeros(1, np.int64)
    loss = hv.iv_views_loss(_p(cams), _p(screens), 2, _p(ids), 2, H, W, s, _p(one.tex), one.tex.shape[0], one.tex.shape[1], one.tex.shape[2], _p(one.F), _p(one.V),
                            IOR, EXT, int(law[2] == "snell"), 1, _p(cls), _p(tape), _p(hits), _p(one.void), _p(one.invalid), _p(targets), None, _p(grad), _p(g_ior),
                            _p(count))
    want = {k: sum(r[k] for r in refs) for k in ("loss", "grad_V", "g_int", "g_ext", "count")}
    rel = abs(loss - want["loss"]) / want["loss"]
    print(f"{order} {law}: loss {loss:.12e} against {want['loss']:.12e} ({rel:.2e}); count {int(count[0])}")
    assert rel <= cases.LOSS_REL and int(count[0]) == want["count"] > 0
    assert cases.close(grad, want["grad_V"]) and cases.close(g_ior[0], want["g_int"]) and cases.close(g_ior[1], want["g_ext"])
    assert not cases.close(grad, refs[0]["grad_V"])                                      # (one view alone is outside the tolerance)


# ---- the argument checks -------------------------------------------------------------------------------------------------------------------
def _bind_args(n=4, H=8, W=6, C=3):
    from drt_amd import render
    cams = [image_cases.camera(5 + k, H, W) for k in range(n)]
    screens = [render.Screen([0, 0, k], [1, 0, 0], [0, 1, 0]) for k in range(n)]
    return dict(cameras=cams, height=H, width=W, screens=screens, targets=np.zeros((n, H, W, C), np.float32))


def test_bind_arguments_of_every_accepted_form():
    from drt_amd import render
    a = _bind_args()
    got = render.check_image_views_args(**a)
    assert got["cameras"].shape == (4, 21) and got["screens"].shape == (4, 9) and got["targets"].shape == (4, 8, 6, 3) and got["weights"] is None
    assert np.array_equal(got["cameras"][2], _cam21(a["cameras"][2])) and np.array_equal(got["screens"][3], a["screens"][3].packed())
    b = np.arange(4 * 8 * 6, dtype=np.uint8).reshape(4, 8, 6)
    got = render.check_image_views_args(**dict(a, targets=b, weights=np.ones((4, 8, 6), np.float32)))
    assert got["channels"] == 1 and np.array_equal(got["targets"][..., 0], b.astype(np.float32) / np.float32(255.0)) and got["weights"].shape == (4, 8, 6)


def _skewed(a):
    sc = a["screens"][3]
    sc.ev = np.array([1e-6, 1.0, 0.0])            # no longer orthogonal to eu = (1, 0, 0)
    return a


@pytest.mark.parametrize("name,change,match", [
    ("a non-orthogonal screen in row 3 of 4", _skewed, r"screens\[3\].*orthogonal"),
    ("fewer screens than cameras", lambda a: dict(a, screens=a["screens"][:3]), "screens"),
    ("a target stack of another height", lambda a: dict(a, targets=np.zeros((4, 7, 6, 3), np.float32)), "targets"),
    ("a target stack of fewer views", lambda a: dict(a, targets=np.zeros((3, 8, 6, 3), np.float32)), "targets"),
    ("two channels", lambda a: dict(a, targets=np.zeros((4, 8, 6, 2), np.float32)), "targets"),
    ("float64 targets", lambda a: dict(a, targets=np.zeros((4, 8, 6, 3))), "targets"),
    ("a weight stack with a channel axis", lambda a: dict(a, weights=np.zeros((4, 8, 6, 1), np.float32)), "weights"),
    ("a weight stack of another width", lambda a: dict(a, weights=np.zeros((4, 8, 5), np.float32)), "weights"),
    ("no views", lambda a: dict(a, cameras=[], screens=[]), "cameras"),
    ("a camera that is no tuple of four", lambda a: dict(a, cameras=a["cameras"][:3] + [a["cameras"][3][:3]]), r"cameras\[3\]"),
    ("a screen that is none", lambda a: dict(a, screens=a["screens"][:3] + [(0, 1, 2)]), r"screens\[3\]"),
    ("no pixels", lambda a: dict(a, height=0), "height"),
])
def test_bind_image_views_names_the_bad_argument(name, change, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.bind_image_views(object(), **change(_bind_args()))


def _fake_binding():
    """A binding with everything the argument checks read and no device table behind it."""
    from drt_amd import render
    b = render.ImageViews.__new__(render.ImageViews)
    b.args = render.check_image_views_args(**_bind_args())
    b.n, b.height, b.width, b.channels, b._h, b._mesh, b.scene = 4, 8, 6, 3, None, None, None
    return b


@pytest.mark.parametrize("ids,kw,match", [([], {}, "view_ids"), (list(range(4)) * 4 + [0], {}, "view_ids"), ([0, 4], {}, "view 4"), ([-1], {}, "view -1"),
                                          ([0.0], {}, "view_ids"), (7, {}, "view_ids"), ([0, 1], {"supersample": 5}, "supersample"),
                                          ([0, 1], {"max_bounces": 9}, "max_bounces"), ([0, 1], {"tir": "mirror"}, "tir"), ([0, 1], {"vertices": 1}, "vertices"),
                                          ([0, 1], {"ior_int": -1.0}, "ior_int"), ([0, 1], {"max_samples": 0}, "max_samples"),
                                          ([0, 1], {"texture": np.zeros((4, 4), np.float32)}, "channels")])
def test_image_loss_views_fused_names_the_bad_argument(ids, kw, match):
    """k = 0, k = 17, an id out of range and the law keywords: raised before anything touches the device."""
    from drt_amd import diffrender
    kw = dict(kw)
    texture = kw.pop("texture", np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_views_fused(object(), _fake_binding(), ids, texture, **kw)
    with pytest.raises(ValueError, match="binding"):
        diffrender.Scene.image_loss_views_fused(object(), object(), [0], texture)


def test_the_bands_of_a_call_cover_the_tall_image():
    from drt_amd import render
    a = render.check_image_views_law(_fake_binding(), [3, 0, 3], np.zeros((4, 4, 3), np.float32), supersample=2, max_samples=6 * 4 * 5)
    assert a["ids"] == [3, 0, 3] and a["height"] == 24 and a["bands"] == render.plan_bands(24, 6, 2, 6 * 4 * 5)
    assert a["bands"][1] == (5, 10) and a["bands"][-1] == (20, 24)                       # (5, 10) straddles the border at row 8


def test_the_table_checks_of_the_library_need_no_device():
    from drt_amd import _lib
    lib = _lib.lib()
    cams, screens = _table(4)
    screens[:, 3:6], screens[:, 6:9] = [2.0, 0.0, 0.0], [0.0, 0.5, 0.0]
    assert lib.drt_image_views_check(4, _p(cams), _p(screens), 8, 6) == 0
    bad = screens.copy()
    bad[3, 6:9] = [1e-6, 0.5, 0.0]
    for args, word in (((4, _p(cams), _p(bad), 8, 6), b"row 3"), ((0, _p(cams), _p(screens), 8, 6), b"n_views"), ((4, None, _p(screens), 8, 6), b"null"),
                       ((4, _p(cams), None, 8, 6), b"null"), ((4, _p(cams), _p(screens), 0, 6), b"height"), ((4, _p(cams), _p(screens), 8, -1), b"width"),
                       ((4, _p(cams), _p(screens), 2 ** 28, 6), b"height")):
        assert lib.drt_image_views_check(*args) == -1 and word in lib.drt_last_error()
    h = ctypes.c_void_p()
    assert lib.drt_image_views_create(None, 4, _p(cams), _p(screens), 8, 6, ctypes.byref(h)) != 0 and not h.value
    assert lib.drt_render_image_loss_views(*([None] * 4), 2, 0, 8, 1, 1.5, 1.0, 2, 0, 1, None, 4, 4, 3, *([None] * 9)) != 0
    lib.drt_image_views_destroy(None)              # no-op


def test_entry_points_are_declared_everywhere():
    from drt_amd import _lib, build, diffrender, optim, captured_data
    assert len(_lib.SIGNATURES["drt_render_image_loss_views"][1]) == 26 and "drt_image_views.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_loss_views(" in header and "int drt_image_views_create(" in header
    assert _lib.lib().drt_version() == 13
    assert callable(diffrender.enqueue_image_views_term) and callable(optim.optimize_photometric) and issubclass(captured_data.PhotoData, captured_data.Data)


def test_the_photo_loop_refuses_a_process_group(tmp_path):
    import torch.distributed as dist
    from drt_amd import optim
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/group", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="torch.distributed"):
            optim.PhotoIteration(object(), object(), dict(optim.HyperParams, image_w=1.0), 0.1)
    finally:
        dist.destroy_process_group()
