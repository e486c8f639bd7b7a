"""CPU: the forward renderer's law of drt_amd/csrc/drt_image.h, compiled for the host by g++ with -ffp-contract=off
(tests/hostsim/image.cpp), against the restatement tests/image_ref.py, and the Python layer's checks that need no GPU.

Tolerance 0 where the two sides are held against each other, derived and not measured: both perform the same correctly rounded IEEE-754
operations in the same order (the law fixes the association of every expression, contraction is off on both sides, torch's elementwise
float64 arithmetic does not fuse).  A difference is a bug in the header or a restatement that reorders."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_ref
from conftest import golden
from drt_amd import render, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int


@pytest.fixture(scope="module")
def hs():
    src = os.path.join(ROOT, "tests", "hostsim", "image.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h", "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.image_rays.argtypes = [_P, _I, _I, _I, _P, _P]
    lib.image_fresnel.argtypes = [_P, _P, _P, _I64, _P]
    lib.image_factor.restype = _D
    lib.image_factor.argtypes = [_I, _D, _D, _D, _D]
    lib.image_axes_ok.argtypes = [_P]
    lib.image_colours.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P]
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _cam21(camera_M):
    return np.ascontiguousarray(np.concatenate([np.asarray(camera_M[3]).reshape(-1), np.asarray(camera_M[2])[:3, :].reshape(-1)]))


def host_fresnel(hs, ci, eta_i, eta_t):
    ci, eta_i, eta_t = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), np.shape(ci)).copy()) for a in (ci, eta_i, eta_t))
    R = np.empty_like(ci)
    hs.image_fresnel(_p(ci), _p(eta_i), _p(eta_t), ci.size, _p(R))
    return R


# ---- sample rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
def test_sample_rays_equal_the_restatement(hs, s):
    H, W = 9, 13
    cam = image_cases.camera(5, H, W)
    o, d = np.empty((H * W * s * s, 3)), np.empty((H * W * s * s, 3))
    hs.image_rays(_p(_cam21(cam)), H, W, s, _p(o), _p(d))
    ro, rd = image_ref.sample_rays(cam[3], cam[2], H, W, s)
    assert same_bits(o, ro.numpy()) and same_bits(d, rd.numpy())
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
    if s == 1:
        # generate_ray adds and subtracts the camera position (up to 1e3 mm) before it normalises: 1e-12 absolute
        go, gd = views.generate_ray(H, W, cam[3], cam[2])
        assert np.abs(o - go.numpy()).max() <= 1e-12 and np.abs(d - gd.numpy()).max() <= 1e-12
    else:
        # the s x s samples of a pixel straddle its centre: their mean direction is the centre ray's to first order
        c = image_ref.sample_rays(cam[3], cam[2], H, W, 1)[1].numpy()
        assert np.abs(d.reshape(H * W, s * s, 3).mean(1) - c).max() < 1e-3


def test_samples_are_pixel_major_and_row_major_within_the_pixel(hs):
    H, W, s = 2, 3, 2
    cam = (None, None, np.eye(4), np.eye(3))            # identity camera: dir is (px, py, 1) normalised
    o, d = np.empty((H * W * s * s, 3)), np.empty((H * W * s * s, 3))
    hs.image_rays(_p(_cam21(cam)), H, W, s, _p(o), _p(d))
    p = (d / d[:, 2:3])[:, :2].reshape(H, W, s, s, 2)
    for y in range(H):
        for x in range(W):
            for b in range(s):
                for a in range(s):
                    assert np.allclose(p[y, x, b, a], [x + (a + 0.5) / s - 0.5, y + (b + 0.5) / s - 0.5], atol=1e-15)
    assert not o.any()


# ---- fresnel_R ------------------------------------------------------------------------------------------------------------------------
def test_fresnel_against_the_references_own_table(hs):
    """tests/golden/unit_tables.npz: fr_R made by the reference's FrDielectric.  1e-14 absolute: about ten correctly rounded operations
    on terms of magnitude up to 2.5 for an R in [0, 1]."""
    g = golden("unit_tables")
    keep = ~g["fr_tir"]
    assert keep.sum() > 100
    ci, ei, et = g["fr_cos"][keep], g["fr_etaI"][keep], g["fr_etaT"][keep]
    R = host_fresnel(hs, ci, ei, et)
    assert np.abs(R - g["fr_R"][keep]).max() <= 1e-14
    assert same_bits(R, image_ref.fresnel_R(ci, ei, et).numpy())
    assert (R >= 0).all() and (R <= 1).all()


@pytest.mark.parametrize("eta_i,eta_t", [(1.00029, 1.4723), (1.4723, 1.00029), (1.0, 1.5), (1.5, 1.0)])
def test_fresnel_closed_forms(hs, eta_i, eta_t):
    normal = host_fresnel(hs, np.array([1.0]), eta_i, eta_t)[0]
    assert normal == pytest.approx(((eta_i - eta_t) / (eta_i + eta_t)) ** 2, abs=1e-15)
    if eta_i < eta_t:                                     # no TIR from the thinner side: grazing incidence reflects everything
        assert host_fresnel(hs, np.array([0.0]), eta_i, eta_t)[0] == 1.0


def test_a_mirrored_interaction_leaves_the_throughput_alone(hs):
    for sg in (1.0, -1.0):
        assert hs.image_factor(1, sg, 0.3, 1.00029, 1.4723) == 1.0
    # a refracting one multiplies by 1 - R with the eta pair of its side
    for sg, (ei, et) in ((1.0, (1.00029, 1.4723)), (-1.0, (1.4723, 1.00029))):
        assert hs.image_factor(0, sg, 0.9, 1.00029, 1.4723) == 1.0 - host_fresnel(hs, np.array([0.9]), ei, et)[0]
    f = hs.image_factor(0, 1.0, 0.9, 1.00029, 1.4723)
    assert 0.0 < f < 1.0


# ---- plane and bilinear -----------------------------------------------------------------------------------------------------------------
def _exit_rays(screen, tex_h, tex_w, rng):
    """Exit rays that cover: the inside, each border exactly, just outside, t <= 0, dot(d, n) = 0, both faces."""
    p0, eu, ev = screen.p0, screen.eu, screen.ev
    n = np.cross(eu, ev)
    n /= np.linalg.norm(n)
    uv = [(rng.uniform(0, tex_w - 1), rng.uniform(0, tex_h - 1)) for _ in range(40)]
    uv += [(0.0, 3.25), (tex_w - 1.0, 3.25), (4.5, 0.0), (4.5, tex_h - 1.0), (0.0, 0.0), (tex_w - 1.0, tex_h - 1.0), (2.0, 5.0), (tex_w - 2.0, tex_h - 2.0)]
    uv += [(-1e-9, 2.0), (tex_w - 1 + 1e-9, 2.0), (2.0, -1e-9), (2.0, tex_h - 1 + 1e-9), (-3.0, -3.0), (tex_w + 5.0, 1.0)]
    o, d, tag = [], [], []
    for k, (u, v) in enumerate(uv):
        q = p0 + u * eu + v * ev
        side = 1.0 if k % 2 == 0 else -1.0                       # both faces of the screen
        origin = q - side * 50.0 * n
        if 40 <= k < 48:                                         # straight along the normal from an exactly representable offset: u, v come out exact
            o.append(origin); d.append(side * n); tag.append("exact")
        else:
            tilt = rng.standard_normal(3) * 0.2
            start = origin + 20.0 * tilt
            dirv = q - start
            o.append(start); d.append(dirv / np.linalg.norm(dirv)); tag.append("in" if k < 40 else "out")
    # t <= 0: looking away, and starting on the plane; dot(d, n) = 0: parallel to the screen
    q = p0 + 3.0 * eu + 3.0 * ev
    o += [q - 10.0 * n, q, q - 10.0 * n]
    d += [-n, n, eu / np.linalg.norm(eu)]
    tag += ["away", "on-plane", "parallel"]
    return np.ascontiguousarray(o), np.ascontiguousarray(d), tag


@pytest.mark.parametrize("channels", [1, 3])
def test_plane_and_bilinear_equal_the_restatement(hs, channels):
    rng = np.random.default_rng(3)
    tex_h, tex_w = 9, 12
    # an axis-aligned screen with power-of-two pitches: u, v of the hand-placed rays are exact, so the borders are hit exactly
    screen = render.Screen([-4.0, 8.0, 16.0], [0.5, 0.0, 0.0], [0.0, -0.25, 0.0])
    tex = rng.random((tex_h, tex_w, channels)).astype(np.float32)
    o, d, tag = _exit_rays(screen, tex_h, tex_w, rng)
    n = len(o)
    cls = np.ascontiguousarray(rng.integers(0, 2, n), dtype=np.int32)
    cls[5] = cls[11] = image_ref.INVALID
    T = np.ascontiguousarray(rng.uniform(0.5, 1.0, n))
    void, invalid = np.array([0.125, 0.25, 0.375][:channels]), np.array([0.5, 0.625, 0.75][:channels])
    col, on, uv = np.full((n, channels), np.nan), np.zeros(n, np.uint8), np.full((n, 2), np.nan)
    hs.image_colours(_p(screen.packed()), _p(tex), tex_h, tex_w, channels, _p(cls), _p(o), _p(d), _p(T), n, _p(void), _p(invalid), _p(col), _p(on), _p(uv))
    rcol, ron, ru, rv, rt, rdn = image_ref.sample_colours(screen, tex, torch.as_tensor(cls.astype(np.int64)), torch.as_tensor(o), torch.as_tensor(d),
                                                          torch.as_tensor(T), void, invalid)
    assert np.array_equal(on.astype(bool), ron.numpy())
    assert same_bits(col, rcol.numpy())
    sel = on.astype(bool)
    assert same_bits(uv[sel, 0], ru.numpy()[sel]) and same_bits(uv[sel, 1], rv.numpy()[sel])
    # the cases are what they claim to be
    looks = cls != image_ref.INVALID
    tag = np.array(tag)
    assert on[(tag == "in") & looks].all() and on[(tag == "exact") & looks].all()
    assert not on[(tag == "out")].any() and not on[np.isin(tag, ["away", "on-plane", "parallel"])].any()
    assert (col[(tag == "out") & looks] == void).all() and (col[~looks] == invalid).all()
    u_exact = uv[tag == "exact", 0][looks[tag == "exact"]]
    assert set(u_exact.tolist()) <= {0.0, tex_w - 1.0, 4.5, 2.0, tex_w - 2.0}
    assert rdn.numpy()[tag == "parallel"][0] == 0.0 and (rdn.numpy()[tag == "in"] > 0).any() and (rdn.numpy()[tag == "in"] < 0).any()
    # a sample exactly on a texel reads that texel, weighted
    k = int(np.nonzero((tag == "exact") & looks)[0][-1])
    ui, vi = int(uv[k, 0]), int(uv[k, 1])
    assert uv[k, 0] == ui and uv[k, 1] == vi and np.array_equal(col[k], T[k] * tex[vi, ui].astype(np.float64))


def test_pixel_mean_is_left_to_right_and_rounded_once():
    col = torch.tensor([[0.1], [0.2], [0.3], [1e-17]], dtype=torch.float64)
    assert image_ref.pixel_mean(col, 2)[0, 0].item() == np.float32((((0.1 + 0.2) + 0.3) + 1e-17) / 4.0)


def test_axes_check(hs):
    ok = lambda *s9: hs.image_axes_ok(_p(np.ascontiguousarray(np.concatenate(s9), dtype=np.float64)))      # noqa: E731
    z = np.zeros(3)
    assert ok(z, [1.0, 0, 0], [0, 2.0, 0]) == 1
    assert ok(z, [1.0, 0, 0], [1e-13, 2.0, 0]) == 1 and ok(z, [1.0, 0, 0], [1e-11, 2.0, 0]) == 0
    assert ok(z, z, [0, 2.0, 0]) == 0 and ok(z, [1.0, 0, 0], [np.nan, 1.0, 0]) == 0 and ok(z, [np.inf, 0, 0], [0, 1.0, 0]) == 0


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,width,s,cap", [(32, 32, 2, 1 << 22), (32, 32, 2, 1500), (7, 5, 3, 100), (9, 40, 1, 39), (1, 1, 4, 1), (1080, 1920, 3, 1 << 22)])
def test_plan_bands(height, width, s, cap):
    bands = render.plan_bands(height, width, s, cap)
    assert bands[0][0] == 0 and bands[-1][1] == height
    assert all(a1 == b0 for (_, a1), (b0, _) in zip(bands, bands[1:])) and all(y0 < y1 for y0, y1 in bands)
    row = width * s * s
    for y0, y1 in bands:
        assert (y1 - y0) * row <= cap or y1 - y0 == 1              # a single row may exceed the cap, nothing else
    if row > cap:
        assert len(bands) == height
    if height * row <= cap:
        assert bands == [(0, height)]


def _args():
    cam = image_cases.camera(5, 8, 8)
    return dict(camera_M=cam, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32))


@pytest.mark.parametrize("key,value", [("camera_M", None), ("camera_M", (np.eye(4),) * 3), ("camera_M", (np.eye(4), np.eye(3), np.eye(3), np.eye(3))),
                                       ("camera_M", (np.eye(4), np.eye(3), np.eye(4), np.full((3, 3), np.nan))),
                                       ("height", 0), ("height", 2.5), ("width", -1), ("supersample", 0), ("supersample", 5), ("supersample", 1.5),
                                       ("max_bounces", 1), ("max_bounces", 9), ("max_bounces", True), ("max_bounces", None), ("max_bounces", "4"), ("max_bounces", 4.0), ("tir", "mirror"), ("refraction", "exact"),
                                       ("refraction", None), ("fresnel", 1), ("fresnel", "on"), ("want_planes", 1), ("screen", (0, 1, 2)),
                                       ("texture", np.zeros((4, 4, 2), np.float32)), ("texture", np.zeros((1, 4, 3), np.float32)),
                                       ("texture", np.zeros((4, 4, 3), np.uint8)), ("texture", np.zeros(4, np.float32)),
                                       ("void", [0.0, 1.0]), ("void", float("nan")), ("invalid", [0.0] * 4), ("invalid", "red"),
                                       ("max_samples", 0), ("max_samples", 1e6)])
def test_render_image_names_the_bad_argument(key, value):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    kw = dict(_args(), **{key: value})
    pos = [kw.pop(k) for k in ("camera_M", "height", "width", "screen", "texture")]
    with pytest.raises(ValueError, match=key):
        diffrender.Scene.render_image(object(), *pos, **kw)


@pytest.mark.parametrize("p0,eu,ev", [([0, 0, 0], [1, 0, 0], [1e-6, 1, 0]), ([0, 0, 0], [0, 0, 0], [0, 1, 0]), ([0, np.nan, 0], [1, 0, 0], [0, 1, 0]),
                                      ([0, 0], [1, 0, 0], [0, 1, 0])])
def test_screen_refuses_bad_axes(p0, eu, ev):
    with pytest.raises(ValueError, match="eu|p0"):
        render.Screen(p0, eu, ev)


def test_screen_behind_is_centred_on_the_view_axis_and_spans_the_extent():
    center, extent = image_cases.frame()
    cam = image_cases.camera(41, 24, 40)
    sc = render.Screen.behind(cam, center, extent, 64, 48, plane_factor=1.5, span=2.0)
    R = cam[0]
    mid = sc.p0 + sc.eu * 31.5 + sc.ev * 23.5
    assert np.allclose(mid, center + 1.5 * extent * R[2, :3], atol=1e-9)
    assert np.linalg.norm(sc.eu) * 63 == pytest.approx(2.0 * extent) and np.linalg.norm(sc.ev) * 47 == pytest.approx(2.0 * extent)
    assert np.allclose(sc.eu / np.linalg.norm(sc.eu), R[0, :3]) and np.allclose(sc.ev / np.linalg.norm(sc.ev), R[1, :3])
    assert abs(np.cross(sc.eu, sc.ev) @ R[2, :3]) == pytest.approx(np.linalg.norm(sc.eu) * np.linalg.norm(sc.ev))
    with pytest.raises(ValueError, match="tex_w"):
        render.Screen.behind(cam, center, extent, 1, 48)


def test_screen_behind_takes_a_camera_that_is_orthonormal_to_float32_only():
    center, extent = image_cases.frame()
    R, K, Rinv, Kinv = image_cases.camera(5, 32, 32)
    R32 = R.astype(np.float32).astype(np.float64)
    R32[1, :3] += 3e-7 * R32[0, :3]                        # a calibrated matrix: rows off the right angle by 1e-7 or so
    assert abs(R32[0, :3] @ R32[1, :3]) > 1e-8
    sc = render.Screen.behind((R32, K, np.linalg.inv(R32), Kinv), center, extent, 64, 64)
    lu, lv = np.linalg.norm(sc.eu), np.linalg.norm(sc.ev)
    assert abs(sc.eu @ sc.ev) <= 1e-12 * lu * lv
    exact = render.Screen.behind((R, K, Rinv, Kinv), center, extent, 64, 64)
    assert np.abs(sc.p0 - exact.p0).max() < 1e-3 and np.abs(sc.eu - exact.eu).max() < 1e-5 and np.abs(sc.ev - exact.ev).max() < 1e-5


@pytest.mark.parametrize("ext", [".npz", ".h5"])
def test_capture_cameras_reads_the_matrices_and_the_image_size_only(tmp_path, ext):
    from drt_amd import captured_data
    cams = [image_cases.camera(k, 6, 10) for k in (5, 41, 7)]
    arrays = {"cam_proj": np.stack([c[0] for c in cams]), "cam_k": cams[0][1], "mask": np.zeros((3, 6, 10), np.uint8),
              "screen_position": np.zeros((3, 6, 10, 3))}
    path = captured_data.write_capture(str(tmp_path / ("cap" + ext)), arrays)
    height, width, got = render.capture_cameras(path, [2, 0])
    assert (height, width) == (6, 10) and sorted(got) == [0, 2]
    for k in (0, 2):
        assert np.array_equal(got[k][0], cams[k][0]) and np.array_equal(got[k][1], cams[k][1])
        assert np.allclose(got[k][2], cams[k][2], atol=1e-12) and np.allclose(got[k][3], cams[k][3], atol=1e-15)
    with pytest.raises(ValueError, match="view 3"):
        render.capture_cameras(path, [3])


def test_procedural_textures():
    c = render.checker(32, 48, 6)
    assert c.shape == (32, 48, 1) and c.dtype == np.float32 and set(np.unique(c).tolist()) == {np.float32(0.1).item(), np.float32(0.9).item()}
    assert c[0, 0, 0] != c[0, 8, 0] and c[0, 0, 0] != c[8, 0, 0] and c[0, 0, 0] == c[8, 8, 0]
    r = render.ramp(16, 33)
    assert r.shape == (16, 33, 3) and r.dtype == np.float32 and r[0, 0, 0] == 0 and r[0, -1, 0] == 1 and r[-1, 0, 1] == 1 and (np.diff(r[:, :, 0], axis=1) > 0).all()


@pytest.mark.parametrize("ext,channels", [(".ppm", 3), (".pgm", 1), (".png", 3), (".png", 1), (".npy", 3)])
def test_write_image_round_trips_and_refuses_to_overwrite(tmp_path, ext, channels):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7, channels)).astype(np.float32) / np.float32(255.0)
    path = str(tmp_path / ("a" + ext))
    if ext == ".npy":
        np.save(path, img)
        written = path
    else:
        written = render.write_image(path, img)
        assert os.path.exists(written) and os.path.splitext(written)[0] == os.path.splitext(path)[0]
        before = open(written, "rb").read()
        with pytest.raises(FileExistsError, match="force"):
            render.write_image(path, np.zeros_like(img))
        assert open(written, "rb").read() == before
        render.write_image(path, img, force=True)
    back = render.load_texture(written)
    assert back.dtype == np.float32 and back.shape == img.shape and np.array_equal(back, img)


def test_write_image_clips_and_rounds():
    assert render.to_bytes(np.array([[-1.0, 0.0, 0.5 / 255, 0.4 / 255, 1.0, 2.0, np.nan]])).reshape(-1).tolist() == [0, 0, 0, 0, 255, 255, 0]
    with pytest.raises(ValueError, match="image"):
        render.to_bytes(np.zeros((2, 2, 2)))


def test_cli_refuses_to_overwrite(tmp_path):
    (tmp_path / "hand_view005.png").write_bytes(b"x")
    with pytest.raises(SystemExit, match="--force"):
        render.main(["--name", "hand", "--view-ids", "5", "-o", str(tmp_path)])
    assert (tmp_path / "hand_view005.png").read_bytes() == b"x"


def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    assert "drt_render_image" in _lib.SIGNATURES and len(_lib.SIGNATURES["drt_render_image"][1]) == 24
    assert "drt_image.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image(" in header
