"""GPU: Scene.render_image -- the refracted image of a mesh in front of a textured screen (drt_render_image, drt_amd/csrc/drt_image.hip)
-- against the float64 restatement tests/image_ref.py on small views of data/hand_vh.ply (tests/image_cases.py).

What must be exact: the ``hit`` and ``through`` planes, on every pixel -- the sample rays have the restatement's bits (tests/test_image_host.py
holds the header to it with tolerance 0) and the tracer contract is shared, as in tests/test_gpu_paths.py.

The image: at most tol = 2^-23 + G * 1e-10 * (1 + t_max) * 21 / pitch (image_cases.tolerance: the project's exit-ray tolerance carried
through the plane hit off the grazing cut and one texel step of the bilinear sample, plus the float32 store): 3.2e-7 for these scenes
(t_max = 348 mm, pitch = 2 * 114.76 mm / 63 = 3.64 mm, G = 0.997: 1.19e-7 + 2.00e-7).  Pixels with a sample that grazes the screen (|dot(d, n)| < 0.05) or lands within 1e-3 texel
of one of its borders are left out of the image comparison -- measured on the CPU with the restatement: 0, 1, 7, 10, 13, 14 of 1 024 and
0, 16, 13 of 960 for the scenes and laws below -- and their share is asserted to stay below 3 %."""
import os

import numpy as np
import pytest
import torch

import image_cases
import image_ref
from conftest import IOR, data_path
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


@pytest.fixture(scope="module")
def hand_scene():
    return Render.Scene(image_cases.hand(), 0)


def _render(scene, name, law=(2, "drop", "reference"), fresnel=True, texture=None, **kw):
    sc = image_cases.scene(name)
    args = dict(supersample=sc["s"], max_bounces=law[0], tir=law[1], refraction=law[2], fresnel=fresnel, void=sc["void"], invalid=sc["invalid"],
                want_planes=True)
    args.update(kw)
    return scene.render_image(sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"] if texture is None else texture, **args)


def _check_against(name, law, fresnel, got):
    image, hit, through = got
    sc = image_cases.scene(name)
    ref = image_cases.reference(name, law, fresnel)
    assert image.dtype == hit.dtype == through.dtype == torch.float32 and image.is_cuda
    assert image.shape == ref["image"].shape == (sc["height"], sc["width"], sc["texture"].shape[2]) and hit.shape == through.shape == image.shape[:2]
    bad = image_cases.sensitive(name, ref)
    tol = image_cases.tolerance(name, ref)
    diff = (image.cpu().double() - ref["image"].double()).abs().amax(2).numpy()
    print(name, law, "fresnel" if fresnel else "geometry", "sensitive pixels", int(bad.sum()), "of", bad.size, "tol", tol, "max diff", diff[~bad].max(),
          "max diff on sensitive pixels", diff[bad].max() if bad.any() else 0.0, "planes differ on", int((hit.cpu() != ref["hit"]).sum()),
          int((through.cpu() != ref["through"]).sum()))
    assert torch.equal(hit.cpu(), ref["hit"]) and torch.equal(through.cpu(), ref["through"])          # exact, every pixel
    assert bad.mean() <= image_cases.SENSITIVE_CAP
    assert np.isfinite(diff).all() and diff[~bad].max() <= tol


# ------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("fresnel", [True, False], ids=["fresnel", "geometry"])
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
@pytest.mark.parametrize("name", ["v5", "v41"])
def test_image_and_planes_against_the_restatement(hand_scene, name, law, fresnel):
    _check_against(name, law, fresnel, _render(hand_scene, name, law, fresnel))
    ref = image_cases.reference(name, law, fresnel)
    cls = ref["cls"].numpy()
    looks = cls != image_ref.INVALID
    # the scene reaches every class and both fills
    assert (cls == 0).sum() > 2000 and (cls == 1).sum() > 900 and (cls == 2).sum() > 50 and (looks & ~ref["on"].numpy()).sum() > 1000
    if law[0] == 6:
        assert (looks & ~(ref["t"] > 0).numpy()).sum() > 50                # exit rays that point away from the screen


@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_non_square_single_channel_image(hand_scene, law):
    """24 x 40 pixels, C = 1: swapped axes cannot pass."""
    _check_against("wide", law, True, _render(hand_scene, "wide", law, True))


# --------------------------------------------------------------------------------------------------------- bands, repeats, modes
def _odd_view(scene, **kw):
    """31 x 32 pixels: bands of ten rows leave a last band of a single row."""
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, 31, 32)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    return scene.render_image(cam, 31, 32, screen, image_cases.texture(3), supersample=2, max_bounces=6, tir="reflect", refraction="snell", void=0.25,
                              invalid=0.75, want_planes=True, **kw)


def test_bands_give_the_bits_of_the_whole_image(hand_scene):
    whole = _odd_view(hand_scene)
    row = 32 * 4
    assert render.plan_bands(31, 32, 2, 10 * row + 5) == [(0, 10), (10, 20), (20, 30), (30, 31)]
    for cap in (10 * row + 5, row - 1, 3 * row):          # four bands the last a single row; 31 single rows, each over the cap; eleven bands
        banded = _odd_view(hand_scene, max_samples=cap)
        for a, b in zip(whole, banded):
            assert torch.equal(a, b)
    assert whole[1].max() == 1 and whole[2].max() == 1 and 0 < whole[2].mean() < whole[1].mean() < 1


def test_two_runs_give_the_same_bits(hand_scene):
    a = _render(hand_scene, "v41", LAWS[2])
    b = _render(hand_scene, "v41", LAWS[2])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    only = _render(hand_scene, "v41", LAWS[2], want_planes=False)
    assert isinstance(only, torch.Tensor) and torch.equal(only, a[0])


def test_deterministic_mode_changes_nothing(hand_scene):
    plain = _render(hand_scene, "v5", LAWS[1])
    was = det.enable(True)
    try:
        fixed = _render(hand_scene, "v5", LAWS[1])
    finally:
        det.enable(was)
    for x, y in zip(plain, fixed):
        assert torch.equal(x, y)


def test_other_calls_on_the_scene_keep_their_bits(deterministic):
    """render_paths and paths_ray_loss_fused share the scene's ray lists with render_image: each gives the same bits before and after one
    (deterministic accumulation, so that the one-pass call's own sums do not depend on the order of its atomics)."""
    mesh = image_cases.hand()
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    cam = image_cases.camera(5, 48, 48)
    o, d = (t.cuda() for t in views.generate_ray(48, 48, cam[3], cam[2]))
    rng = np.random.default_rng(5)
    sp = torch.tensor(rng.standard_normal((48 * 48, 3)) * 40.0 + np.asarray(image_cases.frame()[0]) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(48 * 48) > 0.1, device="cuda")

    def others():
        with torch.no_grad():
            out = [t.clone() for t in scene.render_paths(o, d, 6, "reflect", "snell")]
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", "snell")
        g, = torch.autograd.grad(loss, V)
        return out + [loss.detach().clone(), g.clone()]

    before = others()
    image = _render(scene, "v5", LAWS[2])
    after = others()
    again = _render(scene, "v5", LAWS[2])
    assert before[2].any() and before[3].item() > 0 and before[4].any()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    for a, b in zip(image, again):
        assert torch.equal(a, b)
    _check_against("v5", LAWS[2], True, image)            # this scene's vertices went through update_verticex: the same image


# ----------------------------------------------------------------------------------------------------------------------- throughput
@pytest.mark.parametrize("law", LAWS, ids=LAW_IDS)
def test_throughput_of_a_constant_texture(hand_scene, law):
    sc = image_cases.scene("v5")
    ones = np.ones((8, 8, 1), np.float32)
    center, extent = image_cases.frame()
    screen = render.Screen.behind(sc["camera_M"], center, extent, 8, 8, span=image_cases.SPAN)
    out = {}
    for fresnel in (True, False):
        out[fresnel] = hand_scene.render_image(sc["camera_M"], 32, 32, screen, ones, supersample=2, max_bounces=law[0], tir=law[1], refraction=law[2],
                                               fresnel=fresnel, void=1.0, invalid=0.0, want_planes=True)
    (img_f, hit_f, thr_f), (img_g, hit_g, thr_g) = out[True], out[False]
    assert torch.equal(hit_f, hit_g) and torch.equal(thr_f, thr_g)
    only = thr_f == 1                                      # every sample of the pixel went through the object
    assert only.sum() > 50
    assert (img_g[only] == 1).all()                         # geometry only: the texture (or the void fill, also 1) unweighted
    assert (img_f[only] > 0).all() and (img_f[only] <= 1).all() and (img_f[only] < 1).any()
    assert (img_f <= img_g).all()
    direct = hit_f == 0
    assert direct.sum() > 400 and (img_f[direct] == 1).all() and (img_g[direct] == 1).all()


# --------------------------------------------------------------------------------------------------------------------- empty scenes
def _pure_direct(sc, cam, screen):
    return image_ref.render(np.zeros((0, 3), np.int64), np.zeros((0, 3)), cam, sc["height"], sc["width"], screen, sc["texture"], sc["s"], 6, "reflect", "snell",
                            True, sc["void"], sc["invalid"], IOR, EXT)


def test_a_scene_without_triangles_renders_every_sample_as_direct():
    sc = image_cases.scene("v5")
    scene = Render.Scene(image_cases.hand(), 0)
    scene.optix_mesh.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), scene.vertices.detach().to(torch.float32))
    image, hit, through = _render(scene, "v5", LAWS[2])
    ref = _pure_direct(sc, sc["camera_M"], sc["screen"])
    assert not hit.any() and not through.any()
    assert (image.cpu().double() - ref["image"].double()).abs().max() <= image_cases.tolerance("v5", ref)
    assert ref["on"].any() and not ref["on"].all()         # the texture and the void fill are both in the picture


def test_a_camera_turned_away_from_the_mesh_sees_the_screen_alone(hand_scene):
    sc = image_cases.scene("v5")
    R, K, Rinv, Kinv = sc["camera_M"]
    R2 = np.diag([-1.0, 1.0, -1.0, 1.0]) @ R               # half a turn about the camera's y axis: the same position, looking the other way
    cam = (R2, K, np.linalg.inv(R2), Kinv)
    center, extent = image_cases.frame()
    screen = render.Screen.behind(cam, np.asarray(center) - 2.0 * 1.2 * extent * R[2, :3], extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    image, hit, through = hand_scene.render_image(cam, sc["height"], sc["width"], screen, sc["texture"], supersample=sc["s"], max_bounces=6, tir="reflect",
                                                  refraction="snell", void=sc["void"], invalid=sc["invalid"], want_planes=True)
    ref = _pure_direct(sc, cam, screen)
    full = image_ref.render(sc["mesh"].faces, sc["mesh"].vertices, cam, sc["height"], sc["width"], screen, sc["texture"], sc["s"], 6, "reflect", "snell", True,
                            sc["void"], sc["invalid"], IOR, EXT)
    assert not full["hit"].any() and torch.equal(full["image"], ref["image"])
    assert not hit.any() and not through.any()
    assert ref["on"].any()
    t = ref["t"].numpy()[ref["on"].numpy()]
    tex = sc["texture"].astype(np.float64)
    G = max(np.abs(np.diff(tex, axis=0)).max(), np.abs(np.diff(tex, axis=1)).max())
    tol = 2.0 ** -23 + G * image_cases.RAY_ABS * (1.0 + t.max()) * (1.0 + 1.0 / image_cases.GRAZING) / np.linalg.norm(screen.eu)
    assert (image.cpu().double() - ref["image"].double()).abs().max() <= tol


# ------------------------------------------------------------------------------------------------------------------- the command line
DATA_DIR = os.path.dirname(data_path("hand_vh.ply"))


def _cli_law():
    return ["--supersample", "2", "--max-bounces", "6", "--tir", "reflect", "--refraction", "snell", "--texture-size", "64", "--format", "ppm"]


def test_cli_writes_the_images_of_turntable_cameras(hand_scene, tmp_path):
    rep = render.main(["--name", "hand", "--data-path", DATA_DIR, "--views", "72", "--view-ids", "5", "41", "--res", "24", "40", "--background", "ramp", "-o", str(tmp_path)] + _cli_law())
    assert [v["view"] for v in rep["views"]] == [5, 41] and (rep["height"], rep["width"]) == (24, 40)
    center, extent = image_cases.frame()
    tex = render.ramp(64, 64)
    for v in rep["views"]:
        cam = views.turntable_cameras(center, extent, 72, 40, 24)[v["view"]]
        image, hit, through = hand_scene.render_image(cam, 24, 40, render.Screen.behind(cam, center, extent, 64, 64), tex, supersample=2, max_bounces=6,
                                                      tir="reflect", refraction="snell", want_planes=True)
        back = render.load_texture(v["image"])
        assert np.array_equal(back, render.to_bytes(image).astype(np.float32) / np.float32(255.0))
        assert v["hit_share"] == pytest.approx(float(hit.mean())) and 0 < v["through_share"] < v["hit_share"] < 1
    with pytest.raises(SystemExit, match="--force"):
        render.main(["--name", "hand", "--data-path", DATA_DIR, "--view-ids", "5", "-o", str(tmp_path)] + _cli_law())


def test_cli_uses_the_cameras_of_a_capture(hand_scene, tmp_path):
    """A small capture file of the reference's schema with a camera that is orthonormal to float32 only: the size comes from its masks."""
    from drt_amd import captured_data
    center, extent = image_cases.frame()
    cams = views.turntable_cameras(center, extent, 4, 40, 24, distance_factor=1.5)
    proj = np.stack([c[0] for c in cams]).astype(np.float32).astype(np.float64)
    path = captured_data.write_capture(str(tmp_path / "hand.h5"), {"cam_proj": proj, "cam_k": cams[0][1], "mask": np.zeros((4, 24, 40), np.uint8),
                                                                    "screen_position": np.zeros((4, 24, 40, 3))})
    rep = render.main(["--name", "hand", "--data-path", DATA_DIR, "--capture", path, "--view-ids", "0", "3", "--res", "8", "8", "--background", "checker", "--no-fresnel",
                       "-o", str(tmp_path / "out")] + _cli_law())
    assert (rep["height"], rep["width"]) == (24, 40) and [v["view"] for v in rep["views"]] == [0, 3]
    tex = render.checker(64, 64, 16)
    for v in rep["views"]:
        cam = (proj[v["view"]], cams[0][1], np.linalg.inv(proj[v["view"]]), np.linalg.inv(cams[0][1]))
        image = hand_scene.render_image(cam, 24, 40, render.Screen.behind(cam, center, extent, 64, 64), tex, supersample=2, max_bounces=6, tir="reflect",
                                        refraction="snell", fresnel=False)
        back = render.load_texture(v["image"])
        assert back.shape == (24, 40, 1) and np.array_equal(back, render.to_bytes(image).astype(np.float32) / np.float32(255.0))
        assert 0 < v["through_share"] < v["hit_share"] < 1


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_errors_leave_the_output_untouched(hand_scene):
    lib = _lib.lib()
    assert lib.drt_version() >= 8
    sc = image_cases.scene("v5")
    a = render.check_render_args(sc["camera_M"], 16, 16, sc["screen"], sc["texture"], 2)
    tex = torch.as_tensor(a["texture"], device="cuda")
    V = hand_scene.vertices.detach().contiguous()
    image = torch.full((16, 16, 3), 7.0, dtype=torch.float32, device="cuda")
    planes = [torch.full((16, 16), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    base = dict(height=16, width=16, y0=0, y1=16, s=2, max_bounces=4, law_flags=3, fresnel=1, screen=a["screen"], tex_h=tex.shape[0], tex_w=tex.shape[1],
                channels=3)

    def call(**kw):
        p = dict(base, **kw)
        screen = np.ascontiguousarray(p["screen"], dtype=np.float64)
        return lib.drt_render_image(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, p["height"], p["width"], p["y0"], p["y1"], p["s"], IOR, EXT,
                                    p["max_bounces"], p["law_flags"], p["fresnel"], screen.ctypes.data, tex.data_ptr(), p["tex_h"], p["tex_w"], p["channels"],
                                    a["void"].ctypes.data, a["invalid"].ctypes.data, image.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)

    skew, flat = a["screen"].copy(), a["screen"].copy()
    skew[6:9] = skew[6:9] + 1e-6 * skew[3:6]
    flat[3:6] = 0.0
    bad = [dict(s=0), dict(s=5), dict(channels=2), dict(channels=4), dict(tex_h=1), dict(tex_w=1), dict(screen=skew), dict(screen=flat), dict(max_bounces=1),
           dict(max_bounces=9), dict(law_flags=4), dict(law_flags=-1), dict(fresnel=2), dict(y0=5, y1=5), dict(y0=9, y1=3), dict(y0=-1, y1=4), dict(y0=0, y1=17),
           dict(height=0, y1=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                        # DRT_E_INVALID
        assert lib.drt_last_error()
    torch.cuda.synchronize()
    assert (image == 7).all() and (planes[0] == 7).all() and (planes[1] == 7).all()
    # the good call writes its band and nothing else; the planes may be NULL
    assert call(y0=3, y1=9) == 0
    torch.cuda.synchronize()
    assert (image[:3] == 7).all() and (image[9:] == 7).all() and (image[3:9] != 7).all() and (planes[0][3:9] <= 1).all() and (planes[1][:3] == 7).all()
    assert lib.drt_render_image(hand_scene.optix_mesh._h, V.data_ptr(), a["camera"].ctypes.data, 16, 16, 0, 16, 2, IOR, EXT, 4, 3, 1, a["screen"].ctypes.data,
                                tex.data_ptr(), tex.shape[0], tex.shape[1], 3, a["void"].ctypes.data, a["invalid"].ctypes.data, image.data_ptr(), None, None,
                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (image != 7).all()


def test_a_workspace_that_would_grow_under_capture_is_refused():
    """The first call of a size allocates; inside a stream capture it is refused with a message, and works after one eager call."""
    scene = Render.Scene(image_cases.hand(), 0)
    sc = image_cases.scene("v5")
    tex = torch.as_tensor(sc["texture"]).cuda()            # on the device already: the capture sees no host copy
    _render(scene, "v5", LAWS[0], texture=tex, supersample=1)      # the workspace now holds 32 x 32 samples
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_lib.DrtError, match="eagerly before capturing"):
        with torch.cuda.graph(g):
            _render(scene, "v5", LAWS[0], texture=tex)     # four times as many
    torch.cuda.synchronize()
    eager = _render(scene, "v5", LAWS[0])
    _check_against("v5", LAWS[0], True, eager)
    assert sc["s"] == 2
