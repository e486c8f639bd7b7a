"""GPU: Gray-code pattern decoding (drt_amd/csrc/drt_decode.hip: k_decode_patterns; drt_amd/structured_light.py).

The C-ABI call against the numpy restatement tests/decode_ref.py with tolerance 0 -- derived, not measured: codes, contrast, mask and
covered are integer arithmetic; the position is (p0 + x eu) + y ev in float64, one correctly rounded operation after the other in that
association on both sides (the library is built with -ffp-contract=off).  Nothing is accumulated, so two runs give the same bits.

End to end: `synthetic_frames` of the hand (the case of tests/test_decode_host.py: 24 x 24 pixels, a 64 x 64 screen) decoded and held
against `render_paths`; and a `PatternData` against `SyntheticData` on the same turntable (64 x 64 pixels, a 128 x 128 screen).  There
`min_contrast` is 4: rendered photographs carry no sensor noise, their only error is the two uint8 roundings (at most 2 levels between a
pattern and its complement), so twice that separates a decodable bit from a tie; the default 16 is for a camera.  With it the restatement
on the CPU (its IOR is 1.5, the device's 1.4723) keeps 231 of the 279 valid pixels of view 0 (83 %; with 16: 204, 73 % -- the image's centre row and column look exactly
between two texels of an even-sized screen, and the margin costs 14 % twice, once for the object frames and once for the background)."""
import ctypes

import numpy as np
import pytest
import torch

import decode_cases
import decode_ref
from conftest import data_path
from drt_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 96          # sentinel elements on both sides of every output
CASES = decode_cases.gpu_cases()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _offset(a, k):
    """The array on the device as a view that starts k bytes into a larger buffer."""
    flat = torch.tensor(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device="cuda")
    view = buf[k:k + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 8 == k % 8
    return buf, view.view(a.shape)


def abi_decode(case, want=("mask", "covered", "positions"), frames_offset=0, background_offset=0):
    """drt_decode_patterns on a case; every output lies between guard bands, which must stay intact.  dict of numpy arrays (None: not asked for)."""
    lib = _lib.lib()
    frames, bg, scr = case["frames"], case["background"], case["screens"]
    n, F, H, W = frames.shape
    keep, d_frames = _offset(frames, frames_offset)
    keep_bg, d_bg = _offset(bg, background_offset) if bg is not None else (None, None)
    d_scr = torch.tensor(scr, device="cuda") if scr is not None else None
    spec = dict(codes=((n, H, W, 2), torch.int16, 77), contrast=((n, H, W), torch.uint8, 77), mask=((n, H, W), torch.uint8, 77),
                covered=((n, H, W), torch.uint8, 77), positions=((n, H * W, 3), torch.float64, float("nan")))
    bufs, outs = {}, {}
    for key, (shape, dtype, fill) in spec.items():
        asked = key in ("codes", "contrast") or (key in want and (scr is not None if key == "positions" else bg is not None))
        bufs[key], outs[key] = _guarded(shape, dtype, fill) if asked else (None, None)
    zero = int(case["zero"] and outs["positions"] is not None)
    stride = 0 if bg is None or bg.ndim == 3 else F * H * W
    _lib.check(lib.drt_decode_patterns(d_frames.data_ptr(), _lib.ptr(d_bg), stride, n, H, W, case["tex_h"], case["tex_w"], case["min_contrast"],
                                       case["mask_shift"], _lib.ptr(d_scr) if outs["positions"] is not None else None, zero, outs["codes"].data_ptr(),
                                       outs["contrast"].data_ptr(), _lib.ptr(outs["mask"]), _lib.ptr(outs["covered"]), _lib.ptr(outs["positions"]), _stream()))
    torch.cuda.synchronize()
    for key, buf in bufs.items():
        if buf is None:
            continue
        band = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert bool(torch.isnan(band).all()) if key == "positions" else bool((band == 77).all()), f"guard band of {key}"
    return {k: None if v is None else v.cpu().numpy() for k, v in outs.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equal_outputs(got, expect):
    for key in ("codes", "contrast", "mask", "covered", "positions"):
        if got[key] is not None:
            assert expect[key] is not None and same_bits(got[key], expect[key]), key


@pytest.mark.parametrize("name,make", CASES, ids=[n for n, _ in CASES])
def test_kernel_equals_the_restatement(name, make):
    case = make()
    got = abi_decode(case)
    assert_equal_outputs(got, case["expect"])
    assert (got["mask"] is None) == (case["background"] is None) and (got["positions"] is None) == (case["screens"] is None)


@pytest.mark.parametrize("frames_offset,background_offset", [(0, 1), (3, 0), (5, 6), (4, 4)])
@pytest.mark.parametrize("index", [4, 13, 19])          # 32 x 20 and 17 x 23 planes, shared and per-view backgrounds
def test_stacks_at_odd_byte_offsets(index, frames_offset, background_offset):
    case = decode_cases.grid_case(index)
    assert case["background"] is not None
    assert_equal_outputs(abi_decode(case, frames_offset=frames_offset, background_offset=background_offset), case["expect"])


def test_two_runs_give_the_same_bits():
    case = decode_cases.big_case(3, 1031)
    a, b = abi_decode(case), abi_decode(case)
    for key in a:
        assert same_bits(a[key], b[key]), key


@pytest.mark.parametrize("want", [(), ("mask",), ("covered",), ("positions",), ("mask", "positions")])
def test_outputs_not_asked_for_change_nothing_in_the_others(want):
    case = decode_cases.big_case(64, 48)
    got = abi_decode(case, want=want)
    assert {k for k in ("mask", "covered", "positions") if got[k] is not None} == set(want)
    assert_equal_outputs(got, case["expect"])


def test_python_layer_equals_the_abi_view_by_view_and_resident():
    from drt_amd import structured_light
    for case in (decode_cases.grid_case(14), decode_cases.grid_case(3), decode_cases.grid_case(12)):
        e = case["expect"]
        targets = None if case["background"] is None else ("object" if case["zero"] else "all")
        kw = dict(tex_h=case["tex_h"], tex_w=case["tex_w"], screens=case["screens"], min_contrast=case["min_contrast"], mask_shift=case["mask_shift"],
                  targets=targets)
        host = structured_light.decode(case["frames"], background=case["background"], **kw)                         # numpy: view by view
        dev = structured_light.decode(torch.tensor(case["frames"], device="cuda"),
                                      background=None if case["background"] is None else torch.tensor(case["background"], device="cuda"), **kw)
        for r in (host, dev):
            got = {k: None if v is None else v.cpu().numpy() for k, v in r._asdict().items()}
            assert_equal_outputs(got, e)
            assert (got["mask"] is None) == (e["mask"] is None) and (got["positions"] is None) == (e["positions"] is None)
    one = structured_light.decode(case["frames"][0], case["tex_h"], case["tex_w"], min_contrast=case["min_contrast"])         # one view, no stack axis
    assert one.codes.shape[0] == 1 and np.array_equal(one.codes[0].cpu().numpy(), e["codes"][0]) and one.mask is None and one.positions is None


def test_abi_argument_checks():
    lib = _lib.lib()
    fr = torch.zeros((2, 8, 4, 5), dtype=torch.uint8, device="cuda")
    bg = torch.zeros((8, 4, 5), dtype=torch.uint8, device="cuda")
    scr = torch.zeros((2, 9), dtype=torch.float64, device="cuda")
    codes = torch.full((2, 4, 5, 2), 77, dtype=torch.int16, device="cuda")
    u8 = [torch.full((2, 4, 5), 77, dtype=torch.uint8, device="cuda") for _ in range(3)]
    pos = torch.full((2, 20, 3), 7.0, dtype=torch.float64, device="cuda")

    def call(**kw):
        a = dict(frames=fr.data_ptr(), bg=bg.data_ptr(), stride=0, n=2, H=4, W=5, tex_h=4, tex_w=4, mc=16, ms=1, scr=scr.data_ptr(), zero=1,
                 codes=codes.data_ptr(), contrast=u8[0].data_ptr(), mask=u8[1].data_ptr(), covered=u8[2].data_ptr(), pos=pos.data_ptr())
        a.update(kw)
        return lib.drt_decode_patterns(*a.values(), _stream())

    def rejected(rc, word):
        assert rc == -1, (rc, word)
        assert word in lib.drt_last_error().decode(), (word, lib.drt_last_error())

    rejected(call(frames=None), "d_frames")
    rejected(call(n=0), "n_views")
    rejected(call(H=0), "height")
    rejected(call(tex_h=1), "tex_h")
    rejected(call(tex_w=32769), "tex_w")
    rejected(call(mc=0), "min_contrast")
    rejected(call(mc=256), "min_contrast")
    rejected(call(ms=0), "mask_shift")
    rejected(call(zero=2), "zero_outside_mask")
    rejected(call(stride=100), "background_view_stride")
    rejected(call(bg=None), "d_background")
    rejected(call(bg=None, mask=None, covered=None), "zero_outside_mask")
    rejected(call(scr=None), "d_screens")
    rejected(call(pos=None), "d_positions")
    rejected(call(codes=None), "d_codes")
    rejected(call(contrast=None), "d_contrast")
    rejected(call(codes=codes.data_ptr() + 1), "d_codes")
    rejected(call(pos=pos.data_ptr() + 4), "d_positions")
    torch.cuda.synchronize()
    assert bool((codes == 77).all()) and all(bool((t == 77).all()) for t in u8) and bool((pos == 7.0).all())          # a refused call touches nothing
    assert call() == 0 and call(tex_h=3, tex_w=3, bg=None, mask=None, covered=None, zero=0) == 0
    torch.cuda.synchronize()
    assert lib.drt_version() == 13


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    from drt_amd import diffrender as Render, views
    gt = Render.Scene(data_path("hand_vh.ply"), 0)
    center, extent = views.mesh_frame(gt.mesh.vertices)
    return gt, center, extent


def _truth(gt, cam, screen, res, tex):
    """What tests/decode_cases.nearest_texel_check takes, from Scene.render_paths: the exit ray's screen coordinates by the renderer's law."""
    from drt_amd import views
    o, d = views.generate_ray(res, res, cam[3], cam[2], device="cuda")
    with torch.no_grad():
        out_ori, out_dir, m = gt.render_paths(o, d, 2, "drop")
        hit = gt.render_mask(o, d) > 0
    p0, eu, ev = (torch.as_tensor(a, device="cuda") for a in (screen.p0, screen.eu, screen.ev))
    nrm = torch.linalg.cross(eu, ev)
    dn = out_dir @ nrm
    t = ((p0 - out_ori) @ nrm) / dn
    q = out_ori + t[:, None] * out_dir
    u, v = ((q - p0) @ eu) / (eu @ eu), ((q - p0) @ ev) / (ev @ ev)
    valid = m[:, 0].bool() & (dn != 0) & (t > 0) & (u >= 0) & (u <= tex - 1) & (v >= 0) & (v <= tex - 1)
    return dict(valid=valid.cpu().numpy(), u=u.cpu().numpy(), v=v.cpu().numpy(), hit=hit.cpu().numpy().reshape(-1), target=q.cpu().numpy())


def test_end_to_end_synthetic_frames_decode_to_the_traced_targets(hand):
    from drt_amd import render, structured_light, views
    gt, center, extent = hand
    E = decode_cases.E2E
    res, tex = E["res"], E["tex"]
    cam = views.turntable_cameras(center, extent, E["n_turntable"], res, res, distance_factor=E["distance_factor"])[E["view"]]
    screen = render.Screen.behind(cam, center, extent, tex, tex)
    frames, background = structured_light.synthetic_frames(gt, cam, res, res, screen, tex, tex)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == tuple(background.shape) == (structured_light.n_frames(tex, tex), res, res)
    r = structured_light.decode(frames, tex, tex, screens=screen, background=background, min_contrast=E["min_contrast"], targets="all")
    expect = decode_ref.decode(frames.cpu().numpy()[None], tex, tex, screen.packed()[None], background.cpu().numpy(), E["min_contrast"], 1, False)
    assert_equal_outputs({k: v.cpu().numpy() for k, v in r._asdict().items()}, expect)
    truth = _truth(gt, cam, screen, res, tex)
    excluded, checked = decode_cases.nearest_texel_check(truth, expect["codes"][0], expect["positions"][0], screen.packed(), E["min_contrast"])
    print(f"valid {truth['valid'].sum()}, checked {checked}, excluded by the margin {100 * excluded:.1f} %")
    assert excluded <= 0.25
    mask, hit = expect["mask"][0].reshape(-1) != 0, truth["hit"]
    assert not (mask & ~hit).any()                              # a direct pixel's frames equal its background frames
    print(f"hit {hit.sum()}, missed by the mask {(hit & ~mask).sum()}")
    obj = structured_light.decode(frames, tex, tex, screens=screen, background=background, min_contrast=E["min_contrast"])       # targets: "object"
    inside = torch.as_tensor(mask, device="cuda")
    assert torch.equal(obj.positions[0], torch.where(inside[:, None], r.positions[0], torch.zeros_like(r.positions[0])))


def test_pattern_data_agrees_with_synthetic_data(hand):
    from drt_amd import captured_data, render, structured_light, views
    gt, center, extent = hand
    res, tex, n, min_contrast = 64, 128, 4, 4
    ids = [0, 1]
    cams = views.turntable_cameras(center, extent, n, res, res)
    screens = [render.Screen.behind(cams[k], center, extent, tex, tex) for k in ids]
    shots = [structured_light.synthetic_frames(gt, cams[k], res, res, screens[i], tex, tex) for i, k in enumerate(ids)]
    data = structured_light.PatternData([cams[k] for k in ids], screens, torch.stack([s[0] for s in shots]), tex, tex, torch.stack([s[1] for s in shots]),
                                        res, res, min_contrast=min_contrast)
    ref = captured_data.SyntheticData(gt, center, extent, res, res, num_view=n, n_total=n, view_ids=ids, path_law=(2, "drop"))
    assert isinstance(data, captured_data.Data) and data.n_total == 2 and sorted(data.ray_view_ids()) == [0, 1]
    for i, k in enumerate(ids):
        sp, valid, soft, origin, ray_dir, camera_M = data.get_view(i)
        sp_r, valid_r, soft_r, origin_r, ray_dir_r, camera_r = ref.get_view(k)
        assert sp.shape == sp_r.shape and sp.dtype == sp_r.dtype and valid.dtype == torch.bool and soft.shape == soft_r.shape and soft.dtype == soft_r.dtype
        assert torch.equal(origin, origin_r) and torch.equal(ray_dir, ray_dir_r) and all(torch.equal(a, b) for a, b in zip(camera_M, camera_r))
        assert torch.equal(valid, sp[:, 0] != 0) and float(soft.min()) >= 0.0 and float(soft.max()) <= 1.0
        both = valid & valid_r
        s9 = screens[i].packed()
        bound = 0.5 * float(np.sqrt((s9[3:6] ** 2).sum() + (s9[6:9] ** 2).sum())) + 1e-9
        worst = float((sp[both] - sp_r[both]).norm(dim=1).max())
        share = float(both.sum()) / float(valid_r.sum())
        print(f"view {k}: {int(valid_r.sum())} valid in SyntheticData, {int(both.sum())} in both ({100 * share:.1f} %), worst distance {worst:.4f} of {bound:.4f}")
        assert worst <= bound
        assert share >= 0.75
        assert not bool(((soft > 0.75) & ~(soft_r > 0.75)).any())              # the mask never leaves the silhouette


def test_existing_loss_runs_on_a_pattern_view(hand):
    """The standard tuple feeds the ray loss as a capture's does."""
    from drt_amd import render, structured_light, views
    gt, center, extent = hand
    res, tex = 32, 64
    cam = views.turntable_cameras(center, extent, 4, res, res)[0]
    screen = render.Screen.behind(cam, center, extent, tex, tex)
    frames, background = structured_light.synthetic_frames(gt, cam, res, res, screen, tex, tex)
    data = structured_light.PatternData([cam], [screen], frames, tex, tex, background, res, res, min_contrast=4)
    sp, valid, _, origin, ray_dir, _ = data.get_view(0)
    with torch.no_grad():
        out_ori, out_dir, m = gt.render_transparent(origin, ray_dir)
    ok = valid & m[:, 0].bool()
    assert int(ok.sum()) > 10
    toward = sp[ok] - out_ori[ok]
    miss = torch.linalg.cross(toward, out_dir[ok]).norm(dim=1)                 # distance of the target from the true exit ray
    s9 = screen.packed()
    assert float(miss.max()) <= 0.5 * float(np.sqrt((s9[3:6] ** 2).sum() + (s9[6:9] ** 2).sum())) + 1e-9


def test_capture_arrays_round_trip_through_a_capture_file(tmp_path):
    from drt_amd import captured_data, structured_light, views
    cls = captured_data.CAMERAS["redmi"]
    H, W, tex = cls.resy, cls.resx, 4
    pat = structured_light.gray_patterns(tex, tex)
    yy, xx = np.meshgrid(np.arange(H) * tex // H, np.arange(W) * tex // W, indexing="ij")
    background = np.ascontiguousarray(pat[:, yy, xx])
    shifted = np.ascontiguousarray(pat[:, yy, (xx + 1) % tex])
    frames = np.stack([background.copy(), background.copy()])
    frames[0, :, 300:700, 500:900] = shifted[:, 300:700, 500:900]
    frames[1, :, 100:200, 100:1500] = 0                                     # no light comes through: in the mask, without a target
    cams = views.turntable_cameras(np.zeros(3), 1.0, 2, W, H)
    screens = np.array([[1.0, 2.0, 3.0, 0.5, 0, 0, 0, 0.5, 0]] * 2)
    arrays = structured_light.capture_arrays(cams, screens, frames, tex, tex, background, camera="redmi")
    assert set(arrays) == {"cam_proj", "cam_k", "screen_position", "mask"}
    assert arrays["cam_proj"].shape == (2, 4, 4) and arrays["cam_k"].shape == (3, 3) and arrays["mask"].shape == (2, H, W) and arrays["mask"].dtype == np.uint8
    assert arrays["screen_position"].shape == (2, H, W, 3) and arrays["screen_position"].dtype == np.float64
    assert int((arrays["mask"][0] != 0).sum()) == 400 * 400 and int((arrays["mask"][1] != 0).sum()) == 100 * 1400
    assert int((arrays["screen_position"][0, ..., 0] != 0).sum()) == 400 * 400 and int((arrays["screen_position"][1, ..., 0] != 0).sum()) == 0
    path = str(tmp_path / "horse.npz")
    captured_data.write_capture(path, arrays)
    data = captured_data.get_data(dict(name="horse", num_view=2), path=path, device="cuda", rng=np.random.RandomState(0), pin=False)
    sp, valid, soft, origin, ray_dir, camera_M = data.get_view(0)
    assert data.n_total == 2 and int(valid.sum()) == 400 * 400 and tuple(sp.shape) == (H * W, 3)
    assert np.array_equal(sp.cpu().numpy().reshape(H, W, 3), arrays["screen_position"][0])
    assert float(soft.view(H, W)[500, 700]) == 1.0 and float(soft.view(H, W)[10, 10]) == 0.0
