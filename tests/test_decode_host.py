"""CPU: the pattern-decoding law of drt_amd/csrc/drt_decode.h, compiled for the host by g++ with -ffp-contract=off
(tests/hostsim/decode.cpp), against the numpy restatement tests/decode_ref.py.

Tolerance 0, derived and not measured: codes, contrast, mask and covered are integer arithmetic; the position is (p0 + x eu) + y ev, two
multiplications and two additions per component, each correctly rounded in the stated association on both sides (contraction is off,
numpy's elementwise float64 arithmetic does not fuse).  A difference is a bug in the header or a restatement that reorders.

End to end on the CPU (tests/image_ref.py + the oracle's tracer; DESIGN.md 10.12 quotes the figures): the hand in front of a 64 x 64
screen, 24 x 24 pixels.  Also here: the argument errors of drt_amd.structured_light that need no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import decode_cases
import decode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

E2E_MASK_MISSED = 32        # hit pixels of the end-to-end case the mask misses, by the restatement, of E2E_HIT
E2E_HIT = 130


@pytest.fixture(scope="module")
def hs():
    src = os.path.join(ROOT, "tests", "hostsim", "decode.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libdecode.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(csrc, "drt_decode.h"), os.path.join(csrc, "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.decode_n_frames.argtypes = [_I, _I]
    lib.decode_patterns.argtypes = [_I, _I, _P]
    lib.decode_host.argtypes = [_P, _P, _I64, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P]
    return lib


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def host_decode(hs, case, want=("mask", "covered", "positions")):
    frames, bg, scr = case["frames"], case["background"], case["screens"]
    n, F, H, W = frames.shape
    out = dict(codes=np.full((n, H, W, 2), 77, np.int16), contrast=np.full((n, H, W), 77, np.uint8),
               mask=np.full((n, H, W), 77, np.uint8) if bg is not None and "mask" in want else None,
               covered=np.full((n, H, W), 77, np.uint8) if bg is not None and "covered" in want else None,
               positions=np.full((n, H * W, 3), np.nan) if scr is not None and "positions" in want else None)
    stride = 0 if bg is None or bg.ndim == 3 else F * H * W
    hs.decode_host(_p(frames), _p(bg), stride, n, H, W, case["tex_h"], case["tex_w"], case["min_contrast"], case["mask_shift"], _p(scr), int(case["zero"]),
                   _p(out["codes"]), _p(out["contrast"]), _p(out["mask"]), _p(out["covered"]), _p(out["positions"]))
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equal_outputs(got, expect):
    for key in ("codes", "contrast", "mask", "covered", "positions"):
        if got[key] is None:
            continue
        assert expect[key] is not None and same_bits(got[key], expect[key]), key


@pytest.mark.parametrize("name,make", decode_cases.host_cases(), ids=[n for n, _ in decode_cases.host_cases()])
def test_host_header_equals_the_restatement(hs, name, make):
    case = make()
    got = host_decode(hs, case)
    assert_equal_outputs(got, case["expect"])
    assert (got["mask"] is None) == (case["background"] is None) and (got["positions"] is None) == (case["screens"] is None)


def test_header_outputs_cover_what_the_cases_are_for(hs):
    """The header's own outputs on the grid cases show every branch of the law: both verdicts of the contrast test, codes beyond a
    non-power-of-two texture, both mask values, every background form."""
    cases = [decode_cases.grid_case(i) for i in range(20)]
    cases = [dict(c, expect=host_decode(hs, c)) for c in cases]
    assert {c["min_contrast"] for c in cases} == {1, 16, 255} and {c["mask_shift"] for c in cases} == {1, 3}
    assert {None if c["background"] is None else c["background"].ndim for c in cases} == {None, 3, 4}
    assert any(c["screens"] is None for c in cases) and any(c["zero"] for c in cases)
    assert any((c["frames"].shape[2] * c["frames"].shape[3]) % 2 for c in cases)
    for c in cases:
        e = c["expect"]
        ok = e["codes"][..., 0] >= 0
        assert ((e["codes"][..., 0] < c["tex_w"]) & (e["codes"][..., 1] < c["tex_h"])).all() and (ok == (e["codes"][..., 1] >= 0)).all()
        if c["frames"].shape[2] * c["frames"].shape[3] >= 35:
            assert ok.any() and not ok.all()
            if e["mask"] is not None:
                assert (e["mask"] == 255).any() and (e["mask"] == 0).any() and set(np.unique(e["mask"])) <= {0, 255}
    beyond = [c for c in cases if (c["tex_w"], c["tex_h"]) == (5, 3)]
    assert beyond and all((c["expect"]["contrast"][c["expect"]["codes"][..., 0] < 0] >= c["min_contrast"]).any() for c in beyond if c["frames"][0, 0].size >= 35)


def test_position_with_x_exactly_zero_is_nudged(hs):
    case = decode_cases.zero_x_case()
    got = host_decode(hs, case)
    assert_equal_outputs(got, case["expect"])
    first = got["positions"][:, 0]
    assert (got["codes"][:, 0, 0] == (3, 1)).all() and (first[:, 0] == 1e-12).all() and (first[:, 1] == 0.75).all()
    assert (got["positions"][..., 0] != 0).sum() == (got["codes"][..., 0] >= 0).sum()


@pytest.mark.parametrize("tex_w,tex_h", decode_cases.TEXTURES)
def test_pattern_round_trip(hs, tex_w, tex_h):
    from drt_amd import structured_light
    pat = structured_light.gray_patterns(tex_h, tex_w)
    F = structured_light.n_frames(tex_h, tex_w)
    assert pat.shape == (F, tex_h, tex_w) and pat.dtype == np.uint8 and F == decode_ref.n_frames(tex_h, tex_w) == hs.decode_n_frames(tex_h, tex_w) <= 60
    assert set(np.unique(pat)) == {0, 255} and np.array_equal(pat, decode_ref.patterns(tex_h, tex_w))
    header = np.empty_like(pat)
    hs.decode_patterns(tex_h, tex_w, _p(header))
    assert np.array_equal(header, pat)
    yy, xx = np.meshgrid(np.arange(tex_h), np.arange(tex_w), indexing="ij")
    case = dict(frames=np.ascontiguousarray(pat[None]), background=None, screens=None, tex_h=tex_h, tex_w=tex_w, min_contrast=255, mask_shift=1, zero=False)
    for codes in (host_decode(hs, case)["codes"], decode_ref.decode(case["frames"], tex_h, tex_w, min_contrast=255)["codes"]):
        assert np.array_equal(codes[0, :, :, 0], xx) and np.array_equal(codes[0, :, :, 1], yy)


def test_end_to_end_on_the_cpu(hs):
    case = decode_cases.hand_e2e()
    truth, e = case["truth"], case["expect"]
    assert_equal_outputs(host_decode(hs, case), e)
    excluded, checked = decode_cases.nearest_texel_check(truth, e["codes"][0], e["positions"][0], case["screens"][0], case["min_contrast"])
    print(f"valid {truth['valid'].sum()}, checked {checked}, excluded by the margin {100 * excluded:.1f} %")
    assert excluded <= 0.25
    mask, hit = e["mask"][0].reshape(-1) != 0, truth["hit"]
    assert not (mask & ~hit).any()                       # exact: a direct pixel's frames equal its background frames
    missed = int((hit & ~mask).sum())
    print(f"hit {hit.sum()}, missed by the mask {missed}")
    assert int(hit.sum()) == E2E_HIT and abs(missed - E2E_MASK_MISSED) <= 1


# ---- the Python layer's argument errors that need no GPU ----------------------------------------------------------------------------
def _args():
    return dict(frames=np.zeros((2, 8, 4, 5), np.uint8), tex_h=4, tex_w=4)


@pytest.mark.parametrize("key,value", [
    ("frames", np.zeros((2, 8, 4, 5), np.float32)), ("frames", np.zeros((4, 5), np.uint8)), ("frames", np.zeros((2, 6, 4, 5), np.uint8)),
    ("frames", np.zeros((2, 8, 0, 5), np.uint8)), ("tex_h", 1), ("tex_w", 32769), ("tex_w", 4.0),
    ("background", np.zeros((8, 4, 6), np.uint8)), ("background", np.zeros((3, 8, 4, 5), np.uint8)), ("background", np.zeros((8, 4, 5), np.int8)),
    ("screens", np.zeros((3, 9))), ("screens", np.zeros((2, 8))), ("screens", np.full((2, 9), np.nan)), ("screens", "left"),
    ("min_contrast", 0), ("min_contrast", 256), ("min_contrast", 16.0), ("mask_shift", 0), ("targets", "mask"), ("targets", "object")])
def test_decode_names_the_bad_argument(key, value):
    from drt_amd import structured_light
    kw = dict(_args(), **{key: value})
    with pytest.raises(ValueError, match=key):
        structured_light.decode(**kw)


def test_frame_count_error_says_what_the_texture_needs():
    from drt_amd import structured_light
    with pytest.raises(ValueError, match="n_frames = 8"):
        structured_light.decode(np.zeros((10, 4, 5), np.uint8), 4, 4)


@pytest.mark.parametrize("kw,key", [(dict(camera="nikon"), "camera"), (dict(frames=np.zeros((1, 8, 4, 5), np.uint8), background=np.zeros((8, 4, 5), np.uint8)), "camera"),
                                    (dict(background=None), "background"), (dict(screens=None), "screens"), (dict(cameras=[]), "cameras"),
                                    (dict(min_contrast=0), "min_contrast"), (dict(tex_w=1), "tex_w")])
def test_capture_arrays_names_the_bad_argument(kw, key):
    from drt_amd import captured_data, structured_light
    cls = captured_data.CAMERAS["redmi"]
    frames = np.broadcast_to(np.zeros((), np.uint8), (1, 8, cls.resy, cls.resx))            # no memory: the checks run before anything reads it
    cam = (np.eye(4), np.eye(3), np.eye(4), np.eye(3))
    args = dict(cameras=[cam], screens=np.ones((1, 9)), frames=frames, tex_h=4, tex_w=4, background=frames[0], camera="redmi")
    args.update(kw)
    with pytest.raises(ValueError, match=key):
        structured_light.capture_arrays(**args)


def test_capture_arrays_wants_one_k():
    from drt_amd import captured_data, structured_light
    cls = captured_data.CAMERAS["redmi"]
    frames = np.broadcast_to(np.zeros((), np.uint8), (2, 8, cls.resy, cls.resx))
    cams = [(np.eye(4), np.eye(3), np.eye(4), np.eye(3)), (np.eye(4), 2 * np.eye(3), np.eye(4), 0.5 * np.eye(3))]
    with pytest.raises(ValueError, match="cam_k"):
        structured_light.capture_arrays(cams, np.ones((1, 9)), frames, 4, 4, frames[0])


def test_cli_refuses_to_overwrite(tmp_path):
    from drt_amd import structured_light
    existing = tmp_path / "x.h5"
    existing.write_text("capture")
    with pytest.raises(SystemExit, match="--force"):
        structured_light.main(["--frames", str(tmp_path / "raw.npz"), "-o", str(existing)])
    assert existing.read_text() == "capture"


def test_unit_symbol_and_version():
    from drt_amd import _lib, build
    assert "drt_decode.hip" in build.UNITS
    assert "drt_decode_patterns" in _lib.SIGNATURES and len(_lib.SIGNATURES["drt_decode_patterns"][1]) == 18
    exports = open(os.path.join(ROOT, "drt_amd", "csrc", "exports.map")).read()
    assert "drt_*" in exports                                   # the map exports the C ABI by prefix: the new symbol leaves the library
    build.build()
    h = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(h, "drt_decode_patterns")
    assert _lib.lib().drt_version() == 13
