"""CPU: the visual-hull law of drt_amd/csrc/drt_hull.h, compiled for the host by g++ with -ffp-contract=off (tests/hostsim/hull.cpp),
against the numpy restatement tests/hull_ref.py on whole small grids.

Tolerance 0, derived and not measured: both sides perform the same correctly rounded IEEE-754 operations in the same order (the law
fixes the association of every expression, contraction is off on both sides, numpy's elementwise float64 arithmetic does not fuse).
A difference is a bug in the header or a restatement that reorders.  Also here: the argument errors of drt_amd.visual_hull that need
no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hull_cases
import hull_ref
from oracle import remesh_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I, _F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def hs():
    src = os.path.join(ROOT, "tests", "hostsim", "hull.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libhull.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(csrc, "drt_hull.h"), os.path.join(csrc, "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hull_field.argtypes = [_P, _I, _I, _I, _P, _P, _D, _P, _I, _P]
    lib.hull_mark.argtypes = [_P, _P, _F, _P, _P, _P, _P]
    lib.hull_emit.argtypes = [_P, _P, _P, _D, _F, _P, _P, _P, _I64, _I64, _P, _P]
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def host_hull(hs, case):
    masks, P, lo = np.ascontiguousarray(case["masks"]), np.ascontiguousarray(case["P"]), np.ascontiguousarray(case["lo"])
    dims = np.asarray(case["dims"], np.int32)
    n, H, W = masks.shape
    N = int(np.prod(case["dims"]))
    field = np.empty(case["dims"], np.float32)
    hs.hull_field(_p(masks), n, H, W, _p(P), _p(lo), case["h"], _p(dims), int(case["outside"] == "keep"), _p(field))
    emask, v_inc, t_inc, totals = np.empty(N, np.uint8), np.empty(N, np.int32), np.empty(N, np.int32), np.zeros(2, np.int64)
    hs.hull_mark(_p(field), _p(dims), case["level"], _p(emask), _p(v_inc), _p(t_inc), _p(totals))
    V, F = np.full((int(totals[0]), 3), np.nan), np.full((int(totals[1]), 3), -1, np.int32)
    hs.hull_emit(_p(field), _p(dims), _p(lo), case["h"], case["level"], _p(emask), _p(v_inc), _p(t_inc), len(V), len(F), _p(V), _p(F))
    return field, V, F


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,make", hull_cases.host_cases(), ids=[n for n, _ in hull_cases.host_cases()])
def test_host_header_equals_the_restatement(hs, name, make):
    case = make()
    field, V, F = host_hull(hs, case)
    assert np.array_equal(field, case["field"])
    assert len(case["F"]) > 0 and np.array_equal(F, case["F"]) and F.dtype == np.int32
    assert same_bits(V, case["V"])
    topo = remesh_oracle.topology(V, F)
    assert topo["ok"], {k: v for k, v in topo.items() if v is False}
    assert remesh_oracle.signed_volume(V, F) > 0


def test_restatement_table_free_orientation_follows_parity():
    """The restatement orients every case geometrically; the header's table is one case list mirrored by the permutation's parity."""
    odd = [0, 1, 1, 0, 0, 1]
    for case in range(1, 15):
        flags = tuple(bool((case >> p) & 1) for p in range(4))
        even = hull_ref.tet_triangles(0, flags)
        for t in range(6):
            assert hull_ref.tet_triangles(t, flags) == (even if not odd[t] else [[a, c, b] for a, b, c in even])


def test_corner_on_the_level_is_outside_and_its_edges_are_clamped(hs):
    case = hull_cases.affine()
    f, lo, h = case["field"], case["lo"], case["h"]
    assert set(np.unique(f).tolist()) == {0.0, 0.25, 0.5, 1.0}
    on = np.argwhere(f == np.float32(0.5))
    assert len(on) > 0, "the input must put a corner exactly on the level"
    _, V, F = host_hull(hs, case)
    inside = f > np.float32(0.5)
    assert not inside[tuple(on.T)].any()
    # every lattice edge from an on-level corner to an inside one carries a vertex at the clamp: s = 2^-10 when the on-level corner is the
    # lower end, 1 - 2^-10 when it is the upper one -- never at the corner itself
    rows = {tuple(r) for r in V.tolist()}
    found = 0
    for c in on:
        for code in range(1, 8):
            off = hull_ref.code_offset(code)
            for sign, s in ((1, hull_ref.S_MIN), (-1, 1.0 - hull_ref.S_MIN)):
                nb = c + sign * off
                if (nb < 0).any() or (nb >= np.array(f.shape)).any() or not inside[tuple(nb)]:
                    continue
                low = c if sign == 1 else nb
                assert tuple((lo + h * (low.astype(np.float64) + s * off.astype(np.float64))).tolist()) in rows
                found += 1
    assert found > 0
    corners = {tuple(r) for r in (lo + h * on.astype(np.float64)).tolist()}
    assert not (rows & corners)


def test_camera_inside_the_box_has_corners_behind_it():
    carve, keep = hull_cases.camera_inside("carve"), hull_cases.camera_inside("keep")
    P0, lo, h = carve["P"][0], carve["lo"], carve["h"]
    i, j, k = np.meshgrid(*[np.arange(n) for n in carve["dims"]], indexing="ij")
    hz = ((P0[2, 0] * (lo[0] + h * i) + P0[2, 1] * (lo[1] + h * j)) + P0[2, 2] * (lo[2] + h * k)) + P0[2, 3]
    behind = hz <= 0
    assert behind.any() and (~behind).any()
    assert (carve["field"][behind] == 0).all()                # carve: a view that does not see the corner cuts it away
    assert (keep["field"][behind] > 0).any()                  # keep: that view is skipped
    assert not np.array_equal(carve["field"], keep["field"])


# ---- the Python layer's argument errors that need no GPU ----------------------------------------------------------------------------
def _args():
    return dict(masks=np.ones((2, 8, 8), np.uint8), P=np.zeros((2, 3, 4)), lo=np.zeros(3), cell=1.0, dims=(5, 5, 5))


@pytest.mark.parametrize("key,value", [("masks", np.ones((2, 8, 8), np.float32)), ("masks", np.ones((8, 8), np.uint8)), ("masks", np.ones((2, 1, 8), np.uint8)),
                                       ("P", np.zeros((3, 3, 4))), ("P", np.zeros((2, 4, 4))), ("lo", np.zeros(2)), ("lo", np.array([0.0, np.nan, 0.0])),
                                       ("cell", 0.0), ("cell", float("inf")), ("dims", (5, 5)), ("dims", (2, 5, 5)), ("dims", (5, 1025, 5)), ("outside", "drop")])
def test_silhouette_field_names_the_bad_argument(key, value):
    from drt_amd import visual_hull
    kw = dict(_args(), **{key: value})
    with pytest.raises(ValueError, match=key):
        visual_hull.silhouette_field(**kw)


@pytest.mark.parametrize("kw,key", [(dict(level=0.0), "level"), (dict(level=1.0), "level"), (dict(cell=-1.0), "cell"), (dict(lo=np.zeros(4)), "lo"),
                                    (dict(field=np.zeros((5, 5), np.float32)), "field"), (dict(field=np.zeros((5, 5, 5), np.float64)), "field")])
def test_extract_surface_names_the_bad_argument(kw, key):
    from drt_amd import visual_hull
    args = dict(field=np.zeros((5, 5, 5), np.float32), lo=np.zeros(3), cell=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=key):
        visual_hull.extract_surface(**args)


@pytest.mark.parametrize("kw,key", [(dict(resolution=2), "resolution"), (dict(resolution=2000), "resolution"), (dict(level=1.5), "level"),
                                    (dict(target_len=0.0), "target_len"), (dict(keep="biggest"), "keep"), (dict(outside="drop"), "outside"),
                                    (dict(bounds=(np.zeros(3), np.zeros(3))), "bounds"), (dict(view_ids=[]), "view_ids")])
def test_visual_hull_names_the_bad_keyword(kw, key):
    from drt_amd import visual_hull
    with pytest.raises(ValueError, match=key):
        visual_hull.visual_hull(object(), **kw)


def test_cli_refuses_to_overwrite_and_never_defaults_to_a_shipped_hull(tmp_path):
    from drt_amd import visual_hull
    assert not os.path.basename(visual_hull.default_output("horse", "./data/")).endswith("_vh.ply")
    existing = tmp_path / "x.ply"
    existing.write_text("ply")
    with pytest.raises(SystemExit, match="--force"):
        visual_hull.main(["--name", "hand", "-o", str(existing)])
    assert existing.read_text() == "ply"
