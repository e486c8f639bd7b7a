"""CPU: the environment law of drt_amd/csrc/drt_image_env.h, compiled for the host by g++ with -ffp-contract=off
(tests/hostsim/image_env.cpp), against the restatement tests/image_env_ref.py, and the Python layer's checks that need no GPU.

What is held to tolerance 0: everything that contains no acos / atan2 -- the direction in the environment frame, the cell, the wrapped
bilinear fetch at a given (u, v), a sample's colour where the screen catches it.  (u, v) themselves: within image_env_ref.UV_ULPS
(Ew * 2^-50, Eh * 2^-50; derived there), and a colour taken from the environment within G_env times that many texels."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_ref
import image_ref
from drt_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
EH, EW = image_env_cases.EH, image_env_cases.EW


def load_hs():
    """The host build of this file, compiled when a source of it is newer, with its signatures."""
    src = os.path.join(ROOT, "tests", "hostsim", "image_env.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libimage_env.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("drt_image_env.h", "drt_image_loss.h", "drt_image.h", "drt_paths.h", "drt_path.h", "drt_shade.h",
                                                    "drt_traverse.h", "drt_common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.env_rot_ok.argtypes = [_P]
    lib.env_uv.argtypes = [_P, _I, _I, _P, _I64, _P, _P]
    lib.env_fetch.argtypes = [_P, _I, _I, _I, _P, _I64, _P, _P]
    lib.env_colours.argtypes = [_P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I64, _P, _P, _P]
    lib.env_reflect.argtypes = [_P, _P, _I, _P, _I, _I, _I, ctypes.c_double, ctypes.c_double, _I, _P, _P, _P, _P, _P]
    lib.env_add_reflection.argtypes = [_P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I64, _P]
    lib.env_lookup_backward.argtypes = [_P, _I, _I, _I, _P, _P, _P, _I64, _P]
    lib.env_clear_colours.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I64, _P, _P, _P]
    lib.env_loss_view.restype = ctypes.c_double
    lib.env_loss_view.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, ctypes.c_double, ctypes.c_double, _I, _I] + [_P] * 11
    return lib


@pytest.fixture(scope="module")
def hs():
    return load_hs()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _directions(rng, R, n=400):
    """Unit directions: random ones, ones next to the wrap seam (phi = +-pi: straight behind, e_z > 0, e_x ~ 0) on both sides of it, ones in
    the top and the bottom half-rows (v < 0, v > Eh - 1), and the centres of the map's four quadrants.  Stated in the environment frame
    and turned back into the world's."""
    e = [_unit(rng.standard_normal((n, 3)))]
    for ex in (1e-3, -1e-3, 1e-9, -1e-9, 0.05, -0.05):
        for ey in (0.0, 0.4, -0.7):
            e.append(_unit([[ex, ey, 1.0]]))
    half_row = math.pi / EH / 2.0                               # theta of v = 0
    for theta in (0.3 * half_row, 0.9 * half_row, math.pi - 0.3 * half_row, math.pi - 0.9 * half_row):
        for phi in (0.3, -2.0, 3.1):
            e.append(np.array([[math.sin(theta) * math.sin(phi), math.cos(theta), -math.sin(theta) * math.cos(phi)]]))
    e = np.concatenate(e)
    return np.ascontiguousarray(e @ R)                          # d = R^T e, row by row


# ---- the lookup ------------------------------------------------------------------------------------------------------------------------
def test_uv_is_the_restatements_within_the_bound_of_acos_and_atan2(hs):
    rng = np.random.default_rng(2)
    R = image_env_ref.rotation()
    d = _directions(rng, R)
    uv, ey = np.empty((len(d), 2)), np.empty(len(d))
    hs.env_uv(_p(np.ascontiguousarray(R)), EH, EW, _p(d), len(d), _p(uv), _p(ey))
    u, v, rey = image_env_ref.env_uv(R, torch.as_tensor(d), EH, EW)
    assert same_bits(ey, rey.numpy())                            # products and sums only
    du, dv = np.abs(uv[:, 0] - u.numpy()).max(), np.abs(uv[:, 1] - v.numpy()).max()
    print("max |du|", du, "bound", EW * image_env_ref.UV_ULPS, "max |dv|", dv, "bound", EH * image_env_ref.UV_ULPS)
    assert du <= EW * image_env_ref.UV_ULPS and dv <= EH * image_env_ref.UV_ULPS
    assert uv[:, 0].min() >= -0.5 and uv[:, 0].max() <= EW - 0.5 and uv[:, 1].min() >= -0.5 and uv[:, 1].max() <= EH - 0.5
    # the cases are what they claim: both sides of the seam, both half-rows
    assert (uv[:, 0] < 0).any() and (uv[:, 0] > EW - 1).any() and (uv[:, 1] < 0).any() and (uv[:, 1] > EH - 1).any()


def test_orientation_of_the_map(hs):
    """Row 0 looks along +y, the map's centre column along -z, three quarters of the way along +x; the rotation's ROWS are the
    environment's axes in the world."""
    eye = np.ascontiguousarray(np.eye(3))
    d = np.ascontiguousarray([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    uv, ey = np.empty((5, 2)), np.empty(5)
    hs.env_uv(_p(eye), EH, EW, _p(d), 5, _p(uv), _p(ey))
    assert uv[0, 1] == -0.5 and uv[1, 1] == pytest.approx(EH - 0.5, abs=1e-13) and uv[2, 1] == pytest.approx(EH / 2 - 0.5, abs=1e-13)
    assert uv[2, 0] == EW / 2 - 0.5 and uv[3, 0] == pytest.approx(0.75 * EW - 0.5, abs=1e-13) and uv[4, 0] == pytest.approx(0.25 * EW - 0.5, abs=1e-13)
    R = image_env_ref.rotation()
    hs.env_uv(_p(np.ascontiguousarray(R)), EH, EW, _p(np.ascontiguousarray(R[1:2])), 1, _p(uv), _p(ey))      # the world direction of the environment's +y
    assert ey[0] == pytest.approx(1.0, abs=1e-15) and uv[0, 1] <= -0.5 + 1e-6
    hs.env_uv(_p(np.ascontiguousarray(R.T)), EH, EW, _p(np.ascontiguousarray(R[1:2])), 1, _p(uv), _p(ey))    # the transposed matrix is another map
    assert abs(ey[0] - 1.0) > 1e-2


@pytest.mark.parametrize("channels", [1, 3])
def test_cell_and_fetch_equal_the_restatement_bit_for_bit(hs, channels):
    rng = np.random.default_rng(4)
    env = rng.random((EH, EW, channels)).astype(np.float32)
    uv = np.stack([rng.uniform(-0.5, EW - 0.5, 300), rng.uniform(-0.5, EH - 0.5, 300)], axis=1)
    edge = [(-0.5, 3.0), (-1e-12, 3.0), (0.0, 3.0), (EW - 1.0, 2.5), (EW - 0.75, 2.5), (EW - 0.5, 2.5), (4.25, -0.5), (4.25, 0.0), (4.25, EH - 1.0), (4.25, EH - 0.5),
            (EW - 0.5, EH - 0.5), (-0.5, -0.5), (7.0, 5.0)]
    uv = np.ascontiguousarray(np.concatenate([uv, np.array(edge)]))
    out, cell = np.empty((len(uv), channels)), np.empty((len(uv), 3), np.int32)
    hs.env_fetch(_p(env), EH, EW, channels, _p(uv), len(uv), _p(out), _p(cell))
    ref = image_env_ref.env_bilinear(env, torch.as_tensor(uv[:, 0].copy()), torch.as_tensor(uv[:, 1].copy()))
    assert same_bits(out, ref.numpy())
    assert cell.min() >= 0 and cell[:, :2].max() <= EW - 1 and cell[:, 2].max() <= EH - 2          # every read inside the map
    k = len(uv) - len(edge)
    assert cell[k].tolist() == [EW - 1, 0, 3] and cell[k + 1].tolist() == [EW - 1, 0, 3] and cell[k + 2].tolist() == [0, 1, 3]     # left of the seam
    assert cell[k + 3].tolist() == [EW - 1, 0, 2] and cell[k + 5].tolist() == [EW - 1, 0, 2]                                      # right of it
    assert cell[k + 6, 2] == 0 and cell[k + 7, 2] == 0 and cell[k + 8, 2] == EH - 2 and cell[k + 9, 2] == EH - 2
    # the two ends of the seam cell meet: u = -0.5 and u = Ew - 0.5 are the same point of the map
    a, b = np.empty((2, channels)), np.empty((2, 3), np.int32)
    hs.env_fetch(_p(env), EH, EW, channels, _p(np.ascontiguousarray([[-0.5, 6.25], [EW - 0.5, 6.25]])), 2, _p(a), _p(b))
    assert np.array_equal(a[0], a[1])
    # on a texel: that texel; above the first row and below the last: the row itself (v is clamped)
    assert np.array_equal(out[-1], env[5, 7].astype(np.float64))
    assert np.array_equal(out[k + 6], out[k + 7]) and np.array_equal(out[k + 8], out[k + 9])


def test_rotation_check(hs):
    ok = lambda R: hs.env_rot_ok(_p(np.ascontiguousarray(R, dtype=np.float64)))      # noqa: E731
    R = image_env_ref.rotation()
    assert ok(np.eye(3)) == 1 and ok(R) == 1 and ok(R.T) == 1 and ok(np.diag([1.0, -1.0, 1.0])) == 1
    assert ok(R * (1 + 1e-11)) == 0 and ok(R * (1 + 1e-13)) == 1 and ok(np.zeros((3, 3))) == 0
    skew = R.copy()
    skew[0] += 1e-9 * skew[1]
    nan = R.copy()
    nan[2, 2] = np.nan
    assert ok(skew) == 0 and ok(nan) == 0


# ---- a sample's colour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_screen", [True, False], ids=["screen", "no-screen"])
@pytest.mark.parametrize("channels", [1, 3])
def test_colours_against_the_restatement(hs, channels, with_screen):
    rng = np.random.default_rng(6)
    tex_h, tex_w = 9, 12
    screen = render.Screen([-4.0, 8.0, 16.0], [0.5, 0.0, 0.0], [0.0, -0.25, 0.0])
    tex = rng.random((tex_h, tex_w, channels)).astype(np.float32)
    env = rng.random((EH, EW, channels)).astype(np.float32)
    R = np.ascontiguousarray(image_env_ref.rotation())
    n = 200
    # exit rays that start around the origin: those that look along +z land on or near the screen (z = 16), the others go elsewhere
    o = np.ascontiguousarray(rng.uniform(-2, 2, (n, 3)))
    aim = np.stack([rng.uniform(-5, 2.5, n), rng.uniform(5.5, 8.5, n), np.full(n, 16.0)], axis=1)      # the screen: x in [-4, 1.5], y in [6, 8]
    d = _unit(aim - o)
    d[n // 2:] = _unit(rng.standard_normal((n - n // 2, 3)))
    d = np.ascontiguousarray(d)
    cls = np.ascontiguousarray(rng.integers(0, 2, n), dtype=np.int32)
    cls[::17] = image_ref.INVALID
    T = np.ascontiguousarray(rng.uniform(0.5, 1.0, n))
    invalid = np.array([0.5, 0.625, 0.75][:channels])
    col, src = np.full((n, channels), np.nan), np.full(n, -1, np.int32)
    hs.env_colours(_p(screen.packed()) if with_screen else None, _p(tex) if with_screen else None, tex_h, tex_w, channels, _p(env), EH, EW, _p(R), _p(cls),
                   _p(o), _p(d), _p(T), n, _p(invalid), _p(col), _p(src))
    ref = image_env_ref.sample_colours(screen if with_screen else None, tex if with_screen else None, env, R, torch.as_tensor(cls.astype(np.int64)),
                                       torch.as_tensor(o), torch.as_tensor(d), torch.as_tensor(T), invalid)
    rsrc, rcol = ref["src"].numpy(), ref["col"].numpy()
    assert np.array_equal(src, rsrc)
    for kind in (image_env_ref.FILL, image_env_ref.SCREEN):
        assert same_bits(col[src == kind], rcol[src == kind])
    G = max(np.abs(np.diff(env.astype(np.float64), axis=0)).max(), np.abs(np.diff(env.astype(np.float64), axis=1)).max(), np.abs(env[:, 0].astype(np.float64) - env[:, -1]).max())
    e = src == image_env_ref.ENV
    assert np.abs(col[e] - rcol[e]).max() <= G * (EW + EH) * image_env_ref.UV_ULPS + 2.0 ** -52
    assert (src == image_env_ref.FILL).sum() >= 10 and e.sum() >= 80 and ((src == image_env_ref.SCREEN).sum() >= 30) == with_screen
    assert (col[src == image_env_ref.FILL] == invalid).all() and np.isfinite(col).all()
    if with_screen:          # what does not see the environment has the bits of the clear function, image_sample_colour
        clear = np.full((n, channels), np.nan)
        hs.env_clear_colours(_p(screen.packed()), _p(tex), tex_h, tex_w, channels, _p(cls), _p(o), _p(d), _p(T), n, _p(np.full(channels, 0.125)), _p(invalid), _p(clear))
        assert same_bits(col[~e], clear[~e]) and (clear[e] == 0.125).all()


# ---- the adjoint of the lookup -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_lookup_backward_against_autograd(hs, channels):
    rng = np.random.default_rng(8)
    R = np.ascontiguousarray(image_env_ref.rotation())
    env = rng.random((EH, EW, channels)).astype(np.float32)
    d = _directions(rng, R, 200)
    g_c = np.ascontiguousarray(rng.standard_normal((len(d), channels)))
    g_d = np.empty((len(d), 3))
    hs.env_lookup_backward(_p(env), EH, EW, channels, _p(R), _p(d), _p(g_c), len(d), _p(g_d))
    dt = torch.as_tensor(d).clone().requires_grad_(True)
    (torch.as_tensor(g_c) * image_env_ref.lookup(env, R, dt)).sum().backward()
    ref = dt.grad.numpy()
    _, v, _ = image_env_ref.env_uv(R, torch.as_tensor(d), EH, EW)
    outside = ((v < 0) | (v > EH - 1)).numpy()
    assert outside.sum() >= 6 and np.isfinite(ref).all() and np.abs(ref).max() > 1.0
    # 1e-9 relative to the row's largest entry: the chain is a dozen operations on values whose quotients (1 / sin(theta) up to
    # 2 Eh / pi * 3 here) the two sides form from (u, v) that differ by UV_ULPS
    scale = np.abs(ref).max(axis=1, keepdims=True)
    assert (np.abs(g_d - ref) <= 1e-9 * scale + 1e-12).all()
    # above the first and below the last row v is clamped: only u carries a gradient there, so g is horizontal in the environment frame
    assert np.abs((g_d[outside] @ R.T)[:, 1]).max() <= 1e-9 * scale[outside].max()
    # a negative control: the transposed rotation in the last step is another gradient
    wrong = (g_d @ R.T) @ R.T
    assert (np.abs(wrong - ref) > 1e-3 * scale).any()


# ---- the outer-surface reflection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snell", [0, 1], ids=["reference", "snell"])
def test_reflected_ray_and_r1_equal_the_restatement_bit_for_bit(hs, snell):
    """`wide`: the first faces are the oracle tracer's; which samples qualify is exact, and ro, wr, R1 -- products, sums, quotients and roots
    only -- have the restatement's bits under either refraction law (the first Bounce's t, n, ci are bounce_forward's in both)."""
    from conftest import IOR
    sc = image_cases.scene("wide")
    ref = image_env_cases.reflected("wide")
    mesh = sc["mesh"]
    faces = np.ascontiguousarray(mesh.faces, dtype=np.int32)
    verts = np.ascontiguousarray(mesh.vertices, dtype=np.float64)
    cam = np.ascontiguousarray(np.concatenate([np.asarray(sc["camera_M"][3]).reshape(-1), np.asarray(sc["camera_M"][2])[:3, :].reshape(-1)]))
    n = sc["height"] * sc["width"] * sc["s"] ** 2
    first = np.ascontiguousarray(ref["face"].numpy(), dtype=np.int32)
    qual, ro, wr, R1 = np.zeros(n, np.uint8), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    hs.env_reflect(_p(faces), _p(verts), len(faces), _p(cam), sc["height"], sc["width"], sc["s"], image_cases.EXT, IOR, snell, _p(first), _p(qual), _p(ro), _p(wr), _p(R1))
    assert np.array_equal(qual.astype(bool), ref["qual"].numpy())
    assert same_bits(ro, ref["ro"].numpy()) and same_bits(wr, ref["wr"].numpy()) and same_bits(R1, ref["R1"].numpy())
    q = qual.astype(bool)
    assert q.sum() > 1000 and (first >= 0).sum() > q.sum() - 1 and ref["seen"].sum() > 900 and (ref["qual"] & ~ref["seen"]).sum() > 5
    assert 0.03 < R1[q].mean() < 0.1 and R1[q].max() > 0.5 and np.abs(np.linalg.norm(wr[q], axis=1) - 1).max() < 1e-14
    # a face outside the mesh and a sample without a face qualify nothing
    first[:] = -1
    first[3] = len(faces)
    hs.env_reflect(_p(faces), _p(verts), len(faces), _p(cam), sc["height"], sc["width"], sc["s"], image_cases.EXT, IOR, snell, _p(first), _p(qual), _p(ro), _p(wr), _p(R1))
    assert not qual.any()


@pytest.mark.parametrize("with_screen", [True, False], ids=["screen", "no-screen"])
def test_the_reflection_term_against_the_restatement(hs, with_screen):
    """c = T B(exit) + R1 B(ro, wr) on the samples of `wide` whose reflection is added, from the restatement's own T B(exit): a reflected
    ray on the screen adds the restatement's bits, one that goes to the environment is within G_env times the (u, v) bound."""
    name, law = "wide", image_cases.LAWS[1]
    sc = image_cases.scene(name)
    env = image_env_cases.environment(1)
    plain = image_env_cases.reference(name, law, with_screen, False)
    ref = image_env_cases.reference(name, law, with_screen, True)
    refl = image_env_cases.reflected(name)
    add = np.ascontiguousarray(ref["added"].numpy(), dtype=np.uint8)
    col = np.ascontiguousarray(plain["col"].numpy().copy())
    hs.env_add_reflection(_p(sc["screen"].packed()) if with_screen else None, _p(sc["texture"]) if with_screen else None, image_cases.TEX, image_cases.TEX, 1,
                          _p(env.texels), EH, EW, _p(np.ascontiguousarray(env.rotation)), _p(add), _p(np.ascontiguousarray(refl["ro"].numpy())),
                          _p(np.ascontiguousarray(refl["wr"].numpy())), _p(np.ascontiguousarray(refl["R1"].numpy())), len(add), _p(col))
    rcol = ref["col"].numpy()
    a = add.astype(bool)
    on = ref["rb"]["on"].numpy() & a
    assert same_bits(col[~a], rcol[~a]) and same_bits(col[on], rcol[on])
    assert on.any() == with_screen and (a & ~on).sum() > 1000 and (col[a] > plain["col"].numpy()[a]).all()
    G = image_env_cases.env_step(1)
    assert np.abs(col[a & ~on] - rcol[a & ~on]).max() <= G * (EW + EH) * image_env_ref.UV_ULPS + 2.0 ** -52
    assert np.array_equal(ref["reflect"].numpy() > 0, a.reshape(sc["height"] * sc["width"], -1).any(1).reshape(sc["height"], sc["width"]))


# ---- the photometric loss and its adjoint ------------------------------------------------------------------------------------------------
def host_loss_of(hs, sc, law, with_screen, reflection, fwd, texels, rotation, target, weight, ii, ie):
    """The header's loss, gradients, count and image of a scene dict (one of image_cases, or one of tests/image_fuzz_cases.py with its own
    texture and environment extents), on the classes, tape and occlusion verdicts of ``fwd`` (``image_env_ref.loss_forward``'s dict)."""
    mesh = sc["mesh"]
    faces, verts = np.ascontiguousarray(mesh.faces, dtype=np.int32), np.ascontiguousarray(mesh.vertices, dtype=np.float64)
    cam = np.ascontiguousarray(np.concatenate([np.asarray(sc["camera_M"][3]).reshape(-1), np.asarray(sc["camera_M"][2])[:3, :].reshape(-1)]))
    tex = np.asarray(sc["texture"], np.float32)
    tex = np.ascontiguousarray(tex[:, :, None] if tex.ndim == 2 else tex)
    texels = np.ascontiguousarray(texels, dtype=np.float32)
    C = tex.shape[2]
    gV, g_ior, count = np.zeros_like(verts), np.zeros(2), np.zeros(1, np.int64)
    image = np.zeros((sc["height"], sc["width"], C), np.float32)
    invalid = np.ascontiguousarray(np.broadcast_to(np.asarray(sc["invalid"], np.float64), (C,)))
    loss = hs.env_loss_view(_p(cam), sc["height"], sc["width"], sc["s"], _p(sc["screen"].packed()) if with_screen else None, _p(tex) if with_screen else None,
                            tex.shape[0], tex.shape[1], C, _p(texels), texels.shape[0], texels.shape[1], _p(np.ascontiguousarray(rotation, dtype=np.float64)), _p(faces),
                            _p(verts), len(faces),
                            ii, ie, int(law[2] == "snell"), int(reflection), _p(np.ascontiguousarray(fwd["cls"].numpy(), dtype=np.int32)),
                            _p(np.ascontiguousarray(fwd["tape"].numpy(), dtype=np.int32)), _p(np.ascontiguousarray(fwd["hits"].numpy(), dtype=np.uint8)),
                            _p(np.ascontiguousarray(fwd["seen"].numpy(), dtype=np.uint8)), _p(invalid), _p(np.ascontiguousarray(target)), _p(weight), _p(gV), _p(g_ior),
                            _p(count), _p(image))
    return dict(loss=loss, grad_V=gV, g_int=g_ior[0], g_ext=g_ior[1], count=int(count[0]), image=image)


def host_loss(hs, name, law, with_screen, reflection, weighted=False, ior=None):
    """The header's loss, gradients, count and image of a case, on the restatement's classes, tape and occlusion verdicts."""
    import image_loss_cases
    from conftest import IOR
    sc = image_cases.scene(name)
    ref = image_env_cases.loss_reference(name, law, with_screen, reflection, weighted)
    env = image_env_cases.environment(sc["texture"].shape[2])
    weight = image_loss_cases.half_weight(name) if weighted else None
    ii, ie = ior if ior is not None else (IOR, image_cases.EXT)
    got = host_loss_of(hs, sc, law, with_screen, reflection, ref["fwd"], env.texels, env.rotation, image_env_cases.loss_target(name, law, with_screen, reflection), weight,
                       ii, ie)
    return got, ref


LOSS_CASES = [("wide", image_cases.LAWS[1], True, True), ("wide", image_cases.LAWS[1], False, True), ("v5", image_cases.LAWS[2], True, True),
              ("v5", image_cases.LAWS[2], False, False), ("v41", image_cases.LAWS[0], True, False), ("v41", image_cases.LAWS[0], False, True)]


@pytest.mark.parametrize("name,law,with_screen,reflection", LOSS_CASES, ids=[f"{n}-{l[0]}-{l[1]}-{l[2]}-{'screen' if w else 'no-screen'}-{'reflection' if r else 'no-reflection'}"
                                                                           for n, l, w, r in LOSS_CASES])
def test_loss_and_gradients_against_autograd(hs, name, law, with_screen, reflection):
    """Loss within LOSS_REL, vertex and IOR gradients within image_loss_cases.close, the count exact (every through sample), the image the
    restatement's float32 within one unit of its store (2^-23: acos / atan2 may move a value across a rounding boundary)."""
    import image_loss_cases
    got, ref = host_loss(hs, name, law, with_screen, reflection)
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    print(name, law, with_screen, reflection, "loss", ref["loss"], "rel", rel, "count", got["count"], "max |dV|", np.abs(got["grad_V"] - ref["grad_V"]).max(),
          "of", np.abs(ref["grad_V"]).max(), "d g_int", got["g_int"] - ref["g_int"], "of", ref["g_int"], "d g_ext", got["g_ext"] - ref["g_ext"])
    assert ref["loss"] > 0.5 and rel <= image_loss_cases.LOSS_REL
    assert got["count"] == ref["count"] > 900
    assert image_loss_cases.close(got["grad_V"], ref["grad_V"]) and np.abs(ref["grad_V"]).max() > 0.5
    assert image_loss_cases.close([got["g_int"], got["g_ext"]], [ref["g_int"], ref["g_ext"]])
    assert np.abs(got["image"].astype(np.float64) - ref["image"].astype(np.float64)).max() <= 2.0 ** -23


@pytest.mark.parametrize("detach", ["reflection", "lookup"])
def test_a_restatement_with_a_term_detached_is_another_gradient(hs, detach):
    """Negative controls: with the reflection term, or with the environment lookup, cut out of autograd's graph the restatement's gradients
    fall outside `close` of the header's -- the header differentiates both."""
    import image_loss_cases
    name, law = "wide", image_cases.LAWS[1]
    got, ref = host_loss(hs, name, law, True, True)
    cut = image_env_cases.loss_reference(name, law, True, True, detach=detach)
    assert cut["loss"] == ref["loss"]
    assert not image_loss_cases.close(got["grad_V"], cut["grad_V"])
    assert not image_loss_cases.close([got["g_int"], got["g_ext"]], [cut["g_int"], cut["g_ext"]])


def test_a_weighted_loss_and_central_differences_in_both_iors(hs):
    """The weight plane, and d loss / d (ior_int, ior_ext) against central differences of the header's own loss (classes, tape and verdicts
    held): h = 1e-6, second-order error ~1e-12 relative, rounding 1e-15 / 1e-6 = 1e-9 of the loss -- 1e-6 relative to the larger partial."""
    import image_loss_cases
    from conftest import IOR
    name, law = "wide", image_cases.LAWS[2]
    got, ref = host_loss(hs, name, law, True, True, weighted=True)
    assert abs(got["loss"] - ref["loss"]) / ref["loss"] <= image_loss_cases.LOSS_REL and image_loss_cases.close(got["grad_V"], ref["grad_V"])
    assert not got["grad_V"][np.abs(ref["grad_V"]).sum(1) == 0].any()
    h = 1e-6
    scale = max(abs(got["g_int"]), abs(got["g_ext"]))
    for k, key in enumerate(("g_int", "g_ext")):
        up = [IOR, image_cases.EXT]
        dn = list(up)
        up[k] += h
        dn[k] -= h
        cd = (host_loss(hs, name, law, True, True, True, up)[0]["loss"] - host_loss(hs, name, law, True, True, True, dn)[0]["loss"]) / (2 * h)
        print(key, got[key], "central difference", cd)
        assert abs(cd - got[key]) <= 1e-6 * scale


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texels,rotation,match", [(np.zeros((4, 8, 2), np.float32), None, "texels"), (np.zeros((1, 8, 3), np.float32), None, "2 x 2"),
                                                   (np.zeros((4, 8, 3), np.uint8), None, "float"), (np.zeros(4, np.float32), None, "texels"), ("sky", None, "texels"),
                                                   (np.zeros((4, 8, 3), np.float32), np.eye(4), "rotation"), (np.zeros((4, 8, 3), np.float32), np.eye(3) * 1.001, "orthonormal"),
                                                   (np.zeros((4, 8, 3), np.float32), np.full((3, 3), np.nan), "rotation"),
                                                   (np.zeros((4, 8, 3), np.float32), image_env_ref.rotation().astype(np.float32), "orthonormal")])
def test_environment_refuses_bad_arguments(texels, rotation, match):
    with pytest.raises(ValueError, match=match):
        render.Environment(texels, rotation)


def test_environment_holds_float32_texels_and_a_float64_rotation():
    e = render.Environment(np.arange(24, dtype=np.float64).reshape(3, 8), image_env_ref.rotation())
    assert e.texels.dtype == np.float32 and e.texels.shape == (3, 8, 1) and e.channels == 1
    assert e.packed().dtype == np.float64 and np.array_equal(e.packed().reshape(3, 3), image_env_ref.rotation())
    assert np.array_equal(render.Environment(np.zeros((2, 2, 3), np.float32)).rotation, np.eye(3))
    Y = render.Environment.yaw(90.0)
    assert np.allclose(Y @ np.array([0.0, 0.0, -1.0]), [1.0, 0.0, 0.0], atol=1e-15) and np.allclose(Y @ Y.T, np.eye(3), atol=1e-15)
    render.Environment(np.zeros((2, 2, 3), np.float32), Y)


def _args():
    cam = image_cases.camera(5, 8, 8)
    return dict(camera_M=cam, height=8, width=8, screen=render.Screen([0, 0, 0], [1, 0, 0], [0, 1, 0]), texture=np.zeros((4, 4, 3), np.float32),
                environment=render.Environment(np.zeros((4, 8, 3), np.float32)))


@pytest.mark.parametrize("change,match", [(dict(environment=np.zeros((4, 8, 3), np.float32)), "environment"), (dict(environment="sky.hdr"), "environment"),
                                          (dict(absorption=0.1), "absorption"), (dict(screen=None), "screen and texture"), (dict(texture=None), "screen and texture"),
                                          (dict(environment=render.Environment(np.zeros((4, 8, 1), np.float32))), "channels"),
                                          (dict(screen=None, texture=None, void=[0.0, 1.0]), "void"), (dict(screen=(0, 1, 2)), "screen"),
                                          (dict(supersample=5), "supersample"), (dict(reflection=1), "reflection"), (dict(reflection=True, environment=None), "reflection"),
                                          (dict(reflection=True, fresnel=False), "reflection")])
def test_render_image_names_the_bad_environment_argument(change, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    kw = dict(_args(), **change)
    pos = [kw.pop(k) for k in ("camera_M", "height", "width", "screen", "texture")]
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.render_image(object(), *pos, **kw)


def test_check_render_args_with_and_without_a_screen():
    a = _args()
    got = render.check_render_args(a["camera_M"], 8, 8, a["screen"], a["texture"], environment=a["environment"])
    assert got["environment"] is a["environment"] and got["channels"] == 3 and got["screen"].shape == (9,)
    mono = render.Environment(np.zeros((4, 8), np.float32))
    got = render.check_render_args(a["camera_M"], 8, 8, None, None, environment=mono, void=0.5)
    assert got["screen"] is None and got["texture"] is None and got["channels"] == 1 and got["void"].shape == (1,)
    assert render.check_render_args(a["camera_M"], 8, 8, a["screen"], a["texture"])["environment"] is None
    with pytest.raises(ValueError, match="screen"):                   # without an environment a screen is required, as before
        render.check_render_args(a["camera_M"], 8, 8, None, None)


# ---- Radiance pictures -------------------------------------------------------------------------------------------------------------------
def _rgbe(rng, h, w):
    px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    px[:, :, 3] = rng.integers(120, 136, (h, w))
    px[0, 0] = (7, 8, 9, 0)                                       # exponent 0: black
    px[1, 2:7] = px[1, 2]                                          # a run (where the row is that long)
    return px


def _decode(px):
    e = px[:, :, 3].astype(np.int32)
    return ((px[:, :, :3].astype(np.float64) + 0.5) * np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)[:, :, None]).astype(np.float32)


def _rle(px):
    """The run-length encoding of Radiance's scanlines: 2 2 hi lo, then per component runs (128 + n, value) and literals (n, bytes)."""
    out = bytearray()
    h, w = px.shape[:2]
    for y in range(h):
        out += bytes([2, 2, w >> 8, w & 255])
        for ch in range(4):
            row, x = px[y, :, ch], 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 3:
                    out += bytes([128 + run, int(row[x])])
                    x += run
                else:
                    n = min(w - x, 5)
                    out += bytes([n]) + row[x:x + n].tobytes()
                    x += n
    return bytes(out)


@pytest.mark.parametrize("encoded", [False, True], ids=["flat", "rle"])
def test_environment_load_reads_radiance_pictures(tmp_path, encoded):
    rng = np.random.default_rng(9)
    px = _rgbe(rng, 6, 12)
    path = str(tmp_path / "sky.hdr")
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\n# made by a test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 6 +X 12\n")
        f.write(_rle(px) if encoded else px.tobytes())
    env = render.Environment.load(path, image_env_ref.rotation())
    assert env.texels.dtype == np.float32 and env.texels.shape == (6, 12, 3) and np.array_equal(env.texels, _decode(px))
    assert not env.texels[0, 0].any() and env.texels.max() > 1.0 and np.array_equal(env.rotation, image_env_ref.rotation())


@pytest.mark.parametrize("content,match", [(b"P6\n2 2\n255\n" + bytes(12), "RADIANCE"), (b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 2 +X 2\n" + bytes(16), "FORMAT"),
                                           (b"#?RADIANCE\n\n+X 2 -Y 2\n" + bytes(16), "orientation"), (b"#?RADIANCE\n\n-Y 2 +X 2\n" + bytes(15), "ends"),
                                           (b"#?RADIANCE\n\n-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 200, 1]), "run|ends"),
                                           (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n", "size line"), (b"#?RADIANCE\n\n-Y 2 +X 2", "size line"),
                                           (b"#?RADIANCE\n\n-Y two +X 2\n" + bytes(16), "size line"), (b"#?RADIANCE\n\n-Y 0 +X 2\n", "empty")])
def test_environment_load_refuses_what_it_cannot_read(tmp_path, content, match):
    """Every refusal names the file."""
    path = str(tmp_path / "bad.hdr")
    with open(path, "wb") as f:
        f.write(content)
    with pytest.raises(ValueError, match=match) as e:
        render.Environment.load(path)
    assert "bad.hdr" in str(e.value)


def test_environment_load_reads_a_header_with_crlf_line_ends(tmp_path):
    px = _rgbe(np.random.default_rng(3), 2, 3)
    path = str(tmp_path / "dos.hdr")
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\r\nFORMAT=32-bit_rle_rgbe\r\n\r\n-Y 2 +X 3\r\n" + px.tobytes())
    assert np.array_equal(render.Environment.load(path).texels, _decode(px))


def test_environment_load_reads_what_load_texture_reads(tmp_path):
    a = np.random.default_rng(1).random((4, 8, 3)).astype(np.float32) * 3.0
    np.save(str(tmp_path / "sky.npy"), a)
    assert np.array_equal(render.Environment.load(str(tmp_path / "sky.npy")).texels, a)
    render.write_image(str(tmp_path / "sky.ppm"), a / 3.0)
    assert render.Environment.load(str(tmp_path / "sky.ppm")).texels.shape == (4, 8, 3)


@pytest.mark.parametrize("argv,match", [(["--no-screen"], "--environment"), (["--env-rotation", "yaw", "30"], "--environment"),
                                        (["--environment", "sky.hdr", "--absorption", "0.1"], "--absorption"), (["--reflection"], "--environment"),
                                        (["--environment", "sky.hdr", "--reflection", "--no-fresnel"], "--no-fresnel"),
                                        (["--environment", "sky.hdr", "--env-rotation", "1", "0", "0"], "nine numbers"),
                                        (["--environment", "sky.hdr", "--env-rotation", "yaw", "east"], "nine numbers")])
def test_cli_refuses_bad_environment_flags_before_it_loads_anything(tmp_path, argv, match):
    with pytest.raises(SystemExit, match=match):
        render.main(["--name", "hand", "-o", str(tmp_path)] + argv)


# ---- the cases and the declarations ------------------------------------------------------------------------------------------------------
def test_a_case_keeps_its_sensitive_share_and_reaches_every_source():
    """`wide` under (6, reflect, reference): the case with the largest share of sensitive pixels (16 of 960 with a screen)."""
    name, law = "wide", image_cases.LAWS[1]
    for with_screen in (True, False):
        ref = image_env_cases.reference(name, law, with_screen)
        bad = image_env_cases.sensitive(name, law, with_screen)
        src = ref["src"].numpy()
        print(name, law, with_screen, "sensitive", int(bad.sum()), "of", bad.size, "tol", image_env_cases.tolerance(name, law, with_screen))
        assert bad.mean() <= image_cases.SENSITIVE_CAP
        assert (src == image_env_ref.FILL).sum() > 20 and (src == image_env_ref.ENV).sum() > 500 and ((src == image_env_ref.SCREEN).sum() > 500) == with_screen
        assert 2.0 ** -23 < image_env_cases.tolerance(name, law, with_screen) < 1e-6
    both = [image_env_cases.reference(name, law, w) for w in (True, False)]
    moved = (both[0]["image"] != both[1]["image"]).any(2)
    assert moved.any() and not moved.all()                        # the screen covers part of the picture


@pytest.mark.parametrize("change,match", [(dict(absorption=0.1), "absorption"), (dict(screen_param=torch.eye(3, dtype=torch.float64), screen=None), "screen_param"),
                                          (dict(texture_param=torch.zeros((4, 4, 3)), texture=None), "texture_param"),
                                          (dict(camera_param=(torch.eye(4, dtype=torch.float64), torch.eye(3, dtype=torch.float64)), camera_M=None), "camera_param"),
                                          (dict(reflection=True, environment=None), "reflection"), (dict(reflection=True, fresnel=False), "reflection"),
                                          (dict(environment="room.hdr"), "environment"), (dict(target=np.zeros((8, 8, 1), np.float32)), "target")])
def test_image_loss_fused_names_the_bad_environment_argument(change, match):
    """Raised before anything touches the device: the method is called on an object that is no scene."""
    from drt_amd import diffrender
    kw = dict(dict(_args(), target=np.zeros((8, 8, 3), np.float32)), **change)
    pos = [kw.pop(k) for k in ("camera_M", "height", "width", "screen", "texture", "target")]
    with pytest.raises(ValueError, match=match):
        diffrender.Scene.image_loss_fused(object(), *pos, **kw)


def test_the_multi_view_call_refuses_an_environment():
    from drt_amd import diffrender
    for kw in (dict(environment=_args()["environment"]), dict(reflection=True)):
        with pytest.raises(ValueError, match="multi-view"):
            diffrender.Scene.image_loss_views_fused(object(), None, [0], np.zeros((4, 4, 3), np.float32), **kw)


def test_entry_point_is_declared_everywhere():
    from drt_amd import _lib, build
    assert len(_lib.SIGNATURES["drt_render_image_env"][1]) == len(_lib.SIGNATURES["drt_render_image"][1]) + 6
    assert "drt_image_env.hip" in build.UNITS
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_render_image_env(" in header
    unit = open(os.path.join(ROOT, "drt_amd", "csrc", "drt_image_env.hip")).read()
    assert "int drt_render_image_env(" in unit and "k_image_resolve<ImageClear, ImageScreenEnv>" in unit and "k_image_resolve<ImageClear, ImageScreenEnvReflect>" in unit
    assert "launch_trace_list(kTraceAny" in unit
    assert len(_lib.SIGNATURES["drt_render_image_loss_env"][1]) == len(_lib.SIGNATURES["drt_render_image_loss"][1]) + 5
    assert "int drt_render_image_loss_env(" in header and "int drt_render_image_loss_env(" in unit and "k_image_reflect_bwd" in unit
    assert "def enqueue_image_env_term(" in open(os.path.join(ROOT, "drt_amd", "diffrender.py")).read()
