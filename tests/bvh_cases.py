"""Meshes on which a BVH build can go wrong: ``make(name) -> (faces int32 [n, 3], verts float32 [v, 3])``, seeded, cached.

SMALL: compared array by array.  LARGE: the two sizes either side of the fused / unfused sort switch (128 / 129 tiles of 2048)."""
import ctypes
import functools
import os
import zlib

import numpy as np

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 12289)
LARGE = ("switch_262144", "switch_262145")
SMALL = tuple("soup_%d" % n for n in SIZES) + (
    "copies_5000", "three_keys", "drop_bits", "quads", "flat_z", "needle", "point", "cell_edges", "mixed_sign", "all_negative",
    "verts_mod0", "verts_mod1", "verts_mod2", "verts_mod3", "outliers", "zero_area", "hand")
ALL = SMALL + LARGE


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def soup(rng, n, extent=(160.0, 210.0, 70.0), origin=(-80.0, -100.0, 10.0), size=0.02):
    """n independent triangles: three points around a random centre inside the box."""
    extent, origin = np.asarray(extent), np.asarray(origin)
    c = rng.random((n, 1, 3)) * extent + origin
    v = c + rng.standard_normal((n, 3, 3)) * size * extent.max()
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3), v.reshape(-1, 3).astype(np.float32)


def _with_box(faces, verts, lo, hi):
    """Two unreferenced vertices that fix the scene box."""
    return faces, np.concatenate([verts, np.array([lo, hi], np.float32)]).astype(np.float32)


def _points(centres, half):
    """One small triangle per centre whose bounding box is centre -/+ half exactly (all values must be exact in float32)."""
    c = np.asarray(centres, np.float64)[:, None, :]
    off = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float64) * half
    v = (c + off).astype(np.float32)
    return np.arange(3 * len(centres), dtype=np.int32).reshape(-1, 3), v.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def make(name):
    """(faces, verts) of a case; shared between tests, so read-only."""
    faces, verts = _make(name)
    faces, verts = np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(verts, np.float32)
    faces.flags.writeable = verts.flags.writeable = False
    return faces, verts


def _make(name):
    rng = _rng(name)
    if name.startswith("soup_") or name.startswith("switch_"):
        return soup(rng, int(name.split("_")[1]))
    if name == "copies_5000":       # every key equal: only stability orders the output
        return np.tile(np.array([[0, 1, 2]], np.int32), (5000, 1)), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    if name == "three_keys":        # three distinct keys, each in more than one sort tile's worth of faces, interleaved at random
        verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [50, 60, 70], [51, 60, 70], [50, 61, 70], [99, 99, 99], [100, 99, 99], [99, 100, 100]], np.float32)
        which = rng.permutation(np.repeat(np.arange(3), (2100, 2500, 2400)))
        return (3 * which[:, None] + np.arange(3)[None, :]).astype(np.int32), verts
    if name == "drop_bits":         # a cubic box: 10 bits per axis, x y z in turn, so the low 6 key bits are the low 2 bits of each axis
        base = rng.integers(0, 256, (40, 3)) * 4
        low = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
        cells = np.concatenate([b + low[rng.permutation(64)] for b in base])       # 64 faces per group of 4 x 4 x 4 cells, in scrambled order
        f, v = _points(cells + 0.5, 0.125)
        return _with_box(f, v, [0, 0, 0], [1024, 1024, 1024])
    if name == "quads":             # a height field of quads, rising along x and y so that the diagonal a-c spans each quad's box: its two halves share a key
        m = 37
        x, y = np.meshgrid(np.arange(m + 1, dtype=np.float64), np.arange(m + 1, dtype=np.float64), indexing="ij")
        v = np.stack([x * 3.0, y * 2.0, 0.5 * x ** 1.5 + 0.3 * y + 0.01 * x * y], -1).reshape(-1, 3)
        i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        a, b, c, d = (i * (m + 1) + j).ravel(), ((i + 1) * (m + 1) + j).ravel(), ((i + 1) * (m + 1) + j + 1).ravel(), (i * (m + 1) + j + 1).ravel()
        return np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int32), v.astype(np.float32)
    if name == "flat_z":            # no extent along z
        f, v = soup(rng, 700)
        v[:, 2] = np.float32(12.5)
        return f, v
    if name == "needle":            # extent ratio 2^22: the long axis is capped at 20 bits
        return soup(rng, 900, extent=(2.0 ** 22, 1.0, 1.0), origin=(-7.0, 3.0, -1.0), size=1e-8)
    if name == "point":             # every vertex the same point: all extents 0
        return np.array([[0, 1, 2], [2, 1, 0], [0, 0, 1], [3, 4, 0], [1, 3, 2]], np.int32), np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (5, 1))
    if name == "cell_edges":        # box centres exactly on cell boundaries of a 1024^3 grid of unit cells, and one AT the box's maximum corner
        c = rng.integers(1, 1024, (300, 3)).astype(np.float64)
        c[:20] = rng.integers(1, 4, (20, 3)) * 256
        f, v = _points(c, 0.25)
        v = np.concatenate([v, np.array([[0, 0, 0]] + [[1024, 1024, 1024]] * 3, np.float32)])
        f = np.concatenate([f, np.array([[len(v) - 3, len(v) - 2, len(v) - 1]], np.int32)])      # zero-area, centre == scene maximum: the clamp
        return f[rng.permutation(len(f))], v
    if name == "mixed_sign":
        return soup(rng, 333, extent=(3.0, 5.0, 2.0), origin=(-1.5, -4.0, -0.001))
    if name == "all_negative":
        return soup(rng, 333, extent=(30.0, 5.0, 20.0), origin=(-100.0, -50.0, -21.0), size=0.001)
    if name.startswith("verts_mod"):        # the vertex count modulo 4, with the box's extremes among the LAST vertices
        want = int(name[-1])
        f, v = soup(rng, 50, size=0.005)
        extra = (want - len(v)) % 4 or 4
        tail = np.array([[-500, 0, 0], [0, 700, 0], [0, 0, -900], [600, -600, 800]], np.float32)[:extra]
        return f, np.concatenate([v, tail])
    if name == "outliers":          # unreferenced vertices far outside the triangles, first and in the middle
        f, v = soup(rng, 200, size=0.005)
        v = np.concatenate([np.array([[-1e4, 0, 0]], np.float32), v[:300], np.array([[0, 2e4, -3e4]], np.float32), v[300:]])
        f = f + 1 + (f >= 300)
        return f.astype(np.int32), v
    if name == "zero_area":         # repeated indices, collinear and coincident corners among ordinary triangles
        f, v = soup(rng, 120)
        f[::7, 1] = f[::7, 0]
        f[3::11] = f[3::11, :1]
        v[f[5::13, 2]] = 0.5 * (v[f[5::13, 0]] + v[f[5::13, 1]])
        return f, v
    if name == "hand":
        from drt_amd import mesh_io
        m = mesh_io.read_ply(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "hand_vh.ply"))
        return np.ascontiguousarray(m.faces, np.int32), np.ascontiguousarray(m.vertices, np.float32)
    raise KeyError(name)


# ---- the same cases through tests/hostsim (the project's headers compiled for the host) ----------------------------------------------
_P, _I64, _INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def hostsim_tree(hs, faces, verts, drop, names=None):
    """{name: array} of hs_create_ex(faces, verts, drop), named and typed as optix_mesh.tree_arrays()."""
    import bvh_ref
    hs.hs_create_ex.restype = _P
    hs.hs_create_ex.argtypes = [_P, _I64, _P, _I64, _INT]
    hs.hs_destroy.argtypes = [_P]
    hs.hs_export.restype = _INT
    hs.hs_export.argtypes = [_P, _INT, _P, _I64]
    faces, verts = np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(verts, np.float32)
    n, inner = len(faces), max(len(faces) - 1, 1)
    h = hs.hs_create_ex(faces.ctypes.data, n, verts.ctypes.data, len(verts), drop)
    try:
        out = {}
        for k, name in enumerate(bvh_ref.ARRAYS):
            if names is not None and name not in names:
                continue
            count = {"params": 1, "nodes": inner, "parent_inner": inner, "range_lo": inner, "range_hi": inner, "wide": inner}.get(name, n)
            a = np.zeros(count, bvh_ref.DTYPES[name])
            assert hs.hs_export(h, k, a.ctypes.data, a.nbytes) == 0, name
            assert hs.hs_export(h, k, a.ctypes.data, a.nbytes + 4) == -1, name
            out[name] = a[0] if name == "params" else a
        return out
    finally:
        hs.hs_destroy(h)


_host = {}


def host_tree(hs, name):
    """hostsim's build of a case with the device's drop bits; computed once."""
    import bvh_ref
    if name not in _host:
        faces, verts = make(name)
        _host[name] = hostsim_tree(hs, faces, verts, bvh_ref.drop_bits(len(faces)))
    return _host[name]
