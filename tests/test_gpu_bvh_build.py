"""Every array of the device BVH build (optix_mesh.tree_arrays) against the numpy restatement tests/bvh_ref.py and against the project's
headers compiled for the host (tests/hostsim), over the corpus of tests/bvh_cases.py: full builds by both update paths, both sides of
the sort switch, update sequences on one tracer, the kept-topology modes, repeatability, and the export's own argument checks.

drt_bvh_check and the brute-force comparison pass on any conservative tree; these tests hold each stage to what it is defined to be."""
import ctypes

import numpy as np
import pytest
import torch

import bvh_cases
import bvh_ref
from test_bvh_host import MAX_SLACK, _ref, quant_report

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def _tracer(mode=0, every=1):
    from drt_amd.optix_mesh import optix_mesh
    t = optix_mesh(0)
    if mode:
        t.tree_mode(mode, every)
    return t


def _update(t, verts, f64):
    """One vertex update by either path: float32 (k_bounds) or float64 (k_cast_verts and its accumulators) of the same values."""
    if f64:
        t.update_vert_f64(_dev(verts).double())
    else:
        t.update_vert(_dev(verts))


def _expect(ref, flat_order):
    """The restatement's build with tris_flat as the device leaves it: the records in the order of the build before (None: face order)."""
    if flat_order is None:
        return ref
    faces = ref["tris"]["face"]
    return dict(ref, tris_flat=ref["tris"][bvh_ref.inverse(faces)[np.asarray(flat_order).astype(np.int64)]])


def _hold(tree, faces, verts, ref, host=None, flat_order=None):
    """A device export equals the restatement (and hostsim's export), is a sound tree, and its bound bytes have the stated properties."""
    assert bvh_ref.differing(tree, _expect(ref, flat_order)) == []
    if host is not None:
        assert bvh_ref.differing(tree, _expect(host, flat_order)) == []
    assert bvh_ref.check_topology(tree, len(faces)) == []
    bad, slack = quant_report(tree, faces, verts)
    assert bad == 0 and slack <= MAX_SLACK


@pytest.mark.parametrize("name", bvh_cases.SMALL)
def test_full_build_equals_restatement_and_hostsim(hostsim, name):
    """update_mesh, then the same vertices again through update_vert and through update_vert_f64: three full builds that must all be
    the restatement's and hostsim's, entry by entry."""
    faces, verts = bvh_cases.make(name)
    ref, host = _ref(name), bvh_cases.host_tree(hostsim, name)
    t = _tracer()
    t.update_mesh(_dev(faces), _dev(verts))
    _hold(t.tree_arrays(), faces, verts, ref, host)                                 # records of the projection pass in face order
    trees = []
    for f64 in (False, True):
        _update(t, verts, f64)
        trees.append(t.tree_arrays())
        _hold(trees[-1], faces, verts, ref, host, flat_order=ref["order"])          # ... in the order of the build before
    assert all(bvh_ref.same(trees[0][k], trees[1][k]) for k in bvh_ref.ARRAYS)


@pytest.mark.parametrize("name", bvh_cases.LARGE)
def test_both_sides_of_the_sort_switch(hostsim, name):
    """128 tiles (fused passes, 24-bit keys) and 129 tiles (histogram / scan / scatter, 30-bit keys): keys and order against numpy,
    every array against hostsim -- whose bound bytes test_bvh_host.py has measured."""
    faces, verts = bvh_cases.make(name)
    ref, host = _ref(name), bvh_cases.host_tree(hostsim, name)
    t = _tracer()
    t.update_mesh(_dev(faces), _dev(verts))
    for f64 in (None, True):
        if f64:
            _update(t, verts, True)
        tree = t.tree_arrays()
        assert bvh_ref.differing(tree, ref, ["params", "keys", "order"]) == []
        assert np.all(np.diff(tree["keys"].astype(np.int64)) >= 0)
        assert bvh_ref.differing(tree, _expect(host, host["order"] if f64 else None)) == []
        assert bvh_ref.check_topology(tree, len(faces)) == []


def test_vertex_updates_on_one_tracer_follow_the_vertices():
    """Large extent, small extent, translated, the two update paths in turn: after each the scene box is that of THOSE vertices (it
    shrinks again), every array is a fresh build's, and the projection pass's records are in the order the build before left."""
    faces, v0 = bvh_cases.make("soup_2049")
    spin = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)
    sets = [v0 * np.float32(50), (v0 @ spin) * np.float32(0.01), v0 * np.float32(0.01) + np.float32(1000), v0[:, [2, 0, 1]], v0]
    t = _tracer()
    t.update_mesh(_dev(faces), _dev(v0))
    before = t.tree_arrays()["order"]
    for k, verts in enumerate(sets):
        verts = np.ascontiguousarray(verts, np.float32)
        _update(t, verts, f64=k % 2 == 1)
        ref = bvh_ref.build(faces, verts)
        tree = t.tree_arrays()
        assert bvh_ref.same(tree["params"], bvh_ref.params(verts))
        assert list(t.build_params()) == [*ref["params"]["lo"], *ref["params"]["inv"], ref["params"]["pad"]]
        _hold(tree, faces, verts, ref, flat_order=before)
        before = tree["order"]


def test_mesh_updates_on_one_tracer_reuse_capacity():
    """More faces, fewer, more than ever (a reallocation), fewer, more: nothing below n (or n - 1) is left from a mesh before."""
    t = _tracer()
    for name in ("soup_4097", "soup_255", "soup_12289", "soup_2049", "soup_1", "soup_4097"):
        faces, verts = bvh_cases.make(name)
        t.update_mesh(_dev(faces), _dev(verts))
        _hold(t.tree_arrays(), faces, verts, _ref(name))
        _update(t, verts, f64=True)
        _hold(t.tree_arrays(), faces, verts, _ref(name), flat_order=_ref(name)["order"])


@pytest.mark.parametrize("name", ["quads", "soup_2049"])
def test_kept_topology_refits_and_rebuilds_every_third_update(hostsim, name):
    """Tree mode 1, every = 3.  Two kept updates: order, links, ranges (and the stale keys) are the first build's; boxes, records,
    padding, margin and wide nodes are the restatement's refit and collapse of that topology with the new vertices.  The third
    update is a full build again."""
    faces, v0 = bvh_cases.make(name)
    rng = np.random.default_rng(5)
    t = _tracer(1, 3)
    t.update_mesh(_dev(faces), _dev(v0))
    first = t.tree_arrays()
    _hold(first, faces, v0, _ref(name), bvh_cases.host_tree(hostsim, name))
    for k in range(2):
        verts = (v0[:, [1, 2, 0]] * np.float32(0.5 + k) + rng.standard_normal(v0.shape).astype(np.float32)).astype(np.float32)
        _update(t, verts, f64=k == 1)
        tree = t.tree_arrays()
        for kept in ("keys", "order", "parent_inner", "parent_leaf", "range_lo", "range_hi"):
            assert bvh_ref.same(tree[kept], first[kept]), kept
        want = bvh_ref.refit_on({f: first[f] for f in ("keys", "order", "nodes", "parent_inner", "parent_leaf", "range_lo", "range_hi")}, faces, verts,
                                flat_order=first["order"])
        assert bvh_ref.same(tree["params"], bvh_ref.params(verts))
        _hold(tree, faces, verts, want)
    verts = np.ascontiguousarray(v0 @ np.array([[1, 0.3, 0], [0.5, 0.2, 0], [0, 0.4, 3]], np.float32))       # sheared: other keys
    _update(t, verts, f64=False)
    ref = bvh_ref.build(faces, verts)
    assert bvh_ref.differing(ref, _ref(name), ["order"]) == ["order"]               # (an update the first order does not survive)
    _hold(t.tree_arrays(), faces, verts, ref, bvh_cases.hostsim_tree(hostsim, faces, verts, bvh_ref.drop_bits(len(faces))), flat_order=first["order"])


@pytest.mark.parametrize("name", ["soup_1", "soup_2", "soup_257", "hand"])
def test_host_built_topology_is_sound_and_refitted(name):
    """Tree mode 2: the host's binned-SAH split is not restated, but its tree must be a tree, and on it the boxes, records and wide
    nodes are the restatement's refit and collapse -- at update_mesh and after updates by either path.  (The projection pass's
    records follow the tree's own order here: the host installs it before the records are written.)"""
    faces, v0 = bvh_cases.make(name)
    t = _tracer(2)
    t.update_mesh(_dev(faces), _dev(v0))
    first = t.tree_arrays()
    for k, verts in enumerate((v0, v0 * np.float32(0.25) - np.float32(3), v0[:, [1, 2, 0]])):
        verts = np.ascontiguousarray(verts, np.float32)
        if k:
            _update(t, verts, f64=k == 2)
        tree = t.tree_arrays()
        assert bvh_ref.check_topology(tree, len(faces)) == []
        for kept in ("order", "parent_inner", "parent_leaf", "range_lo", "range_hi"):
            assert bvh_ref.same(tree[kept], first[kept]), kept
        want = bvh_ref.refit_on({f: first[f] for f in ("order", "nodes", "parent_inner", "parent_leaf", "range_lo", "range_hi")}, faces, verts,
                                flat_order=first["order"])
        _hold(tree, faces, verts, want)


@pytest.mark.parametrize("name", ["hand", "three_keys"])
def test_two_builds_of_one_input_are_byte_identical(name):
    faces, verts = bvh_cases.make(name)
    trees = []
    for _ in range(2):
        t = _tracer()
        t.update_mesh(_dev(faces), _dev(verts))
        _update(t, verts, f64=True)
        trees.append(t.tree_arrays())
    for k in bvh_ref.ARRAYS[:-1]:
        assert trees[0][k].tobytes() == trees[1][k].tobytes(), k
    assert all(trees[0]["params"][f].tobytes() == trees[1]["params"][f].tobytes() for f in bvh_ref.PARAMS.names)      # (not the struct's padding)


def test_export_rejects_a_wrong_size_and_an_unbuilt_scene():
    from drt_amd import _lib
    faces, verts = bvh_cases.make("soup_65")
    t = _tracer()
    lib, stream = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.full((1 << 14,), 0xAB, dtype=torch.uint8, device="cuda")
    for what in range(12):
        assert lib.drt_bvh_export(t._h, what, buf.data_ptr(), 0, stream) != 0       # no mesh yet
    t.update_mesh(_dev(faces), _dev(verts))
    sizes = [4 * 65, 4 * 65, 64 * 64, 4 * 64, 4 * 65, 4 * 64, 4 * 64, 64 * 64, 48 * 65, 48 * 65, 4 * 65, 100]
    for what, size in enumerate(sizes):
        for wrong in (size - 4, size + 4, 0):
            assert lib.drt_bvh_export(t._h, what, buf.data_ptr(), wrong, stream) != 0
            assert b"bytes" in lib.drt_last_error()
    assert lib.drt_bvh_export(t._h, 12, buf.data_ptr(), 4, stream) != 0 and lib.drt_bvh_export(t._h, -1, buf.data_ptr(), 4, stream) != 0
    assert lib.drt_bvh_export(t._h, 0, None, sizes[0], stream) != 0
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())                                                # nothing was written
    for what, size in enumerate(sizes):
        assert lib.drt_bvh_export(t._h, what, buf.data_ptr(), size, stream) == 0
    empty = _tracer()
    empty.update_mesh(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), torch.zeros((0, 3), dtype=torch.float32, device="cuda"))
    assert [len(empty.tree_arrays()[k]) for k in bvh_ref.ARRAYS[:-1]] == [0] * 11
