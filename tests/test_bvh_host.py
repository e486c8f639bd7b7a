"""The BVH build of the project's headers (tests/hostsim, with the low key bits dropped as the device drops them) against the numpy
restatement tests/bvh_ref.py, array by array, over the corpus of tests/bvh_cases.py.  tests/test_gpu_bvh_build.py holds the device
to both."""
import numpy as np
import pytest

import bvh_cases
import bvh_ref

# The most grid steps a quantised bound byte of hostsim's wide nodes can move inwards and stay conservative, over the whole corpus
# (test_quantised_bounds_are_not_loose prints the figure per case).  See that test's docstring for why it is not 0.
MAX_SLACK = 1


def _ref(name, _cache={}):
    if name not in _cache:
        faces, verts = bvh_cases.make(name)
        _cache[name] = bvh_ref.build(faces, verts, upto="order" if name in bvh_cases.LARGE else "all")
    return _cache[name]


def quant_report(tree, faces, verts):
    """(violations, slack) of the wide nodes of an export, against the boxes of its own order, ranges and BuildParams (which the
    caller has compared or checked)."""
    leaf = bvh_ref.leaf_boxes(faces, verts, tree["order"], tree["params"]["pad"])
    box, used = bvh_ref.wide_slot_boxes(tree["wide"], tree["range_lo"], tree["range_hi"], leaf)
    written = np.r_[True, (tree["range_hi"] > tree["range_lo"])[1:]]
    return bvh_ref.quant_report(tree["wide"], box, used, written)


def test_layouts_are_the_librarys():
    from drt_amd.optix_mesh import optix_mesh
    assert bvh_ref.ARRAYS == optix_mesh.TREE_ARRAYS
    for mine, theirs, size in ((bvh_ref.NODE, optix_mesh.NODE_DTYPE, 64), (bvh_ref.NODE4Q, optix_mesh.NODE4Q_DTYPE, 64),
                               (bvh_ref.TRIREC, optix_mesh.TRIREC_DTYPE, 48), (bvh_ref.PARAMS, optix_mesh.PARAMS_DTYPE, 100)):
        assert mine == np.dtype(theirs) and mine.itemsize == size


def test_corpus_holds_what_it_promises():
    """The cases are what their names say, judged by the restatement's own keys."""
    for name in bvh_cases.SMALL:
        faces, verts = bvh_cases.make(name)
        assert faces.min() >= 0 and faces.max() < len(verts)
    key = lambda name, drop: bvh_ref.keys(*bvh_cases.make(name), bvh_ref.params(bvh_cases.make(name)[1]), drop)
    assert len(np.unique(key("copies_5000", 0))) == 1
    k, c = np.unique(key("three_keys", 6), return_counts=True)
    assert len(k) == 3 and c.min() > bvh_ref.SORT_TILE
    k = key("drop_bits", 0).reshape(-1, 64)
    assert np.all((k >> 6) == (k[:, :1] >> 6)) and all(len(np.unique(g)) == 64 for g in k) and np.any(np.diff(k.astype(np.int64), axis=1) < 0)
    k = key("quads", 0).reshape(-1, 2)
    assert np.all(k[:, 0] == k[:, 1]) and len(np.unique(k)) > len(k) // 2
    assert bvh_ref.params(bvh_cases.make("flat_z")[1])["inv"][2] == 0
    p = bvh_ref.params(bvh_cases.make("needle")[1])
    assert list(p["bits"]) == [20, 5, 5] and p["inv"][1] / p["inv"][0] >= 2 ** 21
    p = bvh_ref.params(bvh_cases.make("point")[1])
    assert not p["inv"].any() and p["pad"] == 0
    faces, verts = bvh_cases.make("cell_edges")
    p = bvh_ref.params(verts)
    t = (np.float32(0.5) * (verts[faces].min(1) + verts[faces].max(1)) - p["lo"]) * p["inv"] * 1024
    assert np.all(t == np.floor(t)) and np.any(np.all(t == 1024, 1)) and key("cell_edges", 0).max() == 2 ** 30 - 1
    assert [len(bvh_cases.make("verts_mod%d" % k)[1]) % 4 for k in range(4)] == [0, 1, 2, 3]
    for name in ("outliers", "verts_mod0", "verts_mod1", "verts_mod2", "verts_mod3"):
        faces, verts = bvh_cases.make(name)
        used = verts[np.unique(faces)]
        assert np.any(verts.min(0) < used.min(0)) or np.any(verts.max(0) > used.max(0))     # unreferenced vertices widen the box
    assert bvh_cases.make("all_negative")[1].max() < 0 and bvh_cases.make("mixed_sign")[1].min() < 0 < bvh_cases.make("mixed_sign")[1].max()
    assert [bvh_ref.drop_bits(n) for n in (1, 262144, 262145)] == [6, 6, 0]


@pytest.mark.parametrize("name", bvh_cases.SMALL)
def test_hostsim_equals_restatement(hostsim, name):
    faces, verts = bvh_cases.make(name)
    host, ref = bvh_cases.host_tree(hostsim, name), _ref(name)
    assert bvh_ref.differing(host, ref) == []
    assert bvh_ref.check_topology(host, len(faces)) == []
    assert bvh_ref.check_topology(ref, len(faces)) == []
    # the float boxes the restatement's collapse put into the slots are the boxes of what the slots cover
    box, used = bvh_ref.wide_slot_boxes(host["wide"], host["range_lo"], host["range_hi"], ref["leaf"])
    assert bvh_ref.same(box[ref["wide_written"]][used[ref["wide_written"]]], ref["wide_box"][ref["wide_written"]][used[ref["wide_written"]]])
    bad, slack = bvh_ref.quant_report(host["wide"], ref["wide_box"], used, ref["wide_written"])
    assert bad == 0 and slack <= MAX_SLACK


@pytest.mark.parametrize("name", bvh_cases.LARGE)
def test_hostsim_equals_restatement_at_the_sort_switch(hostsim, name):
    faces, verts = bvh_cases.make(name)
    host, ref = bvh_cases.host_tree(hostsim, name), _ref(name)
    assert bvh_ref.differing(host, ref, ["params", "keys", "order"]) == []
    assert bvh_ref.check_topology(host, len(faces)) == []
    bad, slack = _host_quant(hostsim, name)
    assert bad == 0 and slack <= MAX_SLACK


def _host_quant(hostsim, name, _cache={}):
    if name not in _cache:
        _cache[name] = quant_report(bvh_cases.host_tree(hostsim, name), *bvh_cases.make(name))
    return _cache[name]


def test_quantised_bounds_are_not_loose(hostsim, capsys):
    """Slack of hostsim's bound bytes over the whole corpus: the observed maximum is 1 grid step (MAX_SLACK).

    Not 0 because quantize_axis finds a byte as floor((lo - o) / s) in float32 and then only ever moves it OUTWARDS until the decoded
    bound is conservative: when the rounded quotient lands just below an integer the true quotient reaches, the byte starts one step
    further out than needed and nothing moves it back.  The quotient's relative error is a few 2^-24 and the bytes are below 2^8, so
    the start can be off by one step at most, never two."""
    worst = {}
    for name in bvh_cases.ALL:
        bad, worst[name] = _host_quant(hostsim, name)
        assert bad == 0, name
    with capsys.disabled():
        print("\nslack per case:", worst)
    assert max(worst.values()) <= MAX_SLACK


def test_restatement_catches_what_the_soundness_checks_do_not():
    """check_topology and the comparison are not vacuous: small defects in a copy of a sound tree are reported."""
    faces, verts = bvh_cases.make("soup_257")
    ref = _ref("soup_257")
    assert bvh_ref.check_topology(ref, len(faces)) == []
    for field, where, value in (("parent_inner", 5, 0), ("parent_leaf", 9, 3), ("range_hi", 7, 256), ("order", 3, 4)):
        broken = dict(ref)
        broken[field] = ref[field].copy()
        broken[field][where] = value
        assert bvh_ref.check_topology(broken, len(faces)) != [], field
    broken = dict(ref, nodes=ref["nodes"].copy())
    broken["nodes"]["child0"][11] = broken["nodes"]["child1"][11]
    assert bvh_ref.check_topology(broken, len(faces)) != []
    # a stable sort of other keys, an order that is only "a permutation"
    other = bvh_ref.build(*bvh_cases.make("drop_bits"), drop=0)
    assert bvh_ref.differing(other, _ref("drop_bits"), ["keys", "order", "slot_of_face"]) == ["keys", "order", "slot_of_face"]
    assert bvh_ref.differing(dict(ref, order=ref["order"][::-1].copy()), ref, ["order"]) == ["order"]
    # fma32 rounds once: 1 + 2^-24 + 2^-60 lies above the tie that float64 rounds it onto
    assert bvh_ref.fma32(1, np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1.0)) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert bvh_ref.fma32(1, np.float32(2.0 ** -24), np.float32(1.0)) == np.float32(1.0)
