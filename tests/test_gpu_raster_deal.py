"""k_raster (drt_raster.hip) with its runs dealt by the previous call's test counts: from the second call on the same rays a wave takes a
contiguous range of runs from a table (k_raster_deal), heavy runs are cut between waves, and what happens once per run is left to the
run's owner.  Whatever the table holds, the keys are the static deal's.

Reference: a scene created under DRT_RASTER=0 -- every primary ray through the tree, no projection pass -- whose mask, out_ori, out_dir
and primary face ids every call here gives bit for bit, and whose second face ids it gives wherever the mask is set.  Every case makes at
least three calls on the same tensors (establishing, trusted, trusted with a table) and asserts through drt_raster_deal_counts which deal
the launches took: two k_raster launches per call, the third and later ones from a table.

Built on the helpers of test_gpu_raster_runs.py; the shapes are the smallest at which the table's paths are taken.  Tried against wrong
builds of the kernel, see profiles/raster_deal.txt section 7."""
import numpy as np
import pytest
import torch

import test_gpu_cull_batch as cb
import test_gpu_cull_direct as base
import test_gpu_raster_runs as rr
from test_gpu_cull_direct import Render  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

PAIR = base.IOR_PAIRS["default"]
DEAL = {"DRT_RASTER_DEAL_MIN_RUNS": "0"}                   # the library deals launches of 16 384 runs and more by a table: here every launch
_same, _scene, _tree, _rays, _mesh = rr._same, rr._scene, rr._tree, rr._rays, rr._mesh


def _call(scene, og, dg, want, deal):
    """One call, its bits the tree's; `deal`: "table", "static" or None (either) -- what both k_raster launches of the call must have taken."""
    tr = scene.optix_mesh
    before = tr.raster_deal_counts()
    with torch.no_grad():
        rec = cb._record(scene, scene.render_transparent(og, dg))
    now = tr.raster_deal_counts()
    rose = (now[0] - before[0], now[1] - before[1])
    assert sum(rose) == 2, rose                            # one sub-batch: one launch per facing
    if deal is not None:
        assert rose == ((2, 0) if deal == "table" else (0, 2)), (deal, rose)
    _same(rec, want)
    return rec


def _three_calls(scene, og, dg, want, more=0):
    _call(scene, og, dg, want, "static")                   # establishing: nothing to deal by
    _call(scene, og, dg, want, None)                       # trusted (the same tensors: the table of the first call serves already)
    for _ in range(1 + more):
        _call(scene, og, dg, want, "table")


# ---- few runs on thousands of waves: every run cut into many slices, most waves with an empty range; large triangles in a shared run ------
@pytest.mark.parametrize("name", ["fan-64", "fan-65", "ico-0", "ico-1"])
def test_runs_shared_by_many_waves(Render, monkeypatch, name):
    """64x64 images: one to six runs.  The icospheres' boxes exceed kRasterMaxPerLane, so the waves that share a run all meet triangles
    that only the owner may list."""
    mesh = _mesh(name)
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 64
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    tree = _scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    tree.update_verticex(V)
    scene = _scene(Render, monkeypatch, mesh, **DEAL)
    scene.update_verticex(V)
    hits = 0
    for n_views in (1, 3):
        o, d = _rays(mesh, 64, 64, n_views, 1.2)
        og, dg = o.cuda(), d.cuda()
        with torch.no_grad():
            want = cb._record(tree, tree.render_transparent(og.clone(), dg.clone()))
        if name.startswith("ico"):
            per_face = torch.bincount(want[3][want[3] >= 0].long())
            assert int(per_face.max()) > 48                # a triangle of more than kRasterMaxPerLane pixels: on the big list
        _three_calls(scene, og, dg, want)
        hits += int((want[3] >= 0).sum())
    assert hits >= 100


# ---- more runs than waves ------------------------------------------------------------------------------------------------------------------
def test_more_runs_than_waves(Render, monkeypatch):
    """icosphere(4) on 128 images of 64x8: 10 240 runs on 8 192 waves, four calls."""
    mesh, (o, d) = rr._many_runs(None)
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 8
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = cb._plain(Render, monkeypatch, mesh, V, og, dg)
    assert int((want[3] >= 0).view(128, -1).sum(1).min()) >= 20
    scene = base._make_scene(Render, monkeypatch, mesh, **DEAL)
    scene.update_verticex(V)
    _three_calls(scene, og, dg, want, more=1)


# ---- a history that describes other vertices ---------------------------------------------------------------------------------------------
def test_stale_history(Render, monkeypatch):
    """The table exists; then the vertices turn by 90 degrees about z, shrink to 0.3, grow by 3: every call deals by the counts of the
    call before, which describe another picture -- the growth sends triangles to the big list that the history knows nothing of."""
    mesh = _mesh("ico-1")
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 64
    o, d = _rays(mesh, 64, 64, 3, 1.2)
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    tree = _scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    scene = _scene(Render, monkeypatch, mesh, **DEAL)

    def reference(verts):
        tree.update_verticex(verts)
        with torch.no_grad():
            return cb._record(tree, tree.render_transparent(og.clone(), dg.clone()))

    scene.update_verticex(V)
    _three_calls(scene, og, dg, reference(V))
    c = V.mean(0)
    rot = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    turned = c + (V - c) @ rot.T
    small = c + (turned - c) * 0.3
    grown = c + (small - c) * 3.0
    sizes = []
    for verts in (turned, small, grown):
        want = reference(verts)
        scene.update_verticex(verts)
        _call(scene, og, dg, want, "table")
        f1 = want[3][want[3] >= 0].long()
        sizes.append(int(torch.bincount(f1).max()) if len(f1) else 0)
    print("largest face, pixels hit:", sizes)
    assert sizes[1] <= 24 and sizes[2] > 24, sizes         # pixels HIT; a box holds about twice as many centres: none above kRasterMaxPerLane = 48 in the shrunk picture, some in the grown one


# ---- a table describes one launch ------------------------------------------------------------------------------------------------------------
def test_tag_mismatch_deals_statically(Render, monkeypatch):
    """(64x4, 1 image) and (128x8, 3 images) in turn on one scene, one workspace: every switch is a static launch, the repeat of a
    shape a table launch."""
    mesh = _mesh("fan-65")
    Render.intIOR, Render.extIOR = PAIR
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    tree = _scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    tree.update_verticex(V)
    scene = _scene(Render, monkeypatch, mesh, **DEAL)
    scene.update_verticex(V)
    shapes = {}
    for key, (w, h, n_views) in {"a": (64, 4, 1), "b": (128, 8, 3)}.items():
        Render.resx, Render.resy = w, h
        o, d = _rays(mesh, w, h, n_views, 1.2)
        og, dg = o.cuda(), d.cuda()
        with torch.no_grad():
            shapes[key] = (w, h, og, dg, cb._record(tree, tree.render_transparent(og.clone(), dg.clone())))
    last = None
    for key in "ababaabb":
        w, h, og, dg, want = shapes[key]
        Render.resx, Render.resy = w, h
        _call(scene, og, dg, want, "table" if key == last else "static")
        last = key


# ---- a captured call ---------------------------------------------------------------------------------------------------------------------
def test_captured_call_with_a_table(Render, monkeypatch):
    """Three eager calls on bound rays, then the call captured (its launches take the table) and replayed three times -- each replay deals
    by the counts of the one before -- then an eager call."""
    mesh, (o, d) = rr._many_runs(None)
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 8
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = cb._plain(Render, monkeypatch, mesh, V, og, dg)
    scene = base._make_scene(Render, monkeypatch, mesh, **DEAL)
    tr = scene.optix_mesh
    handle = scene.bind_rays(og, dg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for k in range(3):
            scene.update_verticex(V)
            _same(cb._record(scene, scene.render_transparent(handle)), want)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert tr.raster_deal_counts() == (4, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        scene.update_verticex(V)
        out = scene.render_transparent(handle)
        f1, f2 = scene.last_face1, scene.last_face2
    assert tr.raster_deal_counts() == (6, 2)
    for k in range(3):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same([out[0], out[1], out[2], f1, f2], want)
    with torch.no_grad():
        scene.update_verticex(V)
        _same(cb._record(scene, scene.render_transparent(handle)), want)
    assert tr.raster_deal_counts() == (8, 2)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_switch_keeps_the_static_deal(Render, monkeypatch):
    mesh = _mesh("ico-1")
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 64
    o, d = _rays(mesh, 64, 64, 3, 1.2)
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = _tree(Render, monkeypatch, mesh, V, og, dg)
    scene = _scene(Render, monkeypatch, mesh, DRT_RASTER_DEAL="0", **DEAL)
    scene.update_verticex(V)
    for _ in range(3):
        _call(scene, og, dg, want, "static")
    assert scene.optix_mesh.raster_deal_counts() == (0, 6)
