"""k_raster (drt_raster.hip) as a loop of persistent waves over RUNS -- (image, 64 consecutive triangles), image-major; the grid is
what is resident and wave v of V takes runs v, v + V, ... on its own 4 KB slice of the block's LDS, with no block barrier.  The shapes
are the smallest at which that loop can go wrong, not the workload's.

Reference: a scene created under DRT_RASTER=0 -- every primary ray through the tree, no projection pass -- whose mask, out_ori, out_dir
and primary face ids every call here must give bit for bit, and whose second face ids it must give wherever the mask is set (that is
where a call defines them); the smallest case is also held against the CPU oracle (exhaustive test) at test_gpu_cull_direct.py's
tolerances.  Every scene gets an establishing call and a trusted one: both run the projection pass on the same workspace.

The fans are open surfaces (a closed mesh has an even number of triangles; the run edges want 1, 63, 65 and 257): their scenes are
created without edge tables, which only the silhouette and smoothness terms read.

Tried against wrong builds of the kernel, see profiles/raster_runs.txt section 7."""
import numpy as np
import pytest
import torch

import test_gpu_cull_batch as cb
import test_gpu_cull_direct as base
from test_gpu_cull_direct import Render  # noqa: F401  (the fixture)
from drt_amd import mesh_io, views

pytestmark = pytest.mark.gpu

PAIR = base.IOR_PAIRS["default"]
_refs = {}


def _fan(n):
    """n triangles around an apex at the origin, rim on a wavy circle: visible from every turntable camera, Morton-sorted into ceil(n / 64) runs."""
    th = 2.0 * np.pi * np.arange(n + 1) / (n + 1)
    rim = np.stack([40.0 * np.cos(th), 40.0 * np.sin(th), 18.0 + 12.0 * np.sin(3.0 * th)], 1)
    verts = np.concatenate([np.zeros((1, 3)), rim])
    faces = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 2 + np.arange(n)], 1)
    return mesh_io.TriMesh(verts, faces)


def _mesh(name):
    kind, n = name.split("-")
    return _fan(int(n)) if kind == "fan" else mesh_io.icosphere(int(n), radius=50.0, noise=0.05, seed=3)


def _rays(mesh, w, h, n_views, dist, n_cams=72):
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, n_cams, w, h, distance_factor=dist)
    ids = [(5 + 24 * k) % n_cams for k in range(n_views)] if n_cams == 72 else list(range(n_views))
    r = [views.generate_ray(h, w, cams[k][3], cams[k][2]) for k in ids]
    return torch.cat([x[0] for x in r]).contiguous(), torch.cat([x[1] for x in r]).contiguous()


def _scene(Render, monkeypatch, mesh, **kw):
    """base._make_scene for a mesh that may be open: no edge tables (and so no watertightness assert) while the scene is created."""
    with monkeypatch.context() as m:
        m.setattr(Render.Scene, "init_edge", lambda self: None)
        return base._make_scene(Render, monkeypatch, mesh, **kw)


def _tree(Render, monkeypatch, mesh, V, og, dg):
    """One call on a scene without the projection pass: (out_ori, out_dir, mask, face1, face2)."""
    tree = _scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    tree.update_verticex(V)
    with torch.no_grad():
        return cb._record(tree, tree.render_transparent(og.clone(), dg.clone()))


def _same(rec, want):
    for k in range(4):                                     # out_ori, out_dir, mask, primary face ids: everywhere
        assert torch.equal(rec[k], want[k]), k
    m = want[2][:, 0]
    assert torch.equal(rec[4][m], want[4][m])


def _two_calls(Render, scene, og, dg, want):
    """The establishing call and a trusted one on the same tensors; both ran the projection pass, each result is the tree's."""
    with torch.no_grad():
        for k in range(2):
            before = scene.optix_mesh.route_counts()
            got = scene.render_transparent(og, dg)
            rose = base._rose(scene, before)
            assert rose["total"] >= 1 and rose["raster" if k == 0 else "trust"] == rose["total"], (k, rose)
            rec = cb._record(scene, got)
            del got
            _same(rec, want)


# ---- triangle counts at the run edges; more waves than runs ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fan-1", "fan-63", "fan-64", "fan-65", "fan-257", "ico-0", "ico-1", "ico-2"])
def test_triangle_counts_at_the_run_edges(Render, monkeypatch, name):
    """One run that is not full, exactly full, one triangle into the second, four and a bit; 1 and 3 images of 64x4, 128x8 and 64x64:
    far fewer runs than waves, so most waves have nothing to do, and the last run of an image ends inside a wave."""
    mesh = _mesh(name)
    Render.intIOR, Render.extIOR = PAIR
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    tree = _scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    tree.update_verticex(V)
    scene = _scene(Render, monkeypatch, mesh)
    scene.update_verticex(V)
    hits = 0
    for w, h in ((64, 4), (128, 8), (64, 64)):
        for n_views in (1, 3):
            Render.resx, Render.resy = w, h
            o, d = _rays(mesh, w, h, n_views, 1.2)
            og, dg = o.cuda(), d.cuda()
            with torch.no_grad():
                want = cb._record(tree, tree.render_transparent(og.clone(), dg.clone()))
            _two_calls(Render, scene, og, dg, want)
            hits += int((want[3] >= 0).sum())
            if name == "fan-1" and (w, h, n_views) == (64, 4, 1):      # the smallest case: also the exhaustive test of the CPU oracle
                sp, valid, wgt = base._targets(mesh, len(o), 3)
                ref = base._oracle(mesh, mesh.vertices, o, d, PAIR, sp, valid, wgt)
                with torch.no_grad():
                    out = scene.render_transparent(og, dg)
                base._close_to_oracle(scene, *out, ref)
                assert int((ref["f1"] >= 0).sum()) >= 1
    assert hits >= 20


# ---- more runs than resident waves: waves go round the loop; an image that is no grid in the middle of the runs -------------------------
def _many_runs(perturbed):
    """icosphere(4): 5 120 triangles, 80 runs an image; 128 images of 64x8 pixels: 10 240 runs, 65 536 rays."""
    if "ico4" not in _refs:
        _refs["ico4"] = mesh_io.icosphere(4, radius=50.0, noise=0.02, seed=5)
    mesh = _refs["ico4"]
    key = ("rays", perturbed)
    if key not in _refs:
        o, d = _rays(mesh, 64, 8, 128, 1.3, n_cams=128)
        if perturbed is not None:                          # one row of one image looks elsewhere: the 8x8 lattice of an 8-row image has a ray in every row
            P, row = 64 * 8, 3
            a = perturbed * P + row * 64
            d[a:a + 64] = torch.nn.functional.normalize(d[a:a + 64] + torch.tensor([0.0, 0.02, 0.01], dtype=torch.float64), dim=1)
        _refs[key] = (o, d)
    return mesh, _refs[key]


@pytest.mark.parametrize("perturbed", [None, 77], ids=["all-grids", "image-77-no-grid"])
def test_more_runs_than_resident_waves(Render, monkeypatch, perturbed):
    mesh, (o, d) = _many_runs(perturbed)
    assert 128 * ((len(mesh.faces) + 63) // 64) > 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count      # runs > waves
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 8
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = cb._plain(Render, monkeypatch, mesh, V, og, dg)
    P = 64 * 8
    per_image = (want[3] >= 0).view(128, P).sum(1)
    assert int(per_image.min()) >= 20                     # every image sees the sphere: the runs behind the first 8 192 (a wave's second) matter
    scene = base._make_scene(Render, monkeypatch, mesh)
    scene.update_verticex(V)
    tr = scene.optix_mesh
    tr.profile_enable(1); tr.profile_read()
    _two_calls(Render, scene, og, dg, want)
    prof = tr.profile_read(); tr.profile_enable(0)
    if perturbed is None:
        assert prof["trace1"][2] == 0                      # no ray needed the tree
    else:
        assert 2 * P <= prof["trace1"][2] < 2 * 4 * P       # the rays of that image, in both calls, and of no other (its 64 x 4 patches)


# ---- a triangle for the big list among small ones of the same run -----------------------------------------------------------------------
def test_big_triangle_inside_a_run(Render, monkeypatch):
    """40 small triangles and one that covers hundreds of pixel centres of a 64x64 image, 41 triangles: ONE run per image, whose wave
    hands the large one to the big list (more than kRasterMaxPerLane = 48 centres in its box) and rasterises the others itself."""
    small = _fan(40)
    sv = small.vertices * 0.12
    big = np.array([[-45.0, -40.0, -8.0], [45.0, -40.0, -8.0], [0.0, 50.0, -8.0]])
    mesh = mesh_io.TriMesh(np.concatenate([sv, big]), np.concatenate([small.faces, [[len(sv), len(sv) + 1, len(sv) + 2]]]))
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 64
    o, d = _rays(mesh, 64, 64, 3, 1.2)
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = _tree(Render, monkeypatch, mesh, V, og, dg)
    f1 = want[3].view(3, -1)
    assert int((f1 == 40).sum(1).max()) > 48 and int(((f1 >= 0) & (f1 < 40)).sum()) >= 10
    scene = _scene(Render, monkeypatch, mesh)
    scene.update_verticex(V)
    _two_calls(Render, scene, og, dg, want)


# ---- the same call again, eager and captured: every launch starts from scratch, no key left behind ---------------------------------------
def test_repeated_and_captured_calls_leave_nothing_behind(Render, monkeypatch):
    """Big, big, small, big on the same rays (a key the large sphere's call left behind is a hit of the small one's; a launch that
    kept state of the one before -- a work counter that was not zeroed -- would skip runs), then the call captured in a graph and
    replayed twice."""
    mesh, (o, d) = _many_runs(None)
    Render.intIOR, Render.extIOR = PAIR
    Render.resx, Render.resy = 64, 8
    og, dg = o.cuda(), d.cuda()
    big = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    small = big.mean(0) + (big - big.mean(0)) / 3.0
    want = {"big": cb._plain(Render, monkeypatch, mesh, big, og, dg), "small": cb._plain(Render, monkeypatch, mesh, small, og, dg)}
    n_big, n_small = int((want["big"][3] >= 0).sum()), int((want["small"][3] >= 0).sum())
    assert n_small > 100 and n_big > 3 * n_small
    scene = base._make_scene(Render, monkeypatch, mesh)
    handle = scene.bind_rays(og, dg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for k, name in enumerate(["big", "big", "small", "big"]):
            scene.update_verticex(big if name == "big" else small)
            rec = cb._record(scene, scene.render_transparent(handle))
            _same(rec, want[name])
            assert int((rec[3] >= 0).sum()) == (n_big if name == "big" else n_small), k
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        scene.update_verticex(big)
        out = scene.render_transparent(handle)
        f1, f2 = scene.last_face1, scene.last_face2
    for k in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same([out[0], out[1], out[2], f1, f2], want["big"])
    with torch.no_grad():                                  # and the key buffer is all-empty behind the replays
        scene.update_verticex(small)
        _same(cb._record(scene, scene.render_transparent(handle)), want["small"])
