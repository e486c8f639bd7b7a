"""k_cull_listed (drt_pipeline.hip) as a batched kernel: runs of four list entries dealt by a cursor word of the sub-batch's counter
block, keys gathered tile by tile into an LDS work list, bounce #1 on dense lanes, one scan and one list reservation per run.  The
shapes are the smallest at which that logic can go wrong; every scene is created under DRT_CULL_DIRECT_MIN_LOG2=0 and every test asserts
its route from `route_counts()`, as in test_gpu_cull_direct.py, whose helpers and tolerances these tests share.

References: (1) a scene created under DRT_RASTER=0 -- every primary ray through the tree, no projection pass, no k_cull_listed -- whose
dense outputs and mask the listed route must give bit for bit, and whose face ids it must give wherever the mask is set; (2) the CPU
oracle at the tolerances of test_gpu_cull_direct.py (mask and face ids exact, out_dir rtol 1e-10 / atol 1e-11, out_ori rtol 1e-10 /
atol 1e-9, loss 1e-10 relative, gradient 1e-9 of its largest entry and 1e-5 absolute), for the dense call, the one-pass loss
(k_cull_listed<true>) and the count of contributing rays.

A run is a batch here (four patches, 1024 work-list entries at most, which is the capacity), so "the batch closes on capacity" is the
case of four patches hit in all 256 pixels: the icosphere filling 128x128 images.  An untrusted patch does not close a batch either:
cull_patch shares nothing with the work list, so the batch stays open around it (test_untrusted_image_between_trusted_ones).

Tried once against three wrong builds of the kernel: the group bits of a run cleared at the top of the run instead of behind the
barrier that ends the gather fails every test of this file and of test_gpu_cull_direct.py (a wave that reads its bit late finds it
gone and leaves its keys to the next call); so does a build that does not reset the keys it consumed; with the cursor on word [8], the
first of k_path's, test_listed_cull_in_front_of_the_one_kernel_path[sphere] fails and nothing else (k_path deals the first 64 entries
per wave statically, so only a list longer than that share ever reads its cursor -- the [hand] case and every other test pass)."""
import numpy as np
import pytest
import torch

import test_gpu_cull_direct as base
from test_gpu_cull_direct import Render  # noqa: F401  (the fixture)
from drt_amd import mesh_io, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu

PAIRS = base.IOR_PAIRS


def _record(scene, out):
    return [out[0].detach().clone(), out[1].detach().clone(), out[2].clone(), scene.last_face1.clone(), scene.last_face2.clone()]


def _plain(Render, monkeypatch, mesh, V, o, d, sp=None, valid=None):
    """One call on a scene that has no projection pass: (out_ori, out_dir, mask, face1, face2[, loss, gradient])."""
    scene = base._make_scene(Render, monkeypatch, mesh, direct=False, DRT_RASTER="0")
    Vp = V.detach().clone().requires_grad_(sp is not None)
    scene.update_verticex(Vp)
    out = scene.render_transparent(o.clone(), d.clone())
    rc = scene.optix_mesh.route_counts()
    assert rc["total"] >= 1 and rc["raster"] == 0 and rc["trust"] == 0 and rc["direct"] == 0, rc
    rec = _record(scene, out)
    if sp is not None:
        loss = Render.ray_loss(*out, sp, valid)
        loss.backward()
        rec += [loss.detach().clone(), Vp.grad.clone()]
    return rec


def _same_as_plain(rec, want):
    assert torch.equal(rec[2], want[2]) and torch.equal(rec[0], want[0]) and torch.equal(rec[1], want[1])
    m = want[2][:, 0]
    assert float(rec[0][~m].abs().sum()) == 0.0 and float(rec[1][~m].abs().sum()) == 0.0
    assert torch.equal(rec[3][m], want[3][m]) and torch.equal(rec[4][m], want[4][m])


def _case(Render, monkeypatch, mesh, w, h, o, d, pair, subs=1, valid=None, seed=21, verts=None, **env):
    """Establish, then one trusted call whose bits are the plain tree's, then the dense call, the one-pass loss and the gradients against
    the oracle -- every trusted call asserted to have run the listed cull with `direct` in each of its `subs` sub-batches."""
    Render.intIOR, Render.extIOR = pair
    Render.resx, Render.resy = w, h
    verts = mesh.vertices if verts is None else verts
    sp, valid0, wgt = base._targets(mesh, len(o), seed)
    valid = valid0 if valid is None else valid
    ref = base._oracle(mesh, verts, o, d, pair, sp, valid, wgt)
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(np.asarray(verts), dtype=torch.float64, device="cuda")
    want = _plain(Render, monkeypatch, mesh, V, og, dg)
    scene = base._make_scene(Render, monkeypatch, mesh, **env)
    scene.update_verticex(V)
    with torch.no_grad():
        before = scene.optix_mesh.route_counts()
        first = scene.render_transparent(og, dg)
        rose = base._rose(scene, before)
        assert rose["total"] == rose["raster"] == subs and rose["trust"] == 0, rose
        del first
        before = scene.optix_mesh.route_counts()
        got = scene.render_transparent(og, dg)
        rose = base._rose(scene, before)
        assert rose["total"] == rose["trust"] == rose["direct"] == subs and rose["mega"] == 0, rose
        _same_as_plain(_record(scene, got), want)
        del got
    base._dense_and_one_pass_against_oracle(Render, scene, mesh, verts, og, dg, ref, sp, valid, wgt, subs=subs)
    return ref, scene, (og, dg)


# ---- one patch, two patches, lists shorter than the grid and no multiple of the run ---------------------------------------------------
@pytest.mark.parametrize("shape", ["64x4", "64x8", "128x4", "192x12", "320x20"])
def test_short_lists(Render, monkeypatch, shape):
    """64x4: one list entry, one run, every other block finds its own run past the end.  64x8 / 128x4: two patches of one run, one above
    the other and side by side.  192x12 (9 patches) and 320x20 (25): fewer entries than blocks, lengths that are no multiple of four."""
    w, h = (int(x) for x in shape.split("x"))
    mesh = base._hand()
    o, d = base._rays(mesh, w, h, (5,), 2.5 if w > 128 else 1.2)
    pair = PAIRS["1.0_1.33"] if shape in ("64x8", "320x20") else PAIRS["default"]      # (two of them mix reflected and refracted rays in a run)
    ref, _, _ = _case(Render, monkeypatch, mesh, w, h, o, d, pair)
    hits = ref["f1"] >= 0
    assert int(hits.sum()) >= 20 and int(ref["mk"][:, 0].sum()) >= 10
    if pair[1] > pair[0]:
        assert 0 < int(ref["tir"].sum()) < int(hits.sum())
    per_patch = hits.view(h // 4, 4, w // 64, 64).permute(0, 2, 1, 3).reshape(-1, 256).sum(1)
    assert int((per_patch > 0).sum()) >= {"64x4": 1, "64x8": 2, "128x4": 2, "192x12": 3, "320x20": 3}[shape]


# ---- a run that fills the work list ---------------------------------------------------------------------------------------------------
def _sphere_case(res, ids):
    mesh = mesh_io.icosphere(2, radius=50.0, noise=0.05, seed=3)
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, 72, res, res, distance_factor=0.9)
    r = [views.generate_ray(res, res, cams[k][3], cams[k][2]) for k in ids]
    return mesh, torch.cat([x[0] for x in r]).contiguous(), torch.cat([x[1] for x in r]).contiguous()


def test_runs_of_four_full_patches_fill_the_work_list(Render, monkeypatch):
    """The icosphere filling 128x128 images: 64 patches an image, nearly all hit in all 256 pixels, so whole runs append exactly the
    1024 entries the work list holds (the last patch of the run lands on the limit) -- and, with `valid` on a checkerboard, exactly
    half of that in the one-pass form."""
    res = 128
    mesh, o, d = _sphere_case(res, (7, 43))
    om = orc.Mesh(mesh.faces, torch.tensor(mesh.vertices, dtype=torch.float64))
    hit = orc.intersect_ids(om, o, d)[1]
    dense = base._per_patch(hit, 2, res) == 256
    assert int(dense.sum()) >= 100
    runs = dense[:len(dense) // 4 * 4].view(-1, 4).all(1)           # (list order is patch order when every patch is listed)
    assert int(runs.sum()) >= 16
    yy, xx = torch.meshgrid(torch.arange(2 * res), torch.arange(res), indexing="ij")
    checker = ((yy + xx) % 2 == 0).reshape(-1)
    ref, _, _ = _case(Render, monkeypatch, mesh, res, res, o, d, PAIRS["default"], valid=checker)
    assert int(ref["mk"][:, 0].sum()) > 10000 and 0.4 < ref["n_contrib"] / int(ref["mk"][:, 0].sum()) < 0.6


def test_a_long_list_is_worked_by_every_resident_block(Render, monkeypatch):
    """Up to 16 runs per block of the two-per-CU grid only that grid works the list, from there on every resident block does: 16 images of
    768x768 filled by the icosphere list more than 2 x CUs x 4 x 16 patches in ONE sub-batch.  Bits of the plain tree (forward only: the
    oracle has no part in which block takes which run)."""
    res, ids = 768, tuple(range(2, 72, 4))[:16]
    mesh = mesh_io.icosphere(2, radius=50.0, noise=0.05, seed=3)
    Render.intIOR, Render.extIOR = PAIRS["default"]
    Render.resx = Render.resy = res
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, 72, res, res, distance_factor=0.9)
    r = [views.generate_ray(res, res, cams[k][3], cams[k][2], device="cuda") for k in ids]
    og, dg = torch.cat([x[0] for x in r]).contiguous(), torch.cat([x[1] for x in r]).contiguous()
    del r
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        want = _plain(Render, monkeypatch, mesh, V, og, dg)
        hit_patches = int((base._per_patch(want[3] >= 0, len(ids), res) > 0).sum())
        assert hit_patches >= 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4 * 16, hit_patches
        scene = base._make_scene(Render, monkeypatch, mesh, DRT_MIN_SUB_LOG2="26")
        scene.update_verticex(V)
        scene.render_transparent(og, dg)
        before = scene.optix_mesh.route_counts()
        got = scene.render_transparent(og, dg)
        rose = base._rose(scene, before)
        assert rose["total"] == rose["trust"] == rose["direct"] == 1 and rose["mega"] == 0, rose
        _same_as_plain(_record(scene, got), want)


# ---- every first bounce reflects ------------------------------------------------------------------------------------------------------
def test_every_first_bounce_reflects(Render, monkeypatch):
    """An exterior index a million times the interior one: every primary hit is reflected at bounce #1.  The hits are counted (count[17],
    read through the stage statistics), list R1 stays empty, face1 is set, the mask is zero everywhere."""
    mesh = base._hand()
    pair = (1.0, 1.0e6)
    o, d = base._rays(mesh, 64, 64, (5, 29), 1.2)
    ref, scene, (og, dg) = _case(Render, monkeypatch, mesh, 64, 64, o, d, pair, seed=22)
    hits = int((ref["f1"] >= 0).sum())
    assert hits > 2000 and int(ref["tir"].sum()) == hits and int(ref["mk"].sum()) == 0
    tr = scene.optix_mesh
    tr.profile_enable(1)
    tr.profile_read()
    before = tr.route_counts()
    with torch.no_grad():
        out = scene.render_transparent(og, dg)
    prof = tr.profile_read()
    tr.profile_enable(0)
    assert base._rose(scene, before)["direct"] == 1
    assert prof["shade1"][2] == hits and prof["trace2"][2] == 0, (prof["shade1"], prof["trace2"])
    assert int(out[2].sum()) == 0 and torch.equal(scene.last_face1.cpu().long(), ref["f1"]) and int((scene.last_face2 >= 0).sum()) == 0


# ---- an untrusted image between trusted ones ------------------------------------------------------------------------------------------
def test_untrusted_image_between_trusted_ones(Render, monkeypatch):
    """Three 64x64 images in one ray tensor; one ray of the MIDDLE one is overwritten, so its verdict falls and its 16 listed patches -- the
    general per-ray path, outside any batch -- come between the other images' patches in the list, inside the blocks' runs."""
    mesh, o, d, _, _ = base._tir_case(Render)
    o, d = o.clone(), d.clone()
    pair = PAIRS["1.0_1.33"]
    scene = base._make_scene(Render, monkeypatch, mesh)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    scene.update_verticex(V)
    with torch.no_grad():
        for _ in range(2):
            scene.render_transparent(o, d)
    assert d._drt_grid[3][0] is True
    at = 4096 + 32 * 64 + 30
    d[at] = d[4096 + 30 * 64 + 20].clone()
    sp, valid, wgt = base._targets(mesh, len(o), 23)
    ref = base._oracle(mesh, mesh.vertices, o.cpu(), d.cpu(), pair, sp, valid, wgt)
    for k in range(3):
        assert int(ref["tir"][k * 4096:(k + 1) * 4096].sum()) >= 20 and int(ref["mk"][k * 4096:(k + 1) * 4096, 0].sum()) >= 40
    want = _plain(Render, monkeypatch, mesh, V, o, d)
    with torch.no_grad():
        before = scene.optix_mesh.route_counts()
        again = scene.render_transparent(o, d)             # the write bumped the version: this call establishes again
        assert base._rose(scene, before)["direct"] == 0
        base._close_to_oracle(scene, *again, ref)
        del again
        assert d._drt_grid[3][0] is None
        before = scene.optix_mesh.route_counts()
        got = scene.render_transparent(o, d)
        rose = base._rose(scene, before)
        assert rose["total"] == rose["trust"] == rose["direct"] == 1 and rose["tree_late"] == 0, rose
        _same_as_plain(_record(scene, got), want)
        del got
    assert d._drt_grid[3][0] is False
    base._dense_and_one_pass_against_oracle(Render, scene, mesh, mesh.vertices, o, d, ref, sp, valid, wgt, all_verified=False)


# ---- keys and group bits are consumed -------------------------------------------------------------------------------------------------
def test_no_key_or_group_bit_survives_a_call(Render, monkeypatch):
    """A call on the mesh, then one on the mesh shrunk to a third about its centroid, on the same rays: a key or a group bit the first
    call left behind is a primary hit (or a listed patch) of the second.  Then the other way round."""
    mesh = base._hand()
    Render.intIOR, Render.extIOR = PAIRS["default"]
    Render.resx, Render.resy = 128, 64
    o, d = base._rays(mesh, 128, 64, (41, 17), 1.2)
    og, dg = o.cuda(), d.cuda()
    big = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    small = big.mean(0) + (big - big.mean(0)) / 3.0
    want = {"big": _plain(Render, monkeypatch, mesh, big, og, dg), "small": _plain(Render, monkeypatch, mesh, small, og, dg)}
    n_big, n_small = int((want["big"][3] >= 0).sum()), int((want["small"][3] >= 0).sum())
    assert n_small > 100 and n_big > 3 * n_small
    scene = base._make_scene(Render, monkeypatch, mesh)
    with torch.no_grad():
        for k, name in enumerate(["big", "big", "small", "big", "small", "small", "big"]):
            scene.update_verticex(big if name == "big" else small)
            before = scene.optix_mesh.route_counts()
            got = scene.render_transparent(og, dg)
            rose = base._rose(scene, before)
            assert rose["direct"] == int(k >= 1) and rose["total"] == 1, (k, rose)
            rec = _record(scene, got)
            del got
            _same_as_plain(rec, want[name])
            assert int((rec[3] >= 0).sum()) == (n_big if name == "big" else n_small), k      # face1 is dense: no hit where the plain tree has none


# ---- sub-batches: two on two streams, six on two streams ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [2, 6])
def test_each_sub_batch_has_its_own_cursor(Render, monkeypatch, n_views):
    """One 64x64 image a sub-batch: two run side by side on the two internal streams, each with the cursor of its own counter block;
    with six, a stream's counter block -- and its cursor -- is used three times in one call, zeroed in front of each."""
    mesh = base._hand()
    ids = (5, 17, 29, 41, 53, 65)[:n_views]
    o, d = base._rays(mesh, 64, 64, ids, 1.2)
    ref, _, _ = _case(Render, monkeypatch, mesh, 64, 64, o, d, PAIRS["1.2_1.5"], subs=n_views, seed=24,
                      DRT_MIN_SUB_LOG2="12", DRT_SUB_PER_STREAM="3")
    for k in range(n_views):
        assert int(ref["mk"][k * 4096:(k + 1) * 4096, 0].sum()) >= 100


# ---- the listed cull in front of the one-kernel path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hand", "sphere"])
def test_listed_cull_in_front_of_the_one_kernel_path(Render, monkeypatch, case):
    """DRT_MEGA_MAX_LOG2: the sub-batch's back half is k_path, whose cursors are words [8..15] of the counter block the listed cull (not
    `direct` on this route: list R0, faces and all) takes its runs from.  k_path hands out the first 64 entries per wave statically and
    only the rest through its cursors: the sphere filling one 768x768 image lists more refracted rays (over half a million) than that
    static share of any grid the kernel can have (8 blocks per CU), the two small images of the hand far fewer."""
    if case == "hand":
        mesh, (w, h), pair = base._hand(), (128, 64), PAIRS["1.0_1.33"]
        o, d = base._rays(mesh, w, h, (41, 17), 1.2)
    else:
        mesh, o, d = _sphere_case(768, (7,))
        (w, h), pair = (768, 768), PAIRS["default"]
    Render.intIOR, Render.extIOR = pair
    Render.resx, Render.resy = w, h
    sp, valid, wgt = base._targets(mesh, len(o), 25)
    ref = base._oracle(mesh, mesh.vertices, o, d, pair, sp, valid, wgt)
    if case == "hand":
        assert int(ref["tir"].sum()) >= 100 and int(ref["mk"][:, 0].sum()) >= 1000
    else:
        assert int((ref["f1"] >= 0).sum()) > 64 * 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count
    og, dg, spg, vg, wg = o.cuda(), d.cuda(), sp.cuda(), valid.cuda(), wgt.cuda()
    V0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = _plain(Render, monkeypatch, mesh, V0, og, dg)
    scene = base._make_scene(Render, monkeypatch, mesh, DRT_MEGA_MAX_LOG2="20")
    scene.update_verticex(V0)
    with torch.no_grad():
        scene.render_transparent(og, dg)
    for _ in range(2):
        V = V0.clone().requires_grad_(True)
        scene.update_verticex(V)
        before = scene.optix_mesh.route_counts()
        out_ori, out_dir, mask = scene.render_transparent(og, dg)
        rose = base._rose(scene, before)
        assert rose["total"] == rose["trust"] == rose["mega"] == 1 and rose["direct"] == 0, rose
        base._close_to_oracle(scene, out_ori, out_dir, mask, ref)
        _same_as_plain(_record(scene, (out_ori, out_dir, mask)), want)
        loss = Render.ray_loss(out_ori, out_dir, mask, spg, vg)
        assert loss.item() == pytest.approx(ref["loss"], rel=1e-10, abs=1e-12)
        (loss + (out_dir * wg).sum() + (out_ori * wg).sum()).backward()
        base._grad_close(V.grad, ref["g_all"])
        del out_ori, out_dir, mask, loss
    V2 = V0.clone().requires_grad_(True)
    scene.update_verticex(V2)
    before = scene.optix_mesh.route_counts()
    lf = scene.ray_loss_fused(og, dg, spg, vg)
    rose = base._rose(scene, before)
    assert rose["trust"] == rose["mega"] == 1 and rose["direct"] == 0, rose
    assert lf.item() == pytest.approx(ref["loss"], rel=1e-10, abs=1e-12)
    lf.backward()
    base._grad_close(V2.grad, ref["g_loss"])


# ---- a captured call ------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_the_eager_bits(Render, monkeypatch):
    """The cursor is zeroed by the memset of the counter block in front of the sub-batch, which is captured with the call: every replay
    deals the runs from zero again.  A replay that started from the last value would visit no patch and leave every key where it is."""
    mesh = base._hand()
    Render.intIOR, Render.extIOR = PAIRS["1.0_1.33"]
    Render.resx, Render.resy = 128, 64
    o, d = base._rays(mesh, 128, 64, (41, 17), 1.2)
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    want = _plain(Render, monkeypatch, mesh, V, og, dg)
    scene = base._make_scene(Render, monkeypatch, mesh)
    handle = scene.bind_rays(og, dg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for k in range(3):
            scene.update_verticex(V)
            before = scene.optix_mesh.route_counts()
            eager = _record(scene, scene.render_transparent(handle))
            assert base._rose(scene, before)["direct"] == int(k >= 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same_as_plain(eager, want)
    graph = torch.cuda.CUDAGraph()
    before = scene.optix_mesh.route_counts()
    with torch.cuda.graph(graph), torch.no_grad():
        scene.update_verticex(V)
        out = scene.render_transparent(handle)
        f1, f2 = scene.last_face1, scene.last_face2
    rose = base._rose(scene, before)
    assert rose["total"] == rose["trust"] == rose["direct"] == 1, rose
    for k in range(3):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        rec = [out[0], out[1], out[2], f1, f2]
        _same_as_plain(rec, eager)
        assert torch.equal(f1, eager[3]) and torch.equal(f2, eager[4]), k


# ---- deterministic accumulation -------------------------------------------------------------------------------------------------------
def test_deterministic_loss_and_gradient_equal_the_plain_tree(Render, monkeypatch):
    """DRT_DETERMINISTIC sums in fixed point: the order of list R1, which this kernel decides, cannot move a bit of loss or gradient."""
    from drt_amd import det
    mesh = base._hand()
    Render.intIOR, Render.extIOR = PAIRS["1.0_1.33"]
    Render.resx, Render.resy = 128, 64
    o, d = base._rays(mesh, 128, 64, (41, 17), 1.2)
    og, dg = o.cuda(), d.cuda()
    sp, valid, _ = base._targets(mesh, len(o), 26)
    spg, vg = sp.cuda(), valid.cuda()
    V0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    was = det.enable(True)
    try:
        want = _plain(Render, monkeypatch, mesh, V0, og, dg, spg, vg)
        assert int(want[2][:, 0].sum()) >= 1000 and float(want[6].abs().max()) > 0
        scene = base._make_scene(Render, monkeypatch, mesh)
        for k in range(3):
            V = V0.clone().requires_grad_(True)
            scene.update_verticex(V)
            before = scene.optix_mesh.route_counts()
            out = scene.render_transparent(og, dg)
            assert base._rose(scene, before)["direct"] == int(k >= 1)
            rec = _record(scene, out)
            loss = Render.ray_loss(*out, spg, vg)
            loss.backward()
            _same_as_plain(rec, want)
            assert torch.equal(loss.detach(), want[5]) and torch.equal(V.grad, want[6]), k
            del out, loss
    finally:
        det.enable(was)
