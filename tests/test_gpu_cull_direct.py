"""The first bounce taken INSIDE the cull stage (drt_pipeline.hip k_cull_listed with `direct`): the route of the headline benchmark,
which a sub-batch takes only from 2^25 rays on.  Every scene here is created under DRT_CULL_DIRECT_MIN_LOG2=0, so that the trusted
calls of test-sized images take it, and every test asserts the route from `optix_mesh.route_counts()` (drt_route_counts): a knob
that did not take would otherwise leave the old route (list R0 -> k_shade1) under test.

References: the CPU oracle (oracle/diffrender_oracle.py) at the tolerances of test_gpu_fuzz's whole-path test -- mask and both face ids
exact, out_dir rtol 1e-10 / atol 1e-11, out_ori rtol 1e-10 / atol 1e-9, loss 1e-10 relative, gradient 1e-9 of its largest entry and 1e-5
absolute -- and a scene created under DRT_CULL_DIRECT=0 (bounce #1 as k_shade1's pass over list R0), whose dense outputs the direct
route must give bit for bit: both run bounce_forward on the same face with the same float64 ray.

What the cases rest on, counted by the oracle (hand_vh.ply, turntable cameras of 72; per image: primary hits / first-bounce total
internal reflections / completed paths).  (a) asserts nine tenths of these as floors, and never fewer than 4 reflections per image under
the two exterior > interior pairs and 40 completed paths per case:

  shape, views             distance   (1.4723, 1.00029)                     (1.0, 1.33)                            (1.2, 1.5)
  64x4     (5)             2.5        55/0/51                               55/7/48                                55/7/48
  64x4     (5)             1.2        114/0/102                             114/11/103                             114/8/106
  64x64    (5, 29, 53)     2.5        361/0/257 343/0/198 220/0/104         361/87/273 343/106/237 220/87/132      361/84/277 343/83/260 220/77/141
  64x64    (5, 29, 53)     1.2        1575/0/1035 1487/0/784 970/0/346      1575/416/1144 1487/535/948 970/415/549 1575/381/1183 1487/427/1056 970/385/570
  128x64   (41, 17)        2.5        1443/0/960 887/0/384                  1443/305/1137 887/293/593              1443/262/1180 887/264/618
  128x64   (41, 17)        1.2        3218/0/2656 1365/0/444                3218/504/2692 1365/788/571             3218/384/2811 1365/708/645

(b), (c), (d) use the 64x64 x 3 images at distance 2.5 under (1.0, 1.33): 280 rows that end in a reflection at bounce #1, which the
direct branch must leave as dead rows (`push = !b.tir`).  (e): six 64x64 views (5, 17, 29, 41, 53, 65) under (1.2, 1.5).  (f): icosphere(2,
radius 50, noise 0.05, seed 3), 320 faces, 768x768 at distance 0.9, views 7, 25, 43, 61: 2291, 2292, 2243, 2273 of 2304 patches hit in all
256 pixels (9099 >= 4 x 2048 blocks, 117 < 2048 others), 2295, 2300, 2253, 2280 with more than 170 hit pixels whose `valid` is set.

Tried once against three wrong builds of k_cull_listed: `push = true` instead of `push = !b.tir` fails every case with an exterior >
interior pair in (a), (b), (c), (d), (e); without the reset of the consumed key every test fails ((a): the projection pass of the next
call on the same mesh changes no key, sets no group bit, and the one-pass loss comes out 0; (b), (d): the moving sequence leaves the
oracle at call 2); a mid-loop flush that drops its entries fails (f) and nothing else."""
import numpy as np
import pytest
import torch

from conftest import IOR, data_path
from drt_amd import mesh_io, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu

EXT = 1.00029
IOR_PAIRS = {"default": (IOR, EXT), "1.0_1.33": (1.0, 1.33), "1.2_1.5": (1.2, 1.5)}
SHAPES = {"64x4": (64, 4, (5,)), "64x64x3": (64, 64, (5, 29, 53)), "128x64x2": (128, 64, (41, 17))}
# the oracle's counts of the docstring: (shape, distance, pair) -> per image (primary hits, reflections at bounce #1, completed paths)
COUNTS = {
    ("64x4", 2.5, "default"): [(55, 0, 51)], ("64x4", 2.5, "1.0_1.33"): [(55, 7, 48)], ("64x4", 2.5, "1.2_1.5"): [(55, 7, 48)],
    ("64x4", 1.2, "default"): [(114, 0, 102)], ("64x4", 1.2, "1.0_1.33"): [(114, 11, 103)], ("64x4", 1.2, "1.2_1.5"): [(114, 8, 106)],
    ("64x64x3", 2.5, "default"): [(361, 0, 257), (343, 0, 198), (220, 0, 104)],
    ("64x64x3", 2.5, "1.0_1.33"): [(361, 87, 273), (343, 106, 237), (220, 87, 132)],
    ("64x64x3", 2.5, "1.2_1.5"): [(361, 84, 277), (343, 83, 260), (220, 77, 141)],
    ("64x64x3", 1.2, "default"): [(1575, 0, 1035), (1487, 0, 784), (970, 0, 346)],
    ("64x64x3", 1.2, "1.0_1.33"): [(1575, 416, 1144), (1487, 535, 948), (970, 415, 549)],
    ("64x64x3", 1.2, "1.2_1.5"): [(1575, 381, 1183), (1487, 427, 1056), (970, 385, 570)],
    ("128x64x2", 2.5, "default"): [(1443, 0, 960), (887, 0, 384)],
    ("128x64x2", 2.5, "1.0_1.33"): [(1443, 305, 1137), (887, 293, 593)],
    ("128x64x2", 2.5, "1.2_1.5"): [(1443, 262, 1180), (887, 264, 618)],
    ("128x64x2", 1.2, "default"): [(3218, 0, 2656), (1365, 0, 444)],
    ("128x64x2", 1.2, "1.0_1.33"): [(3218, 504, 2692), (1365, 788, 571)],
    ("128x64x2", 1.2, "1.2_1.5"): [(3218, 384, 2811), (1365, 708, 645)],
}
KNOBS = ("DRT_CULL_DIRECT", "DRT_CULL_DIRECT_MIN_LOG2", "DRT_CULL_PARK", "DRT_FILL_OVERLAP", "DRT_FILL_AFTER_SHADE1", "DRT_MIN_SUB_LOG2",
         "DRT_SUB_PER_STREAM", "DRT_MEGA_MAX_LOG2", "DRT_RASTER", "DRT_STREAMS")
_SAVED = ("intIOR", "extIOR", "resx", "resy", "RECYCLE_OUTPUTS", "RECYCLE_MIN_RAYS", "PREFILL_NEXT", "PREFILL_MIN_RAYS", "HIT_SEED", "DENSE_FACE_IDS")
_cache = {}


@pytest.fixture()
def Render():
    from drt_amd import det, diffrender
    old = {k: getattr(diffrender, k) for k in _SAVED}
    assert not det.on()
    yield diffrender
    for k, v in old.items():
        setattr(diffrender, k, v)


def _hand():
    if "hand" not in _cache:
        _cache["hand"] = mesh_io.read_ply(data_path("hand_vh.ply"))
    return _cache["hand"]


def _make_scene(Render, monkeypatch, mesh, direct=True, **env):
    """A scene whose trusted sub-batches of ANY size take bounce #1 inside the cull stage -- or, `direct=False`, never do.  (The library
    reads the knobs when the scene is created.)"""
    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        if direct:
            m.setenv("DRT_CULL_DIRECT_MIN_LOG2", "0")
        else:
            m.setenv("DRT_CULL_DIRECT", "0")
        for k, v in env.items():
            m.setenv(k, v)
        return Render.Scene(mesh, 0)


def _rose(scene, before):
    now = scene.optix_mesh.route_counts()
    return {k: now[k] - before[k] for k in now}


def _rays(mesh, w, h, ids, dist):
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, 72, w, h, distance_factor=dist)
    r = [views.generate_ray(h, w, cams[k][3], cams[k][2]) for k in ids]
    return torch.cat([x[0] for x in r]).contiguous(), torch.cat([x[1] for x in r]).contiguous()


def _targets(mesh, n, seed):
    rng = np.random.default_rng(seed)
    c, _ = views.mesh_frame(mesh.vertices)
    sp = torch.tensor(rng.standard_normal((n, 3)) * 40.0 + np.asarray(c) + np.array([0.0, 0.0, 150.0]))
    return sp, torch.tensor(rng.random(n) > 0.2), torch.tensor(rng.standard_normal((n, 3)))


def _oracle(mesh, verts, o, d, pair, sp, valid, wgt):
    """The oracle's outputs, face ids, loss, d loss / d vertices and d (loss + <wgt, out_ori> + <wgt, out_dir>) / d vertices."""
    Vc = torch.tensor(np.asarray(verts), dtype=torch.float64, requires_grad=True)
    oo, od, mk, aux = orc.render_transparent(orc.Mesh(mesh.faces, Vc), o, d, pair[0], pair[1], return_aux=True)
    loss = orc.ray_loss(oo, od, mk, sp, valid)
    g_loss, = torch.autograd.grad(loss, Vc, retain_graph=True)
    g_lin, = torch.autograd.grad((od * wgt).sum() + (oo * wgt).sum(), Vc)
    f2 = aux["face2"].clone()
    f2[~mk[:, 0]] = -1
    tir = torch.zeros(len(o), dtype=torch.bool)
    tir[aux["ind1"][~aux["b1"]["refracted"]]] = True
    return dict(oo=oo.detach(), od=od.detach(), mk=mk, f1=aux["face1"], f2=f2, tir=tir, loss=loss.item(), g_loss=g_loss, g_all=g_loss + g_lin,
                n_contrib=int((valid & mk[:, 0]).sum()))


def _close_to_oracle(scene, out_ori, out_dir, mask, ref):
    assert torch.equal(mask.cpu(), ref["mk"])
    assert torch.equal(scene.last_face1.cpu().long(), ref["f1"])
    assert torch.equal(scene.last_face2.cpu().long(), ref["f2"])
    torch.testing.assert_close(out_dir.detach().cpu(), ref["od"], rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(out_ori.detach().cpu(), ref["oo"], rtol=1e-10, atol=1e-9)


def _grad_close(got, ref):
    err = (got.cpu() - ref).abs().max().item()
    assert err <= 1e-5 and err <= 1e-9 * max(1.0, ref.abs().max().item()), err


def _dense_and_one_pass_against_oracle(Render, scene, mesh, verts, o, d, ref, sp, valid, wgt, subs=1, all_verified=True):
    """One trusted render_transparent + ray_loss + backward and the one-pass loss (through Scene.ray_loss_fused, and once more through
    enqueue_ray_term for the count of contributing rays) on ray tensors that have been through a call already; each against `ref`, each
    asserted to have taken the direct route in every one of its `subs` sub-batches."""
    from drt_amd.optix_mesh import _on
    og, dg, spg, vg, wg = o, d, sp.cuda(), valid.cuda(), wgt.cuda()
    V = torch.tensor(np.asarray(verts), dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    before = scene.optix_mesh.route_counts()
    out_ori, out_dir, mask = scene.render_transparent(og, dg)
    rose = _rose(scene, before)
    assert rose["total"] == rose["trust"] == rose["direct"] == subs and rose["mega"] == 0, rose
    assert rose["tree_late"] == (subs if all_verified else 0), rose
    _close_to_oracle(scene, out_ori, out_dir, mask, ref)
    assert float(out_ori.detach()[~mask].abs().sum()) == 0.0 and float(out_dir.detach()[~mask].abs().sum()) == 0.0
    loss = Render.ray_loss(out_ori, out_dir, mask, spg, vg)
    assert loss.item() == pytest.approx(ref["loss"], rel=1e-10, abs=1e-12)
    (loss + (out_dir * wg).sum() + (out_ori * wg).sum()).backward()
    _grad_close(V.grad, ref["g_all"])
    # the one-pass loss: k_cull_listed<true>
    V2 = V.detach().clone().requires_grad_(True)
    scene.update_verticex(V2)
    before = scene.optix_mesh.route_counts()
    lf = scene.ray_loss_fused(og, dg, spg, vg)
    rose = _rose(scene, before)
    assert rose["total"] == rose["trust"] == rose["direct"] == subs and rose["mega"] == 0 and rose["park"] == 0, rose
    assert lf.item() == pytest.approx(ref["loss"], rel=1e-10, abs=1e-12)
    lf.backward()
    _grad_close(V2.grad, ref["g_loss"])
    acc_loss = torch.zeros((), dtype=torch.float64, device="cuda")
    acc_grad = torch.zeros_like(V2.detach())
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    before = scene.optix_mesh.route_counts()
    with _on(acc_grad.device):
        keep = Render.enqueue_ray_term(scene, V2.detach(), og, dg, spg, vg, None, acc_loss.data_ptr(), acc_grad.data_ptr(), count.data_ptr())
    torch.cuda.synchronize()
    del keep
    assert _rose(scene, before)["direct"] == subs
    assert int(count) == ref["n_contrib"]
    assert acc_loss.item() == pytest.approx(ref["loss"], rel=1e-10, abs=1e-12)
    _grad_close(acc_grad, ref["g_loss"])


# ---- (a) the direct route against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(IOR_PAIRS))
@pytest.mark.parametrize("dist", [2.5, 1.2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_direct_route_equals_the_oracle_dense_and_one_pass(Render, monkeypatch, shape, dist, pair):
    mesh = _hand()
    w, h, ids = SHAPES[shape]
    o, d = _rays(mesh, w, h, ids, dist)
    n, P = len(o), w * h
    sp, valid, wgt = _targets(mesh, n, 11)
    ior = IOR_PAIRS[pair]
    ref = _oracle(mesh, mesh.vertices, o, d, ior, sp, valid, wgt)
    # what the case rests on, from the oracle
    paths = 0
    for k, (hits0, tir0, paths0) in enumerate(COUNTS[shape, dist, pair]):
        sl = slice(k * P, (k + 1) * P)
        hits, tir = int((ref["f1"][sl] >= 0).sum()), int(ref["tir"][sl].sum())
        paths += int(ref["mk"][sl, 0].sum())
        assert hits >= 0.9 * hits0 and hits > 0 and tir >= 0.9 * tir0 and int(ref["mk"][sl, 0].sum()) >= 0.9 * paths0, (k, hits, tir)
        if ior[1] > ior[0]:
            assert tir >= 4, (k, tir)
        assert torch.equal(ref["f2"][sl][ref["tir"][sl]], torch.full((tir,), -1, dtype=torch.long))     # a reflected ray has no second face
    assert paths >= 40
    Render.intIOR, Render.extIOR = ior
    Render.resx, Render.resy = w, h
    scene = _make_scene(Render, monkeypatch, mesh)
    og, dg = o.cuda(), d.cuda()
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda"))
    before = scene.optix_mesh.route_counts()
    with torch.no_grad():
        first = scene.render_transparent(og, dg)          # establishes the verdicts: every ray is read and verified, not the direct route
    rose = _rose(scene, before)
    assert rose["total"] == rose["raster"] == 1 and rose["trust"] == rose["direct"] == 0, rose
    _close_to_oracle(scene, *first, ref)
    del first
    _dense_and_one_pass_against_oracle(Render, scene, mesh, mesh.vertices, og, dg, ref, sp, valid, wgt)


# ---- (b), (d): the direct route gives the bits of the route without it ------------------------------------------------------------------
def _moving(mesh, steps):
    """Vertices that drift and, in turn, grow and shrink about their centroid: at every step pixels are left by the mesh (80, 7, 493, 9, 876
    of the 64x64 x 3 images, by the oracle) and others see its surface further away than the step before."""
    v0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    c = v0.mean(0)
    return [c + (v0 - c) * (1.0 + 0.05 * k * (-1) ** k) + 0.3 * k for k in range(steps)]


def _sequence(Render, scene, Vs, o, d, sp, valid, grads=True, after_first=None):
    """A call per vertex set on one pair of ray tensors: (out_ori, out_dir, mask, face1, face2[, loss, gradient]) clones and the route
    counters each call added.  The outputs are let go of before the next call, as an optimisation step does."""
    out = []
    for k, V in enumerate(Vs):
        V = V.clone().requires_grad_(grads)
        scene.update_verticex(V)
        before = scene.optix_mesh.route_counts()
        oo, od, mk = scene.render_transparent(o, d)
        rose = _rose(scene, before)
        rec = [oo.detach().clone(), od.detach().clone(), mk.clone(), scene.last_face1.clone(), scene.last_face2.clone()]
        if grads:
            loss = Render.ray_loss(oo, od, mk, sp, valid)
            loss.backward()
            rec += [loss.detach().clone(), V.grad.clone()]
            del loss
        del oo, od, mk
        out.append((rec, rose))
        if k == 0 and after_first is not None:
            after_first()
    return out


def _tir_case(Render):
    """64x64 x 3 images of the hand under (1.0, 1.33): 280 of the 924 primary hits are reflected at bounce #1."""
    mesh = _hand()
    Render.intIOR, Render.extIOR = IOR_PAIRS["1.0_1.33"]
    Render.resx = Render.resy = 64
    if "tir_case" not in _cache:
        o, d = _rays(mesh, 64, 64, SHAPES["64x64x3"][2], 2.5)
        sp, valid, _ = _targets(mesh, len(o), 12)
        _cache["tir_case"] = (o.cuda(), d.cuda(), sp.cuda(), valid.cuda())
    return (mesh,) + _cache["tir_case"]


def _oracle_sequence(Render, steps):
    """(mask, face1, face2, out_dir) of the oracle for every vertex set of `_moving`; computed once."""
    key = ("oracle_sequence", steps)
    if key not in _cache:
        mesh, o, d, _, _ = _tir_case(Render)
        out = []
        for V in _moving(mesh, steps):
            oo, od, mk, aux = orc.render_transparent(orc.Mesh(mesh.faces, V.cpu()), o.cpu(), d.cpu(), *IOR_PAIRS["1.0_1.33"], return_aux=True)
            f2 = aux["face2"].clone()
            f2[~mk[:, 0]] = -1
            out.append((mk, aux["face1"], f2, od))
        _cache[key] = out
    return _cache[key]


def _plain_reference(Render, monkeypatch, steps, deterministic):
    """The sequence on a scene that never takes the direct route: fresh outputs filled by memsets, dense face ids; computed once.  Its
    trusted calls run k_cull_listed too (without `direct`) and share its handling of the key buffer: what anchors the sequence is the
    oracle, call by call."""
    key = ("plain", steps, deterministic)
    if key not in _cache:
        mesh, o, d, sp, valid = _tir_case(Render)
        Render.RECYCLE_OUTPUTS, Render.PREFILL_NEXT, Render.HIT_SEED, Render.DENSE_FACE_IDS = False, False, False, True
        scene = _make_scene(Render, monkeypatch, mesh, direct=False)
        seq = _sequence(Render, scene, _moving(mesh, steps), o.clone(), d.clone(), sp, valid)
        for k, ((rec, rose), (mk, f1, f2, od)) in enumerate(zip(seq, _oracle_sequence(Render, steps))):
            assert rose["total"] == 1 and rose["direct"] == 0 and rose["mega"] == 0, rose
            assert 200 < int(rec[2][:, 0].sum()) < 2000
            assert torch.equal(rec[2].cpu(), mk) and torch.equal(rec[3].cpu().long(), f1) and torch.equal(rec[4].cpu().long(), f2), k
            torch.testing.assert_close(rec[1].cpu(), od, rtol=1e-10, atol=1e-11)
        _cache[key] = [rec for rec, _ in seq]
    return _cache[key]


def _same_bits(rec, ref, k, sparse=False):
    oo, od, mk, f1, f2 = rec[:5]
    assert torch.equal(mk, ref[2]) and torch.equal(oo, ref[0]) and torch.equal(od, ref[1]), k
    assert float(oo[~mk].abs().sum()) == 0.0 and float(od[~mk].abs().sum()) == 0.0, k
    m = mk[:, 0] if sparse else slice(None)
    assert torch.equal(f1[m], ref[3][m]) and torch.equal(f2[m], ref[4][m]), k


VARIANTS = {
    # name: (module settings, scene knobs, the counters a trusted call must add: call number -> value, None = either)
    "fresh": (dict(RECYCLE_OUTPUTS=False), {}, dict(park=lambda k: 0, late_fill=lambda k: 1, tree_late=lambda k: 1)),
    "recycled": (dict(RECYCLE_OUTPUTS=True, RECYCLE_MIN_RAYS=0), {}, dict(park=lambda k: 1 if k >= 2 else None, tree_late=lambda k: 1)),
    "recycled_no_park": (dict(RECYCLE_OUTPUTS=True, RECYCLE_MIN_RAYS=0), {"DRT_CULL_PARK": "0"}, dict(park=lambda k: 0)),
    "prefilled": (dict(RECYCLE_OUTPUTS=False, PREFILL_NEXT=True, PREFILL_MIN_RAYS=0), {}, dict(park=lambda k: 0, late_fill=lambda k: 1)),
    "fills_in_front": (dict(RECYCLE_OUTPUTS=False), {"DRT_FILL_OVERLAP": "0"}, dict(late_fill=lambda k: 0, park=lambda k: 0)),
    "fills_behind_the_cull": (dict(RECYCLE_OUTPUTS=False), {"DRT_FILL_AFTER_SHADE1": "0"}, dict(late_fill=lambda k: 1)),
    "not_all_verified": (dict(RECYCLE_OUTPUTS=False), {}, dict(tree_late=lambda k: 0, late_fill=lambda k: 1)),
    "sparse_face_ids": (dict(RECYCLE_OUTPUTS=True, RECYCLE_MIN_RAYS=0, DENSE_FACE_IDS=False), {}, dict(park=lambda k: 1 if k >= 2 else None, tree_late=lambda k: 1)),
    "hit_seed": (dict(RECYCLE_OUTPUTS=False, HIT_SEED=True), {}, dict(tree_late=lambda k: 1)),
}
STEPS = 6


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_companion_route_gives_the_bits_of_the_scene_without_direct(Render, monkeypatch, variant):
    from drt_amd import det
    settings, knobs, expect = VARIANTS[variant]
    for deterministic in (False, True):
        was = det.enable(deterministic)
        try:
            ref = _plain_reference(Render, monkeypatch, STEPS, deterministic)
            mesh, o, d, sp, valid = _tir_case(Render)
            Render.RECYCLE_OUTPUTS, Render.PREFILL_NEXT, Render.HIT_SEED, Render.DENSE_FACE_IDS = False, False, False, True
            for k, v in settings.items():
                setattr(Render, k, v)
            scene = _make_scene(Render, monkeypatch, mesh, **knobs)
            o, d = o.clone(), d.clone()                # (ray tensors of this scene's own: the verdict and the seeds live on them)

            def demote():                              # verdicts established, but never read back: trusted calls without DRT_GRID_ALL_VERIFIED
                d._drt_grid[3][0] = False
            seq = _sequence(Render, scene, _moving(mesh, STEPS), o, d, sp, valid, after_first=demote if variant == "not_all_verified" else None)
            if variant == "hit_seed":
                assert getattr(d, "_drt_seed2", None) is not None and int((d._drt_seed2 >= 0).sum()) > 200
            if variant == "prefilled":
                assert scene.optix_mesh._prefilled is not None
            for k, (rec, rose) in enumerate(seq):
                assert rose["total"] == rose["raster"] == 1 and rose["mega"] == 0, (k, rose)
                assert rose["trust"] == rose["direct"] == int(k >= 1), (k, rose)
                if k >= 1:
                    for name, want in expect.items():
                        assert want(k) is None or rose[name] == want(k), (k, name, rose)
                _same_bits(rec, ref[k], k, sparse=settings.get("DENSE_FACE_IDS") is False)
                if deterministic:
                    assert torch.equal(rec[5], ref[k][5]) and torch.equal(rec[6], ref[k][6]), k
                else:
                    assert rec[5].item() == pytest.approx(ref[k][5].item(), rel=1e-12)
                    scale = ref[k][6].abs().max().item()
                    assert scale > 0 and (rec[6] - ref[k][6]).abs().max().item() <= 1e-12 * scale, k
        finally:
            det.enable(was)


# ---- (c) trusted and untrusted images in one call ---------------------------------------------------------------------------------------
def test_untrusted_and_trusted_images_share_one_direct_call(Render, monkeypatch):
    mesh, o, d, _, _ = _tir_case(Render)
    o, d = o.clone(), d.clone()
    pair = IOR_PAIRS["1.0_1.33"]
    scene = _make_scene(Render, monkeypatch, mesh)
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda"))
    with torch.no_grad():
        for _ in range(2):
            scene.render_transparent(o, d)
    assert d._drt_grid[3][0] is True                       # three verified images
    d[32 * 64 + 27:32 * 64 + 37] = d[30 * 64 + 20:30 * 64 + 30].clone()      # ten rays of image 0 now point elsewhere (no ray of the 8 x 8 lattice)
    sp, valid, wgt = _targets(mesh, len(o), 13)
    ref = _oracle(mesh, mesh.vertices, o.cpu(), d.cpu(), pair, sp, valid, wgt)
    assert int((ref["f1"][32 * 64 + 27:32 * 64 + 37] >= 0).sum()) >= 5 and int(ref["tir"][4096:].sum()) >= 100
    before = scene.optix_mesh.route_counts()
    with torch.no_grad():
        again = scene.render_transparent(o, d)             # the write bumped the version: this call establishes again
    assert _rose(scene, before)["direct"] == 0
    _close_to_oracle(scene, *again, ref)
    del again
    assert d._drt_grid[3][0] is None
    tr = scene.optix_mesh
    tr.profile_enable(1)
    tr.profile_read()
    # image 0 through cull_patch (list R0, its ten foreign rays through the tree), images 1 and 2 through the direct branch (list R1)
    _dense_and_one_pass_against_oracle(Render, scene, mesh, mesh.vertices, o, d, ref, sp, valid, wgt, all_verified=False)
    prof = tr.profile_read()
    tr.profile_enable(0)
    assert d._drt_grid[3][0] is False
    assert prof["trace1"][2] > 0


# ---- (d) the key buffer across consecutive calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("recycle", [False, True])
def test_consecutive_direct_calls_on_a_moving_mesh(Render, monkeypatch, recycle):
    """k_cull_listed's direct branch consumes the keys of the projection pass and clears the group bits itself; a key or a bit it left
    behind is a primary hit (or a listed patch) of the NEXT call, whose mesh has moved on."""
    steps = STEPS
    ref = _plain_reference(Render, monkeypatch, steps, False)
    mesh, o, d, sp, valid = _tir_case(Render)
    Render.RECYCLE_OUTPUTS, Render.RECYCLE_MIN_RAYS, Render.PREFILL_NEXT, Render.HIT_SEED, Render.DENSE_FACE_IDS = recycle, 0, False, False, True
    scene = _make_scene(Render, monkeypatch, mesh)
    with torch.no_grad():
        seq = _sequence(Render, scene, _moving(mesh, steps), o.clone(), d.clone(), sp, valid, grads=False)
    changed = 0
    for k, (rec, rose) in enumerate(seq):
        assert rose["total"] == 1 and rose["direct"] == int(k >= 1) and rose["mega"] == 0, (k, rose)
        assert rose["park"] == int(recycle) or k < 2, (k, rose)
        _same_bits(rec, ref[k], k)
        if k:
            changed += int((rec[3] != seq[k - 1][0][3]).sum())
            assert int(((rec[3] < 0) & (seq[k - 1][0][3] >= 0)).sum()) > 0, k      # pixels the mesh has left: a key left behind would still hit there
    assert changed > 500


# ---- (e) sub-batches on two streams -----------------------------------------------------------------------------------------------------
def test_direct_sub_batches_on_two_streams(Render, monkeypatch):
    mesh = _hand()
    ids = (5, 17, 29, 41, 53, 65)
    pair = IOR_PAIRS["1.2_1.5"]
    Render.intIOR, Render.extIOR = pair
    Render.resx = Render.resy = 64
    o, d = _rays(mesh, 64, 64, ids, 2.5)
    sp, valid, wgt = _targets(mesh, len(o), 14)
    ref = _oracle(mesh, mesh.vertices, o, d, pair, sp, valid, wgt)
    for k in range(len(ids)):
        sl = slice(k * 4096, (k + 1) * 4096)
        assert int(ref["tir"][sl].sum()) >= 4 and int(ref["mk"][sl, 0].sum()) >= 40, k
    # six sub-batches of one image each, dealt to the two internal streams in turn: three a stream, each stream with its own lists,
    # the verdict cache indexed by the image's number in the call
    scene = _make_scene(Render, monkeypatch, mesh, DRT_MIN_SUB_LOG2="12", DRT_SUB_PER_STREAM="3")
    og, dg = o.cuda(), d.cuda()
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda"))
    before = scene.optix_mesh.route_counts()
    with torch.no_grad():
        first = scene.render_transparent(og, dg)
    rose = _rose(scene, before)
    assert rose["total"] == rose["raster"] == len(ids) and rose["direct"] == 0, rose
    _close_to_oracle(scene, *first, ref)
    del first
    _dense_and_one_pass_against_oracle(Render, scene, mesh, mesh.vertices, og, dg, ref, sp, valid, wgt, subs=len(ids))


# ---- (f) the staging area flushed inside the patch loop ---------------------------------------------------------------------------------
def _per_patch(flags, n_views, res):
    """Set entries of a per-ray flag per 64x4 patch."""
    return flags.view(n_views, res // 4, 4, res // 64, 64).permute(0, 1, 3, 2, 4).reshape(-1, 256).sum(1)


def test_staging_area_is_flushed_inside_the_patch_loop(Render, monkeypatch):
    """A block of k_cull_listed stages the entries of its patches in LDS (768 entries) and flushes once more than 512 are held: after the
    third of three dense patches in a row.  With 8 blocks per CU that needs more listed patches than any other test has: an object that
    fills 768 x 768 images.  Block b takes the list entries b, b + gs, b + 2 gs, ...: when fewer than gs patches of the whole call are NOT
    dense, some block finds its first four entries dense -- it flushes behind the third and stages the fourth."""
    mesh = mesh_io.icosphere(2, radius=50.0, noise=0.05, seed=3)
    assert len(mesh.faces) == 320
    res, P = 768, 768 * 768
    gs = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    pair = IOR_PAIRS["default"]
    Render.intIOR, Render.extIOR = pair
    Render.resx = Render.resy = res
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, 72, res, res, distance_factor=0.9)
    om = orc.Mesh(mesh.faces, torch.tensor(mesh.vertices, dtype=torch.float64))
    rng = np.random.default_rng(15)
    rays, dense, dense_valid, valids = [], 0, 0, []
    for k in (7, 25, 43, 61, 16, 34, 52, 70):
        o_k, d_k = views.generate_ray(res, res, cams[k][3], cams[k][2])
        hit = orc.intersect_ids(om, o_k, d_k)[1]
        valid_k = torch.tensor(rng.random(P) > 0.2)
        rays.append((o_k, d_k)); valids.append(valid_k)
        dense += int((_per_patch(hit, 1, res) == 256).sum())
        dense_valid += int((_per_patch(hit & valid_k, 1, res) > 170).sum())       # three of these are more than 512 entries (one-pass form: `valid` gates the list)
        patches = len(rays) * (P // 256)
        if min(dense, dense_valid) >= 4 * gs and patches - min(dense, dense_valid) < gs:
            break
    n_views = len(rays)
    patches = n_views * (P // 256)
    assert dense >= 4 * gs and patches - dense < gs and dense_valid >= 4 * gs and patches - dense_valid < gs, (gs, n_views, dense, dense_valid)
    o = torch.cat([r[0] for r in rays]).contiguous(); d = torch.cat([r[1] for r in rays]).contiguous()
    valid = torch.cat(valids)
    sp, _, wgt = _targets(mesh, len(o), 16)
    ref = _oracle(mesh, mesh.vertices, o, d, pair, sp, valid, wgt)
    assert int(ref["tir"].sum()) == 0 and int(ref["mk"][:, 0].sum()) > 100000
    og, dg = o.cuda(), d.cuda()
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    plain = _make_scene(Render, monkeypatch, mesh, direct=False)
    plain.update_verticex(V)
    oc, dc = og.clone(), dg.clone()
    with torch.no_grad():
        for _ in range(2):
            want = plain.render_transparent(oc, dc)
    want = [t.clone() for t in want] + [plain.last_face1.clone(), plain.last_face2.clone()]
    assert plain.optix_mesh.route_counts()["direct"] == 0 and plain.optix_mesh.route_counts()["trust"] == 1
    del plain
    scene = _make_scene(Render, monkeypatch, mesh)
    scene.update_verticex(V)
    with torch.no_grad():
        scene.render_transparent(og, dg)
        before = scene.optix_mesh.route_counts()
        got = scene.render_transparent(og, dg)
        rose = _rose(scene, before)
        assert rose["total"] == rose["direct"] == rose["tree_late"] == 1 and rose["mega"] == 0, rose
        got = list(got) + [scene.last_face1, scene.last_face2]
        for j in range(5):
            assert torch.equal(got[j], want[j]), j
    del got, want
    _dense_and_one_pass_against_oracle(Render, scene, mesh, mesh.vertices, og, dg, ref, sp, valid, wgt)
