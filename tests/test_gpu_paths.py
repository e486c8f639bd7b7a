"""GPU: Scene.render_paths -- refraction paths of up to K interactions with internal reflection (drt_render_paths_forward / _backward,
drt_amd/csrc/drt_paths.hip) -- against the chain of the reference's own pieces (tests/golden/hand_r64_v5_paths.npz), the float64
restatement tests/paths_ref.py on the big meshes, and render_transparent at (K = 2, drop).

The comparison leaves nothing out: tapes, hit counts and masks are compared for EVERY ray (ids and masks exact).  Rays: 1e-10 absolute.
Gradients: the project's 1e-9 relative (to the largest entry of the reference gradient) and 1e-5 absolute -- the depth-8 disagreement of the
kernels' own code with the restatement's autograd, measured on the CPU (tests/test_paths_adjoint.py MEASURED_DEPTH8_REL = 7.2e-16), is
far below a tenth of that, so the project's tolerances stand."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import paths_ref
import trajectory_case as tc
from conftest import HEADLINE_FIXTURE, IOR, ROOT, data_path, fixture_mesh, fixture_view, golden
from drt_amd import det, diffrender as Render, mesh_io, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu
EXT = orc.EXT_IOR
RAY_ABS, GRAD_REL, GRAD_ABS, LOSS_REL = 1e-10, 1e-9, 1e-5, 1e-10


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR, Render.resx, Render.resy)
    Render.intIOR, Render.extIOR = IOR, EXT
    yield
    Render.intIOR, Render.extIOR, Render.resx, Render.resy = saved


@pytest.fixture
def deterministic():
    was = det.enable(True)
    yield
    det.enable(was)


def _grad_close(got, ref):
    got, ref = got.detach().cpu().numpy(), np.asarray(ref)
    diff = np.abs(got - ref).max()
    assert np.isfinite(got).all()
    assert diff <= GRAD_ABS and diff <= GRAD_REL * np.abs(ref).max(), (diff, np.abs(ref).max())
    return diff / np.abs(ref).max()


def _scene(mesh):
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene, V


def _lin_weights(seed, P):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal((P, 3))), torch.tensor(rng.standard_normal((P, 3)))


def _hand():
    g = golden("hand_r64_v5")
    o, d, sp, valid = fixture_view(g)
    return mesh_io.read_ply(data_path("hand_vh.ply")), o, d, sp, valid


# ------------------------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("tag,max_bounces,tir", [("k6_reflect", 6, "reflect"), ("k4_drop", 4, "drop")])
def test_fixture_of_the_reference_chain(tag, max_bounces, tir):
    g = golden("hand_r64_v5_paths")
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    out_ori, out_dir, mask = scene.render_paths(o.cuda(), d.cuda(), max_bounces, tir)
    assert out_ori.dtype == out_dir.dtype == torch.float64 and mask.dtype == torch.bool and mask.shape == (o.shape[0], 3)
    # ids and masks: exact, every ray
    assert np.array_equal(scene.last_path_faces.cpu().numpy(), g[f"{tag}_tape"])
    assert scene.last_path_faces.dtype == torch.int32 and scene.last_path_hits.dtype == torch.uint8
    assert np.array_equal(scene.last_path_hits.cpu().numpy(), g[f"{tag}_hits"])
    assert np.array_equal(mask[:, 0].cpu().numpy(), g[f"{tag}_mask"]) and torch.equal(mask[:, 0], mask[:, 1]) and torch.equal(mask[:, 0], mask[:, 2])
    vi = torch.tensor(g[f"{tag}_valid_ind"]).cuda()
    assert np.abs(out_ori[vi].detach().cpu().numpy() - g[f"{tag}_out_ori"]).max() <= RAY_ABS
    assert np.abs(out_dir[vi].detach().cpu().numpy() - g[f"{tag}_out_dir"]).max() <= RAY_ABS
    dead = ~mask[:, 0]
    assert not out_ori[dead].any() and not out_dir[dead].any()
    loss = Render.ray_loss(out_ori, out_dir, mask, sp.cuda(), valid.cuda())
    assert loss.item() == pytest.approx(float(g[f"{tag}_ray_loss"]), rel=LOSS_REL)
    g_ray, = torch.autograd.grad(loss, V, retain_graph=True)
    r1 = _grad_close(g_ray, g[f"{tag}_grad_ray_loss"])
    w_ori, w_dir = _lin_weights(int(g["lin_seed"]), o.shape[0])
    lin = (out_ori * w_ori.cuda()).sum() + (out_dir * w_dir.cuda()).sum()
    assert lin.item() == pytest.approx(float(g[f"{tag}_lin"]), rel=LOSS_REL)
    g_lin, = torch.autograd.grad(lin, V)
    r2 = _grad_close(g_lin, g[f"{tag}_grad_lin"])
    print(tag, "valid", int(mask[:, 0].sum()), "gradient disagreement (relative to max): ray_loss", r1, "lin", r2)


# -------------------------------------------------------------------------------------------------------------- bigger meshes
def _big(name):
    if name == "horse50k":
        g = golden(HEADLINE_FIXTURE)
        o, d, sp, valid = fixture_view(g)
        return fixture_mesh(g), o, d, sp, valid, int(g["res"])
    mesh = mesh_io.read_ply(data_path("monkey_vh.ply"))
    res, view_id = 256, 7
    center, extent = views.mesh_frame(mesh.vertices)
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, 72, res, res)[view_id]
    o, d = views.generate_ray(res, res, Kinv, Rinv)
    rng = np.random.default_rng(100 + view_id)
    sp = rng.standard_normal((res * res, 3)) * 40.0 + np.asarray(center) + np.array([0.0, 0.0, 150.0])
    valid = rng.random(res * res) > 0.1
    return mesh, o, d, torch.tensor(sp), torch.tensor(valid), res


@pytest.mark.parametrize("name,expect_valid", [("horse50k", 2481), ("monkey", 3530)])
def test_big_mesh_against_the_restatement(name, expect_valid):
    mesh, o, d, sp, valid, res = _big(name)
    scene, V = _scene(mesh)
    out_ori, out_dir, mask = scene.render_paths(o.cuda(), d.cuda(), 8, "reflect")
    Vc = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
    oo, od, mk, aux = paths_ref.render_paths(mesh.faces, Vc, o, d, IOR, EXT, 8, "reflect")
    assert int(aux["valid"].sum()) == expect_valid and int(aux["hits"].max()) == 8
    assert torch.equal(scene.last_path_faces.cpu().long(), aux["tape"])
    assert torch.equal(scene.last_path_hits.cpu().long(), aux["hits"])
    assert torch.equal(mask.cpu(), mk)
    assert (out_ori.detach().cpu() - oo.detach()).abs().max().item() <= RAY_ABS
    assert (out_dir.detach().cpu() - od.detach()).abs().max().item() <= RAY_ABS
    loss = Render.ray_loss(out_ori, out_dir, mask, sp.cuda(), valid.cuda())
    loss_c = orc.ray_loss(oo, od, mk, sp, valid)
    assert loss.item() == pytest.approx(loss_c.item(), rel=LOSS_REL)
    g_ray, = torch.autograd.grad(loss, V, retain_graph=True)
    gc_ray, = torch.autograd.grad(loss_c, Vc, retain_graph=True)
    r1 = _grad_close(g_ray, gc_ray.numpy())
    w_ori, w_dir = _lin_weights(3, o.shape[0])
    g_lin, = torch.autograd.grad((out_ori * w_ori.cuda()).sum() + (out_dir * w_dir.cuda()).sum(), V)
    gc_lin, = torch.autograd.grad((oo * w_ori).sum() + (od * w_dir).sum(), Vc)
    r2 = _grad_close(g_lin, gc_lin.numpy())
    print(name, "valid", expect_valid, "gradient disagreement (relative to max): ray_loss", r1, "lin", r2)


# ------------------------------------------------------------------------------------------ K = 2, drop IS render_transparent
def _two_bounce_pair(use_det):
    mesh, o, d, sp, valid = _hand()
    Render.resx = Render.resy = 64
    out = []
    for paths in (False, True):
        scene, V = _scene(mesh)                                   # fresh tensors for either call
        oc, dc = o.clone().cuda(), d.clone().cuda()
        res = scene.render_paths(oc, dc, 2, "drop") if paths else scene.render_transparent(oc, dc)
        loss = Render.ray_loss(*res, sp.clone().cuda(), valid.clone().cuda())
        loss.backward()
        out.append((res, loss.detach(), V.grad, scene))
    return out


def test_two_bounces_drop_equals_render_transparent():
    (ra, la, ga, sa), (rb, lb, gb, sb) = _two_bounce_pair(False)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    assert int(rb[2][:, 0].sum()) == 257
    keep = rb[2][:, 0]
    assert torch.equal(sb.last_path_faces[0][keep], sa.last_face1[keep]) and torch.equal(sb.last_path_faces[1][keep], sa.last_face2[keep])
    assert la.item() == pytest.approx(lb.item(), rel=1e-14)
    assert (ga - gb).abs().max().item() <= 1e-12 * ga.abs().max().item()


def test_two_bounces_drop_gradient_bits_deterministic(deterministic):
    (ra, la, ga, _), (rb, lb, gb, _) = _two_bounce_pair(True)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    assert torch.equal(la, lb)
    assert torch.equal(ga, gb) and ga.abs().max() > 0


# ------------------------------------------------------------------------------------------------------------- determinism
def test_two_calls_and_a_graph_replay_give_the_same_gradient_bits(deterministic):
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    oc, dc, spc, vc = o.cuda(), d.cuda(), sp.cuda(), valid.cuda()

    def step():
        # a step as the loop runs it: vertices in, tree rebuilt, paths traced.  The update belongs INSIDE the captured region, as in the
        # graph tests of render_transparent: a consumer of the tree waits for the build's event, and a capture cannot wait for an event
        # that was recorded outside it.
        scene.update_verticex(V)
        out_ori, out_dir, mask = scene.render_paths(oc, dc, 6, "reflect")
        loss = Render.ray_loss(out_ori, out_dir, mask, spc, vc)
        g, = torch.autograd.grad(loss, V)
        return loss.detach(), g

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(g1, g2) and torch.equal(l1, l2) and g1.abs().max() > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l3, g3 = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g3, g1) and torch.equal(l3, l1)
    g3.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g3, g1)


# -------------------------------------------------------------------------------------------------------------- edge inputs
def test_no_rays_and_nothing_hit_return_zeros():
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    out_ori, out_dir, mask = scene.render_paths(e, e, 4, "reflect")
    assert out_ori.shape == out_dir.shape == mask.shape == (0, 3) and mask.dtype == torch.bool
    assert scene.last_path_hits.shape == (0,) and scene.last_path_faces.shape == (4, 0)
    (out_ori.sum() + out_dir.sum()).backward()
    assert V.grad is None or not V.grad.any()
    # a view that misses the mesh: every camera ray reversed
    out_ori, out_dir, mask = scene.render_paths(o.cuda(), -d.cuda(), 4, "reflect")
    assert not mask.any() and not out_ori.any() and not out_dir.any()
    assert not scene.last_path_hits.any() and (scene.last_path_faces == -1).all()
    V.grad = None
    Render.ray_loss(out_ori, out_dir, mask, sp.cuda(), valid.cuda()).backward()
    assert V.grad is not None and not V.grad.any()


def test_ray_count_that_is_not_a_multiple_of_64():
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    full = [t.clone() for t in scene.render_paths(o.cuda(), d.cuda(), 6, "reflect")]
    tape, hits = scene.last_path_faces.clone(), scene.last_path_hits.clone()
    lo, hi = 1000, 3003                       # 2003 rays
    part = scene.render_paths(o[lo:hi].cuda(), d[lo:hi].cuda(), 6, "reflect")
    assert int(part[2][:, 0].sum()) > 50
    for a, b in zip(full, part):
        assert torch.equal(a[lo:hi], b)
    assert torch.equal(tape[:, lo:hi], scene.last_path_faces) and torch.equal(hits[lo:hi], scene.last_path_hits)


def test_a_path_of_exactly_k_interactions_is_invalid_at_k_minus_one():
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    o6, d6, m6 = scene.render_paths(o.cuda(), d.cuda(), 6, "reflect")
    hits6, tape6 = scene.last_path_hits.clone(), scene.last_path_faces.clone()
    six = hits6 == 6
    assert int(six.sum()) >= 1 and m6[six].all()
    o5, d5, m5 = scene.render_paths(o.cuda(), d.cuda(), 5, "reflect")
    assert not m5[six].any() and not o5[six].any() and not scene.last_path_hits[six].any()
    assert torch.equal(scene.last_path_faces[:, six], tape6[:5][:, six])      # the same ray, the same five faces, then out of interactions
    rest = ~six
    assert torch.equal(m5[rest], m6[rest]) and torch.equal(o5[rest], o6[rest]) and torch.equal(d5[rest], d6[rest])
    assert torch.equal(scene.last_path_hits[rest], hits6[rest])


def test_arguments_are_checked():
    mesh, o, d, sp, valid = _hand()
    scene, V = _scene(mesh)
    oc, dc = o.cuda(), d.cuda()
    for k in (1, 9, 0, 2.5, True):
        with pytest.raises(ValueError, match="max_bounces"):
            scene.render_paths(oc, dc, k, "drop")
    with pytest.raises(ValueError, match="tir"):
        scene.render_paths(oc, dc, 4, "mirror")
    with pytest.raises(NotImplementedError):
        scene.render_paths(oc.clone().requires_grad_(True), dc, 4, "reflect")
    with pytest.raises(NotImplementedError):
        scene.render_paths(oc, dc.clone().requires_grad_(True), 4, "reflect")
    Render.intIOR = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        scene.render_paths(oc, dc, 4, "reflect")
    Render.intIOR = torch.tensor(IOR, dtype=torch.float64, device="cuda")          # a tensor IOR without a gradient is read to the host
    a = scene.render_paths(oc, dc, 4, "reflect")
    Render.intIOR = IOR
    b = scene.render_paths(oc, dc, 4, "reflect")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the C ABI refuses a bad K with a message
    from drt_amd import _lib
    rc = _lib.lib().drt_render_paths_forward(scene.optix_mesh._h, None, None, None, 0, IOR, EXT, 9, 1, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"max_bounces" in _lib.lib().drt_last_error()
    assert _lib.lib().drt_version() >= 3


# ---------------------------------------------------------------------------------------------------------------------- loop
def test_optimize_with_six_bounces_and_reflection(monkeypatch):
    from drt_amd import optim as O
    g = tc.load("hand_trajectory")
    hand = tc.frame_mesh("hand_trajectory")
    Render.intIOR = float(g["ior"])
    Render.resx = Render.resy = int(g["res"])
    scene = Render.Scene(mesh_io.TriMesh(g["vertices"].astype(np.float64), hand.faces), 0)
    data = tc.RecordedCapture(g, hand.vertices, "cuda")
    hp = dict(O.HyperParams, IOR=float(g["ior"]), Pass=1, Iters=10, start_lr=float(g["lr"]), max_bounces=6, tir="reflect")
    losses, used = [], []
    all_loss, render_paths = O.Loss_calculator.all_loss, Render.Scene.render_paths

    def recording(self):
        loss, parts = all_loss(self)
        losses.append(float(loss.detach()))
        return loss, parts

    def counting(self, *a, **k):
        used.append(a[2:])
        return render_paths(self, *a, **k)

    monkeypatch.setattr(O.Loss_calculator, "all_loss", recording)
    monkeypatch.setattr(Render.Scene, "render_paths", counting)
    V0 = scene.vertices.detach().clone()
    scene, history = O.optimize(scene, data, hp, remesh=None, output=False, fused=False)
    assert len(losses) == 10 and np.isfinite(losses).all() and len(history) == 1
    assert used == [(6, "reflect")] * 10
    moved = (scene.vertices.detach() - V0).abs().max().item()
    assert np.isfinite(moved) and moved > 1e-3


def test_loops_refuse_what_they_do_not_support():
    from drt_amd import optim as O
    hp = dict(O.HyperParams, max_bounces=6, tir="reflect")
    with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
        O.optimize(None, None, hp, remesh=None, fused=True)
    with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
        O.optimize_sharded(None, None, hp, remesh=None)
    with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
        O.FusedIteration(None, None, hp, 0.1)
    with pytest.raises(NotImplementedError, match="ior_lr"):
        O.optimize(None, None, dict(hp, ior_lr=1e-4), remesh=None, fused=False)
    with pytest.raises(NotImplementedError):
        O.optimize(None, None, dict(O.HyperParams, tir="reflect"), remesh=None, fused=True)      # K = 2 with reflection is not the default law
    for bad in (dict(max_bounces=9), dict(max_bounces=1), dict(tir="mirror")):
        with pytest.raises(ValueError):
            O.optimize(None, None, dict(O.HyperParams, **bad), remesh=None)
    assert O.path_law(O.HyperParams) is None and O.path_law(dict(O.HyperParams, max_bounces=2, tir="drop")) is None


def test_reconstruct_flags_reach_the_report(tmp_path):
    cmd = [sys.executable, "-m", "drt_amd.reconstruct", "--name", "hand", "--res", "64", "--views", "8", "--num-view", "8", "--passes", "1",
           "--iters", "4", "--max-bounces", "6", "--tir", "reflect", "--data-path", data_path(""), "--result-path", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rep = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")][-1]
    assert rep["max_bounces"] == 6 and rep["tir"] == "reflect" and rep["iterations"] == 4
