"""GPU: gradients of render_transparent / ray_loss w.r.t. the camera rays and the indices of refraction (drt_render_backward_inputs,
drt_render_backward_ray_loss_inputs) against the reference's own autograd (tests/golden/hand_r64_v5_inputs.npz), the oracle
restatement (tests/inputs_ref.py) and the in-repo stepwise route; the vertex gradient they leave unchanged; and the IOR fit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inputs_ref
from conftest import HEADLINE_FIXTURE, IOR, ROOT, data_path, fixture_mesh, fixture_view, golden
from drt_amd import det, diffrender as Render, mesh_io, views

pytestmark = pytest.mark.gpu
EXT = 1.00029


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR)
    yield
    Render.intIOR, Render.extIOR = saved


@pytest.fixture
def deterministic():
    was = det.enable(True)
    yield
    det.enable(was)


def _rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _hand_view():
    g = golden("hand_r64_v5")
    o, d, sp, valid = fixture_view(g)
    return mesh_io.read_ply(data_path("hand_vh.ply")), o, d, sp, valid


def _leaves(o, d, ext_device="cpu"):
    origin = o.cuda().requires_grad_(True)
    ray_dir = d.cuda().requires_grad_(True)
    ti = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
    te = torch.tensor(EXT, dtype=torch.float64, device=ext_device, requires_grad=True)
    return origin, ray_dir, ti, te


def test_dropin_matches_reference_autograd():
    g = golden("hand_r64_v5_inputs")
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    origin, ray_dir, ti, te = _leaves(o, d)
    Render.intIOR, Render.extIOR = ti, te
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
    loss = Render.ray_loss(out_ori, out_dir, mask, sp.cuda(), valid.cuda())
    assert loss.item() == pytest.approx(float(g["ray_loss"]), rel=1e-11)
    loss.backward()
    assert origin.grad is None                       # out_ori is detached by the loss: the reference reports origin unused
    assert _rel(ray_dir.grad, g["grad_ray_loss_dir"]) < 1e-9
    assert int((ray_dir.grad != 0).any(1).sum()) == int(g["contributing_rows"])
    assert ti.grad.device.type == "cuda" and te.grad.device.type == "cpu" and ti.grad.shape == ()
    assert ti.grad.item() == pytest.approx(float(g["grad_ray_loss_ior_int"]), rel=1e-9)
    assert te.grad.item() == pytest.approx(float(g["grad_ray_loss_ior_ext"]), rel=1e-9)

    origin, ray_dir, ti, te = _leaves(o, d, "cuda")
    Render.intIOR, Render.extIOR = ti, te
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
    rng = np.random.default_rng(int(g["lin_seed"]))
    P = o.shape[0]
    w_ori, w_dir = torch.tensor(rng.standard_normal((P, 3))).cuda(), torch.tensor(rng.standard_normal((P, 3))).cuda()
    lin = (out_ori * w_ori).sum() + (out_dir * w_dir).sum()
    assert lin.item() == pytest.approx(float(g["lin"]), rel=1e-11)
    lin.backward()
    assert _rel(origin.grad, g["grad_lin_origin"]) < 1e-9
    assert _rel(ray_dir.grad, g["grad_lin_dir"]) < 1e-9
    assert ti.grad.item() == pytest.approx(float(g["grad_lin_ior_int"]), rel=1e-9)
    assert te.grad.item() == pytest.approx(float(g["grad_lin_ior_ext"]), rel=1e-9)


def test_horse50k_vs_oracle_autograd():
    g = golden(HEADLINE_FIXTURE)
    mesh = fixture_mesh(g)
    o, d, sp, valid = fixture_view(g)
    res = int(g["res"])
    Render.resx = Render.resy = res
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    origin, ray_dir, ti, te = _leaves(o, d, "cuda")
    Render.intIOR, Render.extIOR = ti, te
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
    rng = np.random.default_rng(3)
    w_ori, w_dir = torch.tensor(rng.standard_normal(o.shape)), torch.tensor(rng.standard_normal(o.shape))
    f = Render.ray_loss(out_ori, out_dir, mask, sp.cuda(), valid.cuda()) + 1e-3 * ((out_ori * w_ori.cuda()).sum() + (out_dir * w_dir.cuda()).sum())
    f.backward()

    Vc = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
    oc, dc = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    tic = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    tec = torch.tensor(EXT, dtype=torch.float64, requires_grad=True)
    from oracle import diffrender_oracle as orc
    oo, od, mk, aux = inputs_ref.render_transparent(mesh.faces, Vc, oc, dc, tic, tec)      # face ids: the oracle's tracer
    assert torch.equal(mask.cpu(), mk) and mk[:, 0].sum() > 1000
    assert torch.equal(scene.last_face1.cpu().long()[mk[:, 0]], aux["face1"][mk[:, 0]])
    assert torch.equal(scene.last_face2.cpu().long()[mk[:, 0]], aux["face2"][mk[:, 0]])
    fc = orc.ray_loss(oo, od, mk, sp, valid) + 1e-3 * ((oo * w_ori).sum() + (od * w_dir).sum())
    fc.backward()
    assert f.item() == pytest.approx(fc.item(), rel=1e-10)
    assert _rel(origin.grad, oc.grad) < 1e-9
    assert _rel(ray_dir.grad, dc.grad) < 1e-9
    assert ti.grad.item() == pytest.approx(tic.grad.item(), rel=1e-9)
    assert te.grad.item() == pytest.approx(tec.grad.item(), rel=1e-9)
    assert _rel(V.grad, Vc.grad) < 1e-7


def _grads(scene, V0, o, d, sp, valid, extras, lin=False):
    """(V.grad, origin.grad, ray_dir.grad, d/d intIOR, d/d extIOR) of ray_loss (or a linear functional) of one render call."""
    V = V0.clone().requires_grad_(True)
    scene.update_verticex(V)
    if extras:
        origin, ray_dir, ti, te = _leaves(o, d, "cuda")
        Render.intIOR, Render.extIOR = ti, te
    else:
        origin, ray_dir, ti, te = o.cuda(), d.cuda(), None, None
        Render.intIOR, Render.extIOR = IOR, EXT
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
    if lin:
        w = torch.tensor(np.random.default_rng(7).standard_normal(o.shape)).cuda()
        f = (out_ori * w).sum() + (out_dir * w).sum()
    else:
        f = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    f.backward()
    return tuple(None if t is None else t.grad for t in (V, origin, ray_dir, ti, te)) if extras else (V.grad,)


@pytest.mark.parametrize("lin", [False, True])
def test_vertex_gradient_unchanged_and_deterministic(deterministic, lin):
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    V0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    sp, valid = sp.cuda(), valid.cuda()
    plain = _grads(scene, V0, o, d, sp, valid, False, lin)
    a = _grads(scene, V0, o, d, sp, valid, True, lin)
    b = _grads(scene, V0, o, d, sp, valid, True, lin)
    assert torch.equal(plain[0], a[0])
    assert (a[1] is None) == (not lin)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)
    assert a[2].abs().max() > 0 and a[3] != 0 and a[4] != 0


def test_ray_loss_fused_with_tensor_ior_falls_back(deterministic):
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    V0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    o, d, sp, valid = o.cuda(), d.cuda(), sp.cuda(), valid.cuda()
    res = []
    for fused in (True, False):
        V = V0.clone().requires_grad_(True)
        scene.update_verticex(V)
        ti = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
        Render.intIOR = ti
        Render.cache_report(reset=True)
        if fused:
            loss = scene.ray_loss_fused(o, d, sp, valid)
            assert Render.cache_report()["fused_fallback_inputs"] == 1
        else:
            loss = Render.ray_loss(*scene.render_transparent(o, d), sp, valid)
        loss.backward()
        res.append((loss.detach(), V.grad, ti.grad))
    for x, y in zip(*res):
        assert torch.equal(x, y)


def test_plain_inputs_keep_their_routes():
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    Render.intIOR, Render.extIOR = IOR, EXT
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    o, d, sp, valid = o.cuda(), d.cuda(), sp.cuda(), valid.cuda()
    Render.cache_report(reset=True)
    lf = scene.ray_loss_fused(o, d, sp, valid)
    out = scene.render_transparent(o, d)
    lu = Render.ray_loss(*out, sp, valid)
    rep = Render.cache_report()
    assert "fused_fallback_inputs" not in rep
    ctx = lu.grad_fn
    assert ctx.stash is not None                     # the eager unit-seed stash: the plain route
    assert lf.item() == pytest.approx(lu.item(), rel=1e-12)


def test_stepwise_route_cross_check():
    """The stepwise route (Dintersect / refract_ray as torch ops) differentiates a tensor IOR and the rays itself."""
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    sp, valid = sp.cuda(), valid.cuda()
    origin, ray_dir, ti, te = _leaves(o, d, "cuda")
    Render.intIOR, Render.extIOR = ti, te
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
    Render.ray_loss(out_ori, out_dir, mask, sp, valid).backward()
    origin2, ray_dir2, ti2, te2 = _leaves(o, d, "cuda")
    Render.intIOR, Render.extIOR = ti2, te2
    ray = scene.trace2(Render.Ray(origin2, ray_dir2))
    P = o.shape[0]
    oo = torch.zeros((P, 3), dtype=torch.float64, device="cuda").index_put((ray.ray_ind,), ray.origin)
    od = torch.zeros((P, 3), dtype=torch.float64, device="cuda").index_put((ray.ray_ind,), ray.direction)
    _, occluded = scene.optix_intersect(ray)
    keep = ray.ray_ind[~occluded]
    mk = torch.zeros((P, 3), dtype=torch.bool, device="cuda")
    mk[keep] = True
    target = sp - oo.detach()
    target = target / target.norm(dim=1, keepdim=True)
    ((od - target)[valid & mk[:, 0]]).pow(2).sum().backward()
    assert torch.equal(mk, mask)
    assert _rel(ray_dir.grad, ray_dir2.grad.cpu().numpy()) < 1e-9
    assert ti.grad.item() == pytest.approx(ti2.grad.item(), rel=1e-9)
    assert te.grad.item() == pytest.approx(te2.grad.item(), rel=1e-9)


def test_tensor_ior_in_graph_capture_raises(monkeypatch):
    """(The capture is simulated: the error is raised before any launch, and a real failed capture is not worth the risk.)"""
    mesh, o, d, sp, valid = _hand_view()
    Render.resx = Render.resy = 64
    scene = Render.Scene(data_path("hand_vh.ply"), 0)
    o, d = o.cuda(), d.cuda()
    Render.intIOR = torch.tensor(IOR, dtype=torch.float64, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        scene.render_transparent(o, d)


def test_fit_ior_alone_on_synthetic_capture():
    """horse_scan at IOR 1.50 (SyntheticData); the same mesh at IOR 1.40, the IOR the only unknown."""
    from drt_amd.captured_data import SyntheticData
    res = 128
    Render.resx = Render.resy = res
    scene = Render.Scene(data_path("horse_scan.ply"), 0)
    center, extent = views.mesh_frame(scene.mesh.vertices)
    Render.intIOR = 1.50
    data = SyntheticData(scene, center, extent, res, res, num_view=8, n_total=8)
    vs = [data.get_view(k) for k in range(8)]
    # secant steps on d loss / d IOR (the first one a fixed 0.01 downhill), each at most 0.05
    x, x_prev, g_prev, path = 1.40, None, None, []
    for it in range(100):
        ior = torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
        Render.intIOR = ior
        loss = sum(Render.ray_loss(*scene.render_transparent(v[3], v[4]), v[0], v[1]) for v in vs)
        loss.backward()
        g = float(ior.grad)
        path.append((x, float(loss.detach()), g))
        step = -0.01 * np.sign(g) if g_prev is None or g == g_prev else -g * (x - x_prev) / (g - g_prev)
        step = float(np.clip(step, -0.05, 0.05))
        x_prev, g_prev, x = x, g, x + step
        if abs(step) < 1e-7:
            break
    assert abs(x - 1.50) < 1e-3, path[-5:]


def test_reconstruct_fit_ior_moves_towards_truth(tmp_path):
    """The hull handed to the CLI is the scanned mesh itself, so that the IOR is the only thing wrong at the start."""
    data = tmp_path / "data"
    data.mkdir()
    for name in ("horse_vh.ply", "horse_scan.ply"):
        os.symlink(data_path("horse_scan.ply"), data / name)
    cmd = [sys.executable, "-m", "drt_amd.reconstruct", "--name", "horse", "--res", "64", "--views", "8", "--num-view", "8", "--passes", "1",
           "--iters", "8", "--ior", "1.5", "--ior-start", "1.4", "--fit-ior", "1e-5", "--data-path", str(data), "--result-path", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rep = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
    assert rep["ior_start"] == 1.4
    assert abs(rep["ior"] - 1.5) < 0.1 and rep["ior"] > 1.4, rep["ior"]


def test_fused_and_sharded_loops_refuse_ior_lr():
    from drt_amd import optim
    hp = dict(optim.HyperParams, ior_lr=1e-4)
    with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
        optim.optimize(None, None, hp, remesh=None, fused=True)
    with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
        optim.optimize_sharded(None, None, hp, remesh=None)
