"""GPU: Snell refraction as the opt-in third element of the K-interaction path law -- Scene.render_paths / paths_ray_loss_fused with
``refraction="snell"``, the drt_render_paths_law_* entry points, and the ``(K, tir, "snell")`` law through SyntheticData, FusedIteration,
ShardedIteration, optimize and ``reconstruct --refraction snell`` (drt_amd/csrc/drt_paths.hip: the SNELL instantiations of k_paths_shade,
k_paths_bwd and k_paths_loss_bwd).

Reference: the float64 restatement tests/snell_ref.py (held against the kernels' own code on the host, the law of sines and time
reversal by tests/test_snell_adjoint.py).  Tolerances are the project's: rays 1e-10; gradients 1e-9 relative to the largest reference entry
and 1e-5 absolute (the depth-8 host figure behind them: test_snell_adjoint.MEASURED_DEPTH8_REL); across routes in float64 mode 1e-12
relative; bit equality in deterministic mode.  hand_vh, view 5 of the 72-view turntable at 64 x 64 (4 096 rays, 342 valid paths at
(6, reflect): more than one 256-ray table fill of the backward kernels) and 128 x 128 (16 384 rays, tapes 8 deep)."""
import datetime
import json
import multiprocessing
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import snell_ref
import trajectory_case as tc
from conftest import IOR, ROOT, data_path, fixture_view, golden
from drt_amd import _lib, det, diffrender as Render, mesh_io, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu
EXT = orc.EXT_IOR
GRAD_REL, GRAD_ABS, RAY_ABS, LOSS_REL, ROUTE_REL = 1e-9, 1e-5, 1e-10, 1e-10, 1e-12
RES, N_VIEWS = 64, 8
CHILD_TIMEOUT = 300


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


@pytest.fixture
def float_mode():
    was = det.enable(False)
    yield
    det.enable(was)


def _grad_close(got, ref):
    got, ref = got.detach().cpu().numpy(), np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref)
    diff = np.abs(got - ref).max()
    assert np.isfinite(got).all()
    assert diff <= GRAD_ABS and diff <= GRAD_REL * np.abs(ref).max(), (diff, np.abs(ref).max())
    return diff / np.abs(ref).max()


def _mesh():
    return mesh_io.read_ply(data_path("hand_vh.ply"))


def _rays(res):
    """(origin, ray_dir, screen_pixel, valid) of hand view 5 on the host: the recorded fixture at 64 x 64, turntable rays with random
    targets at 128 x 128."""
    if res == 64:
        return fixture_view(golden("hand_r64_v5"))
    mesh = _mesh()
    center, extent = views.mesh_frame(mesh.vertices)
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, 72, res, res)[5]
    o, d = views.generate_ray(res, res, Kinv, Rinv)
    rng = np.random.default_rng(1)
    sp = torch.tensor(rng.standard_normal((res * res, 3)) * 40.0 + center + np.array([0, 0, 150.0]))
    return o, d, sp, torch.tensor(rng.random(res * res) > 0.1)


def _hand(res=64):
    o, d, sp, valid = _rays(res)
    mesh = _mesh()
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene, V, o.cuda(), d.cuda(), sp.cuda(), valid.cuda()


_REF = {}


def _reference(res, k, tir):
    """The restatement's outputs and gradients of one case, computed once and shared (read-only)."""
    key = (res, k, tir)
    if key not in _REF:
        o, d, sp, valid = _rays(res)
        mesh = _mesh()
        Vt = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
        out_ori, out_dir, mask, aux = snell_ref.render_paths(mesh.faces, Vt, o, d, IOR, EXT, k, tir, "snell")
        loss = orc.ray_loss(out_ori, out_dir, mask, sp, valid)
        g_ray, = torch.autograd.grad(loss, Vt, retain_graph=True)
        rng = np.random.default_rng(3)
        w_ori, w_dir = torch.tensor(rng.standard_normal(tuple(o.shape))), torch.tensor(rng.standard_normal(tuple(o.shape)))
        g_lin, = torch.autograd.grad((out_ori * w_ori).sum() + (out_dir * w_dir).sum(), Vt)
        _REF[key] = dict(out_ori=out_ori.detach(), out_dir=out_dir.detach(), mask=mask, aux=aux, loss=loss.item(), g_ray=g_ray, g_lin=g_lin,
                         w_ori=w_ori, w_dir=w_dir)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("res,k,tir,n_valid", [(64, 6, "reflect", 342), (64, 2, "drop", 226), (128, 8, "reflect", 1428)])
def test_render_paths_snell_against_the_restatement(float_mode, res, k, tir, n_valid):
    ref = _reference(res, k, tir)
    scene, V, o, d, sp, valid = _hand(res)
    out_ori, out_dir, mask = scene.render_paths(o, d, k, tir, refraction="snell")
    aux = ref["aux"]
    # nothing is excluded: validity, hit count and tape of EVERY ray
    assert torch.equal(mask.cpu(), ref["mask"]) and int(mask[:, 0].sum()) == n_valid
    assert torch.equal(scene.last_path_hits.cpu().long(), aux["hits"])
    assert torch.equal(scene.last_path_faces.cpu().long(), aux["tape"])
    assert (out_ori.detach().cpu() - ref["out_ori"]).abs().max().item() <= RAY_ABS
    assert (out_dir.detach().cpu() - ref["out_dir"]).abs().max().item() <= RAY_ABS
    loss = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    g_ray, = torch.autograd.grad(loss, V, retain_graph=True)
    assert loss.item() == pytest.approx(ref["loss"], rel=LOSS_REL)
    r1 = _grad_close(g_ray, ref["g_ray"])
    g_lin, = torch.autograd.grad((out_ori * ref["w_ori"].cuda()).sum() + (out_dir * ref["w_dir"].cuda()).sum(), V)
    r2 = _grad_close(g_lin, ref["g_lin"])
    print(res, k, tir, "snell: valid", n_valid, "max hits", int(aux["hits"].max()), "gradient disagreement (relative to max): ray_loss", r1, "lin", r2)


# ---------------------------------------------------------------------------------------------------- 2. the default did not move
def test_reference_refraction_passed_explicitly_is_the_call_without_it():
    scene, V, o, d, sp, valid = _hand()
    a = scene.render_paths(o, d, 6, "reflect")
    hits_a, faces_a = scene.last_path_hits.clone(), scene.last_path_faces.clone()
    b = scene.render_paths(o, d, 6, "reflect", refraction="reference")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(hits_a, scene.last_path_hits) and torch.equal(faces_a, scene.last_path_faces)
    assert int(a[2][:, 0].sum()) == 346
    c = scene.render_paths(o, d, 6, "reflect", refraction="snell")
    assert int(c[2][:, 0].sum()) == 342 and not torch.equal(c[1], a[1])          # (the flag is not ignored)
    with pytest.raises(ValueError, match="refraction"):
        scene.render_paths(o, d, 6, "reflect", refraction="bent")
    with pytest.raises(ValueError, match="refraction"):
        scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", refraction=1)


def _explicit_reference_child(out):
    det.enable(True)
    Render.intIOR, Render.extIOR = IOR, EXT
    scene, V, o, d, sp, valid = _hand()
    res = {}
    for tag, kw in (("plain", {}), ("explicit", {"refraction": "reference"})):
        out_ori, out_dir, mask = scene.render_paths(o, d, 6, "reflect", **kw)
        g, = torch.autograd.grad(Render.ray_loss(out_ori, out_dir, mask, sp, valid), V)
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect", **kw)
        g1, = torch.autograd.grad(loss, V)
        res[tag + "_dense"], res[tag + "_fused"], res[tag + "_loss"] = g.cpu().numpy(), g1.cpu().numpy(), loss.detach().cpu().numpy()
    np.savez(out, **res)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_reference_refraction_passed_explicitly_gives_the_same_gradient_bits(tmp_path):
    """Deterministic mode, in a fresh process (the mode is a property of the process's library state)."""
    out = str(tmp_path / "explicit.npz")
    kid = multiprocessing.get_context("spawn").Process(target=_explicit_reference_child, args=(out,))
    kid.start()
    kid.join(CHILD_TIMEOUT)
    if kid.is_alive():
        kid.kill()
        kid.join()
    assert kid.exitcode == 0
    r = np.load(out)
    assert np.abs(r["plain_dense"]).max() > 0
    for what in ("dense", "fused", "loss"):
        assert np.array_equal(_bits(r["plain_" + what]), _bits(r["explicit_" + what])), what


# ------------------------------------------------------------------------------------------------------------- 3. the one-pass form
def _dense(scene, V, o, d, sp, valid, law):
    out_ori, out_dir, mask = scene.render_paths(o, d, *law)
    loss = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    g, = torch.autograd.grad(loss, V)
    return loss.detach(), g, mask[:, 0].clone()


def _fused(scene, V, o, d, sp, valid, law):
    loss = scene.paths_ray_loss_fused(o, d, sp, valid, *law)
    assert loss.shape == () and loss.dtype == torch.float64
    g, = torch.autograd.grad(loss, V)
    return loss.detach(), g


SNELL6 = (6, "reflect", "snell")


def test_one_pass_snell_gives_the_bits_of_the_dense_route_in_deterministic_mode(deterministic):
    scene, V, o, d, sp, valid = _hand()
    l_ref, g_ref, mask = _dense(scene, V, o, d, sp, valid, SNELL6)
    assert int(mask.sum()) == 342
    l_got, g_got = _fused(scene, V, o, d, sp, valid, SNELL6)
    assert g_ref.abs().max() > 0
    assert torch.equal(l_got, l_ref)
    assert torch.equal(g_got, g_ref)


def test_one_pass_snell_agrees_with_the_dense_route_in_float64_mode(float_mode):
    scene, V, o, d, sp, _ = _hand()
    valid = torch.ones(o.shape[0], dtype=torch.bool, device="cuda")
    l_ref, g_ref, mask = _dense(scene, V, o, d, sp, valid, SNELL6)
    l_got, g_got = _fused(scene, V, o, d, sp, valid, SNELL6)
    assert int(scene.last_path_count) == 342
    assert abs(l_got.item() - l_ref.item()) <= ROUTE_REL * abs(l_ref.item())
    assert (g_got - g_ref).abs().max().item() <= ROUTE_REL * g_ref.abs().max().item()
    _grad_close(g_got, g_ref)


# ----------------------------------------------------------------------------------------------------------------------- 4. C ABI
def _fwd(name, scene, V, o, d, k, flag):
    n = o.shape[0]
    out = dict(out_ori=torch.empty((n, 3), dtype=torch.float64, device="cuda"), out_dir=torch.empty((n, 3), dtype=torch.float64, device="cuda"),
               mask=torch.empty((n, 3), dtype=torch.uint8, device="cuda"), tape=torch.empty((k, n), dtype=torch.int32, device="cuda"),
               hits=torch.empty(n, dtype=torch.uint8, device="cuda"), valid_idx=torch.zeros(n, dtype=torch.int32, device="cuda"),
               n_valid=torch.zeros(1, dtype=torch.int64, device="cuda"))
    rc = getattr(_lib.lib(), name)(scene.optix_mesh._h, V.data_ptr(), o.data_ptr(), d.data_ptr(), n, IOR, EXT, k, flag, out["out_ori"].data_ptr(),
                                   out["out_dir"].data_ptr(), out["mask"].data_ptr(), out["tape"].data_ptr(), out["hits"].data_ptr(),
                                   out["valid_idx"].data_ptr(), out["n_valid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    return rc, out


def _bwd(name, scene, V, o, d, k, flag, f, g_ori, g_dir):
    grad = det.acc(V)
    rc = getattr(_lib.lib(), name)(scene.optix_mesh._h, V.data_ptr(), o.data_ptr(), d.data_ptr(), o.shape[0], IOR, EXT, k, flag, f["tape"].data_ptr(),
                                   f["hits"].data_ptr(), f["valid_idx"].data_ptr(), f["n_valid"].data_ptr(), g_ori.data_ptr(), g_dir.data_ptr(),
                                   grad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return rc, grad


def _one_pass(name, scene, V, o, d, sp, va, k, flag):
    loss, grad, count = det.scalar(V.device), det.acc(V), torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = getattr(_lib.lib(), name)(scene.optix_mesh._h, V.data_ptr(), o.data_ptr(), d.data_ptr(), sp.data_ptr(), va.data_ptr(), o.shape[0], IOR, EXT,
                                   k, flag, loss.data_ptr(), grad.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return rc, loss, grad, count


def test_law_entry_points(deterministic):
    lib = _lib.lib()
    assert lib.drt_version() >= 5
    scene, V, o, d, sp, valid = _hand()
    Vd, va = V.detach(), valid.view(torch.uint8)
    rng = np.random.default_rng(5)
    g_ori, g_dir = (torch.tensor(rng.standard_normal(tuple(o.shape)), device="cuda") for _ in range(2))
    # law_flags = DRT_LAW_REFLECT: the bits of the namesakes with reflect = 1
    rc_a, fa = _fwd("drt_render_paths_forward", scene, Vd, o, d, 6, 1)
    rc_b, fb = _fwd("drt_render_paths_law_forward", scene, Vd, o, d, 6, 1)
    assert rc_a == 0 and rc_b == 0 and int(fa["n_valid"]) == 346
    nv = int(fa["n_valid"])
    for key in fa:
        if key == "valid_idx":          # (the list's order across blocks is the order their appends landed in: compare it as a set)
            assert torch.equal(fa[key][:nv].sort().values, fb[key][:nv].sort().values)
        else:
            assert torch.equal(fa[key], fb[key]), key
    rc_a, ga = _bwd("drt_render_paths_backward", scene, Vd, o, d, 6, 1, fa, g_ori, g_dir)
    rc_b, gb = _bwd("drt_render_paths_law_backward", scene, Vd, o, d, 6, 1, fb, g_ori, g_dir)
    assert rc_a == 0 and rc_b == 0 and torch.equal(ga, gb) and det.value(ga, Vd).abs().max() > 0
    a = _one_pass("drt_render_paths_ray_loss_fused", scene, Vd, o, d, sp, va, 6, 1)
    b = _one_pass("drt_render_paths_law_ray_loss_fused", scene, Vd, o, d, sp, va, 6, 1)
    assert a[0] == 0 and b[0] == 0 and int(a[3]) > 256
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    # DRT_LAW_REFLECT | DRT_LAW_SNELL is what the Scene call runs
    rc, fs = _fwd("drt_render_paths_law_forward", scene, Vd, o, d, 6, 3)
    out_ori, out_dir, mask = scene.render_paths(o, d, 6, "reflect", refraction="snell")
    assert rc == 0 and int(fs["n_valid"]) == 342 and torch.equal(fs["out_dir"], out_dir.detach()) and torch.equal(fs["tape"], scene.last_path_faces)
    # any other bit is DRT_E_INVALID and the message names the argument; the namesakes keep their own check
    assert _fwd("drt_render_paths_law_forward", scene, Vd, o, d, 6, 4)[0] == -1 and b"law_flags" in lib.drt_last_error()
    assert _bwd("drt_render_paths_law_backward", scene, Vd, o, d, 6, 4, fa, g_ori, g_dir)[0] == -1 and b"law_flags" in lib.drt_last_error()
    assert _one_pass("drt_render_paths_law_ray_loss_fused", scene, Vd, o, d, sp, va, 6, 4)[0] == -1 and b"law_flags" in lib.drt_last_error()
    assert _fwd("drt_render_paths_law_forward", scene, Vd, o, d, 9, 3)[0] == -1 and b"max_bounces" in lib.drt_last_error()
    assert _fwd("drt_render_paths_forward", scene, Vd, o, d, 6, 2)[0] == -1 and b"reflect" in lib.drt_last_error()


# --------------------------------------------------------------------------------------------------------------- 5. law consistency
def test_the_true_mesh_explains_snell_targets_only_under_snell(float_mode):
    """The reason for the feature.  Targets traced through hand_vh itself by Snell's law (SyntheticData(path_law=(2, "drop", "snell"))):
    the refraction term of the SAME mesh is zero under Snell -- at most 1e-20 per contributing ray -- while under the reference's formula it
    is what the restatements compute for that view from the same targets (6.15 on view 5 in the probe behind the feature: a correct mesh
    would be deformed to make up for it)."""
    from drt_amd import captured_data
    Render.resx = Render.resy = RES
    mesh = _mesh()
    center, extent = views.mesh_frame(mesh.vertices)
    scene = Render.Scene(mesh, 0)
    data = captured_data.SyntheticData(scene, center, extent, RES, RES, num_view=72, n_total=72, view_ids=[5], seed=0, name="hand",
                                       path_law=(2, "drop", "snell"))
    target, valid, _, origin, ray_dir, _ = data.get_view(5)
    n_targets = int(valid.sum())          # (the paths valid under Snell, less any whose exit ray runs away from the screen plane)
    assert 150 < n_targets <= 226
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    same = scene.paths_ray_loss_fused(origin, ray_dir, target, valid, 2, "drop", refraction="snell")
    n_same = int(scene.last_path_count)
    print("Snell targets, Snell fit: loss", same.item(), "over", n_same, "rays")
    assert n_same == n_targets and same.item() <= 1e-20 * n_same
    other = scene.paths_ray_loss_fused(origin, ray_dir, target, valid, 2, "drop")
    n_other = int(scene.last_path_count)
    o, d = origin.cpu(), ray_dir.cpu()
    out_ori, out_dir, mask, _ = snell_ref.render_paths(mesh.faces, torch.tensor(mesh.vertices, dtype=torch.float64), o, d, IOR, EXT, 2, "drop",
                                                       "reference")
    ref = orc.ray_loss(out_ori, out_dir, mask, target.cpu(), valid.cpu().bool()).item()
    print("Snell targets, reference fit: loss", other.item(), "over", n_other, "rays; restatement", ref)
    assert n_other == int((mask[:, 0] & valid.cpu().bool()).sum()) and 150 < n_other < n_targets
    assert ref > 1.0 and abs(other.item() - ref) <= 1e-9 * ref


# ------------------------------------------------------------------------------------------------------------------------ 6. graph
def test_eager_snell_call_and_graph_replays_give_the_same_bits(deterministic):
    scene, V, o, d, sp, valid = _hand()

    def step():
        # (the update belongs inside the captured region: a consumer of the tree waits for the build's event)
        scene.update_verticex(V)
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, *SNELL6)
        g, = torch.autograd.grad(loss, V)
        return loss.detach(), g

    l1, g1 = step()
    assert g1.abs().max() > 0
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
    l3.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g3, g1) and torch.equal(l3, l1)


# ------------------------------------------------------------------------------------------------------------------------- 7. loop
def test_fused_iteration_with_the_snell_law_follows_the_drop_in_loop(monkeypatch, float_mode):
    """10 iterations of FusedIteration(path_law=(6, "reflect", "snell")) against optimize(fused=False) with the HyperParams spelling on
    the recorded hand capture: the same terms, float64 sums in another order -- the parameters agree within the 1e-12 mm that
    tests/test_gpu_trajectory.py asserts for its replays."""
    from drt_amd import optim as O
    g = tc.load("hand_trajectory")
    hand = tc.frame_mesh("hand_trajectory")
    Render.intIOR = float(g["ior"])
    Render.resx = Render.resy = int(g["res"])
    lr = float(g["lr"])
    hp0 = dict(O.HyperParams, IOR=float(g["ior"]), Pass=1, Iters=10, start_lr=lr)

    def fresh():
        return Render.Scene(mesh_io.TriMesh(g["vertices"].astype(np.float64), hand.faces), 0), tc.RecordedCapture(g, hand.vertices, "cuda")

    made = []
    setup_opt = O.setup_opt
    monkeypatch.setattr(O, "setup_opt", lambda *a, **k: made.append(setup_opt(*a, **k)) or made[-1])
    scene, data = fresh()
    O.optimize(scene, data, dict(hp0, max_bounces=6, tir="reflect", refraction="snell"), remesh=None, output=False, fused=False)
    ref = made[0][1].detach()

    scene, data = fresh()
    it = O.FusedIteration(scene, data, hp0, lr, path_law=SNELL6)
    assert it.law == SNELL6
    for _ in range(10):
        it.step()
    torch.cuda.synchronize()
    diff = (it.parameter - ref).abs().max().item()
    print(f"FusedIteration(path_law={SNELL6}) against the drop-in loop after 10 iterations: parameter difference {diff:.3e} mm, "
          f"largest parameter {ref.abs().max().item():.3e} mm")
    assert ref.abs().max().item() > 1e-3
    assert diff <= 1e-12

    # and the law is not the reference's: the same loop under (6, "reflect") ends elsewhere
    scene, data = fresh()
    it_ref = O.FusedIteration(scene, data, hp0, lr, path_law=(6, "reflect", "reference"))
    assert it_ref.law == (6, "reflect")
    for _ in range(10):
        it_ref.step()
    assert (it_ref.parameter - it.parameter).abs().max().item() > 1e-6


# ------------------------------------------------------------------------------------------------------------------------ 8. ranks
LAW = (4, "reflect", "snell")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(rank, world, hp):
    """hand_vh and a synthetic capture (traced with LAW) of N_VIEWS views of which this rank renders only its own; deterministic mode."""
    from drt_amd import captured_data, dist as ddist
    det.enable(True)
    Render.intIOR = IOR
    Render.resx = Render.resy = RES
    mesh = _mesh()
    center, extent = views.mesh_frame(mesh.vertices)
    gt = Render.Scene(views.displaced_ground_truth(mesh, sigma=0.3, seed=0), 0)
    ray_ids = captured_data.ray_view_ids(N_VIEWS, hp["num_view"], "hand")
    mine = sorted(set(ddist.owned_views(ray_ids, rank, world)) | set(ddist.owned_views(captured_data.silh_view_ids(N_VIEWS), rank, world)))
    data = captured_data.SyntheticData(gt, center, extent, RES, RES, num_view=hp["num_view"], n_total=N_VIEWS, view_ids=mine, seed=0, name="hand",
                                       path_law=LAW)
    return Render.Scene(mesh, 0), data


def _case(rank, world):
    from drt_amd import optim as O
    hp = dict(O.HyperParams, num_view=N_VIEWS)
    scene, data = _setup(rank, world, hp)
    it = O.ShardedIteration(scene, data, hp, 0.1, views_per_step=2, path_law=LAW)
    assert it.law == LAW
    losses = []
    for _ in range(4):
        total, parts = it.step()
        losses.append(torch.cat([total.view(1), parts]).cpu().numpy())
    torch.cuda.synchronize()
    return {"param": it.parameter.cpu().numpy(), "losses": np.array(losses)}


def _init_group(rank, world, port):
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                         timeout=datetime.timedelta(seconds=120))


def _child(rank, world, port, out_dir):
    torch.cuda.set_device(0)
    _init_group(rank, world, port)
    try:
        np.savez(os.path.join(out_dir, f"snell_rank{rank}.npz"), **_case(rank, world))
    finally:
        torch.distributed.destroy_process_group()


@pytest.fixture()
def det_restored():
    yield
    det.enable(os.environ.get("DRT_DETERMINISTIC", "0") not in ("", "0"))


def test_two_ranks_equal_one_rank_bit_for_bit_under_snell(det_restored, tmp_path):
    port = _free_port()
    kid = multiprocessing.get_context("spawn").Process(target=_child, args=(1, 2, port, str(tmp_path)))
    kid.start()
    try:
        _init_group(0, 2, port)
        try:
            r0 = _case(0, 2)
        finally:
            torch.distributed.destroy_process_group()
    finally:
        kid.join(CHILD_TIMEOUT)
        if kid.is_alive():
            kid.kill()
            kid.join()
    assert kid.exitcode == 0
    r1 = dict(np.load(tmp_path / "snell_rank1.npz"))
    one = _case(0, 1)
    assert np.abs(one["param"]).max() > 1e-3 and np.isfinite(one["param"]).all() and (one["losses"][:, 1] > 0).all()
    for r in (r0, r1):
        assert np.array_equal(_bits(r["param"]), _bits(one["param"])) and np.array_equal(_bits(r["losses"]), _bits(one["losses"]))


# -------------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_reconstruct_refraction_snell_fused_paths(tmp_path):
    cmd = [sys.executable, "-m", "drt_amd.reconstruct", "--name", "hand", "--res", "64", "--views", "8", "--num-view", "8", "--passes", "1",
           "--iters", "4", "--max-bounces", "4", "--tir", "reflect", "--refraction", "snell", "--fused-paths", "--data-path", data_path(""),
           "--result-path", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rep = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")][-1]
    assert rep["refraction"] == "snell" and rep["max_bounces"] == 4 and rep["tir"] == "reflect" and rep["path_route"] == "fused"
    assert rep["iterations"] == 4
