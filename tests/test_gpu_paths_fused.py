"""GPU: the one-pass form of the K-interaction law -- Scene.paths_ray_loss_fused / drt_render_paths_ray_loss_fused (loss and vertex
gradient of one view in one call, nothing dense written; drt_amd/csrc/drt_paths.hip) and the ``path_law=(K, tir)`` keyword that takes it
into FusedIteration, ShardedIteration, optimize, optimize_sharded and ``reconstruct --fused-paths``.

References: the chain of the reference's own pieces (tests/golden/hand_r64_v5_paths.npz), the dense route render_paths + ray_loss +
backward (bit for bit in deterministic mode: both routes run ray_loss_term and the drt_paths.h functions on the same parked bits, and
the fixed-point sums are exact at every level), and the two-bounce one-pass kernel at (2, drop).  Tolerances are the project's: loss 1e-10
relative; gradients 1e-9 relative to the largest reference entry and 1e-5 absolute; across routes in float64 mode 1e-12 relative.
hand_vh at 64 x 64, view 5 (4096 rays): 346 valid paths at (6, reflect), more than one 256-ray table fill of the last kernel."""
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

import trajectory_case as tc
from conftest import IOR, ROOT, data_path, fixture_view, golden
from drt_amd import _lib, det, diffrender as Render, mesh_io
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu
EXT = orc.EXT_IOR
GRAD_REL, GRAD_ABS, LOSS_REL, ROUTE_REL = 1e-9, 1e-5, 1e-10, 1e-12
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


def _hand():
    g = golden("hand_r64_v5")
    o, d, sp, valid = fixture_view(g)
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene, V, o.cuda(), d.cuda(), sp.cuda(), valid.cuda()


def _dense(scene, V, o, d, sp, valid, k, tir):
    """(loss, d loss / d V, mask) of render_paths + ray_loss + backward with a unit seed."""
    out_ori, out_dir, mask = scene.render_paths(o, d, k, tir)
    loss = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    g, = torch.autograd.grad(loss, V)
    return loss.detach(), g, mask[:, 0].clone()


def _fused(scene, V, o, d, sp, valid, k, tir):
    loss = scene.paths_ray_loss_fused(o, d, sp, valid, k, tir)
    assert loss.shape == () and loss.dtype == torch.float64
    g, = torch.autograd.grad(loss, V)
    return loss.detach(), g


# ---------------------------------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("tag,k,tir", [("k6_reflect", 6, "reflect"), ("k4_drop", 4, "drop")])
def test_golden_chain_of_the_reference(tag, k, tir):
    g = golden("hand_r64_v5_paths")
    scene, V, o, d, sp, valid = _hand()
    before = Render.cache_report().get("paths_fused_calls", 0)          # (a counter: absent until the first call)
    loss = scene.paths_ray_loss_fused(o, d, sp, valid, k, tir)
    loss.backward()
    assert Render.cache_report()["paths_fused_calls"] == before + 1
    assert loss.item() == pytest.approx(float(g[f"{tag}_ray_loss"]), rel=LOSS_REL)
    r = _grad_close(V.grad, g[f"{tag}_grad_ray_loss"])
    assert scene.last_path_count.dtype == torch.int64 and scene.last_path_count.is_cuda
    assert int(scene.last_path_count) == int((torch.tensor(g[f"{tag}_mask"]).cuda() & valid).sum())
    print(tag, "contributing rays", int(scene.last_path_count), "gradient disagreement (relative to max)", r)


# --------------------------------------------------------------------------------------- 2. the dense route's bits, deterministic mode
@pytest.mark.parametrize("k,tir,expect_valid", [(6, "reflect", 346), (2, "drop", 257)])
def test_bits_of_the_dense_route_in_deterministic_mode(deterministic, k, tir, expect_valid):
    scene, V, o, d, sp, valid = _hand()
    l_ref, g_ref, mask = _dense(scene, V, o, d, sp, valid, k, tir)
    assert int(mask.sum()) == expect_valid
    l_got, g_got = _fused(scene, V, o, d, sp, valid, k, tir)
    assert g_ref.abs().max() > 0
    assert torch.equal(l_got, l_ref)
    assert torch.equal(g_got, g_ref)


# --------------------------------------------------------------------------------------------- 3. the two-bounce one-pass kernel
def test_two_bounces_drop_agrees_with_ray_loss_fused(float_mode):
    scene, V, o, d, sp, valid = _hand()
    Render.resx = Render.resy = 64
    l_got, g_got = _fused(scene, V, o, d, sp, valid, 2, "drop")
    l_ref = scene.ray_loss_fused(o, d, sp, valid)
    g_ref, = torch.autograd.grad(l_ref, V)
    assert g_ref.abs().max() > 0
    assert abs(l_got.item() - l_ref.item()) <= ROUTE_REL * abs(l_ref.item())
    assert (g_got - g_ref).abs().max().item() <= ROUTE_REL * g_ref.abs().max().item()


# -------------------------------------------------------------------------------------------------------------------- 4. targets
def test_rays_without_a_target_do_not_contribute(float_mode):
    scene, V, o, d, sp, _ = _hand()
    n = o.shape[0]
    valid = torch.tensor(np.random.default_rng(7).random(n) > 0.25).cuda()
    l_ref, g_ref, mask = _dense(scene, V, o, d, sp, valid, 6, "reflect")
    assert int((mask & valid).sum()) > 0 and int((mask & ~valid).sum()) > 0
    l_got, g_got = _fused(scene, V, o, d, sp, valid, 6, "reflect")
    assert int(scene.last_path_count) == int((mask & valid).sum())
    assert l_got.item() == pytest.approx(l_ref.item(), rel=LOSS_REL)
    _grad_close(g_got, g_ref)


# -------------------------------------------------------------------------------------------------------------- 5. nothing dense
def _abi(scene, V, o, d, sp, va, k, reflect, loss, grad, count):
    return _lib.lib().drt_render_paths_ray_loss_fused(scene.optix_mesh._h, V.data_ptr(), _lib.ptr(o), _lib.ptr(d), _lib.ptr(sp), _lib.ptr(va),
                                                      0 if o is None else o.shape[0], IOR, EXT, k, reflect, _lib.ptr(loss), _lib.ptr(grad),
                                                      _lib.ptr(count), torch.cuda.current_stream().cuda_stream)


def test_the_inputs_are_not_written():
    scene, V, o, d, sp, valid = _hand()
    keep = [t.clone() for t in (o, d, sp, valid)]
    _fused(scene, V, o, d, sp, valid, 6, "reflect")
    torch.cuda.synchronize()
    for a, b in zip(keep, (o, d, sp, valid)):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int64), b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int64))


def test_two_calls_accumulate_into_the_same_cells(deterministic):
    """The views of a step add into ONE loss cell and ONE gradient array (ShardedIteration): two calls into the same accumulators give
    the exact sum of the two single calls."""
    scene, V, o, d, sp, valid = _hand()
    Vd = V.detach()
    va = valid.view(torch.uint8)
    halves = [(o[:2048].contiguous(), d[:2048].contiguous(), sp[:2048].contiguous(), va[:2048].contiguous()),
              (o[2048:].contiguous(), d[2048:].contiguous(), sp[2048:].contiguous(), va[2048:].contiguous())]
    singles = []
    both = (det.scalar(Vd.device), det.acc(Vd), torch.zeros(1, dtype=torch.int64, device="cuda"))
    for h in halves:
        one = (det.scalar(Vd.device), det.acc(Vd), torch.zeros(1, dtype=torch.int64, device="cuda"))
        assert one[0].dtype == torch.int64
        _lib.check(_abi(scene, Vd, *h, 6, 1, *one))
        _lib.check(_abi(scene, Vd, *h, 6, 1, *both))
        singles.append(one)
    s = torch.cuda.current_stream().cuda_stream
    for j in (0, 1):
        total = singles[0][j].clone()
        _lib.check(_lib.lib().drt_fx_add(total.data_ptr(), singles[1][j].data_ptr(), total.numel() // 3, s))
        assert torch.equal(total, both[j])
        assert torch.equal(det.value(total, Vd if j else None), det.value(both[j], Vd if j else None))
    assert int(singles[0][2]) > 50 and int(singles[1][2]) > 50
    assert int(both[2]) == int(singles[0][2]) + int(singles[1][2])
    _lib.check(_abi(scene, Vd, *halves[0], 6, 1, both[0], both[1], None))          # the count is optional


# ---------------------------------------------------------------------------------------------------------------------- 6. edges
def _marked(V):
    rng = np.random.default_rng(11)
    return (torch.tensor(rng.standard_normal(()), device="cuda"), torch.tensor(rng.standard_normal(tuple(V.shape)), device="cuda"),
            torch.full((1,), 12345, dtype=torch.int64, device="cuda"))


def test_calls_that_contribute_nothing_leave_the_accumulators_alone(float_mode):
    scene, V, o, d, sp, valid = _hand()
    Vd, va = V.detach(), valid.view(torch.uint8)
    acc = _marked(Vd)
    keep = [t.clone() for t in acc]
    _lib.check(_abi(scene, Vd, None, None, None, None, 6, 1, *acc))                                         # no rays
    _lib.check(_abi(scene, Vd, o, (-d).contiguous(), sp, va, 6, 1, *acc))                                    # every camera ray reversed: all miss
    _lib.check(_abi(scene, Vd, o, d, sp, torch.zeros_like(va), 6, 1, *acc))                                  # no ray has a target
    torch.cuda.synchronize()
    for a, b in zip(keep, acc):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # and through the Scene method: zero loss, zero gradient
    e = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    loss = scene.paths_ray_loss_fused(e, e, e, torch.zeros(0, dtype=torch.bool, device="cuda"), 4, "reflect")
    g, = torch.autograd.grad(loss, V)
    assert loss.item() == 0.0 and not g.any() and int(scene.last_path_count) == 0
    loss = scene.paths_ray_loss_fused(o, -d, sp, valid, 4, "reflect")
    assert loss.item() == 0.0 and int(scene.last_path_count) == 0


def test_ray_count_that_is_not_a_multiple_of_64(float_mode):
    scene, V, o, d, sp, valid = _hand()
    part = [t[:4001].contiguous() for t in (o, d, sp, valid)]
    l_ref, g_ref, mask = _dense(scene, V, *part, 6, "reflect")
    assert int(mask.sum()) > 256
    l_got, g_got = _fused(scene, V, *part, 6, "reflect")
    assert int(scene.last_path_count) == int((mask & part[3]).sum())
    assert l_got.item() == pytest.approx(l_ref.item(), rel=LOSS_REL)
    _grad_close(g_got, g_ref)


def test_arguments_are_checked():
    scene, V, o, d, sp, valid = _hand()
    Vd, va = V.detach(), valid.view(torch.uint8)
    acc = _marked(Vd)
    for k in (1, 9):
        rc = _abi(scene, Vd, o, d, sp, va, k, 1, *acc)
        assert rc == -1 and b"max_bounces" in _lib.lib().drt_last_error()          # DRT_E_INVALID
    assert _abi(scene, Vd, o, d, sp, va, 4, 2, *acc) == -1 and b"reflect" in _lib.lib().drt_last_error()
    assert _lib.lib().drt_version() >= 4
    for k in (1, 9, 2.5, True):
        with pytest.raises(ValueError, match="max_bounces"):
            scene.paths_ray_loss_fused(o, d, sp, valid, k, "drop")
    with pytest.raises(ValueError, match="tir"):
        scene.paths_ray_loss_fused(o, d, sp, valid, 4, "mirror")
    with pytest.raises(NotImplementedError):
        scene.paths_ray_loss_fused(o.clone().requires_grad_(True), d, sp, valid, 4, "reflect")
    with pytest.raises(NotImplementedError):
        scene.paths_ray_loss_fused(o, d.clone().requires_grad_(True), sp, valid, 4, "reflect")
    Render.intIOR = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        scene.paths_ray_loss_fused(o, d, sp, valid, 4, "reflect")
    Render.intIOR = IOR
    # a RayBinding lends its rays
    a = scene.paths_ray_loss_fused(scene.bind_rays(o, d), None, sp, valid, 4, "reflect")
    b = scene.paths_ray_loss_fused(o, d, sp, valid, 4, "reflect")
    assert a.item() == pytest.approx(b.item(), rel=ROUTE_REL) and a.item() > 0


# ---------------------------------------------------------------------------------------------------------------------- 7. graph
def test_eager_call_and_graph_replays_give_the_same_bits(deterministic):
    scene, V, o, d, sp, valid = _hand()

    def step():
        # (the update belongs inside the captured region: a consumer of the tree waits for the build's event)
        scene.update_verticex(V)
        loss = scene.paths_ray_loss_fused(o, d, sp, valid, 6, "reflect")
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


# ----------------------------------------------------------------------------------------------------------------------- 8. loop
def test_fused_iteration_with_a_law_follows_the_drop_in_loop(monkeypatch, float_mode):
    """10 iterations of FusedIteration(path_law=(6, "reflect")) against optimize(fused=False) with the HyperParams law on the recorded hand
    capture: the same terms, float64 sums in another order -- the parameters agree within the 1e-12 mm that
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
    O.optimize(scene, data, dict(hp0, max_bounces=6, tir="reflect"), remesh=None, output=False, fused=False)
    ref = made[0][1].detach()

    scene, data = fresh()
    it = O.FusedIteration(scene, data, hp0, lr, path_law=(6, "reflect"))
    assert it.law == (6, "reflect")
    for _ in range(10):
        it.step()
    torch.cuda.synchronize()
    diff = (it.parameter - ref).abs().max().item()
    print(f"FusedIteration(path_law=(6, 'reflect')) against the drop-in loop after 10 iterations: parameter difference {diff:.3e} mm, "
          f"largest parameter {ref.abs().max().item():.3e} mm")
    assert ref.abs().max().item() > 1e-3
    assert diff <= 1e-12

    # the whole loop through the keyword gives what the stepper gave
    scene, data = fresh()
    scene, _ = O.optimize(scene, data, hp0, remesh=None, output=False, fused=True, path_law=(6, "reflect"))
    assert (scene.vertices - it._vertices).abs().max().item() <= 1e-12          # (both hold the vertices the tenth iteration rendered)
    # without a law the object is today's
    scene, data = fresh()
    assert O.FusedIteration(scene, data, hp0, lr).law is None and O.FusedIteration(scene, data, hp0, lr, path_law=(2, "drop")).law is None


# ---------------------------------------------------------------------------------------------------------------------- 9. ranks
LAW = (4, "reflect")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(rank, world, hp):
    """hand_vh and a synthetic capture (traced with LAW) of N_VIEWS views of which this rank renders only its own; deterministic mode."""
    from drt_amd import captured_data, dist as ddist, views
    det.enable(True)
    Render.intIOR = IOR
    Render.resx = Render.resy = RES
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    center, extent = views.mesh_frame(mesh.vertices)
    gt = Render.Scene(views.displaced_ground_truth(mesh, sigma=0.3, seed=0), 0)
    ray_ids = captured_data.ray_view_ids(N_VIEWS, hp["num_view"], "hand")
    mine = sorted(set(ddist.owned_views(ray_ids, rank, world)) | set(ddist.owned_views(captured_data.silh_view_ids(N_VIEWS), rank, world)))
    data = captured_data.SyntheticData(gt, center, extent, RES, RES, num_view=hp["num_view"], n_total=N_VIEWS, view_ids=mine, seed=0, name="hand",
                                       path_law=LAW)
    return Render.Scene(mesh, 0), data


def _run(make, n_iter):
    it = make()
    losses = []
    for _ in range(n_iter):
        total, parts = it.step()
        losses.append(torch.cat([total.view(1), parts]).cpu().numpy())
    torch.cuda.synchronize()
    return {"param": it.parameter.cpu().numpy(), "losses": np.array(losses)}


def _case(rank, world):
    from drt_amd import optim as O
    hp = dict(O.HyperParams, num_view=N_VIEWS)
    scene, data = _setup(rank, world, hp)
    return _run(lambda: O.ShardedIteration(scene, data, hp, 0.1, views_per_step=2, path_law=LAW), 6)


def _init_group(rank, world, port):
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                         timeout=datetime.timedelta(seconds=120))


def _child(rank, world, port, out_dir):
    torch.cuda.set_device(0)
    _init_group(rank, world, port)
    try:
        np.savez(os.path.join(out_dir, f"law_rank{rank}.npz"), **_case(rank, world))
    finally:
        torch.distributed.destroy_process_group()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture()
def det_restored():
    yield
    det.enable(os.environ.get("DRT_DETERMINISTIC", "0") not in ("", "0"))


def test_two_ranks_equal_one_rank_bit_for_bit(det_restored, tmp_path):
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
    r1 = dict(np.load(tmp_path / "law_rank1.npz"))
    one = _case(0, 1)
    assert np.abs(one["param"]).max() > 1e-3 and np.isfinite(one["param"]).all() and (one["losses"][:, 1] > 0).all()
    for r in (r0, r1):
        assert np.array_equal(_bits(r["param"]), _bits(one["param"])) and np.array_equal(_bits(r["losses"]), _bits(one["losses"]))


def test_one_rank_one_view_is_the_fused_iteration(det_restored):
    from drt_amd import optim as O
    hp = dict(O.HyperParams, num_view=N_VIEWS)
    runs = []
    for cls in (O.FusedIteration, O.ShardedIteration):
        scene, data = _setup(0, 1, hp)
        data.rng = np.random.RandomState(0)
        runs.append(_run(lambda: cls(scene, data, hp, 0.1, path_law=LAW), 5))
    a, b = runs
    assert np.abs(a["param"]).max() > 1e-3 and (a["losses"][:, 1] > 0).all()
    assert np.array_equal(_bits(a["param"]), _bits(b["param"])) and np.array_equal(_bits(a["losses"]), _bits(b["losses"]))


# ----------------------------------------------------------------------------------------------------------------------- 10. CLI
def test_reconstruct_fused_paths(tmp_path):
    cmd = [sys.executable, "-m", "drt_amd.reconstruct", "--name", "hand", "--res", "64", "--views", "8", "--num-view", "8", "--passes", "1",
           "--iters", "4", "--max-bounces", "6", "--tir", "reflect", "--fused-paths", "--data-path", data_path(""), "--result-path", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rep = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")][-1]
    assert rep["max_bounces"] == 6 and rep["tir"] == "reflect" and rep["path_route"] == "fused" and rep["iterations"] == 4
