"""The multi-rank reconstruction loop (drt_amd.optim.ShardedIteration / optimize_sharded, python -m drt_amd.reconstruct --views-per-step):
the post-exchange kernels against the chains they replace, one rank against the single-process loop, two and three ranks (gloo, every
rank on cuda:0) against one, the collective count, and the CLI under torch.distributed.run.  Rank 0 of a multi-rank case is this process,
the others are spawned: never more than three processes hold the GPU."""
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

from conftest import IOR, ROOT, data_path, golden

pytestmark = pytest.mark.gpu

RES, N_VIEWS = 64, 8
CHILD_TIMEOUT = 300


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- 4. the new kernels equal the chains they replace --------------------------------------------------------------------------------

def _random_cells(rng, m):
    """m fixed-point cells (hi, lo, flags) as int64 [m, 3]: values from ~4e-9 to ~3e7 of either sign, some with sticky flags set."""
    cells = np.zeros((m, 3), dtype=np.int64)
    scale = rng.integers(-40, 24, m)                       # value ~ 2^scale
    for i in range(m):
        q = int(rng.integers(1 << 52, 1 << 53)) << max(0, 80 + int(scale[i]) - 52)
        if rng.random() < 0.5:
            q = -q
        q %= 1 << 128
        lo, hi = q & ((1 << 64) - 1), q >> 64
        cells[i, 0] = hi - (1 << 64) if hi >= 1 << 63 else hi
        cells[i, 1] = lo - (1 << 64) if lo >= 1 << 63 else lo
    flags = rng.random(m)
    cells[flags < 0.01, 2] = 1                             # NaN
    cells[(flags >= 0.01) & (flags < 0.02), 2] = 2         # +inf / huge
    cells[(flags >= 0.02) & (flags < 0.03), 2] = 4         # -inf / huge
    cells[(flags >= 0.03) & (flags < 0.035), 2] = 6        # both: NaN after the sum
    return cells


def test_limbs_step_equals_from_limbs_finalize_limit_sgd_step3():
    """drt_fx_limbs_limit_sgd_step3 == drt_fx_from_limbs -> drt_fx_finalize -> drt_limit_sgd_step3, bit for bit: parameter, momentum,
    gradient, loss parts and total, over two steps (first and later), on the rank sum of two ranks' exchange words."""
    from drt_amd import _lib
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    n = 3 * 1111                                           # (not a multiple of the block)
    m = 3 * n + 3
    w = torch.tensor([40 * 217.5 / 64 / 64 / 3, 2e-3 * 217.5 / 64, 0.08 * 3.3 / 10], dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    param_a = torch.tensor(rng.standard_normal(n), device=dev)
    param_b = param_a.clone()
    buf_a, buf_b = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    saw_clamp = saw_nan = 0
    for first in (1, 0):
        limbs = torch.zeros(m * 4, dtype=torch.int64, device=dev)
        for _ in range(2):                                 # two ranks' words, summed as the all-reduce sums them
            cells = torch.tensor(_random_cells(rng, m).reshape(-1), device=dev)
            one = torch.empty(m * 4, dtype=torch.int64, device=dev)
            _lib.check(lib.drt_fx_to_limbs(cells.data_ptr(), m, one.data_ptr(), s))
            limbs += one
        # the chain
        summed = torch.empty(m * 3, dtype=torch.int64, device=dev)
        vals = torch.empty(m, dtype=torch.float64, device=dev)
        grad_a, parts_a, total_a = torch.empty(n, dtype=torch.float64, device=dev), vals[3 * n:], torch.empty((), dtype=torch.float64, device=dev)
        _lib.check(lib.drt_fx_from_limbs(limbs.data_ptr(), m, summed.data_ptr(), s))
        _lib.check(lib.drt_fx_finalize(summed.data_ptr(), m, vals.data_ptr(), 0, s))
        _lib.check(lib.drt_limit_sgd_step3(param_a.data_ptr(), grad_a.data_ptr(), buf_a.data_ptr(), n, 0.1, 0.95, 1, first, 1.0, vals.data_ptr(),
                                           w.data_ptr(), parts_a.data_ptr(), total_a.data_ptr(), s))
        # the one kernel
        grad_b, parts_b, total_b = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev), torch.empty((), dtype=torch.float64, device=dev)
        _lib.check(lib.drt_fx_limbs_limit_sgd_step3(limbs.data_ptr(), n, param_b.data_ptr(), grad_b.data_ptr(), buf_b.data_ptr(), 0.1, 0.95, 1, first,
                                                    1.0, w.data_ptr(), parts_b.data_ptr(), total_b.data_ptr(), s))
        torch.cuda.synchronize()
        for a, b in ((param_a, param_b), (buf_a, buf_b), (grad_a, grad_b), (parts_a, parts_b), (total_a, total_b)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        t = vals[:3 * n]
        saw_clamp += int((grad_a.abs() == 1.0).sum())
        saw_nan += int(torch.isnan(t).sum())
    assert saw_clamp > 100 and saw_nan > 10 and bool(torch.isinf(vals).any())


def test_weighted_partial_then_step_total_equals_limit_sgd_step3():
    """Float64 form: drt_weight_terms3 -> drt_limit_sgd_step_total == drt_limit_sgd_step3 on the same terms (one rank), bit for bit."""
    from drt_amd import _lib
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    n = 3 * 777
    terms = torch.tensor(rng.standard_normal(3 * n) * np.exp(rng.uniform(-8, 6, 3 * n)), device=dev)
    terms[::97] = float("nan")
    parts = torch.tensor(rng.random(3) * 100, device=dev)
    w = torch.tensor([0.0212, 6.7968e-3, 0.0263], dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    pa = torch.tensor(rng.standard_normal(n), device=dev)
    pb = pa.clone()
    ba, bb = torch.empty_like(pa), torch.empty_like(pa)
    for first in (1, 0):
        ga, ta = torch.empty_like(pa), torch.empty((), dtype=torch.float64, device=dev)
        _lib.check(lib.drt_limit_sgd_step3(pa.data_ptr(), ga.data_ptr(), ba.data_ptr(), n, 0.1, 0.95, 1, first, 1.0, terms.data_ptr(), w.data_ptr(),
                                           parts.data_ptr(), ta.data_ptr(), s))
        x = torch.empty(n + 3, dtype=torch.float64, device=dev)
        x[n:] = parts
        tb = torch.empty((), dtype=torch.float64, device=dev)
        _lib.check(lib.drt_weight_terms3(terms.data_ptr(), w.data_ptr(), n, x.data_ptr(), s))
        _lib.check(lib.drt_limit_sgd_step_total(pb.data_ptr(), x.data_ptr(), bb.data_ptr(), n, 0.1, 0.95, 1, first, 1.0, w.data_ptr(),
                                                x[n:].data_ptr(), tb.data_ptr(), s))
        torch.cuda.synchronize()
        for a, b in ((pa, pb), (ba, bb), (ga, x[:n]), (ta, tb)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert int((ga.abs() == 1.0).sum()) > 100


# ---- the loop on 1, 2 and 3 ranks ---------------------------------------------------------------------------------------------------

def _setup(rank, world, det_mode, hp, smooth=False):
    """hand_vh (``smooth``: its smoothed form, on which every dihedral term is finite) and a synthetic capture of N_VIEWS views of which
    this rank renders only its own."""
    from drt_amd import captured_data, det, diffrender as Render, dist as ddist, mesh_io, views
    det.enable(det_mode)
    Render.intIOR = IOR
    Render.resx = Render.resy = RES
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    center, extent = views.mesh_frame(mesh.vertices)
    gt = Render.Scene(views.displaced_ground_truth(mesh, sigma=0.3, seed=0), 0)
    ray_ids = captured_data.ray_view_ids(N_VIEWS, hp["num_view"], "hand")
    mine = sorted(set(ddist.owned_views(ray_ids, rank, world)) | set(ddist.owned_views(captured_data.silh_view_ids(N_VIEWS), rank, world)))
    data = captured_data.SyntheticData(gt, center, extent, RES, RES, num_view=hp["num_view"], n_total=N_VIEWS, view_ids=mine, seed=0, name="hand")
    assert sorted(data.Views) == mine
    if smooth:
        mesh = mesh_io.TriMesh(golden("hand_smooth_sm")["vertices"].astype(np.float64), mesh.faces)
    return Render.Scene(mesh, 0), data


def _hp(**kw):
    from drt_amd import optim as O
    return dict(O.HyperParams, num_view=N_VIEWS, **kw)


def _case(case, rank, world):
    """One rank's part of a case; returns a dict of numpy arrays (bit patterns where they are compared bit for bit)."""
    from drt_amd import optim as O
    if case == "remesh":          # 6 + 9: deterministic, k = 4, two passes with the device remesher
        hp = _hp(Pass=2, Iters=3, start_len=6, end_len=4)
        scene, data = _setup(rank, world, True, hp)
        scene, history, stats = O.optimize_sharded(scene, data, hp, views_per_step=4, output=False)
        torch.cuda.synchronize()
        return {"V": scene.vertices.detach().cpu().numpy(), "F": scene.faces.cpu().numpy(), "history": np.array(history),
                "stats": np.array([stats["iterations"], stats["allreduces"], stats["passes"], stats["broadcasts"], stats["allreduces_per_iteration"],
                                   stats["broadcasts_per_pass"]], dtype=np.float64)}
    if case in ("empty", "float"):
        # empty (7): deterministic, k = 2 on three ranks, no silhouette term -- the ranks that draw none of their refraction views own
        # nothing in that iteration (the silhouette term draws all N_VIEWS views every iteration: with it every rank would own some)
        # float (8): float64 mode, k = 4, all three terms
        det_mode, k = (True, 2) if case == "empty" else (False, 4)
        hp = _hp(vh_w=0) if case == "empty" else _hp()
        scene, data = _setup(rank, world, det_mode, hp)
        it = O.ShardedIteration(scene, data, hp, 0.1, views_per_step=k)
        losses, owned = [], []
        for _ in range(6):
            total, parts = it.step()
            losses.append(torch.cat([total.view(1), parts]).cpu().numpy())
            owned.append(it.last_owned)
        torch.cuda.synchronize()
        return {"param": it.parameter.cpu().numpy(), "losses": np.array(losses), "owned": np.array(owned), "n_allreduce": np.array(it.n_allreduce)}
    raise ValueError(case)


def _init_group(rank, world, port):
    torch.distributed.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                         timeout=datetime.timedelta(seconds=120))


def _child(case, rank, world, port, out_dir):
    torch.cuda.set_device(0)
    _init_group(rank, world, port)
    try:
        np.savez(os.path.join(out_dir, f"{case}_rank{rank}.npz"), **_case(case, rank, world))
    finally:
        torch.distributed.destroy_process_group()


def _ranks(case, world, tmp_path):
    """Runs `case` on `world` ranks (rank 0 here, the rest spawned); returns every rank's result."""
    port = _free_port()
    ctx = multiprocessing.get_context("spawn")
    kids = [ctx.Process(target=_child, args=(case, r, world, port, str(tmp_path))) for r in range(1, world)]
    for p in kids:
        p.start()
    try:
        _init_group(0, world, port)
        try:
            res0 = _case(case, 0, world)
        finally:
            torch.distributed.destroy_process_group()
    finally:
        for p in kids:
            p.join(CHILD_TIMEOUT)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(p.exitcode == 0 for p in kids), [p.exitcode for p in kids]
    return [res0] + [dict(np.load(tmp_path / f"{case}_rank{r}.npz")) for r in range(1, world)]


def _restore_det():
    from drt_amd import det
    det.enable(os.environ.get("DRT_DETERMINISTIC", "0") not in ("", "0"))


@pytest.fixture()
def det_restored():
    yield
    _restore_det()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("det_mode", [True, False])
def test_one_rank_one_view_is_the_fused_loop(det_restored, det_mode):
    """World 1, k = 1: ShardedIteration == FusedIteration over five iterations on the same capture and seed -- bit for bit in
    deterministic mode, to 1e-12 relative in float64 mode (order of the float64 atomics)."""
    from drt_amd import optim as O
    hp = _hp()
    runs = []
    for cls in (O.FusedIteration, O.ShardedIteration):
        scene, data = _setup(0, 1, det_mode, hp)
        data.rng = np.random.RandomState(0)
        it = cls(scene, data, hp, 0.1)
        losses = []
        for _ in range(5):
            total, parts = it.step()
            losses.append(torch.cat([total.view(1), parts]).cpu().numpy())
        torch.cuda.synchronize()
        runs.append((it.parameter.cpu().numpy(), np.array(losses)))
    (pf, lf), (ps, ls) = runs
    assert np.abs(pf).max() > 1e-3 and np.isfinite(pf).all() and (lf[:, 1:] > 0).all()
    if det_mode:
        assert np.array_equal(_bits(pf), _bits(ps)) and np.array_equal(_bits(lf), _bits(ls))
    else:
        assert np.abs(pf - ps).max() <= 1e-12 * np.abs(pf).max()
        np.testing.assert_allclose(ls, lf, rtol=1e-12)


# ---- the one-pass terms: one enqueue function per term behind the autograd Functions and behind the loops ------------------------------

def _drawn_schedule(data):
    """(first refraction view, the one after it, the first eight silhouette views) of the capture's generators."""
    ray, silh = data.ray_view_generator(), data.silh_view_generator()
    first, second = next(ray), next(ray)
    assert first != second
    return first, second, [next(silh) for _ in range(8)]


@pytest.mark.parametrize("law", [None, (4, "reflect")], ids=["two-bounce", "4-reflect"])
def test_the_functions_and_the_loop_share_their_terms(det_restored, law):
    """Deterministic mode, one mesh state, one drawn schedule (one refraction view, eight silhouette views): the per-term losses and
    [V, 3] gradients of Scene.ray_loss_fused (paths_ray_loss_fused under a law) / vh_loss_fused_views / sm_loss_fused through autograd
    with unit seeds ARE those of a FusedIteration step from the same state (lr = 0) -- torch.equal, the sums are exact integers.  An
    argument that reached the shared enqueue functions differently from the two callers, or a wrong offset into the accumulator block,
    would show here.  Negative control: the refraction term of the NEXT view differs."""
    from drt_amd import optim as O
    hp = _hp()
    scene, data = _setup(0, 1, True, hp, smooth=True)
    data.rng = np.random.RandomState(0)
    ray_id, next_ray_id, silh_ids = _drawn_schedule(data)
    V = scene.vertices.detach().clone().requires_grad_(True)
    scene.update_verticex(V)

    def through_autograd(term):
        V.grad = None
        loss = term()
        loss.backward()
        return loss.detach().clone(), V.grad.clone()

    def ray_term(view_id):
        target, valid, _, origin, ray_dir, _ = data.get_view(view_id)
        if law is None:
            return scene.ray_loss_fused(origin, ray_dir, target, valid)
        return scene.paths_ray_loss_fused(origin, ray_dir, target, valid, *law)

    def vh_term():
        views_ = []
        for v in silh_ids:
            _, _, soft_mask, origin, _, camera_M = data.get_view(v)
            views_.append((camera_M, origin[0], soft_mask))
        return scene.vh_loss_fused_views(views_)

    want = [through_autograd(lambda: ray_term(ray_id)), through_autograd(vh_term), through_autograd(scene.sm_loss_fused)]
    other = through_autograd(lambda: ray_term(next_ray_id))
    it = O.FusedIteration(scene, data, hp, 0.0, path_law=law, schedule=(iter([ray_id]), iter(silh_ids)))
    total, parts = it.step()
    torch.cuda.synchronize()
    assert not it.parameter.any()                               # (lr = 0: the state the Functions saw)
    for k, (loss, grad) in enumerate(want):
        print(f"term {k}: loss {float(loss):.17g}, largest gradient entry {float(grad.abs().max()):.3e}")
        assert np.isfinite(float(loss)) and float(loss) != 0 and float(grad.abs().max()) > 0 and bool(torch.isfinite(grad).all())
        assert torch.equal(parts[k], loss), (k, float(parts[k]), float(loss))
        assert torch.equal(it.grads[k], grad), (k, float((it.grads[k] - grad).abs().max()))
    assert not torch.equal(parts[0], other[0]) and not torch.equal(it.grads[0], other[1])


@pytest.mark.parametrize("form", ["FusedIteration", "ShardedIteration"])
def test_a_step_keeps_what_its_kernels_read(det_restored, form):
    """After step(), both iteration forms hold every tensor the enqueue functions returned -- the refraction view's rays, targets and
    flags, the silhouette views' cameras, eyes and masks -- next to the vertices, until the next step replaces the list."""
    from drt_amd import optim as O
    from drt_amd.silhouette import pack_camera
    hp = _hp()
    scene, data = _setup(0, 1, True, hp, smooth=True)
    data.rng = np.random.RandomState(0)
    first, second, silh_ids = _drawn_schedule(data)
    it = getattr(O, form)(scene, data, hp, 0.1, schedule=(iter([first, second]), iter(silh_ids + silh_ids)))
    assert it._keep == []

    def read_by_the_ray_term(view_id):         # (without the origins: the silhouette term reads every view's first one, the eye)
        target, valid, _, _, ray_dir, _ = data.get_view(view_id)
        return {t.data_ptr() for t in (ray_dir, target, valid)}

    it.step()
    keep, vertices = it._keep, it._vertices
    held = {t.data_ptr() for t in keep}
    assert len(keep) == 4 + 3 * 8 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in keep)
    assert read_by_the_ray_term(first) <= held and not read_by_the_ray_term(second) & held
    for v in silh_ids:
        _, _, soft_mask, origin, _, camera_M = data.get_view(v)
        assert {soft_mask.data_ptr(), origin.data_ptr(), pack_camera(camera_M).data_ptr()} <= held
    it.step()
    torch.cuda.synchronize()
    assert it._keep is not keep and it._vertices is not vertices and len(it._keep) == len(keep)
    held = {t.data_ptr() for t in it._keep}
    assert read_by_the_ray_term(second) <= held and not read_by_the_ray_term(first) & held


def test_device_remesher_repeats_itself():
    """The assumption behind comparing remeshed runs across processes: the same input bits give the same mesh twice."""
    from drt_amd import diffrender as Render, mesh_io
    from drt_amd.remesh_gpu import GpuMeshlabserver
    Render.intIOR = IOR
    out = []
    for _ in range(2):
        scene = Render.Scene(mesh_io.read_ply(data_path("hand_vh.ply")), 0)
        GpuMeshlabserver().remesh(scene, 6.0)
        GpuMeshlabserver().remesh(scene, 4.0)
        torch.cuda.synchronize()
        out.append((scene.vertices.cpu().numpy(), scene.faces.cpu().numpy()))
    assert out[0][1].shape == out[1][1].shape and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))


def test_two_ranks_with_remesh_equal_one_rank_bit_for_bit_and_count_their_collectives(det_restored, tmp_path):
    """Deterministic mode, k = 4, two passes with a remesh before each: both ranks end with the same vertex and face bits as the one-rank
    run; one all-reduce per iteration and one mesh broadcast per pass on every rank."""
    r0, r1 = _ranks("remesh", 2, tmp_path)
    one = _case("remesh", 0, 1)
    for r in (r0, r1):
        assert r["F"].shape == one["F"].shape and np.array_equal(r["F"], one["F"])
        assert np.array_equal(_bits(r["V"]), _bits(one["V"])) and np.array_equal(_bits(r["history"]), _bits(one["history"]))
        iters, allreduces, passes, broadcasts, per_it, per_pass = r["stats"]
        assert (iters, allreduces, passes, broadcasts, per_it, per_pass) == (6, 6, 2, 2, 1.0, 1.0)
    assert one["stats"][1] == 0 and one["stats"][3] == 0          # one process: nothing to exchange
    assert len(one["history"]) == 2 and np.isfinite(one["history"]).all()


def test_three_ranks_where_some_own_nothing_equal_one_rank(det_restored, tmp_path):
    """Deterministic mode, k = 2 on three ranks: in some iterations a rank owns no view at all, still joins the exchange, and the
    parameters and losses equal the one-rank run's bits."""
    rs = _ranks("empty", 3, tmp_path)
    one = _case("empty", 0, 1)
    idle = sum(int((r["owned"].sum(axis=1) == 0).sum()) for r in rs)
    assert idle > 0, [r["owned"].tolist() for r in rs]
    assert (sum(r["owned"][:, 0] for r in rs) == 2).all()          # every drawn view evaluated by exactly one rank
    for r in rs:
        assert int(r["n_allreduce"]) == 6
        assert np.array_equal(_bits(r["param"]), _bits(one["param"])) and np.array_equal(_bits(r["losses"]), _bits(one["losses"]))
    assert np.abs(one["param"]).max() > 1e-3


def test_two_ranks_float64_agree_with_one_rank(det_restored, tmp_path):
    """Float64 mode, k = 4: the ranks are bit-identical to each other and within 1e-10 relative of one rank (the tolerance of
    tests/test_gpu_dist.py: the all-reduce changes the order of a float64 sum)."""
    r0, r1 = _ranks("float", 2, tmp_path)
    one = _case("float", 0, 1)
    assert np.array_equal(_bits(r0["param"]), _bits(r1["param"])) and np.array_equal(_bits(r0["losses"]), _bits(r1["losses"]))
    scale = np.abs(one["param"]).max()
    assert scale > 1e-3
    assert np.abs(r0["param"] - one["param"]).max() <= 1e-10 * scale
    np.testing.assert_allclose(r0["losses"], one["losses"], rtol=1e-10)


# ---- 10. the CLI --------------------------------------------------------------------------------------------------------------------

CLI = ["-m", "drt_amd.reconstruct", "--name", "hand", "--res", "64", "--views", "8", "--passes", "2", "--iters", "3", "--views-per-step", "4"]


def _cli(cmd, result, extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    p = subprocess.run(cmd + ["--result-path", str(result)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return lines[0]


def test_cli_two_ranks_write_one_result_equal_to_one_process(tmp_path):
    from drt_amd import mesh_io
    env = {"DRT_DETERMINISTIC": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    if torch.cuda.device_count() < 2:
        env["DRT_DIST_BACKEND"] = "gloo"
    two = _cli([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port())] + CLI, tmp_path / "two", env)
    assert sorted(os.listdir(tmp_path / "two")) == ["hand_recons.ply", "hand_report.json"]
    rep = json.load(open(tmp_path / "two" / "hand_report.json"))
    assert rep == two
    assert rep["world"] == 2 and rep["collectives_per_iteration"] == 1 and rep["broadcasts_per_pass"] == 1
    assert rep["views_per_step"] == 4 and rep["iterations"] == 6 and rep["seconds_per_iteration"] > 0
    one = _cli([sys.executable] + CLI, tmp_path / "one", {"DRT_DETERMINISTIC": "1"})
    assert one["world"] == 1 and one["collectives_per_iteration"] == 0
    a, b = mesh_io.read_ply(str(tmp_path / "one" / "hand_recons.ply")), mesh_io.read_ply(str(tmp_path / "two" / "hand_recons.ply"))
    assert np.array_equal(a.faces, b.faces) and np.array_equal(_bits(a.vertices), _bits(b.vertices))
    assert rep["result_faces"] == one["result_faces"]
