"""ARMED_LOSS (drt_amd/diffrender.py, include/drt_hip.h drt_render_loss_arm): a render call on a RayBinding that carries its targets does the
ray loss itself -- every sub-batch adds the loss + unit-seed vertex gradient of the paths it completed on its own internal stream, in front
of the join -- and ray_loss on the untouched outputs with the bound targets issues no native call.  In every case the reference is the plain
route on the same scene state (arm and SPLIT_LOSS off: one drt_ray_loss_listed_grad behind the join): loss to 1e-12 relative and the
vertex gradient to 1e-11 of its largest entry (what test_gpu_recycle.py asks of the split loss against the plain one), bit-equal in
deterministic mode; dense outputs, mask, face ids and the set of listed rows exactly."""
import numpy as np
import pytest
import torch

from conftest import IOR, data_path
from drt_amd import mesh_io, views

pytestmark = pytest.mark.gpu

RES = 64           # (a tile hint needs a width that is a multiple of 64)
P = RES * RES


@pytest.fixture()
def R(monkeypatch):
    from drt_amd import diffrender as Render, det
    keep = (Render.ARMED_LOSS, Render.ARMED_LOSS_MIN_RAYS, Render.SPLIT_LOSS, Render.SPLIT_LOSS_MIN_RAYS, Render.resx, Render.resy, Render.intIOR)
    was = det.on()
    Render.intIOR = IOR
    Render.resx = Render.resy = RES
    Render.ARMED_LOSS_MIN_RAYS = Render.SPLIT_LOSS_MIN_RAYS = 0
    monkeypatch.setenv("DRT_MIN_SUB_LOG2", "12")        # read by drt_create: a sub-batch per 64 x 64 image, as far as the streams go
    yield Render
    det.enable(was)
    (Render.ARMED_LOSS, Render.ARMED_LOSS_MIN_RAYS, Render.SPLIT_LOSS, Render.SPLIT_LOSS_MIN_RAYS, Render.resx, Render.resy, Render.intIOR) = keep


def _hand():
    return mesh_io.read_ply(data_path("hand_vh.ply"))


def _two_balls():
    """A ball and a larger one behind it: from the side views the exit rays of the first run into the second (occluded exit rays)."""
    a, b = mesh_io.icosphere(2, 40.0), mesh_io.icosphere(2, 60.0)
    vb = b.vertices + np.array([0.0, 0.0, 120.0])
    return mesh_io.TriMesh(np.concatenate([a.vertices, vb]), np.concatenate([a.faces, b.faces + len(a.vertices)])), a


def _views(mesh, nv, miss=(), seed=5, which=None):
    """nv whole images of rays around the mesh (the rays of the images in `miss` turned away from it), random targets, ~10 % invalid."""
    c, ext = views.mesh_frame(mesh.vertices)
    cams = views.turntable_cameras(c, ext, 8, RES, RES)
    rays = [views.generate_ray(RES, RES, cams[k][3], cams[k][2], device="cuda") for k in (which or range(nv))]
    o = torch.cat([r[0] for r in rays]).contiguous()
    d = torch.cat([r[1] for r in rays]).contiguous()
    for k in miss:
        d[k * P:(k + 1) * P] *= -1.0
    rng = np.random.default_rng(seed)
    sp = torch.tensor(rng.standard_normal((o.shape[0], 3)) * 40.0 + np.asarray(c) + np.array([0.0, 0.0, 150.0]), device="cuda")
    valid = torch.tensor(rng.random(o.shape[0]) > 0.1, device="cuda")
    return o, d, sp, valid


def _scene(Render, monkeypatch, mesh, per_stream=1, **env):
    monkeypatch.setenv("DRT_SUB_PER_STREAM", str(per_stream))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return Render.Scene(mesh, 0)


def _subs(scene):
    from drt_amd import _lib
    c = (np.zeros(8, dtype=np.int64))
    _lib.check(_lib.lib().drt_route_counts(scene.optix_mesh._h, c.ctypes.data))
    return int(c[0])


def _call(Render, scene, V, handle, sp, valid, armed, loss_targets=None, touch=False, loss=True):
    """One render (+ ray_loss + backward) at vertices V on the handle; armed=False is the plain route.  Everything a caller can see."""
    from drt_amd import _lib
    Render.ARMED_LOSS = Render.SPLIT_LOSS = armed
    Vg = V.clone().requires_grad_(True)
    scene.update_verticex(Vg)
    before = _subs(scene)
    oo, od, mk = scene.render_transparent(handle)
    out = {"subs": _subs(scene) - before, "taken": bool(_lib.lib().drt_render_loss_taken(scene.optix_mesh._h)),
           "oo": oo.clone(), "od": od.clone(), "mk": mk.clone(), "f1": scene.last_face1.clone(), "f2": scene.last_face2.clone()}
    paths, n_paths = od._drt_link.paths
    out["listed"] = torch.sort(paths[:int(n_paths.item())].long()).values
    if loss:
        if touch:
            od.add_(0.0)                          # written in place: no longer "the outputs of the call" for ray_loss
        tsp, tva = loss_targets if loss_targets is not None else (sp, valid)
        l = Render.ray_loss(oo, od, mk, tsp, tva)
        l.backward()
        out["loss"], out["grad"] = l.detach().clone(), Vg.grad.clone()
    return out


def _same(a, b, exact=False):
    assert torch.equal(a["mk"], b["mk"]) and torch.equal(a["oo"], b["oo"]) and torch.equal(a["od"], b["od"])
    lit = a["mk"][:, 0]
    assert torch.equal(a["f1"][lit], b["f1"][lit]) and torch.equal(a["f2"][lit], b["f2"][lit])
    assert torch.equal(a["listed"], b["listed"]) and torch.equal(a["listed"], torch.nonzero(lit).flatten())
    if "loss" in a:
        print("loss", float(a["loss"]), float(b["loss"]), "grad diff", float((a["grad"] - b["grad"]).abs().max()), "of", float(b["grad"].abs().max()))
        if exact:
            assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])
        else:
            assert float(a["loss"]) == pytest.approx(float(b["loss"]), rel=1e-12)
            assert float(b["grad"].abs().max()) > 0 and float((a["grad"] - b["grad"]).abs().max()) <= 1e-11 * float(b["grad"].abs().max())


def _verts(mesh, k=0):
    v0 = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda")
    c = v0.mean(0)
    return c + (v0 - c) * (1.0 + 0.03 * k) + 0.2 * k


# nv images, sub-batches dealt to each of the two streams, images whose rays miss, the cut that must come out
# (7 images dealt three to a stream: six sub-batches of 4 864 rays -- a multiple of the 256-ray unit, no whole images -- the last one 4 352)
CUTS = [(2, 1, (), 2), (3, 2, (), 3), (4, 2, (), 4), (7, 3, (), 6), (3, 2, (1,), 3), (1, 1, (), 1)]


@pytest.mark.parametrize("nv,per_stream,miss,subs", CUTS, ids=["2on2", "3on2", "4on2", "partial", "empty-segment", "unsplit"])
def test_every_cut_of_the_call_gives_the_plain_loss(R, monkeypatch, nv, per_stream, miss, subs):
    mesh = _hand()
    o, d, sp, valid = _views(mesh, nv, miss)
    scene = _scene(R, monkeypatch, mesh, per_stream)
    handle = scene.bind_rays(o, d, sp, valid)
    R.cache_report(reset=True)
    for k in range(3):                            # the establishing call, then two trusting ones (a stream reuses its list R2)
        V = _verts(mesh, k)
        a = _call(R, scene, V, handle, sp, valid, True)
        b = _call(R, scene, V, handle, sp, valid, False)
        assert a["subs"] == subs and a["taken"] and not b["taken"]
        for j in miss:
            assert not a["mk"][j * P:(j + 1) * P].any()
        assert int(a["mk"][:, 0].sum()) > 100
        _same(a, b)
    rep = R.cache_report()
    assert rep.get("loss_armed", 0) == 3 and rep.get("loss_arm_used", 0) == 3 and rep.get("loss_arm_dropped", 0) == 0


def test_invalid_targets_and_occluded_exit_rays(R, monkeypatch):
    mesh, front = _two_balls()
    o, d, sp, valid = _views(mesh, 4, which=(3, 4, 5, 4))        # (camera 4 looks along the axis of the two balls, the small one in front)
    valid[P // 4: P // 2] = False                 # a block of zeros next to the scattered ones
    valid[2 * P: 3 * P] = False                   # ... and a whole sub-batch without a valid target
    scene = _scene(R, monkeypatch, mesh, 2)
    handle = scene.bind_rays(o, d, sp, valid)
    V = _verts(mesh)
    a = _call(R, scene, V, handle, sp, valid, True)
    b = _call(R, scene, V, handle, sp, valid, False)
    assert a["subs"] == 4 and a["taken"]
    _same(a, b)
    # the front ball alone completes paths that the ball behind it takes away: rows k_shade2 wrote and write_dead took back
    alone = R.Scene(front, 0).render_transparent(o, d)[2][:, 0]
    hits_front = (a["f1"] >= 0) & (a["f1"] < len(front.faces))
    assert int((alone & hits_front & ~a["mk"][:, 0]).sum()) > 10
    assert int((a["mk"][:, 0] & ~valid).sum()) > 50          # completed paths the loss must leave out


def test_a_loss_that_cannot_use_the_armed_result_takes_the_plain_route(R, monkeypatch):
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 3)
    _, _, sp2, valid2 = _views(mesh, 3, seed=11)
    scene = _scene(R, monkeypatch, mesh, 2)
    handle = scene.bind_rays(o, d, sp, valid)
    V = _verts(mesh)
    _call(R, scene, V, handle, sp, valid, True)                  # (establishes the grid)
    R.cache_report(reset=True)
    # other targets than the bound ones; copies of the bound ones (equal content, other tensors)
    for tg in ((sp2, valid2), (sp.clone(), valid.clone())):
        a = _call(R, scene, V, handle, sp, valid, True, loss_targets=tg)
        b = _call(R, scene, V, handle, sp, valid, False, loss_targets=tg)
        assert a["taken"]
        _same(a, b)
    rep = R.cache_report()
    assert rep.get("loss_armed", 0) == 2 and rep.get("loss_arm_used", 0) == 0 and rep.get("loss_arm_dropped", 0) == 2
    # ray_loss never called: the armed result is dropped with the call, the next call starts from zeros
    a0 = _call(R, scene, _verts(mesh, 2), handle, sp, valid, True, loss=False)
    assert a0["taken"]
    a = _call(R, scene, V, handle, sp, valid, True)
    b = _call(R, scene, V, handle, sp, valid, False)
    assert a["taken"] and R.cache_report().get("loss_arm_used", 0) == 1
    _same(a, b)
    # out_dir written in place before the loss (last: the write stays in the version counter of the handle's output set)
    a = _call(R, scene, V, handle, sp, valid, True, touch=True)
    b = _call(R, scene, V, handle, sp, valid, False, touch=True)
    assert a["taken"] and R.cache_report().get("loss_arm_used", 0) == 1
    _same(a, b)

    assert R.cache_report().get("loss_arm_used", 0) == 1


def test_the_step_of_the_optimisation_loop(R, monkeypatch):
    """optim.full_batch_step on a handle with targets -- the path the benchmark times -- against the plain route, vertices moving."""
    from drt_amd import optim as O
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 4)
    res = []
    for armed in (True, False):
        R.ARMED_LOSS = R.SPLIT_LOSS = armed
        R.cache_report(reset=True)
        scene = _scene(R, monkeypatch, mesh, 2)
        handle = scene.bind_rays(o, d, sp, valid)
        init_vertices, parameter, opt = O.setup_opt(scene, 0.1, O.HyperParams, hook=False, fused=True)
        losses = [O.full_batch_step(scene, [(sp, valid, handle)], init_vertices, parameter, opt, 40 * 217.5 / RES / RES, fused=False).item() for _ in range(3)]
        res.append((np.array(losses), parameter.detach().cpu().numpy()))
        rep = R.cache_report()
        assert rep.get("loss_armed", 0) == (3 if armed else 0) and rep.get("loss_arm_used", 0) == (3 if armed else 0)
    print("losses", res[0][0], res[1][0], "param diff", np.abs(res[0][1] - res[1][1]).max(), "of", np.abs(res[1][1]).max())
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-12)
    scale = np.abs(res[1][1]).max()
    assert scale > 1e-3 and np.abs(res[0][1] - res[1][1]).max() <= 1e-11 * scale


def test_deterministic_mode_gives_the_bits_of_the_plain_route_for_any_cut(R, monkeypatch):
    from drt_amd import det
    det.enable(True)
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 4)
    V = _verts(mesh, 1)
    got = []
    for per_stream, subs in ((2, 4), (1, 2)):
        scene = _scene(R, monkeypatch, mesh, per_stream)
        handle = scene.bind_rays(o, d, sp, valid)
        _call(R, scene, V, handle, sp, valid, True)              # (establishes)
        a = _call(R, scene, V, handle, sp, valid, True)
        b = _call(R, scene, V, handle, sp, valid, False)
        assert a["subs"] == subs and a["taken"]
        _same(a, b, exact=True)
        got.append(a)
    _same(got[0], got[1], exact=True)


def test_the_one_kernel_path_declines_the_arm(R, monkeypatch):
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 3)
    scene = _scene(R, monkeypatch, mesh, 2, DRT_MEGA_MAX_LOG2="24")
    handle = scene.bind_rays(o, d, sp, valid)
    V = _verts(mesh)
    R.cache_report(reset=True)
    for _ in range(2):
        a = _call(R, scene, V, handle, sp, valid, True)
        b = _call(R, scene, V, handle, sp, valid, False)
        assert not a["taken"] and a["subs"] == 3
        _same(a, b)
    rep = R.cache_report()
    assert rep.get("loss_arm_declined", 0) == 2 and rep.get("loss_armed", 0) == 0 and rep.get("loss_arm_used", 0) == 0


def test_a_captured_call_declines_the_arm(R, monkeypatch):
    """Inside a capture the Python layer does not arm; an arm registered through the C ABI is declined by the call and adds nothing."""
    from drt_amd import _lib
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 2)
    scene = _scene(R, monkeypatch, mesh, 1)
    handle = scene.bind_rays(o, d, sp, valid)
    V = _verts(mesh)
    ref = _call(R, scene, V, handle, sp, valid, False)
    R.ARMED_LOSS = R.SPLIT_LOSS = True
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            assert _call(R, scene, V, handle, sp, valid, True)["taken"]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    loss_acc = torch.zeros((), dtype=torch.float64, device="cuda")
    grad_acc = torch.zeros_like(V)
    Vg = V.clone().requires_grad_(True)
    R.cache_report(reset=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.update_verticex(Vg)
        _lib.check(_lib.lib().drt_render_loss_arm(scene.optix_mesh._h, sp.data_ptr(), valid.view(torch.uint8).data_ptr(), loss_acc.data_ptr(), grad_acc.data_ptr(), o.shape[0]))
        oo, od, mk = scene.render_transparent(handle)
        taken = bool(_lib.lib().drt_render_loss_taken(scene.optix_mesh._h))
        loss = R.ray_loss(oo, od, mk, sp, valid)
    rep = R.cache_report()
    assert not taken and rep.get("loss_armed", 0) == 0 and rep.get("loss_arm_used", 0) == 0
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert float(loss_acc) == 0.0 and float(grad_acc.abs().max()) == 0.0
    assert torch.equal(mk, ref["mk"]) and torch.equal(oo, ref["oo"]) and torch.equal(od, ref["od"])
    assert float(loss) == pytest.approx(float(ref["loss"]), rel=1e-12)
    loss.backward()
    assert float((Vg.grad - ref["grad"]).abs().max()) <= 1e-11 * float(ref["grad"].abs().max())


def test_an_arm_is_one_shot_and_only_for_its_size(R, monkeypatch):
    """The C ABI by hand: a call of another size drops the registration, a failing call clears it, and neither adds to the accumulators."""
    from drt_amd import _lib
    from drt_amd.optix_mesh import _stream
    mesh = _hand()
    o, d, sp, valid = _views(mesh, 2)
    scene = _scene(R, monkeypatch, mesh, 1)
    R.ARMED_LOSS = R.SPLIT_LOSS = False
    lib, h, n = _lib.lib(), scene.optix_mesh._h, o.shape[0]
    loss_acc = torch.zeros((), dtype=torch.float64, device="cuda")
    grad_acc = torch.zeros((len(mesh.vertices), 3), dtype=torch.float64, device="cuda")
    va = valid.view(torch.uint8)

    def arm(rays):
        _lib.check(lib.drt_render_loss_arm(h, sp.data_ptr(), va.data_ptr(), loss_acc.data_ptr(), grad_acc.data_ptr(), rays))

    assert lib.drt_render_loss_arm(h, None, va.data_ptr(), loss_acc.data_ptr(), grad_acc.data_ptr(), n) != 0
    arm(n)
    scene.render_transparent(o[:P].contiguous(), d[:P].contiguous())       # another size: dropped ...
    assert not lib.drt_render_loss_taken(h)
    scene.render_transparent(o, d)                                           # ... for good
    assert not lib.drt_render_loss_taken(h)
    arm(n)
    junk = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    assert lib.drt_render_forward(h, None, o.data_ptr(), d.data_ptr(), n, IOR, 1.00029, junk.data_ptr(), junk.data_ptr(), junk.data_ptr(),
                                  ids.data_ptr(), ids.data_ptr(), None, None, RES, RES, 0, None, _stream()) != 0
    scene.render_transparent(o, d)                                           # the failed call cleared it
    assert not lib.drt_render_loss_taken(h)
    torch.cuda.synchronize()
    assert float(loss_acc) == 0.0 and float(grad_acc.abs().max()) == 0.0
    arm(n)
    oo, od, mk = scene.render_transparent(o, d)                              # unbound rays: the arm is the library's business, it is served
    assert lib.drt_render_loss_taken(h)
    Vg = scene.vertices.detach().clone().requires_grad_(True)
    scene.update_verticex(Vg)
    oo, od, mk = scene.render_transparent(o, d)
    assert not lib.drt_render_loss_taken(h)
    l = R.ray_loss(oo, od, mk, sp, valid)
    l.backward()
    print("by hand: loss", float(loss_acc), float(l), "grad diff", float((grad_acc - Vg.grad).abs().max()), "of", float(Vg.grad.abs().max()))
    assert float(loss_acc) == pytest.approx(float(l), rel=1e-12)
    assert float((grad_acc - Vg.grad).abs().max()) <= 1e-11 * float(Vg.grad.abs().max())
