"""GPU: the IOR gradient of the K-interaction law -- Scene.paths_ray_loss_ior_fused / drt_render_paths_law_ray_loss_ior_fused
(k_paths_loss_bwd_ior, drt_amd/csrc/drt_paths.hip) -- and the fit built on it (drt_amd.calibrate.fit_ior).

References: torch autograd of the float64 restatement tests/ior_ref.py (IOR partials 1e-9 relative to the sum of the absolute per-path
contributions; tests/test_paths_ior_host.py measures 1.5e-16 for the same code on the host), the unchanged one-pass call
paths_ray_loss_fused (vertex gradient: bit for bit in deterministic mode, 1e-12 relative in float64 mode) and, at (2, drop, reference),
the two-bounce route render_transparent + ray_loss + backward with tensor IORs.  hand_vh at 64 x 64, view 5 with a target on every ray:
226 / 342 / 346 / 257 contributing paths at the four laws -- at (6, reflect) more than one 256-ray table fill of the kernel.

The bounds of the fit come from the CPU restatement (``python tests/ior_ref.py``): end error 2.2e-6 at (2, drop, snell),
-1.7e-4 at (6, reflect, snell), +3.4e-4 at (6, reflect, reference)."""
import numpy as np
import pytest
import torch

import ior_ref
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import _lib, calibrate, det, diffrender as Render, mesh_io, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu
EXT = orc.EXT_IOR
LOSS_REL, IOR_REL, ROUTE_REL = 1e-10, 1e-9, 1e-12
LAWS = [(2, "drop", "snell", 226), (6, "reflect", "snell", 342), (6, "reflect", "reference", 346), (2, "drop", "reference", 257)]
FIT_VIEWS = (5, 23, 41, 59)
CPU_END_ERROR_6_REFLECT_REFERENCE = 3.44e-4          # python tests/ior_ref.py: fitted 1.4726440 against 1.4723


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR, Render.resx, Render.resy)
    Render.intIOR, Render.extIOR = IOR, EXT
    Render.resx = Render.resy = 64
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


_mesh = []
_refs = {}


def _hand_mesh():
    if not _mesh:
        _mesh.append(mesh_io.read_ply(data_path("hand_vh.ply")))
    return _mesh[0]


def _rays():
    o, d, sp, _ = fixture_view(golden("hand_r64_v5"))
    return o, d, sp, torch.ones(o.shape[0], dtype=torch.bool)


def _ref(k, tir, refraction):
    """The restatement's loss, IOR partials and their per-path scale for one law: computed once, shared read-only."""
    key = (k, tir, refraction)
    if key not in _refs:
        mesh = _hand_mesh()
        o, d, sp, valid = _rays()
        _refs[key] = ior_ref.loss_and_grads(mesh.faces, torch.tensor(mesh.vertices, dtype=torch.float64), o, d, sp, valid, IOR, EXT, k, tir, refraction)
    return _refs[key]


def _hand():
    mesh = _hand_mesh()
    scene = Render.Scene(mesh, 0)
    V = torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return (scene, V) + tuple(t.cuda() for t in _rays())


def _iors(ext_device="cuda"):
    return (torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True),
            torch.tensor(EXT, dtype=torch.float64, device=ext_device, requires_grad=True))


def _call(scene, V, o, d, sp, valid, law, vertices=True):
    """(loss, d / d ior_int, d / d ior_ext, d / d V or None) of one call with tensor IORs."""
    ti, te = _iors()
    loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, ti, te, *law, vertices=vertices)
    assert loss.shape == () and loss.dtype == torch.float64
    gi, ge = torch.autograd.grad(loss, (ti, te), retain_graph=vertices)
    gv = torch.autograd.grad(loss, V)[0] if vertices else None
    return loss.detach(), gi, ge, gv


# ------------------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("k,tir,refraction,n_valid", LAWS)
def test_loss_and_ior_partials_against_the_restatement(float_mode, k, tir, refraction, n_valid):
    ref = _ref(k, tir, refraction)
    scene, V, o, d, sp, valid = _hand()
    loss, gi, ge, _ = _call(scene, V, o, d, sp, valid, (k, tir, refraction))
    count = int(scene.last_path_count)
    print(f"({k}, {tir}, {refraction}): contributing rays {count}; loss {loss.item():.12e} (restatement {ref['loss']:.12e}); "
          f"g_int {gi.item():.12e} ({ref['g_int']:.12e}, disagreement {abs(gi.item() - ref['g_int']) / ref['abs_int']:.3e} of sum |per path|); "
          f"g_ext {ge.item():.12e} ({ref['g_ext']:.12e}, {abs(ge.item() - ref['g_ext']) / ref['abs_ext']:.3e})")
    assert count == n_valid == ref["count"]
    assert scene.last_path_count.dtype == torch.int64 and scene.last_path_count.is_cuda
    assert abs(loss.item() - ref["loss"]) <= LOSS_REL * abs(ref["loss"])
    assert gi.shape == () and gi.is_cuda and ge.shape == ()
    assert abs(gi.item() - ref["g_int"]) <= IOR_REL * ref["abs_int"]
    assert abs(ge.item() - ref["g_ext"]) <= IOR_REL * ref["abs_ext"]


def test_ior_arguments_floats_tensors_devices_and_the_default_exterior(float_mode):
    scene, V, o, d, sp, valid = _hand()
    law = (6, "reflect", "snell")
    l0, gi0, ge0, _ = _call(scene, V, o, d, sp, valid, law)
    # a CPU tensor gets its gradient on the CPU; a float IOR is a constant; ior_ext=None is Render.extIOR; the globals are not consulted otherwise
    ti, te = _iors("cpu")
    Render.intIOR = 1.9
    loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, ti, te, *law, vertices=False)
    gi, ge = torch.autograd.grad(3.0 * loss, (ti, te))
    assert gi.is_cuda and not ge.is_cuda
    assert gi.item() == pytest.approx(3.0 * gi0.item(), rel=ROUTE_REL) and ge.item() == pytest.approx(3.0 * ge0.item(), rel=ROUTE_REL)
    loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, IOR, None, *law)
    assert loss.item() == pytest.approx(l0.item(), rel=ROUTE_REL)
    Render.extIOR = 1.1
    assert scene.paths_ray_loss_ior_fused(o, d, sp, valid, IOR, None, *law).item() != pytest.approx(l0.item(), rel=1e-6)
    # a RayBinding lends its rays; rays that require grad are refused
    a = scene.paths_ray_loss_ior_fused(scene.bind_rays(o, d), None, sp, valid, IOR, EXT, *law)
    assert a.item() == pytest.approx(l0.item(), rel=ROUTE_REL)
    with pytest.raises(NotImplementedError):
        scene.paths_ray_loss_ior_fused(o.clone().requires_grad_(True), d, sp, valid, IOR, EXT, *law)
    with pytest.raises(NotImplementedError):
        scene.paths_ray_loss_ior_fused(o, d.clone().requires_grad_(True), sp, valid, IOR, EXT, *law)


# ------------------------------------------------------------------------------------------------------------- 2. vertex gradient
def _plain(scene, V, o, d, sp, valid, law):
    loss = scene.paths_ray_loss_fused(o, d, sp, valid, *law)
    return loss.detach(), torch.autograd.grad(loss, V)[0]


def test_vertex_gradient_has_the_bits_of_paths_ray_loss_fused_in_deterministic_mode(deterministic):
    scene, V, o, d, sp, valid = _hand()
    for law in ((6, "reflect", "snell"), (6, "reflect", "reference")):
        l_ref, g_ref = _plain(scene, V, o, d, sp, valid, law)
        loss, _, _, gv = _call(scene, V, o, d, sp, valid, law)
        assert g_ref.abs().max() > 0
        assert torch.equal(loss, l_ref) and torch.equal(gv, g_ref)


def test_vertex_gradient_agrees_with_paths_ray_loss_fused_in_float_mode(float_mode):
    scene, V, o, d, sp, valid = _hand()
    law = (6, "reflect", "snell")
    l_ref, g_ref = _plain(scene, V, o, d, sp, valid, law)
    loss, _, _, gv = _call(scene, V, o, d, sp, valid, law)
    assert abs(loss.item() - l_ref.item()) <= ROUTE_REL * abs(l_ref.item())
    assert (gv - g_ref).abs().max().item() <= ROUTE_REL * g_ref.abs().max().item()


# ------------------------------------------------------------------------------------------------------------ 3. vertices=False
def test_without_vertices_same_loss_and_partials_bit_for_bit_in_deterministic_mode(deterministic):
    scene, V, o, d, sp, valid = _hand()
    for law in ((6, "reflect", "snell"), (2, "drop", "reference")):
        l1, gi1, ge1, gv = _call(scene, V, o, d, sp, valid, law, vertices=True)
        n1 = int(scene.last_path_count)
        l0, gi0, ge0, _ = _call(scene, V, o, d, sp, valid, law, vertices=False)
        assert gv.abs().max() > 0 and gi1.item() != 0
        assert torch.equal(l0, l1) and torch.equal(gi0, gi1) and torch.equal(ge0, ge1) and int(scene.last_path_count) == n1


def test_without_vertices_the_mesh_receives_no_gradient(float_mode):
    scene, V, o, d, sp, valid = _hand()
    law = (6, "reflect", "snell")
    l1, gi1, ge1, _ = _call(scene, V, o, d, sp, valid, law, vertices=True)
    ti, te = _iors()
    loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, ti, te, *law, vertices=False)
    loss.backward()
    assert V.grad is None and scene.vertices.grad is None
    assert abs(loss.item() - l1.item()) <= ROUTE_REL * abs(l1.item())
    assert abs(ti.grad.item() - gi1.item()) <= ROUTE_REL * abs(gi1.item()) and abs(te.grad.item() - ge1.item()) <= ROUTE_REL * abs(ge1.item())


# ------------------------------------------------------------------------------------------------------- 4. the two-bounce route
def test_two_bounces_drop_reference_agrees_with_render_transparent(float_mode):
    scene, V, o, d, sp, valid = _hand()
    loss, gi, ge, gv = _call(scene, V, o, d, sp, valid, (2, "drop", "reference"))
    ti, te = _iors()
    Render.intIOR, Render.extIOR = ti, te
    out_ori, out_dir, mask = scene.render_transparent(o, d)
    l_ref = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    l_ref.backward()
    Render.intIOR, Render.extIOR = IOR, EXT
    print("two-bounce route: g_int", gi.item(), ti.grad.item(), "g_ext", ge.item(), te.grad.item())
    assert abs(loss.item() - l_ref.item()) <= LOSS_REL * abs(l_ref.item())
    assert ti.grad.item() != 0 and te.grad.item() != 0
    assert abs(gi.item() - ti.grad.item()) <= IOR_REL * abs(ti.grad.item())
    assert abs(ge.item() - te.grad.item()) <= IOR_REL * abs(te.grad.item())
    assert (gv - V.grad).abs().max().item() <= IOR_REL * V.grad.abs().max().item()


# ------------------------------------------------------------------------------------------------- 5. determinism, capture, C ABI
def _abi(scene, V, o, d, sp, va, k, flags, loss, grad_v, grad_ior, count):
    return _lib.lib().drt_render_paths_law_ray_loss_ior_fused(
        scene.optix_mesh._h, V.data_ptr(), _lib.ptr(o), _lib.ptr(d), _lib.ptr(sp), _lib.ptr(va), 0 if o is None else o.shape[0], IOR, EXT, k, flags,
        _lib.ptr(loss), _lib.ptr(grad_v), _lib.ptr(grad_ior), _lib.ptr(count), torch.cuda.current_stream().cuda_stream)


def _cells(Vd):
    return det.scalar(Vd.device), det.acc(Vd), det.acc(torch.empty(2, dtype=torch.float64, device=Vd.device)), torch.zeros(1, dtype=torch.int64, device="cuda")


def test_same_bits_run_to_run_and_eager_against_graph_replay(deterministic):
    scene, V, o, d, sp, valid = _hand()
    first = _call(scene, V, o, d, sp, valid, (6, "reflect", "snell"))
    again = _call(scene, V, o, d, sp, valid, (6, "reflect", "snell"))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    Vd, va = V.detach(), valid.view(torch.uint8)
    two = torch.empty(2, dtype=torch.float64)

    def step(with_verts):
        # (the update belongs inside the captured region: a consumer of the tree waits for the build's event)
        scene.update_verticex(V)
        loss, gv, gior, count = _cells(Vd)
        assert gior.dtype == torch.int64 and gior.numel() == 6
        _lib.check(_abi(scene, Vd, o, d, sp, va, 6, 3, loss, gv if with_verts else None, gior, count))
        return det.value(loss), det.value(gior, two), det.value(gv, Vd), count

    for with_verts in (True, False):
        e = step(with_verts)                 # the first eager call allocates
        assert torch.equal(e[0], first[0]) and torch.equal(e[1][0], first[1]) and torch.equal(e[1][1], first[2]) and int(e[3]) == 342
        assert torch.equal(e[2], first[3]) if with_verts else not e[2].any()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(with_verts)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g = step(with_verts)
        for _ in range(2):
            for t in g[:3]:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(g[:3], e[:3])) and int(g[3]) == 342


def test_several_views_add_into_one_pair_of_accumulators(deterministic):
    scene, V, o, d, sp, valid = _hand()
    Vd, va = V.detach(), valid.view(torch.uint8)
    halves = [tuple(t[:2048].contiguous() for t in (o, d, sp, va)), tuple(t[2048:].contiguous() for t in (o, d, sp, va))]
    both, singles = _cells(Vd), []
    for h in halves:
        one = _cells(Vd)
        _lib.check(_abi(scene, Vd, *h, 6, 3, *one))
        _lib.check(_abi(scene, Vd, *h, 6, 3, *both))
        singles.append(one)
    s = torch.cuda.current_stream().cuda_stream
    for j in (0, 1, 2):
        total = singles[0][j].clone()
        _lib.check(_lib.lib().drt_fx_add(total.data_ptr(), singles[1][j].data_ptr(), total.numel() // 3, s))
        assert torch.equal(total, both[j])
    assert int(singles[0][3]) > 50 and int(singles[1][3]) > 50 and int(both[3]) == int(singles[0][3]) + int(singles[1][3]) == 342
    assert det.value(both[2], torch.empty(2, dtype=torch.float64)).abs().min() > 0
    _lib.check(_abi(scene, Vd, *halves[0], 6, 3, both[0], None, both[2], None))          # the vertex gradient and the count are optional


def test_c_abi_arguments_are_checked(float_mode):
    scene, V, o, d, sp, valid = _hand()
    Vd, va = V.detach(), valid.view(torch.uint8)
    lib = _lib.lib()
    assert lib.drt_version() >= 6
    rng = np.random.default_rng(11)
    acc = (torch.tensor(rng.standard_normal(()), device="cuda"), torch.tensor(rng.standard_normal(tuple(V.shape)), device="cuda"),
           torch.tensor(rng.standard_normal(2), device="cuda"), torch.full((1,), 12345, dtype=torch.int64, device="cuda"))
    keep = [t.clone() for t in acc]
    assert _abi(scene, Vd, o, d, sp, va, 6, 3, acc[0], acc[1], None, acc[3]) == -1 and b"d_grad_ior" in lib.drt_last_error()          # DRT_E_INVALID
    assert _abi(scene, Vd, o, d, sp, va, 6, 4, *acc) == -1 and b"law_flags" in lib.drt_last_error()
    for k in (1, 9):
        assert _abi(scene, Vd, o, d, sp, va, k, 3, *acc) == -1 and b"max_bounces" in lib.drt_last_error()
    _lib.check(_abi(scene, Vd, None, None, None, None, 6, 3, *acc))                                          # no rays: DRT_OK, nothing touched
    _lib.check(_abi(scene, Vd, o, d, sp, torch.zeros_like(va), 6, 3, *acc))                                 # no ray has a target
    torch.cuda.synchronize()
    for a, b in zip(keep, acc):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # float64 accumulators are added to
    _lib.check(_abi(scene, Vd, o, d, sp, va, 6, 3, *acc))
    _, gi, ge, _ = _call(scene, V, o, d, sp, valid, (6, "reflect", "snell"), vertices=False)
    assert (acc[2][0] - keep[2][0]).item() == pytest.approx(gi.item(), rel=1e-12) and (acc[2][1] - keep[2][1]).item() == pytest.approx(ge.item(), rel=1e-12)
    assert int(acc[3]) == 12345 + 342


# ------------------------------------------------------------------------------------------------------------------ 6. the fit
class _Capture:
    """Views of the 72-view turntable of the hand hull at 64 x 64 with targets traced on the GPU by render_paths under ``law`` at the
    IOR of conftest (1.4723): screen_pixel = out_ori + 50 out_dir on the rays whose path completes."""

    def __init__(self, scene, law, view_ids):
        mesh = _hand_mesh()
        center, extent = views.mesh_frame(mesh.vertices)
        cams = views.turntable_cameras(center, extent, 72, 64, 64)
        self._views, self._ids = {}, list(view_ids)
        for v in view_ids:
            R, K, Rinv, Kinv = cams[v]
            o, d = (t.cuda() for t in views.generate_ray(64, 64, Kinv, Rinv))
            with torch.no_grad():
                out_ori, out_dir, mask = scene.render_paths(o, d, *law)
            self._views[v] = ((out_ori + 50.0 * out_dir).contiguous(), mask[:, 0].clone(), None, o, d, None)

    def get_view(self, v):
        return self._views[v]

    def ray_view_ids(self):
        return self._ids


_fit_scenes = {}


def _fit_case(law):
    """(scene, capture) of one law: built once, shared (the fit changes neither)."""
    if law not in _fit_scenes:
        scene = Render.Scene(_hand_mesh(), 0)
        _fit_scenes[law] = (scene, _Capture(scene, law, FIT_VIEWS))
    return _fit_scenes[law]


@pytest.mark.parametrize("law,bound", [((2, "drop", "snell"), 1e-4), ((6, "reflect", "snell"), 1e-3),
                                       ((6, "reflect", "reference"), 5 * CPU_END_ERROR_6_REFLECT_REFERENCE)])
def test_fit_recovers_the_ior_the_targets_were_traced_with(float_mode, law, bound):
    scene, data = _fit_case(law)
    fit = calibrate.fit_ior(scene, data, law, bracket=(1.3, 1.7), halvings=14)
    lo, hi = fit["bracket"]
    print(law, "fitted", fit["ior"], "error", fit["ior"] - IOR, "final bracket", fit["bracket"], "evaluations", fit["evaluations"])
    assert fit["evaluations"] == 16 and hi - lo == pytest.approx(0.4 / 2 ** 14, rel=1e-9)
    assert all(h[3] > 200 for h in fit["history"])
    assert scene.vertices.grad is None
    assert abs(fit["ior"] - IOR) <= bound


@pytest.mark.parametrize("law", [(2, "drop", "snell"), (6, "reflect", "snell")])
def test_sign_of_the_summed_derivative_around_the_true_ior(float_mode, law):
    scene, data = _fit_case(law)
    at_true = calibrate.evaluate_views(scene, data, IOR, law, FIT_VIEWS)
    assert at_true[0] <= 1e-18 * at_true[2]          # the targets are this mesh's own exit rays
    for x in (1.40, 1.43, 1.46, 1.47, 1.475, 1.48, 1.50, 1.55):
        loss, g, rays = calibrate.evaluate_views(scene, data, x, law, FIT_VIEWS)
        print(law, "ior", x, "loss", loss, "d loss / d ior", g, "rays", rays)
        assert loss > 0 and (g < 0) == (x < IOR) and g != 0
