"""GPU: the pass of the eight gradient kernels over their list (sink_pass, drt_amd/csrc/drt_pathsink.h) visits every listed item exactly
once, whatever the list length.

A path's contribution depends only on its ray and the mesh, and in deterministic mode the sums are exact integers.  So for a ray set R
the cells of the loss, of the vertex gradient and (where the call has them) of the two IOR partials after ONE call on R equal, word for
word, the cells after the calls on R[:m] and R[m:] into the same accumulators -- unless the pass drops or repeats an item at the end of
a batch, at the end of the list, or where a block moves on to its second batch.

    cut points   m such that R[:m] holds exactly 1, B - 1, B and B + 1 completed paths (the forward's mask), B the batch of the route:
                 kBwdBatch = 1024 for the two-bounce kernels, kPathsBwdBatch = 256 for the K-interaction ones
    long lists   more completed paths than gridDim.x * B = DRT_BWD_BPC * n_cu * B (n_cu read from the device; 524 288 and 131 072 on
                 an MI355X) in the whole set, fewer in each half: only the whole call makes blocks take a second batch

The rays are the test's own, aimed at data/hand_vh.ply: each at a point inside a random face, along the face normal from two extents
away (88 % of them complete the two-bounce path on the CPU oracle; a camera's rays at this size do not reach the thresholds).  Every
route goes through the Python entry points; `_SharedCells` hands all calls made under it one set of accumulators."""
import numpy as np
import pytest
import torch

import image_cases
from conftest import IOR, data_path
from drt_amd import _lib, det, diffrender as Render, mesh_io, render, views
from oracle import diffrender_oracle as orc

pytestmark = pytest.mark.gpu
EXT = orc.EXT_IOR
B2, BK, BPC = 1024, 256, 2             # kBwdBatch, kPathsBwdBatch, DRT_BWD_BPC (drt_pathsink.h)
LAW = (6, "reflect")
N_LONG2, N_LONGK = 1 << 20, 3 << 16      # rays of the long cases: 0.88 x 2^20 > 524 288 > 2^19; 0.88 x 196 608 > 131 072 > 98 304
N_SHORT2, N_SHORTK = 8192, 2048          # rays of the cut-point cases (8192: two sub-batches of a scene made with DRT_MIN_SUB_LOG2=12)


@pytest.fixture(autouse=True)
def _globals():
    saved = (Render.intIOR, Render.extIOR)
    Render.intIOR, Render.extIOR = IOR, EXT
    was = det.enable(True)
    yield
    det.enable(was)
    Render.intIOR, Render.extIOR = saved


@pytest.fixture(scope="module")
def hand():
    return mesh_io.read_ply(data_path("hand_vh.ply"))


@pytest.fixture(scope="module")
def rays(hand):
    """The N_LONG2 aimed rays; computed once, never modified (the tests slice them)."""
    return aimed_rays(hand, N_LONG2)


def aimed_rays(hand, n):
    """(origin, ray_dir, screen_pixel, valid) of n aimed rays on the device, every one with a target."""
    g = torch.Generator().manual_seed(20)
    V = torch.tensor(hand.vertices, dtype=torch.float64)
    F = torch.tensor(np.asarray(hand.faces), dtype=torch.long)
    center, extent = views.mesh_frame(hand.vertices)
    f = torch.randint(len(F), (n,), generator=g)
    w = torch.rand((n, 3), generator=g, dtype=torch.float64) + 0.25
    tri = V[F[f]]
    p = (tri * (w / w.sum(1, keepdim=True))[:, :, None]).sum(1)
    nrm = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    o = p - 2.0 * extent * nrm / nrm.norm(dim=1, keepdim=True)
    d = p - o
    d = d / d.norm(dim=1, keepdim=True)
    sp = torch.randn((n, 3), generator=g, dtype=torch.float64) * 40.0 + torch.tensor(np.asarray(center) + np.array([0.0, 0.0, 150.0]))
    return o.contiguous().cuda(), d.contiguous().cuda(), sp.cuda(), torch.ones(n, dtype=torch.bool, device="cuda")


def _scene(hand):
    scene = Render.Scene(hand, 0)
    V = torch.tensor(hand.vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene, V


class _SharedCells:
    """While active, every accumulator the package asks det for is the ONE zero-initialised array of its size kept here (scalar: the loss;
    2 values: the IOR partials; else the vertex gradient), so that successive calls add into the same cells."""

    def __enter__(self):
        self.cells = {}
        self._saved = (det.acc, det.scalar)
        det.acc = lambda like: self._get(like.numel(), like.device)
        det.scalar = lambda device: self._get(1, device)
        return self

    def _get(self, n, device):
        if n not in self.cells:
            self.cells[n] = torch.zeros(3 * n, dtype=torch.int64, device=device)
        return self.cells[n]

    def __exit__(self, *exc):
        det.acc, det.scalar = self._saved
        torch.cuda.synchronize()


def _cells_of(route, ray_sets):
    with _SharedCells() as shared:
        for r in ray_sets:
            route(*r)
    return shared.cells


def _cut(r, a, b):
    return tuple(t[a:b].contiguous() for t in r)


def _assert_same(whole, parts, sizes):
    assert set(whole) == set(parts) == set(sizes), (sorted(whole), sorted(parts), sorted(sizes))
    for n in whole:
        assert whole[n].any() and torch.equal(whole[n], parts[n]), n


def _check_cuts(route, r, mask, batch, sizes):
    """One call on r against the two calls on r[:m], r[m:] for the four cut points around `batch` completed paths."""
    done = mask.to(torch.int64).cumsum(0)
    assert int(done[-1]) > batch + 1
    whole = _cells_of(route, [r])
    for c in (1, batch - 1, batch, batch + 1):
        m = int((done >= c).nonzero()[0]) + 1
        assert int(mask[:m].sum()) == c and 0 < m < len(mask)
        _assert_same(whole, _cells_of(route, [_cut(r, 0, m), _cut(r, m, len(mask))]), sizes)


def _check_long(route, r, mask, batch, sizes):
    """The whole set (longer than gridDim.x x batch) against its two halves (shorter)."""
    threshold = BPC * torch.cuda.get_device_properties(0).multi_processor_count * batch
    n = len(mask)
    total, first = int(mask.sum()), int(mask[:n // 2].sum())
    print(f"{total} completed paths of {n} rays, {first} in the first half; a second batch starts beyond {threshold}")
    assert total > threshold > max(first, total - first)
    _assert_same(_cells_of(route, [r]), _cells_of(route, [_cut(r, 0, n // 2), _cut(r, n // 2, n)]), sizes)


# ------------------------------------------------------------------------------------------------------------------------------- routes
def _ior_leaf():
    return torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)


def _two_bounce_routes(scene, V, monkeypatch):
    """name -> (route, sizes of the accumulators it fills); each route is named by the kernel it reaches."""
    nv = V.numel()

    def dropin(ior):
        def route(o, d, sp, va):
            Render.intIOR = _ior_leaf() if ior else IOR
            loss = Render.ray_loss(*scene.render_transparent(o, d), sp, va)
            torch.autograd.grad(loss, [V, Render.intIOR] if ior else [V])
            Render.intIOR = IOR
        return route

    def fused(o, d, sp, va):
        torch.autograd.grad(scene.ray_loss_fused(o, d, sp, va), V)

    def switched(route, **flags):
        def inner(*r):
            for k, v in flags.items():
                monkeypatch.setattr(Render, k, v)
            route(*r)
        return inner

    return {"k_loss_bwd_fused": (fused, {1, nv}),
            "k_loss_bwd_listed": (dropin(False), {1, nv}),                                                  # the eager unit-seed stash
            "k_render_bwd_rows": (switched(dropin(False), EAGER_LOSS_GRAD=False), {1, nv}),                 # the row-list hand-off
            "k_render_bwd_rows-inputs": (dropin(True), {1, nv, 2}),                                         # (a tensor IOR: no eager stash)
            "k_render_bwd": (switched(dropin(False), SPARSE_LOSS_GRAD=False), {1, nv}),                     # the dense fallback
            "k_render_bwd-inputs": (switched(dropin(True), SPARSE_LOSS_GRAD=False), {1, nv, 2})}


TWO_BOUNCE = ["k_loss_bwd_fused", "k_loss_bwd_listed", "k_render_bwd_rows", "k_render_bwd_rows-inputs", "k_render_bwd", "k_render_bwd-inputs"]


def _k_law_routes(scene, V, refraction="reference"):
    nv = V.numel()

    def dense(o, d, sp, va):
        torch.autograd.grad(Render.ray_loss(*scene.render_paths(o, d, *LAW, refraction), sp, va), V)

    def fused(o, d, sp, va):
        torch.autograd.grad(scene.paths_ray_loss_fused(o, d, sp, va, *LAW, refraction), V)

    def ior(vertices):
        def route(o, d, sp, va):
            ti = _ior_leaf()
            loss = scene.paths_ray_loss_ior_fused(o, d, sp, va, ti, EXT, *LAW, refraction, vertices=vertices)
            torch.autograd.grad(loss, [V, ti] if vertices else [ti])
        return route

    return {"k_paths_bwd": (dense, {1, nv}), "k_paths_loss_bwd": (fused, {1, nv}),
            "k_paths_loss_bwd_ior-verts": (ior(True), {1, nv, 2}), "k_paths_loss_bwd_ior": (ior(False), {1, 2})}


K_LAW = ["k_paths_bwd", "k_paths_loss_bwd", "k_paths_loss_bwd_ior-verts", "k_paths_loss_bwd_ior"]


def _mask2(scene, r):
    with torch.no_grad():
        return scene.render_transparent(r[0], r[1])[2][:, 0].clone()


def _mask_k(scene, r, refraction="reference"):
    with torch.no_grad():
        return scene.render_paths(r[0], r[1], *LAW, refraction)[2][:, 0].clone()


# -------------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", TWO_BOUNCE)
def test_two_bounce_cut_points(hand, rays, monkeypatch, name):
    """The scene cuts a call of 8192 rays into two sub-batches (plan_call: 8192 / 2^12 = 2), so the whole call of the drop-in route
    reads its list through drt_ray_loss_listed_grad_split's offset form -- once its targets went through an earlier ray_loss -- while
    the parts, single sub-batches, take the plain form."""
    monkeypatch.setenv("DRT_MIN_SUB_LOG2", "12")
    monkeypatch.setattr(Render, "SPLIT_LOSS_MIN_RAYS", 0)
    scene, V = _scene(hand)
    r = _cut(rays, 0, N_SHORT2)
    route, sizes = _two_bounce_routes(scene, V, monkeypatch)[name]
    split_calls = []
    entry = _lib.lib().drt_ray_loss_listed_grad_split
    monkeypatch.setattr(_lib.lib(), "drt_ray_loss_listed_grad_split", lambda *a: split_calls.append(a[4]) or entry(*a))
    route(*r)                                  # (registers the targets: diffrender._targets_seen_before)
    del split_calls[:]
    _check_cuts(route, r, _mask2(scene, r), B2, sizes)
    if name == "k_loss_bwd_listed":
        assert split_calls == [N_SHORT2]       # the whole call, and only it


@pytest.mark.parametrize("name", TWO_BOUNCE)
def test_two_bounce_list_longer_than_the_grid(hand, rays, monkeypatch, name):
    scene, V = _scene(hand)
    route, sizes = _two_bounce_routes(scene, V, monkeypatch)[name]
    _check_long(route, rays, _mask2(scene, rays), B2, sizes)


@pytest.mark.parametrize("refraction", ["reference", "snell"])
@pytest.mark.parametrize("name", K_LAW)
def test_k_law_cut_points(hand, rays, name, refraction):
    scene, V = _scene(hand)
    r = _cut(rays, 0, N_SHORTK)
    route, sizes = _k_law_routes(scene, V, refraction)[name]
    _check_cuts(route, r, _mask_k(scene, r, refraction), BK, sizes)


@pytest.mark.parametrize("name", K_LAW)
def test_k_law_list_longer_than_the_grid(hand, rays, name):
    scene, V = _scene(hand)
    r = _cut(rays, 0, N_LONGK)
    route, sizes = _k_law_routes(scene, V)[name]
    _check_long(route, r, _mask_k(scene, r), BK, sizes)


@pytest.mark.parametrize("vertices", [True, False], ids=["verts", "fixed-mesh"])
def test_image_loss_list_longer_than_the_grid(hand, vertices):
    """k_image_loss_bwd: 512 x 512 pixels at s = 2 as one band of 2^20 samples against eight bands of 2^17 = 131 072 samples, each
    shorter than the threshold whatever goes through; the bands add into the call's own accumulators, so the finalised values compare."""
    H = W = 512
    s = 2
    scene, V = _scene(hand)
    center, extent = image_cases.frame()
    cam = image_cases.camera(5, H, W)
    screen = render.Screen.behind(cam, center, extent, image_cases.TEX, image_cases.TEX, span=image_cases.SPAN)
    target = np.random.default_rng(3).random((H, W, 3), dtype=np.float32)
    law = dict(supersample=s, max_bounces=LAW[0], tir=LAW[1], refraction="snell", void=0.25, invalid=0.75)
    threshold = BPC * torch.cuda.get_device_properties(0).multi_processor_count * BK
    _, _, through = scene.render_image(cam, H, W, screen, image_cases.texture(3), want_planes=True, **law)
    listed = int(round(float(through.double().sum()) * s * s))
    print(f"{listed} through samples of {H * W * s * s}; a second batch starts beyond {threshold}")
    assert listed > threshold >= (1 << 17) and render.plan_bands(H, W, s, 1 << 17) == [(y, y + 64) for y in range(0, H, 64)]

    def call(**kw):
        ti, te = _ior_leaf(), torch.tensor(EXT, dtype=torch.float64, device="cuda", requires_grad=True)
        loss = scene.image_loss_fused(cam, H, W, screen, image_cases.texture(3), target, ior_int=ti, ior_ext=te, vertices=vertices, **law, **kw)
        return (loss.detach().clone(),) + tuple(g.clone() for g in torch.autograd.grad(loss, ([V] if vertices else []) + [ti, te]))

    whole, banded = call(), call(max_samples=1 << 17)
    assert float(whole[0]) > 0 and all(g.abs().max() > 0 for g in whole[1:])
    for a, b in zip(whole, banded):
        assert torch.equal(a, b)
