"""GPU: the deterministic sink rule of the one-pass loss terms (drt_amd.diffrender._UnitSeedTerm) on the two routes that also hand IOR
gradients to autograd: while ``det.begin_sink()`` is armed in deterministic mode, the backward of ``image_loss_fused`` and of
``paths_ray_loss_ior_fused`` leaves exactly one ``(cells, incoming gradient)`` entry and gives the vertices no gradient;
``det.collect`` of that entry is, bit for bit, the vertex gradient of the same call without a sink; the IOR gradients arrive through
autograd, with the same bits, either way.  The hand with image case `v5` (32 x 32, its own supersampling), and the ray fixture of
tests/test_gpu_paths_ior.py (hand_vh, view 5 at 64 x 64, a target on every ray)."""
import pytest
import torch

import image_cases
import image_loss_cases as cases
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import det, diffrender as Render, mesh_io

pytestmark = pytest.mark.gpu
EXT = cases.EXT
LAW = (6, "reflect", "snell")
SEED = 0.75                  # the downstream factor: what the backward is seeded with


@pytest.fixture(autouse=True)
def _globals():
    saved = (Render.intIOR, Render.extIOR, Render.resx, Render.resy)
    Render.intIOR, Render.extIOR = IOR, EXT
    Render.resx = Render.resy = 64
    was = det.enable(True)
    yield
    det.end_sink()
    det.enable(was)
    Render.intIOR, Render.extIOR, Render.resx, Render.resy = saved


def _scene(mesh):
    scene = Render.Scene(mesh, 0)
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda", requires_grad=True))
    return scene


def _with_and_without_a_sink(scene, call):
    """``call(ior_int, ior_ext)`` -> loss, once plainly and once with the sink armed."""
    def run():
        ii = torch.tensor(IOR, dtype=torch.float64, device="cuda", requires_grad=True)
        ie = torch.tensor(EXT, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(call(ii, ie) * SEED, [scene.vertices, ii, ie], allow_unused=True)

    gv, gi, ge = run()
    assert gv is not None and gv.abs().max() > 0 and float(gi) != 0 and float(ge) != 0
    entries = det.begin_sink()
    assert entries == []
    sunk = run()
    assert det.end_sink() is entries and len(entries) == 1
    cells, scale = entries[0]
    assert cells.dtype == torch.int64 and cells.numel() == 3 * scene.vertices.numel() and float(scale) == SEED
    assert sunk[0] is None                                                      # the vertices receive nothing from autograd
    assert torch.equal(sunk[1], gi) and torch.equal(sunk[2], ge)                 # the IOR gradients still do
    assert sunk[2].device.type == "cpu" and sunk[1].is_cuda
    assert torch.equal(det.collect(entries, scene.vertices, lambda t: t, scale), gv)


def test_image_loss_fused_under_an_armed_sink():
    sc = image_cases.scene("v5")
    scene, target = _scene(image_cases.hand()), cases.target("v5", LAW, True)
    _with_and_without_a_sink(scene, lambda ii, ie: scene.image_loss_fused(
        sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"], target, ior_int=ii, ior_ext=ie, supersample=sc["s"],
        max_bounces=LAW[0], tir=LAW[1], refraction=LAW[2], void=sc["void"], invalid=sc["invalid"]))


def test_paths_ray_loss_ior_fused_under_an_armed_sink():
    scene = _scene(mesh_io.read_ply(data_path("hand_vh.ply")))
    o, d, sp, _ = (t.cuda() for t in fixture_view(golden("hand_r64_v5")))
    valid = torch.ones(o.shape[0], dtype=torch.bool, device="cuda")
    _with_and_without_a_sink(scene, lambda ii, ie: scene.paths_ray_loss_ior_fused(o, d, sp, valid, ii, ie, *LAW))
