"""GPU: optim.PhotoIteration on a capture taken in a room, without a screen: a captured_data.SyntheticPhotoData of
data/hand_vh.ply -- 8 photographs of 32 x 32 at 2 x 2 samples per pixel of views.displaced_ground_truth in the [16, 32, 3] environment of
tests/image_env_cases.py, with the light reflected off the outer surface, under (6, "reflect", "snell") with the Fresnel term.  The
photometric term of the drawn views is ONE drt_render_image_loss_views_env call per step."""
import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_env_ref
from conftest import IOR, golden
from drt_amd import captured_data, det, diffrender as Render, mesh_io, metrics, optim, views

pytestmark = pytest.mark.gpu
EXT = image_cases.EXT
LAW = (6, "reflect", "snell")
RES, S = 32, 2
HP = dict(optim.HyperParams, IOR=IOR, image_w=100.0, ray_w=0, vh_w=0, sm_w=0, momentum=0)
LR = 0.1


@pytest.fixture(autouse=True)
def _ior_globals():
    saved = (Render.intIOR, Render.extIOR)
    Render.intIOR, Render.extIOR = IOR, EXT
    yield
    Render.intIOR, Render.extIOR = saved


@pytest.fixture
def deterministic():
    was = det.enable(True)
    yield
    det.enable(was)


def _scene(mesh):
    scene = Render.Scene(mesh, 0)
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64, device="cuda"))
    return scene


_DATA = {}


def _data():
    """The eight photographs of the displaced hand in the room, rendered once per process."""
    if not _DATA:
        center, extent = image_cases.frame()
        gt = _scene(views.displaced_ground_truth(image_cases.hand()))
        _DATA[8] = captured_data.SyntheticPhotoData(gt, center, extent, RES, RES, None, num_view=8, path_law=LAW, supersample=S,
                                                    environment=image_env_cases.environment(3), reflection=True, screen=False)
    data = _DATA[8]
    data.rng = np.random.RandomState(0)              # every test draws the same schedule
    return data


def _stepper(scene, data, hp=HP, views_per_step=2, lr=LR):
    return optim.PhotoIteration(scene, data, hp, lr, views_per_step=views_per_step, path_law=LAW, fresnel=True, supersample=S, reflection=True)


def test_the_capture_has_no_screen_and_carries_the_room():
    data = _data()
    assert data.screens is None and data.texture is None and data.environment is image_env_cases.environment(3) and data.reflection
    assert tuple(data.photos.shape) == (8, RES, RES, 3) and float(data.photos.max()) > 0
    bare = captured_data.PhotoData(data.cameras, None, None, data.photos, [v[2] for v in data.Views], RES, RES)
    with pytest.raises(ValueError, match="environment"):
        optim.PhotoIteration(_scene(image_cases.hand()), bare, HP, LR, reflection=True)


def test_one_step_is_the_term(deterministic):
    """vh_w = sm_w = 0, no momentum: after one step the parameter is -lr limit_hook(w grad) with grad from image_loss_views_fused on the
    drawn views and w = image_w / (views_per_step H W) -- bit for bit."""
    data = _data()
    scene = _scene(image_cases.hand())
    it = _stepper(scene, data)
    assert it.binding.env is not None and it.texture is None
    total, parts = it.step()
    ids = list(it.last_views)
    assert len(ids) == 2 and all(0 <= v < 8 for v in ids)
    parts, total, param = parts.clone(), total.clone(), it.parameter.clone()
    V = it.init_vertices.clone().requires_grad_(True)
    scene.update_verticex(V)
    loss = scene.image_loss_views_fused(it.binding, ids, None, ior_int=IOR, supersample=S, max_bounces=LAW[0], tir=LAW[1], refraction=LAW[2], reflection=True)
    grad = torch.autograd.grad(loss, V)[0]
    w = HP["image_w"] / (2 * RES * RES)
    assert float(loss.detach()) > 0 and grad.abs().max() > 0 and int(scene.last_image_count) > 0
    assert torch.equal(param, -(LR * optim.limit_hook(w * grad)))
    assert torch.equal(parts[0], loss.detach()) and float(parts[1]) == 0 and float(parts[2]) == 0 and float(total) == w * float(loss.detach())
    plain = scene.image_loss_views_fused(it.binding, ids, None, ior_int=IOR, supersample=S, max_bounces=LAW[0], tir=LAW[1], refraction=LAW[2])
    assert not torch.equal(plain.detach(), loss.detach())                                          # (the reflection took part)


def test_three_steps_against_the_restatement():
    """Three such steps against their replay on the CPU: image_env_ref.loss_and_grads of every drawn view at the replay's own vertices,
    limit_hook and plain SGD; within the project's cap of 1e-9 of the mesh extent (DESIGN.md 10.10 records the measured difference)."""
    data = _data()
    mesh = image_cases.hand()
    scene = _scene(mesh)
    it = _stepper(scene, data)
    w = HP["image_w"] / (2 * RES * RES)
    photos = data.photos.cpu().numpy()
    env = data.environment
    V0 = torch.tensor(mesh.vertices, dtype=torch.float64)
    param = torch.zeros_like(V0)
    for step in range(3):
        it.step()
        g = torch.zeros_like(V0)
        for v in it.last_views:
            ref = image_env_ref.loss_and_grads(mesh.faces, (V0 + param).numpy(), data.cameras[v], RES, RES, None, None, env.texels, env.rotation, photos[v], S, LAW,
                                               0.0, IOR, EXT, reflect=True)
            g += torch.as_tensor(ref["grad_V"])
        param = param - LR * optim.limit_hook(w * g)
        diff = float((it.parameter.cpu() - param).abs().max())
        print(f"step {step}: views {it.last_views}, largest parameter entry {float(param.abs().max()):.3e}, GPU against the replay {diff:.3e}")
    _, extent = image_cases.frame()
    assert float(param.abs().max()) > 1e-3 and diff <= 1e-9 * extent


FIT_HP = dict(optim.HyperParams, IOR=IOR, image_w=100.0, ray_w=0)


def test_the_loop_fits(deterministic):
    """All three terms, 8 views per step (every step sees all 8 photographs), 30 steps from the visual hull (its smoothed form) toward the
    displaced ground truth: the image part of the loss ends below its start and everything stays finite.  The ratio and the distances to
    the ground truth are printed as measurements, not asserted."""
    data = _data()
    hull = mesh_io.TriMesh(golden("hand_smooth_sm")["vertices"].astype(np.float64), image_cases.hand().faces)
    scene = _scene(hull)
    it = _stepper(scene, data, FIT_HP, views_per_step=8, lr=0.05)
    series = []
    for _ in range(30):
        total, parts = it.step()
        series.append(torch.cat([parts, total.reshape(1)]).clone())
    series = torch.stack(series).cpu()
    print(f"image loss {float(series[0, 0]):.6e} -> {float(series[-1, 0]):.6e} (ratio {float(series[-1, 0] / series[0, 0]):.4f}); "
          f"vh {float(series[0, 1]):.4e} -> {float(series[-1, 1]):.4e}; sm {float(series[0, 2]):.4e} -> {float(series[-1, 2]):.4e}")
    gt = views.displaced_ground_truth(image_cases.hand())
    d0 = metrics.distance_stats(metrics.vertex_to_surface(it.init_vertices, gt))
    d1 = metrics.distance_stats(metrics.vertex_to_surface(it.init_vertices + it.parameter, gt))
    print(f"vertex to ground-truth surface distance: mean {d0['mean']:.4f} -> {d1['mean']:.4f}, rms {d0['rms']:.4f} -> {d1['rms']:.4f}, max {d0['max']:.4f} -> {d1['max']:.4f}")
    assert torch.isfinite(series).all() and torch.isfinite(it.parameter).all()
    assert series[:, 1].max() > 0 and series[:, 2].abs().max() > 0                       # the other two terms took part
    assert float(series[-1, 0]) < float(series[0, 0])
