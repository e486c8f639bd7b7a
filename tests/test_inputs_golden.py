"""CPU: the float64 restatement with differentiable rays and IORs (tests/inputs_ref.py) reproduces the reference's own autograd
(tests/golden/hand_r64_v5_inputs.npz, tests/golden/make_golden_inputs.py)."""
import numpy as np
import torch

import inputs_ref
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import mesh_io


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_fixture_anchor():
    g = golden("hand_r64_v5_inputs")
    assert float(g["ray_loss"]) == 857.6437912504243 and int(g["contributing_rows"]) == 234
    assert int((g["grad_ray_loss_dir"] != 0).any(1).sum()) == 234
    assert round(float(g["grad_ray_loss_ior_int"]), 4) == -46.1437
    assert bool(g["origin_unused_by_ray_loss"])


def test_restatement_reproduces_reference_autograd():
    g = golden("hand_r64_v5_inputs")
    base = golden("hand_r64_v5")           # same view: its targets and ray_loss
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    o, d, sp, valid = fixture_view(base)
    V = torch.tensor(mesh.vertices, dtype=torch.float64)
    origin, ray_dir = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    ti = torch.tensor(IOR, dtype=torch.float64, requires_grad=True)
    te = torch.tensor(float(g["ext_ior"]), dtype=torch.float64, requires_grad=True)
    out_ori, out_dir, mask, _ = inputs_ref.render_transparent(mesh.faces, V, origin, ray_dir, ti, te)
    from oracle import diffrender_oracle as orc
    loss = orc.ray_loss(out_ori, out_dir, mask, sp, valid)
    assert abs(loss.item() - float(g["ray_loss"])) <= 1e-11 * float(g["ray_loss"])
    g_o, g_d, g_i, g_e = torch.autograd.grad(loss, (origin, ray_dir, ti, te), retain_graph=True, allow_unused=True)
    assert g_o is None or not g_o.any()
    assert _rel(g_d, g["grad_ray_loss_dir"]) < 1e-10
    assert abs(g_i.item() - float(g["grad_ray_loss_ior_int"])) <= 1e-10 * abs(float(g["grad_ray_loss_ior_int"]))
    assert abs(g_e.item() - float(g["grad_ray_loss_ior_ext"])) <= 1e-10 * abs(float(g["grad_ray_loss_ior_ext"]))

    rng = np.random.default_rng(int(g["lin_seed"]))
    P = o.shape[0]
    w_ori, w_dir = torch.tensor(rng.standard_normal((P, 3))), torch.tensor(rng.standard_normal((P, 3)))
    lin = (out_ori * w_ori).sum() + (out_dir * w_dir).sum()
    assert abs(lin.item() - float(g["lin"])) <= 1e-11 * abs(float(g["lin"]))
    l_o, l_d, l_i, l_e = torch.autograd.grad(lin, (origin, ray_dir, ti, te))
    assert _rel(l_o, g["grad_lin_origin"]) < 1e-10
    assert _rel(l_d, g["grad_lin_dir"]) < 1e-10
    assert abs(l_i.item() - float(g["grad_lin_ior_int"])) <= 1e-10 * abs(float(g["grad_lin_ior_int"]))
    assert abs(l_e.item() - float(g["grad_lin_ior_ext"])) <= 1e-10 * abs(float(g["grad_lin_ior_ext"]))
