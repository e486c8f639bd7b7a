"""CPU: the float64 restatement of paths of up to K interactions (tests/paths_ref.py) reproduces the chain of the reference's own
Dintersect / refract_ray / Reflect / optix_intersect and its autograd (tests/golden/hand_r64_v5_paths.npz, make_golden_paths.py)."""
import numpy as np
import pytest
import torch

import paths_ref
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import mesh_io
from oracle import diffrender_oracle as orc

CASES = [("k6_reflect", 6, "reflect"), ("k4_drop", 4, "drop")]


def test_fixture_anchor():
    g = golden("hand_r64_v5_paths")
    assert list(g["cases"]) == [c[0] for c in CASES]
    # completed paths: 346 with six interactions and reflection, 259 with four and none (257 today)
    assert int(g["k6_reflect_mask"].sum()) == 346 and int(g["k4_drop_mask"].sum()) == 259
    assert np.bincount(g["k6_reflect_hits"], minlength=7).tolist() == [3750, 0, 257, 54, 26, 8, 1]
    assert np.bincount(g["k4_drop_hits"], minlength=5).tolist() == [3837, 0, 257, 0, 2]
    assert float(g["k6_reflect_ray_loss"]) == 1112.4517080542087 and float(g["k4_drop_ray_loss"]) == 865.2697653393643
    base = golden("hand_r64_v5")            # the two-interaction paths of today's fixture are the K = 2 rows of both cases
    for tag, _, _ in CASES:
        two = g[f"{tag}_hits"] == 2
        assert np.array_equal(np.nonzero(two)[0], base["valid_ind"])


@pytest.mark.parametrize("tag,max_bounces,tir", CASES)
def test_restatement_reproduces_the_reference_chain(tag, max_bounces, tir):
    g = golden("hand_r64_v5_paths")
    assert int(g[f"{tag}_max_bounces"]) == max_bounces and str(g[f"{tag}_tir"]) == tir
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    o, d, sp, valid = fixture_view(golden("hand_r64_v5"))
    V = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
    out_ori, out_dir, mask, aux = paths_ref.render_paths(mesh.faces, V, o, d, IOR, orc.EXT_IOR, max_bounces, tir)
    assert np.array_equal(aux["tape"].numpy(), g[f"{tag}_tape"].astype(np.int64))
    assert np.array_equal(aux["hits"].numpy(), g[f"{tag}_hits"].astype(np.int64))
    assert np.array_equal(mask[:, 0].numpy(), g[f"{tag}_mask"])
    vi = torch.tensor(g[f"{tag}_valid_ind"])
    # the chained trace and its recomputation from the tape are the same path
    assert np.abs(aux["out_ori"].numpy() - out_ori.detach().numpy()).max() <= 1e-10
    np.testing.assert_allclose(out_ori.detach()[vi].numpy(), g[f"{tag}_out_ori"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(out_dir.detach()[vi].numpy(), g[f"{tag}_out_dir"], rtol=0, atol=1e-10)
    loss = orc.ray_loss(out_ori, out_dir, mask, sp, valid)
    assert abs(loss.item() - float(g[f"{tag}_ray_loss"])) <= 1e-11 * float(g[f"{tag}_ray_loss"])
    g_ray, = torch.autograd.grad(loss, V, retain_graph=True)
    ref = g[f"{tag}_grad_ray_loss"]
    assert np.abs(g_ray.numpy() - ref).max() <= min(1e-5, 1e-9 * np.abs(ref).max())
    rng = np.random.default_rng(int(g["lin_seed"]))
    P = o.shape[0]
    w_ori, w_dir = torch.tensor(rng.standard_normal((P, 3))), torch.tensor(rng.standard_normal((P, 3)))
    lin = (out_ori * w_ori).sum() + (out_dir * w_dir).sum()
    assert abs(lin.item() - float(g[f"{tag}_lin"])) <= 1e-11 * abs(float(g[f"{tag}_lin"]))
    g_lin, = torch.autograd.grad(lin, V)
    ref = g[f"{tag}_grad_lin"]
    assert np.abs(g_lin.numpy() - ref).max() <= min(1e-5, 1e-9 * np.abs(ref).max())
