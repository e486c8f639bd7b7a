#!/usr/bin/env python3
"""Generate tests/golden/hand_r64_v5_inputs.npz: the gradients of the refraction path w.r.t. the camera rays and the indices of
refraction, from the REFERENCE's own autograd.

Run in the build container only (it needs the reference, which never travels):

    python tests/golden/make_golden_inputs.py

The reference is imported exactly as tests/golden/make_golden.py imports it (its stand-ins for trimesh / imageio / the OptiX
extension).  Its path is plain torch autograd, so making ``DiffRender.intIOR`` / ``extIOR`` float64 tensors and the rays leaves that
require grad differentiates every input.  Same view as hand_r64_v5.npz (hand_vh, 64 x 64, turntable view 5) and the same targets
(seed 105) and linear functional (seed 205).  Stored: the two losses, d ray_loss / d ray_dir (dense, [P,3]), d ray_loss / d intIOR
and / d extIOR, and for lin = sum(out_ori * w_ori) + sum(out_dir * w_dir): d lin / d origin, d lin / d ray_dir and its two IOR
partials.  ``origin_unused_by_ray_loss`` records that autograd reports origin as unused by ray_loss (the loss detaches out_ori).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402  (puts the repository on sys.path)

from drt_amd import mesh_io, views  # noqa: E402

RES, VIEW_ID = 64, 5
EXT_IOR = 1.00029


def main():
    torch.manual_seed(0)
    np.random.seed(0)
    DR, _ = mg._import_reference()
    path = os.path.join(mg.REPO, "data", "hand_vh.ply")
    mesh = mesh_io.read_ply(path)
    center, extent = views.mesh_frame(mesh.vertices)
    scene = DR.Scene(path)
    DR.resx = DR.resy = RES
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, 72, RES, RES)[VIEW_ID]
    origin0, ray_dir0 = views.generate_ray(RES, RES, Kinv, Rinv)
    P = origin0.shape[0]
    scene.update_verticex(torch.tensor(mesh.vertices, dtype=torch.float64))

    ior_int = torch.tensor(mg.IOR, dtype=torch.float64, requires_grad=True)
    ior_ext = torch.tensor(EXT_IOR, dtype=torch.float64, requires_grad=True)
    DR.intIOR, DR.extIOR = ior_int, ior_ext
    origin = origin0.clone().requires_grad_(True)
    ray_dir = ray_dir0.clone().requires_grad_(True)
    out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)

    sp, valid = mg._targets(P, center, seed=100 + VIEW_ID)
    tsp, tvalid = torch.tensor(sp), torch.tensor(valid)
    target = tsp - out_ori.detach()
    target = target / target.norm(dim=1, keepdim=True)
    vm = tvalid * mask[:, 0]
    ray_loss = (out_dir - target)[vm].pow(2).sum()
    g_o, g_d, g_int, g_ext = torch.autograd.grad(ray_loss, (origin, ray_dir, ior_int, ior_ext), retain_graph=True, allow_unused=True)

    rng = np.random.default_rng(200 + VIEW_ID)
    w_ori = rng.standard_normal((P, 3))
    w_dir = rng.standard_normal((P, 3))
    lin = (out_ori * torch.tensor(w_ori)).sum() + (out_dir * torch.tensor(w_dir)).sum()
    l_o, l_d, l_int, l_ext = torch.autograd.grad(lin, (origin, ray_dir, ior_int, ior_ext))

    rows = int(vm.sum())
    rec = dict(res=RES, view_id=VIEW_ID, ior=mg.IOR, ext_ior=EXT_IOR, target_seed=100 + VIEW_ID, lin_seed=200 + VIEW_ID,
               ray_loss=ray_loss.item(), contributing_rows=rows, origin_unused_by_ray_loss=g_o is None,
               grad_ray_loss_dir=g_d.numpy(), grad_ray_loss_ior_int=g_int.item(), grad_ray_loss_ior_ext=g_ext.item(),
               lin=lin.item(), grad_lin_origin=l_o.numpy(), grad_lin_dir=l_d.numpy(), grad_lin_ior_int=l_int.item(),
               grad_lin_ior_ext=l_ext.item())
    out = os.path.join(HERE, "hand_r64_v5_inputs.npz")
    np.savez_compressed(out, **rec)
    print(f"ray_loss {ray_loss.item()!r} rows {rows} nonzero d/d ray_dir rows {int((g_d != 0).any(1).sum())} "
          f"d/d intIOR {g_int.item():.6g} d/d extIOR {g_ext.item():.6g} origin unused: {g_o is None}")
    print(f"lin {lin.item()!r} d/d intIOR {l_int.item():.6g} d/d extIOR {l_ext.item():.6g} -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
