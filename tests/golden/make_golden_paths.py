#!/usr/bin/env python3
"""Generate tests/golden/hand_r64_v5_paths.npz: refraction paths of up to K interactions with internal reflection, chained from the
REFERENCE's own pieces.

Run in the build container only (it needs the reference, which never travels):

    python tests/golden/make_golden_paths.py

The reference is imported exactly as tests/golden/make_golden.py imports it (its stand-ins for trimesh / imageio / the OptiX
extension).  Its render_transparent is hard-wired to two bounces, so the path law of Scene.render_paths is chained here from its own
``Scene.Dintersect``, ``Scene.refract_ray``, ``Reflect`` and ``Scene.optix_intersect``: a TIR hit either ends the path ("drop", what
trace2 does) or continues mirrored ("reflect": ``Reflect(wo, n)`` with the normal refract_ray has flipped in place, origin
``o + t d`` then ``+= 1e-5 * wr`` -- refract_ray's own two statements with the commented-out ``new_dir = wr`` of DiffRender.py:530).
Same view as hand_r64_v5.npz (hand_vh, 64 x 64, turntable view 5), the same targets (seed 105) and linear functional (seed 205).
Two cases, (K = 6, reflect) and (K = 4, drop); per case: the face tape, hit counts, mask, out_ori / out_dir of the valid rows,
ray_loss, d ray_loss / d vertices and d lin / d vertices (the reference's autograd).
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
CASES = (("k6_reflect", 6, "reflect"), ("k4_drop", 4, "drop"))


def chain(DR, scene, origin, ray_dir, max_bounces, tir):
    P = origin.shape[0]
    tape = torch.full((max_bounces, P), -1, dtype=torch.long)
    hits = torch.zeros(P, dtype=torch.long)
    refr = torch.zeros(P, dtype=torch.long)
    done = []                                     # (ray indices, origin, direction) of the paths that ended valid
    ray = DR.Ray(origin, ray_dir, torch.arange(P))
    for k in range(max_bounces + 1):
        if len(ray) == 0:
            break
        if k < max_bounces:
            it, hitted = scene.Dintersect(ray)
        else:
            _, hitted = scene.optix_intersect(ray)
        gone = ray.select(torch.logical_not(hitted))
        ok = (refr[gone.ray_ind] > 0) & (refr[gone.ray_ind] % 2 == 0)
        done.append((gone.ray_ind[ok], gone.origin[ok], gone.direction[ok]))
        if k == max_bounces:
            break
        ind = it.ray.ray_ind
        tape[k, ind] = it.faces_ind
        hits[ind] = k + 1
        refracted, new_ray = scene.refract_ray(it)       # (flips it.n in place where the ray leaves)
        if tir == "reflect":
            wr = DR.Reflect(-it.ray.direction, it.n)
            ro = it.ray.origin + it.t.view(-1, 1) * it.ray.direction
            ro = ro + 1e-5 * wr
            sel = refracted.view(-1, 1)
            ray = DR.Ray(torch.where(sel, new_ray.origin, ro), torch.where(sel, new_ray.direction, wr), ind)
            refr[ind] += refracted.long()
        else:
            ray = new_ray.select(refracted)
            refr[ray.ray_ind] += 1
    vi = torch.cat([a for a, _, _ in done])
    zeros = torch.zeros((P, 3), dtype=torch.float64)
    out_ori = zeros.index_put((vi,), torch.cat([a for _, a, _ in done]))
    out_dir = zeros.index_put((vi,), torch.cat([a for _, _, a in done]))
    mask = torch.zeros(P, dtype=torch.bool)
    mask[vi] = True
    hits[torch.logical_not(mask)] = 0
    return out_ori, out_dir, mask, tape, hits


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
    origin, ray_dir = views.generate_ray(RES, RES, Kinv, Rinv)
    P = origin.shape[0]
    sp, valid = mg._targets(P, center, seed=100 + VIEW_ID)
    tsp, tvalid = torch.tensor(sp), torch.tensor(valid)
    rng = np.random.default_rng(200 + VIEW_ID)
    w_ori, w_dir = rng.standard_normal((P, 3)), rng.standard_normal((P, 3))
    rec = dict(res=RES, view_id=VIEW_ID, ior=mg.IOR, target_seed=100 + VIEW_ID, lin_seed=200 + VIEW_ID,
               cases=np.array([c[0] for c in CASES]))
    for tag, k, tir in CASES:
        V = torch.tensor(mesh.vertices, dtype=torch.float64, requires_grad=True)
        scene.update_verticex(V)
        out_ori, out_dir, mask, tape, hits = chain(DR, scene, origin, ray_dir, k, tir)
        target = tsp - out_ori.detach()
        target = target / target.norm(dim=1, keepdim=True)
        vm = tvalid * mask
        ray_loss = (out_dir - target)[vm].pow(2).sum()
        g_ray, = torch.autograd.grad(ray_loss, V, retain_graph=True)
        lin = (out_ori * torch.tensor(w_ori)).sum() + (out_dir * torch.tensor(w_dir)).sum()
        g_lin, = torch.autograd.grad(lin, V)
        vi = torch.nonzero(mask).squeeze(1)
        rec.update({f"{tag}_max_bounces": k, f"{tag}_tir": tir, f"{tag}_tape": tape.numpy().astype(np.int32),
                    f"{tag}_hits": hits.numpy().astype(np.uint8), f"{tag}_mask": mask.numpy(), f"{tag}_valid_ind": vi.numpy(),
                    f"{tag}_out_ori": out_ori.detach()[vi].numpy(), f"{tag}_out_dir": out_dir.detach()[vi].numpy(),
                    f"{tag}_ray_loss": ray_loss.item(), f"{tag}_grad_ray_loss": g_ray.numpy(), f"{tag}_lin": lin.item(),
                    f"{tag}_grad_lin": g_lin.numpy()})
        print(tag, "valid", len(vi), "hits histogram", np.bincount(hits.numpy(), minlength=k + 1).tolist(), "ray_loss", repr(ray_loss.item()),
              "rows", int(vm.sum()), "lin", repr(lin.item()))
    out = os.path.join(HERE, "hand_r64_v5_paths.npz")
    np.savez_compressed(out, **rec)
    print("->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
