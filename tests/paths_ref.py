"""Float64 restatement of refraction paths of up to K interactions with internal reflection (Scene.render_paths; test only).

The path law of drt_amd/csrc/drt_paths.h, built from the oracle's bounce / moller_trumbore / refract_dir (in the style of
tests/inputs_ref.py): ``trace`` chains ``oracle.diffrender_oracle.bounce`` -- so the face ids come from the oracle's tracer -- and adds
the reflect continuation, the reference's Reflect (DiffRender.py:31-33) with refract_ray's flipped normal and the 1e-5 offset of the line
the reference leaves commented out at DiffRender.py:530; ``render_paths`` then recomputes the completed paths from the face tape in torch,
so autograd supplies the gradients w.r.t. the vertices."""
import torch

from oracle import diffrender_oracle as orc
from oracle.diffrender_oracle import _dot, fresnel_tir, moller_trumbore, refract_dir

BVH_FACES = 20000        # meshes above this many faces are traced through the oracle's tree instead of its loop over every face (same contract)


def _reflect(o, d, t, n):
    """Reflect continuation of hits (o, d) at distance t with the flipped normal n: (new_o, wr)."""
    wo = -d
    wr = -wo + 2 * _dot(wo, n).view(-1, 1) * n
    return (o + t.view(-1, 1) * d) + 1e-5 * wr, wr


def trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir):
    """Chain the oracle's bounce: dict(tape int64 [K,P] (-1 where there was no such interaction; the interactions of a path that ends
    invalid stay recorded), hits int64 [P] (0 on invalid rows), valid bool [P], out_ori / out_dir [P,3] with zeros on invalid rows)."""
    assert 2 <= max_bounces <= 8 and tir in ("drop", "reflect")
    P = origin.shape[0]
    mesh = orc.Mesh(faces, V.detach())
    old_bvh, orc.USE_BVH = orc.USE_BVH, len(mesh.faces) > BVH_FACES
    try:
        tape = torch.full((max_bounces, P), -1, dtype=torch.long)
        hits = torch.zeros(P, dtype=torch.long)
        refr = torch.zeros(P, dtype=torch.long)
        valid = torch.zeros(P, dtype=torch.bool)
        out_ori = torch.zeros((P, 3), dtype=torch.float64)
        out_dir = torch.zeros((P, 3), dtype=torch.float64)
        idx = torch.arange(P)
        o, d = origin.detach(), ray_dir.detach()
        for k in range(max_bounces + 1):
            if len(idx) == 0:
                break
            if k < max_bounces:
                b = orc.bounce(mesh, o, d, ior_int, ior_ext)
                hitted = b["hitted"]
            else:
                _, hitted = orc.intersect_ids(mesh, o, d)
            missed = torch.logical_not(hitted)
            mi = idx[missed]
            ok = (refr[mi] > 0) & (refr[mi] % 2 == 0)
            valid[mi[ok]] = True
            out_ori[mi[ok]] = o[missed][ok]
            out_dir[mi[ok]] = d[missed][ok]
            if k == max_bounces:
                break
            hi = idx[hitted]
            tape[k, hi] = b["face"]
            hits[hi] = k + 1
            refracted = b["refracted"]
            if tir == "reflect":
                ro, rd = _reflect(o[hitted], d[hitted], b["t"], b["n"])
                sel = refracted.view(-1, 1)
                o, d = torch.where(sel, b["new_o"], ro), torch.where(sel, b["new_d"], rd)
                refr[hi] += refracted.long()
                idx = hi
            else:
                o, d = b["new_o"][refracted], b["new_d"][refracted]
                idx = hi[refracted]
                refr[idx] += 1
        hits[torch.logical_not(valid)] = 0
    finally:
        orc.USE_BVH = old_bvh
    return dict(tape=tape, hits=hits, valid=valid, out_ori=out_ori, out_dir=out_dir)


def interact(o, d, tri, ior_int, ior_ext):
    """One interaction of every row, differentiable: (new_o, new_d, tir).  Rows with the TIR flag continue mirrored."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, torch.full_like(t, ior_int), torch.full_like(t, ior_ext))
    eta_t = torch.where(leaving, torch.full_like(t, ior_ext), torch.full_like(t, ior_int))
    n = n * sgn.view(-1, 1)
    tir = fresnel_tir(cos_i * sgn, eta_i, eta_t)
    wt = refract_dir(wo, n, eta_i / eta_t)
    to = (o + t.view(-1, 1) * d) + 1e-5 * wt
    ro, wr = _reflect(o, d, t, n)
    sel = tir.view(-1, 1)
    return torch.where(sel, ro, to), torch.where(sel, wr, wt), tir


def render_paths(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, aux=None):
    """(out_ori, out_dir, mask, aux) of Scene.render_paths, differentiable in V (and the rays).  ``aux``: an earlier ``trace`` to re-use."""
    if aux is None:
        aux = trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir)
    F = torch.as_tensor(faces, dtype=torch.long)
    vi = torch.nonzero(aux["valid"]).squeeze(1)
    o, d = origin[vi], ray_dir[vi]
    n_hits = aux["hits"][vi]
    for k in range(max_bounces):
        sel = torch.nonzero(n_hits > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, flag = interact(o[sel], d[sel], V[F[aux["tape"][k, vi[sel]]]], ior_int, ior_ext)
        assert tir == "reflect" or not flag.any()
        o = o.index_put((sel,), no)
        d = d.index_put((sel,), nd)
    P = origin.shape[0]
    zeros = torch.zeros((P, 3), dtype=torch.float64)
    out_ori = zeros.index_put((vi,), o)
    out_dir = zeros.index_put((vi,), d)
    mask = torch.zeros((P, 3), dtype=torch.bool)
    mask[vi] = True
    return out_ori, out_dir, mask, aux
