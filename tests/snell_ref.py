"""Float64 restatement of the K-interaction path law with the refraction formula as its third element (Scene.render_paths(...,
refraction=); test only).

``refraction="reference"`` is tests/paths_ref.py itself.  ``refraction="snell"`` is the same law with ONE statement of a refracting bounce
changed (drt_amd/csrc/drt_shade.h bounce_forward_snell): cosThetaT = sqrt(max(1 - eta^2 * sin2ThetaI, 0)), so that
sin(theta_t) = eta * sin(theta_i), where the reference's Refract takes sqrt(1 - sin2ThetaI).  It is built from the oracle's pieces --
``intersect_ids`` (so the face ids come from the oracle's tracer), ``moller_trumbore``, ``fresnel_tir`` -- and ``paths_ref._reflect``, plus
the local ``refract_dir_snell``; nothing of ``oracle.diffrender_oracle`` is replaced.  ``render_paths`` recomputes the completed paths from
the face tape in torch, so autograd supplies the gradients w.r.t. the vertices."""
import torch

import paths_ref
from oracle import diffrender_oracle as orc
from oracle.diffrender_oracle import _dot, _norm, fresnel_tir, moller_trumbore, refract_dir

REFRACTIONS = ("reference", "snell")


def refract_dir_snell(wo, n, eta):
    """Snell's refracted direction in the reference's form wt = eta * -wo + (eta * cos_i - cos_t) * n, normalised.  The guard of the
    adjoint is spelled out: where 1 - eta^2 * sin2_i is not positive cos_t is the constant 0 and no gradient passes through it (sqrt's own
    derivative there would be inf)."""
    eta = eta.view(-1, 1)
    cos_i = _dot(n, wo).view(-1, 1)
    sin2_i = (1 - cos_i * cos_i).clamp(min=0)
    arg = 1.0 - (eta * eta) * sin2_i
    arg = torch.where(arg < 0, torch.zeros_like(arg), arg)
    pos = arg > 0
    cos_t = torch.where(pos, torch.sqrt(torch.where(pos, arg, torch.ones_like(arg))), torch.zeros_like(arg))
    wt = eta * -wo + (eta * cos_i - cos_t) * n
    return wt / _norm(wt)


def _refract(refraction):
    assert refraction in REFRACTIONS
    return refract_dir_snell if refraction == "snell" else refract_dir


def _bounce(mesh, o, d, ior_int, ior_ext, refraction):
    """oracle.bounce (one Dintersect + refract_ray) with the refraction formula chosen."""
    ids, hitted = orc.intersect_ids(mesh, o, d)
    fid = ids[hitted]
    tri = mesh.vertices[mesh.faces[fid]]
    oh, dh = o[hitted], d[hitted]
    t, n, wo, eta, tir = _frame(oh, dh, tri, ior_int, ior_ext)
    wt = _refract(refraction)(wo, n, eta)
    new_o = (oh + t.view(-1, 1) * dh) + 1e-5 * wt
    return dict(hitted=hitted, face=fid, t=t, n=n, refracted=torch.logical_not(tir), new_o=new_o, new_d=wt)


def trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction="reference"):
    """paths_ref.trace under the chosen refraction: dict(tape, hits, valid, out_ori, out_dir) with its conventions."""
    if refraction == "reference":
        return paths_ref.trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir)
    assert 2 <= max_bounces <= 8 and tir in ("drop", "reflect") and refraction == "snell"
    P = origin.shape[0]
    mesh = orc.Mesh(faces, V.detach())
    old_bvh, orc.USE_BVH = orc.USE_BVH, len(mesh.faces) > paths_ref.BVH_FACES
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
                b = _bounce(mesh, o, d, ior_int, ior_ext, refraction)
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
                ro, rd = paths_ref._reflect(o[hitted], d[hitted], b["t"], b["n"])
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


def _frame(o, d, tri, ior_int, ior_ext):
    """What refract_ray sets up at a hit: (t, flipped normal, wo, eta, tir flag)."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, torch.full_like(t, ior_int), torch.full_like(t, ior_ext))
    eta_t = torch.where(leaving, torch.full_like(t, ior_ext), torch.full_like(t, ior_int))
    return t, n * sgn.view(-1, 1), wo, eta_i / eta_t, fresnel_tir(cos_i * sgn, eta_i, eta_t)


def refract_only(o, d, tri, ior_int, ior_ext, refraction="snell"):
    """The refract continuation of every row whatever its TIR flag says, differentiable: (new_o, wt, tir)."""
    t, n, wo, eta, tir = _frame(o, d, tri, ior_int, ior_ext)
    wt = _refract(refraction)(wo, n, eta)
    return (o + t.view(-1, 1) * d) + 1e-5 * wt, wt, tir


def interact(o, d, tri, ior_int, ior_ext, refraction="reference"):
    """One interaction of every row, differentiable: (new_o, new_d, tir).  Rows with the TIR flag continue mirrored."""
    if refraction == "reference":
        return paths_ref.interact(o, d, tri, ior_int, ior_ext)
    t, n, wo, eta, tir = _frame(o, d, tri, ior_int, ior_ext)
    wt = _refract(refraction)(wo, n, eta)
    to = (o + t.view(-1, 1) * d) + 1e-5 * wt
    ro, wr = paths_ref._reflect(o, d, t, n)
    sel = tir.view(-1, 1)
    return torch.where(sel, ro, to), torch.where(sel, wr, wt), tir


def render_paths(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction="reference", aux=None):
    """(out_ori, out_dir, mask, aux) of Scene.render_paths, differentiable in V (and the rays).  ``aux``: an earlier ``trace`` to re-use."""
    if aux is None:
        aux = trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction)
    F = torch.as_tensor(faces, dtype=torch.long)
    vi = torch.nonzero(aux["valid"]).squeeze(1)
    o, d = origin[vi], ray_dir[vi]
    n_hits = aux["hits"][vi]
    for k in range(max_bounces):
        sel = torch.nonzero(n_hits > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, flag = interact(o[sel], d[sel], V[F[aux["tape"][k, vi[sel]]]], ior_int, ior_ext, refraction)
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
