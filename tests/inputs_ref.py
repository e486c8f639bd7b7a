"""Float64 restatement of the refraction path with the rays and the indices of refraction as differentiable torch inputs (test only).

Built from the oracle's moller_trumbore / refract_dir; the face ids come from the oracle's tracer (oracle.diffrender_oracle
.render_transparent), and the completed paths are then recomputed from them in torch, so autograd differentiates origin, ray_dir,
the vertices and both IORs -- what the reference's own autograd does (tests/golden/make_golden_inputs.py)."""
import torch

from oracle import diffrender_oracle as orc
from oracle.diffrender_oracle import moller_trumbore, refract_dir


def bounce(o, d, tri, ior_int, ior_ext):
    """One bounce of the reference's refract_ray (DiffRender.py:503-535) with tensor IORs: (new_o, new_d)."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = (wo * n).sum(1).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, ior_int, ior_ext)
    eta_t = torch.where(leaving, ior_ext, ior_int)
    n = n * sgn.view(-1, 1)
    wt = refract_dir(wo, n, eta_i / eta_t)
    return o + t.view(-1, 1) * d + 1e-5 * wt, wt


def _f(x):
    return float(x.detach()) if isinstance(x, torch.Tensor) else float(x)


def render_transparent(faces, V, origin, ray_dir, ior_int, ior_ext, aux=None):
    """(out_ori, out_dir, mask, aux) as the reference's render_transparent, differentiable in every tensor input.  ``aux``: the face
    ids of an earlier call (oracle render_transparent's aux) to re-use."""
    if aux is None:
        mesh = orc.Mesh(faces, V.detach())
        aux = orc.render_transparent(mesh, origin.detach(), ray_dir.detach(), _f(ior_int), _f(ior_ext), return_aux=True)[3]
    vi = aux["valid_ind"]
    F = torch.as_tensor(faces, dtype=torch.long)
    o2, d2 = bounce(origin[vi], ray_dir[vi], V[F[aux["face1"][vi]]], ior_int, ior_ext)
    o3, d3 = bounce(o2, d2, V[F[aux["face2"][vi]]], ior_int, ior_ext)
    P = origin.shape[0]
    zeros = torch.zeros((P, 3), dtype=torch.float64)
    out_ori = zeros.index_put((vi,), o3)
    out_dir = zeros.index_put((vi,), d3)
    mask = torch.zeros((P, 3), dtype=torch.bool)
    mask[vi] = True
    return out_ori, out_dir, mask, aux
