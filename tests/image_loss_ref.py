"""Float64 restatement of the photometric loss of the refracted image (Scene.image_loss_fused; drt_amd/csrc/drt_image_loss.h; test only),
differentiable in the vertices and the two indices of refraction by torch autograd.

Built from what the other restatements already state: ``image_ref.sample_rays`` (the sample rays), ``snell_ref.trace`` (classes and the
face tape, from the oracle's tracer, with the IORs' values), ``ior_ref.interact`` on that tape (the path, differentiable in V and the
IORs), ``image_ref.screen_uv`` / ``image_ref.bilinear`` (plane and texture) and the pixel mean in float64.  ONE function is restated:
``fresnel_R`` with ``torch.sqrt`` where ``image_ref`` takes a detached, correctly rounded root (whose value is kept) -- and with the guard of the adjoint
spelled out as ``snell_ref.refract_dir_snell`` spells its own: where the argument of a root is not positive the root is the constant 0
and no gradient passes through it.  The class of a sample, the tape, the TIR flags, the entering / leaving branch, ``floor`` and the
on-screen test carry no gradient, as in torch."""
import numpy as np
import torch

import image_ref
import ior_ref
import snell_ref
from oracle.diffrender_oracle import _dot, fresnel_tir, moller_trumbore

F64 = torch.float64


def _guarded_sqrt(x):
    """torch.sqrt behind the guard, with the VALUE of image_ref's correctly rounded root: torch's vectorised float64 root may be one unit
    in the last place off, differently on different machines; the difference (exact: the two are neighbours) is added as a constant, so
    the derivative stays torch.sqrt's own."""
    pos = x > 0
    safe = torch.where(pos, x, torch.ones_like(x))
    y = torch.sqrt(safe)
    y = y + (image_ref._sqrt(safe) - y).detach()
    return torch.where(pos, y, torch.zeros_like(x))


def fresnel_R(ci, eta_i, eta_t):
    """image_ref.fresnel_R, differentiable in its three arguments."""
    ci, eta_i, eta_t = (torch.as_tensor(v, dtype=F64) for v in (ci, eta_i, eta_t))
    sin_i = _guarded_sqrt((1 - ci * ci).clamp(0, 1))
    sin_t = sin_i * eta_i / eta_t
    cos_t = _guarded_sqrt((1 - sin_t * sin_t).clamp(min=0))
    r_parl = ((eta_t * ci) - (eta_i * cos_t)) / ((eta_t * ci) + (eta_i * cos_t))
    r_perp = ((eta_i * ci) - (eta_t * cos_t)) / ((eta_i * ci) + (eta_t * cos_t))
    return (r_parl * r_parl + r_perp * r_perp) / 2


def interaction_factor(o, d, tri, ior_int, ior_ext):
    """image_ref.interaction_factor with tensor IORs and this module's fresnel_R: 1 - R per row, 1 where the TIR flag is set."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    ii, ie = torch.ones_like(t) * ior_int, torch.ones_like(t) * ior_ext
    eta_i = torch.where(leaving, ii, ie)
    eta_t = torch.where(leaving, ie, ii)
    tir = fresnel_tir((cos_i * sgn).detach(), eta_i.detach(), eta_t.detach())
    ci = _dot(n * sgn.view(-1, 1), wo)
    return torch.where(tir, torch.ones_like(t), 1 - fresnel_R(ci, eta_i, eta_t))


def forward(faces, V, camera_M, height, width, screen, texture, s, law, fresnel, void, invalid, ior_int, ior_ext, detach_T=False):
    """dict(mean float64 [H * W, C] (the pixel mean before its float32 store), cls, on, T, u, v, dn, through_on: number of through samples
    on the screen).  V, ior_int, ior_ext: tensors autograd may track (V [nv, 3]; the IORs 0-dim), or plain values."""
    max_bounces, tir, refraction = law
    V = torch.as_tensor(np.asarray(V) if not isinstance(V, torch.Tensor) else V, dtype=F64)
    vi_int, vi_ext = ior_ref._value(ior_int), ior_ref._value(ior_ext)
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    P = o.shape[0]
    tex = np.asarray(texture)
    tex = tex[:, :, None] if tex.ndim == 2 else tex
    C = tex.shape[2]
    if len(faces) == 0:
        cls = torch.zeros(P, dtype=torch.long)
        out_o, out_d, T = o, d, torch.ones(P, dtype=F64)
    else:
        aux = snell_ref.trace(faces, V.detach(), o, d, vi_int, vi_ext, max_bounces, tir, refraction)
        hit, valid = aux["tape"][0] >= 0, aux["valid"]
        cls = torch.where(hit, torch.where(valid, image_ref.THROUGH, image_ref.INVALID), image_ref.DIRECT)
        F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
        vi = torch.nonzero(valid).squeeze(1)
        po, pd, n_hits, Tv = o[vi], d[vi], aux["hits"][vi], torch.ones(len(vi), dtype=F64)
        for k in range(max_bounces):
            sel = torch.nonzero(n_hits > k).squeeze(1)
            if len(sel) == 0:
                break
            tri = V[F[aux["tape"][k, vi[sel]]]]
            if fresnel:
                Tv = Tv.index_put((sel,), Tv[sel] * interaction_factor(po[sel], pd[sel], tri, ior_int, ior_ext))
            no, nd, _ = ior_ref.interact(po[sel], pd[sel], tri, ior_int, ior_ext, refraction)
            po = po.index_put((sel,), no)
            pd = pd.index_put((sel,), nd)
        out_o, out_d = o.index_put((vi,), po), d.index_put((vi,), pd)
        T = torch.ones(P, dtype=F64).index_put((vi,), Tv)
    if detach_T:
        T = T.detach()
    on, u, v, t, dn = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], out_o, out_d)
    on = on & (cls != image_ref.INVALID)
    col = torch.as_tensor(np.broadcast_to(np.asarray(void, np.float64), (C,)).copy()).view(1, C).repeat(P, 1)
    idx = torch.nonzero(on).squeeze(1)
    col = col.index_put((idx,), T[idx].view(-1, 1) * image_ref.bilinear(tex, u[idx], v[idx]))
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    return dict(mean=acc / float(s2), cls=cls, on=on, T=T, u=u, v=v, dn=dn, through_on=int((on & (cls == image_ref.THROUGH)).sum()))


def loss_of(mean, target, weight=None):
    """sum_p w_p ((r_0^2 + r_1^2) + r_2^2), r = mean - float64(target)."""
    tgt = torch.as_tensor(np.asarray(target, dtype=np.float32)).to(F64).reshape(mean.shape)
    r = mean - tgt
    term = r[:, 0] * r[:, 0]
    for ch in range(1, r.shape[1]):
        term = term + r[:, ch] * r[:, ch]
    if weight is not None:
        term = torch.as_tensor(np.asarray(weight, dtype=np.float32)).to(F64).reshape(-1) * term
    return term.sum()


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, target, s, law, fresnel, void, invalid, ior_int, ior_ext, weight=None,
                   throughput_gradient=True):
    """dict(loss, grad_V [nv, 3], g_int, g_ext, count, image float32 [H, W, C], fwd).  ``throughput_gradient=False`` detaches T: the
    geometry-only gradient, which is NOT the derivative of the law (the tests' negative control)."""
    Vt = torch.as_tensor(np.asarray(V), dtype=F64).clone().requires_grad_(True)
    ii = torch.tensor(float(ior_int), dtype=F64, requires_grad=True)
    ie = torch.tensor(float(ior_ext), dtype=F64, requires_grad=True)
    fwd = forward(faces, Vt, camera_M, height, width, screen, texture, s, law, fresnel, void, invalid, ii, ie, detach_T=not throughput_gradient)
    mean = fwd["mean"]
    loss = loss_of(mean, target, weight)
    if loss.requires_grad:
        gV, gi, ge = torch.autograd.grad(loss, (Vt, ii, ie), allow_unused=True)
    else:
        gV = gi = ge = None
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    C = mean.shape[1]
    return dict(loss=float(loss.detach()), grad_V=z(gV, Vt).numpy(), g_int=float(z(gi, ii)), g_ext=float(z(ge, ie)), count=fwd["through_on"],
                image=mean.detach().to(torch.float32).view(height, width, C).numpy(), fwd=fwd)
