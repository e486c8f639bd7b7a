"""Float64 restatement of the absorbing refracted image and its photometric loss (Scene.render_image / Scene.image_loss_fused with
``absorption``; drt_amd/csrc/drt_image_absorb.h; test only), differentiable in the vertices, the two indices of refraction and the
absorption coefficients by torch autograd.

Built on ``image_loss_ref`` and ``image_ref``: the sample rays, ``snell_ref.trace`` (classes and the face tape), ``ior_ref.interact`` on
that tape (the path), ``image_loss_ref.interaction_factor`` (the throughput), ``image_ref.screen_uv`` / ``image_ref.bilinear``.  What is
added: the interior length ``L`` -- the sum, in interaction order, of the ``t`` of ``moller_trumbore`` over the interactions of the
recorded tape whose incoming ray travels inside the object (``not dot(-d, n) > 0``, refracting or mirrored) --, ``A = exp(-(sigma L))``
and the colour ``(A T) B`` of a through or direct sample on the screen (``L = 0`` on a direct one).  The VALUE of ``L`` is taken from
``length_values``, the same path in numpy with correctly rounded roots (torch's vectorised roots and norms may be a unit in the last
place off, which a comparison with tolerance 0 cannot take); its derivative is autograd's of the torch graph.  The class, the tape, the TIR flags,
the inside test, ``floor`` and the on-screen test carry no gradient."""
import numpy as np
import torch

import image_loss_ref
import image_ref
import ior_ref
import snell_ref
from oracle.diffrender_oracle import _dot, moller_trumbore

F64 = torch.float64


def inside_t(o, d, tri):
    """(t, inside bool) of one interaction of every row: moller_trumbore's t, and whether the incoming ray travels inside the object."""
    _, _, t, n = moller_trumbore(o, d, tri)
    cos_i = _dot(-d, n).clamp(-1, 1)
    return t, torch.logical_not(cos_i > 0).detach()


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def interact_values(o, d, tri, ior_int, ior_ext, refraction):
    """One interaction of every row in numpy float64, one rounding per operation in the law's association with correctly rounded roots
    (torch's vectorised roots and norms may be a unit in the last place off, differently on different machines): (t, inside, new_o,
    new_d) -- refracted, or mirrored where the TIR flag is set."""
    col = lambda x: x[:, None]      # noqa: E731
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    inv = 1.0 / _dot3(e1, _cross3(d, e2))
    q = _cross3(o - v0, e1)
    t = _dot3(e2, q) * inv
    m = _cross3(e1, e2)
    n0 = m / col(np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]))
    wo = -d
    c = np.clip(_dot3(wo, n0), -1.0, 1.0)
    inside = ~(c > 0)
    eta_i, eta_t = np.where(inside, ior_int, ior_ext), np.where(inside, ior_ext, ior_int)
    c = np.where(inside, -c, c)
    n = col(np.where(inside, -1.0, 1.0)) * n0
    tir = np.sqrt(np.clip(1.0 - c * c, 0.0, 1.0)) * eta_i / eta_t >= 1.0
    eta = eta_i / eta_t
    ci = _dot3(n, wo)
    s2 = np.maximum(1.0 - ci * ci, 0.0)
    ct = np.sqrt(np.maximum(1.0 - (eta * eta) * s2, 0.0)) if refraction == "snell" else np.sqrt(1.0 - np.minimum(s2, 1.0))
    w = col(eta) * d + col(eta * ci - ct) * n
    wt = w / col(np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]))
    wr = d + col(2.0 * ci) * n
    out_d = np.where(col(tir), wr, wt)
    return t, inside, (o + col(t) * d) + 1e-5 * out_d, out_d


def length_values(F, V, o, d, tape, n_hits, ior_int, ior_ext, max_bounces, refraction):
    """The interior length of every row along its recorded tape [K, rows], by interact_values."""
    o, d, L = o.copy(), d.copy(), np.zeros(len(o))
    for k in range(max_bounces):
        sel = np.nonzero(n_hits > k)[0]
        if len(sel) == 0:
            break
        t, inside, no, nd = interact_values(o[sel], d[sel], V[F[tape[k, sel]]], ior_int, ior_ext, refraction)
        L[sel] = np.where(inside, L[sel] + t, L[sel])
        o[sel], d[sel] = no, nd
    return L


def forward(faces, V, camera_M, height, width, screen, texture, s, law, fresnel, void, invalid, ior_int, ior_ext, sigma, detach_L=False):
    """dict(mean float64 [H * W, C], col [P, C], cls, on, T, L, A [P, C] (1 off the through samples), u, v, t, dn, through_on).  V, ior_int,
    ior_ext, sigma: tensors autograd may track (sigma [C]), or plain values."""
    max_bounces, tir, refraction = law
    V = torch.as_tensor(np.asarray(V) if not isinstance(V, torch.Tensor) else V, dtype=F64)
    vi_int, vi_ext = ior_ref._value(ior_int), ior_ref._value(ior_ext)
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    P = o.shape[0]
    tex = np.asarray(texture)
    tex = tex[:, :, None] if tex.ndim == 2 else tex
    C = tex.shape[2]
    sigma = sigma if isinstance(sigma, torch.Tensor) else torch.as_tensor(np.broadcast_to(np.asarray(sigma, np.float64), (C,)).copy())
    if len(faces) == 0:
        cls = torch.zeros(P, dtype=torch.long)
        out_o, out_d, T, L = o, d, torch.ones(P, dtype=F64), torch.zeros(P, dtype=F64)
    else:
        aux = snell_ref.trace(faces, V.detach(), o, d, vi_int, vi_ext, max_bounces, tir, refraction)
        hit, valid = aux["tape"][0] >= 0, aux["valid"]
        cls = torch.where(hit, torch.where(valid, image_ref.THROUGH, image_ref.INVALID), image_ref.DIRECT)
        F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
        vi = torch.nonzero(valid).squeeze(1)
        po, pd, n_hits = o[vi], d[vi], aux["hits"][vi]
        Tv, Lv = torch.ones(len(vi), dtype=F64), torch.zeros(len(vi), dtype=F64)
        for k in range(max_bounces):
            sel = torch.nonzero(n_hits > k).squeeze(1)
            if len(sel) == 0:
                break
            tri = V[F[aux["tape"][k, vi[sel]]]]
            t, inside = inside_t(po[sel], pd[sel], tri)
            Lv = Lv.index_put((sel,), torch.where(inside, Lv[sel] + t, Lv[sel]))
            if fresnel:
                Tv = Tv.index_put((sel,), Tv[sel] * image_loss_ref.interaction_factor(po[sel], pd[sel], tri, ior_int, ior_ext))
            no, nd, _ = ior_ref.interact(po[sel], pd[sel], tri, ior_int, ior_ext, refraction)
            po = po.index_put((sel,), no)
            pd = pd.index_put((sel,), nd)
        out_o, out_d = o.index_put((vi,), po), d.index_put((vi,), pd)
        T = torch.ones(P, dtype=F64).index_put((vi,), Tv)
        # the VALUE of L from the elementwise statement of the path (the difference, a few units in the last place, enters as a constant:
        # the derivative stays autograd's, as image_loss_ref._guarded_sqrt keeps its root's)
        Lx = torch.from_numpy(length_values(F.numpy(), V.detach().numpy(), o[vi].numpy(), d[vi].numpy(), aux["tape"][:, vi].numpy(), n_hits.numpy(),
                                            vi_int, vi_ext, max_bounces, refraction))
        assert len(vi) == 0 or float((Lx - Lv.detach()).abs().max()) <= 1e-9
        Lv = Lv + (Lx - Lv).detach()
        L = torch.zeros(P, dtype=F64).index_put((vi,), Lv)
    if detach_L:
        L = L.detach()
    on, u, v, t, dn = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], out_o, out_d)
    on = on & (cls != image_ref.INVALID)
    A = torch.exp(-(sigma.view(1, C) * L.view(-1, 1)))
    col = torch.as_tensor(np.broadcast_to(np.asarray(void, np.float64), (C,)).copy()).view(1, C).repeat(P, 1)
    idx = torch.nonzero(on).squeeze(1)
    col = col.index_put((idx,), (A[idx] * T[idx].view(-1, 1)) * image_ref.bilinear(tex, u[idx], v[idx]))
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    return dict(mean=acc / float(s2), col=col, cls=cls, on=on, T=T, L=L, A=A, u=u, v=v, t=t, dn=dn, through_on=int((on & (cls == image_ref.THROUGH)).sum()))


def length_plane(fwd, height, width, s):
    """float32 [H, W]: the mean of L over a pixel's through samples (summed in sample order), 0 where there are none."""
    s2 = s * s
    thr = (fwd["cls"] == image_ref.THROUGH).view(-1, s2)
    L = torch.where(thr, fwd["L"].detach().view(-1, s2), torch.zeros((), dtype=F64))
    acc = L[:, 0].clone()
    for j in range(1, s2):
        acc = acc + L[:, j]
    n = thr.sum(1)
    return torch.where(n > 0, acc / n.clamp(min=1).to(F64), torch.zeros((), dtype=F64)).to(torch.float32).view(height, width)


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, target, s, law, fresnel, void, invalid, ior_int, ior_ext, sigma, weight=None,
                   length_gradient=True):
    """dict(loss, grad_V [nv, 3], g_int, g_ext, g_sigma [C], count, image float32 [H, W, C], fwd).  ``length_gradient=False`` detaches L
    everywhere but in d / d sigma's own factor -- the adjoint that drops the length term, which is NOT the derivative of the law (the
    tests' negative control)."""
    Vt = torch.as_tensor(np.asarray(V), dtype=F64).clone().requires_grad_(True)
    ii = torch.tensor(float(ior_int), dtype=F64, requires_grad=True)
    ie = torch.tensor(float(ior_ext), dtype=F64, requires_grad=True)
    tex = np.asarray(texture)
    C = 1 if tex.ndim == 2 else tex.shape[2]
    sg = torch.as_tensor(np.broadcast_to(np.asarray(sigma, np.float64), (C,)).copy()).requires_grad_(True)
    fwd = forward(faces, Vt, camera_M, height, width, screen, texture, s, law, fresnel, void, invalid, ii, ie, sg, detach_L=not length_gradient)
    mean = fwd["mean"]
    loss = image_loss_ref.loss_of(mean, target, weight)
    if loss.requires_grad:
        gV, gi, ge, gs = torch.autograd.grad(loss, (Vt, ii, ie, sg), allow_unused=True)
    else:
        gV = gi = ge = gs = None
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    return dict(loss=float(loss.detach()), grad_V=z(gV, Vt).numpy(), g_int=float(z(gi, ii)), g_ext=float(z(ge, ie)), g_sigma=z(gs, sg).numpy(),
                count=fwd["through_on"], image=mean.detach().to(torch.float32).view(height, width, C).numpy(), fwd=fwd)
