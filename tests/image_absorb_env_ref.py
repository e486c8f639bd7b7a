"""Float64 restatement of absorbing glass in front of an environment (Scene.image_loss_views_fused with ``absorption`` on a binding with
an environment; drt_amd/csrc/drt_image_env.h with ABSORB / LENGTH; test only), differentiable in the vertices, the two
indices of refraction and the absorption coefficients by torch autograd.

The path comes from ``image_env_ref.loss_forward``: classes, the face tape, hit counts, the throughput ``T`` and the unweighted background
``B`` of every exit ray (texture where the ray lands on the screen, the environment lookup otherwise) are its values and its graph.  What is
added is ``image_absorb_ref``'s: the interior length ``L`` of a through sample -- ``inside_t`` along that tape with ``ior_ref.interact`` as
the continuation, its VALUE from ``length_values`` (correctly rounded roots), its derivative autograd's -- and ``A = exp(-(sigma L))``.
The transmitted colour is ``(A T) B`` whether ``B`` came from the screen or from the environment (``L = 0`` on a direct sample).  The
reflection ``R1 B(ro, wr)`` is recomputed from V as ``loss_forward`` does it and is NOT attenuated: that light never entered the object,
so it carries no gradient to sigma and none through L.  A multi-view result is the sum of per-view results."""
import numpy as np
import torch

import image_absorb_ref
import image_env_ref
import image_loss_ref
import image_ref
import ior_ref
import paths_ref
from oracle.diffrender_oracle import _cross, _dot, moller_trumbore

F64 = torch.float64


def interior_length(faces, V, o, d, cls, tape, hits, ior_int, ior_ext, law):
    """L float64 [P] of every sample along the recorded tape (0 off the through samples): the torch graph of image_absorb_ref.forward's
    loop, the value of image_absorb_ref.length_values."""
    max_bounces, _, refraction = law
    P = o.shape[0]
    if len(faces) == 0:
        return torch.zeros(P, dtype=F64)
    vi_int, vi_ext = ior_ref._value(ior_int), ior_ref._value(ior_ext)
    F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    vi = torch.nonzero(cls == image_ref.THROUGH).squeeze(1)
    po, pd, n_hits = o[vi], d[vi], hits[vi]
    Lv = torch.zeros(len(vi), dtype=F64)
    for k in range(max_bounces):
        sel = torch.nonzero(n_hits > k).squeeze(1)
        if len(sel) == 0:
            break
        tri = V[F[tape[k, vi[sel]]]]
        t, inside = image_absorb_ref.inside_t(po[sel], pd[sel], tri)
        Lv = Lv.index_put((sel,), torch.where(inside, Lv[sel] + t, Lv[sel]))
        no, nd, _ = ior_ref.interact(po[sel], pd[sel], tri, ior_int, ior_ext, refraction)
        po = po.index_put((sel,), no)
        pd = pd.index_put((sel,), nd)
    Lx = torch.from_numpy(image_absorb_ref.length_values(F.numpy(), V.detach().numpy(), o[vi].numpy(), d[vi].numpy(), tape[:, vi].numpy(), n_hits.numpy(),
                                                         vi_int, vi_ext, max_bounces, refraction))
    assert len(vi) == 0 or float((Lx - Lv.detach()).abs().max()) <= 1e-9
    Lv = Lv + (Lx - Lv).detach()
    return torch.zeros(P, dtype=F64).index_put((vi,), Lv)


def forward(faces, V, camera_M, height, width, screen, texture, env, R, s, law, invalid, ior_int, ior_ext, sigma, reflect=False, detach_L=False,
            sigma_sees_reflection=False):
    """dict(mean float64 [H * W, C], trans [P, C] (the transmitted colour (A T) B of every row), cls, T, L, A, bg, through, tape, hits, seen,
    and with ``reflect`` added bool [P]).  V, ior_int, ior_ext, sigma: tensors autograd may track (sigma [C]), or plain values.  The two
    switches are the tests' negative controls, NOT the derivative of the law: ``detach_L`` cuts the gradient through the interior length;
    ``sigma_sees_reflection`` lets the reflected light into d / d sigma as if it had been attenuated (same values)."""
    V = torch.as_tensor(np.asarray(V) if not isinstance(V, torch.Tensor) else V, dtype=F64)
    C = np.asarray(env).shape[2]
    sigma = sigma if isinstance(sigma, torch.Tensor) else torch.as_tensor(np.broadcast_to(np.asarray(sigma, np.float64), (C,)).copy())
    base = image_env_ref.loss_forward(faces, V, camera_M, height, width, screen, texture, env, R, s, law, invalid, ior_int, ior_ext, reflect=False)
    cls, T, bg = base["cls"], base["T"], base["bg"]
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    L = interior_length(faces, V, o, d, cls, base["tape"], base["hits"], ior_int, ior_ext, law)
    if detach_L:
        L = L.detach()
    A = torch.exp(-(sigma.view(1, C) * L.view(-1, 1)))
    trans = (A * T.view(-1, 1)) * bg["B"]
    col = trans
    out = dict(cls=cls, T=T, L=L, A=A, bg=bg, through=base["through"], tape=base["tape"], hits=base["hits"], seen=torch.zeros(len(o), dtype=torch.bool))
    if reflect and len(faces):
        F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
        r0 = image_env_ref.reflection(faces, V.detach(), o, d, ior_ref._value(ior_int), ior_ref._value(ior_ext))
        added = r0["seen"] & (cls == image_ref.THROUGH)
        ai = torch.nonzero(added).squeeze(1)
        tri = V[F[r0["face"][ai]]]
        _, _, t, _ = moller_trumbore(o[ai], d[ai], tri)
        m = _cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n = m / torch.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).view(-1, 1)      # (entering: the normal is not flipped)
        ci = _dot(n, -d[ai])
        ro, wr = paths_ref._reflect(o[ai], d[ai], t, n)
        R1 = image_loss_ref.fresnel_R(ci, torch.ones_like(ci) * ior_ext, torch.ones_like(ci) * ior_int)
        rb = image_env_ref.background(screen, texture, env, R, ro, wr)
        term = R1.view(-1, 1) * rb["B"]
        if sigma_sees_reflection:
            Aa = torch.exp(-(sigma.view(1, C) * L[ai].detach().view(-1, 1)))
            term = term * (Aa / Aa.detach())
        col = col.index_put((ai,), col[ai] + term)
        out.update(added=added, rb=rb, seen=r0["seen"])
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    out.update(mean=acc / float(s2), trans=trans)
    return out


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, env, R, target, s, law, invalid, ior_int, ior_ext, sigma, weight=None, reflect=False,
                   length_gradient=True, sigma_sees_reflection=False):
    """dict(loss, grad_V [nv, 3], g_int, g_ext, g_sigma [C], count (every through sample), image float32 [H, W, C], fwd)."""
    Vt = torch.as_tensor(np.asarray(V), dtype=F64).clone().requires_grad_(True)
    ii = torch.tensor(float(ior_int), dtype=F64, requires_grad=True)
    ie = torch.tensor(float(ior_ext), dtype=F64, requires_grad=True)
    C = np.asarray(env).shape[2]
    sg = torch.as_tensor(np.broadcast_to(np.asarray(sigma, np.float64), (C,)).copy()).requires_grad_(True)
    fwd = forward(faces, Vt, camera_M, height, width, screen, texture, env, R, s, law, invalid, ii, ie, sg, reflect, not length_gradient, sigma_sees_reflection)
    loss = image_loss_ref.loss_of(fwd["mean"], target, weight)
    gV, gi, ge, gs = torch.autograd.grad(loss, (Vt, ii, ie, sg), allow_unused=True) if loss.requires_grad else (None,) * 4
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    return dict(loss=float(loss.detach()), grad_V=z(gV, Vt).numpy(), g_int=float(z(gi, ii)), g_ext=float(z(ge, ie)), g_sigma=z(gs, sg).detach().numpy(),
                count=fwd["through"], image=fwd["mean"].detach().to(torch.float32).view(height, width, C).numpy(), fwd=fwd)
