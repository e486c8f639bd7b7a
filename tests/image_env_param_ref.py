"""Float64 restatement of the environment's texel and rotation gradients (Scene.image_loss_fused with ``env_texels_param`` /
``env_rotation_param``; drt_amd/csrc/drt_image_env_param.h; test only), differentiable by autograd.

``image_env_ref.env_dir`` and ``env_bilinear`` pass the rotation and the texels through ``np.asarray``, which cuts the graph; the two are
restated here with tensor inputs, statement for statement.  Everything else is taken from the existing modules and carries no gradient
here: classes and tape from ``snell_ref.trace``, exit rays from ``ior_ref.interact``, throughputs from
``image_loss_ref.interaction_factor``, the reflection's rays, ``R1`` and verdicts from ``image_env_ref.reflection``, the screen stage from
``image_ref.screen_uv``, the loss from ``image_loss_ref.loss_of``."""
import math

import numpy as np
import torch

import image_env_ref
import image_loss_ref
import image_ref
import ior_ref
import snell_ref

F64 = torch.float64


def env_dir(R, d):
    """image_env_ref.env_dir with a tensor R (the graph is kept)."""
    return [(R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1]) + R[r, 2] * d[:, 2] for r in range(3)]


def env_uv(R, d, eh, ew):
    ex, ey, ez = env_dir(R, d)
    theta = torch.acos(ey.clamp(-1, 1))
    phi = torch.atan2(ex, -ez)
    u = ((phi / (2.0 * math.pi)) + 0.5) * float(ew) - 0.5
    v = (theta / math.pi) * float(eh) - 0.5
    return u, v, ey


def env_bilinear(E, u, v):
    """image_env_ref.env_bilinear with a float64 tensor E [Eh, Ew, C] (the graph is kept): float64 [P, C]."""
    eh, ew = E.shape[:2]
    vc = v.clamp(0, eh - 1)
    y0 = torch.floor(vc).clamp(max=eh - 2)
    x0 = torch.floor(u).clamp(-1, ew - 1)
    fx, fy = (u - x0).view(-1, 1), (vc - y0).view(-1, 1)
    yi, xa, xb = y0.detach().long(), (x0.detach().long() + ew) % ew, (x0.detach().long() + 1) % ew
    t00, t01, t10, t11 = E[yi, xa], E[yi, xb], E[yi + 1, xa], E[yi + 1, xb]
    return ((t00 * (1 - fx) + t01 * fx) * (1 - fy)) + ((t10 * (1 - fx) + t11 * fx) * fy)


def samples(faces, V, camera_M, height, width, screen, texture, s, law, ior_int, ior_ext, reflect):
    """What a view's samples are, none of it differentiable here: dict(cls, o / d (camera rays), out_o / out_d (exit rays; the camera ray of
    a direct sample), T, on (the screen catches the exit ray), B_screen [P, C] or None, tape, hits, and with ``reflect`` refl
    (image_env_ref.reflection's dict), added, r_on and Br_screen of the reflected rays)."""
    max_bounces, tir, refraction = law
    V = torch.as_tensor(np.asarray(V), dtype=F64)
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    P = o.shape[0]
    F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    if len(faces) == 0:
        cls = torch.zeros(P, dtype=torch.long)
        out_o, out_d, T = o, d, torch.ones(P, dtype=F64)
        tape, hits = torch.full((max_bounces, P), -1, dtype=torch.long), torch.zeros(P, dtype=torch.long)
    else:
        aux = snell_ref.trace(faces, V, o, d, ior_int, ior_ext, max_bounces, tir, refraction)
        hit, valid = aux["tape"][0] >= 0, aux["valid"]
        tape, hits = aux["tape"], aux["hits"]
        cls = torch.where(hit, torch.where(valid, image_ref.THROUGH, image_ref.INVALID), image_ref.DIRECT)
        vi = torch.nonzero(valid).squeeze(1)
        po, pd, n_hits, Tv = o[vi], d[vi], aux["hits"][vi], torch.ones(len(vi), dtype=F64)
        for k in range(max_bounces):
            sel = torch.nonzero(n_hits > k).squeeze(1)
            if len(sel) == 0:
                break
            tri = V[F[aux["tape"][k, vi[sel]]]]
            Tv = Tv.index_put((sel,), Tv[sel] * image_loss_ref.interaction_factor(po[sel], pd[sel], tri, ior_int, ior_ext))
            no, nd, _ = ior_ref.interact(po[sel], pd[sel], tri, ior_int, ior_ext, refraction)
            po = po.index_put((sel,), no)
            pd = pd.index_put((sel,), nd)
        out_o, out_d = o.index_put((vi,), po), d.index_put((vi,), pd)
        T = torch.ones(P, dtype=F64).index_put((vi,), Tv)
    out = dict(cls=cls, o=o, d=d, out_o=out_o.detach(), out_d=out_d.detach(), T=T.detach(), tape=tape, hits=hits, on=torch.zeros(P, dtype=torch.bool), B_screen=None)

    def screen_stage(ro, rd):
        tex = np.asarray(texture)
        on, su, sv, _, _ = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], ro, rd)
        B = torch.zeros((len(ro), tex.shape[2]), dtype=F64)
        idx = torch.nonzero(on).squeeze(1)
        B[idx] = image_ref.bilinear(tex, su[idx], sv[idx])
        return on, B
    if screen is not None:
        out["on"], out["B_screen"] = screen_stage(out["out_o"], out["out_d"])
    if reflect and len(faces):
        refl = image_env_ref.reflection(faces, V, o, d, ior_int, ior_ext)
        out.update(refl=refl, added=refl["seen"] & (cls == image_ref.THROUGH), r_on=torch.zeros(P, dtype=torch.bool), Br_screen=None)
        if screen is not None:
            out["r_on"], out["Br_screen"] = screen_stage(refl["ro"], refl["wr"])
    return out


def loss_forward(sm, E, R, s, invalid, detach=None):
    """The loss's pixel means float64 [H * W, C] from ``samples``' dict, the float64 texels E [Eh, Ew, C] and the rotation R [3, 3] (both
    tensors that may require grad), with the reads: dict(mean, u / v / ey and read bool [P] of the exit / direct reads, and ru / rv / rey /
    r_read of the reflection's).  ``detach``: "direct" / "reflection" cut those reads out of the graph -- NOT the derivative of the law
    (negative controls)."""
    eh, ew, C = E.shape
    cls, T = sm["cls"], sm["T"]
    u, v, ey = env_uv(R, sm["out_d"], eh, ew)
    B = env_bilinear(E, u, v)
    if detach == "direct":
        B = torch.where((cls == image_ref.DIRECT).view(-1, 1), B.detach(), B)
    read = (cls != image_ref.INVALID) & ~sm["on"]
    if sm["B_screen"] is not None:
        B = torch.where(sm["on"].view(-1, 1), sm["B_screen"], B)
    col = T.view(-1, 1) * B
    out = dict(u=u.detach(), v=v.detach(), ey=ey.detach(), read=read, w=T)
    if "refl" in sm:
        refl, added = sm["refl"], sm["added"]
        ai = torch.nonzero(added).squeeze(1)          # (the added rows only: a row without a reflection has wr = 0, whose atan2 has no derivative)
        ru, rv, rey = env_uv(R, refl["wr"][ai], eh, ew)
        Br = env_bilinear(E, ru, rv)
        if sm["Br_screen"] is not None:
            Br = torch.where(sm["r_on"][ai].view(-1, 1), sm["Br_screen"][ai], Br)
        term = refl["R1"][ai].view(-1, 1) * Br
        if detach == "reflection":
            term = term.detach()
        col = col.index_put((ai,), col[ai] + term)
        out.update(ai=ai, ru=ru.detach(), rv=rv.detach(), rey=rey.detach(), r_read=~sm["r_on"][ai], rw=refl["R1"][ai])
    fill = torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C)
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), fill, col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    out["mean"] = acc / float(s2)
    return out


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, env, R, target, s, law, invalid, ior_int, ior_ext, weight=None, reflect=False,
                   detach=None, sm=None):
    """dict(loss, g_env float64 [Eh, Ew, C] w.r.t. a float64 copy of the float32 texels, g_R float64 [3, 3] w.r.t. the nine entries as
    independent inputs, sm (``samples``), fwd (``loss_forward``))."""
    if sm is None:
        sm = samples(faces, V, camera_M, height, width, screen, texture, s, law, ior_int, ior_ext, reflect)
    E = torch.as_tensor(np.asarray(env, dtype=np.float32)).to(F64).clone().requires_grad_(True)
    Rt = torch.as_tensor(np.asarray(R, dtype=np.float64)).clone().requires_grad_(True)
    fwd = loss_forward(sm, E, Rt, s, invalid, detach)
    loss = image_loss_ref.loss_of(fwd["mean"], target, weight)
    gE, gR = torch.autograd.grad(loss, (E, Rt), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    return dict(loss=float(loss.detach()), g_env=z(gE, E).numpy(), g_R=z(gR, Rt).numpy(), sm=sm, fwd=fwd,
                image=fwd["mean"].detach().to(torch.float32).view(height, width, -1).numpy())
