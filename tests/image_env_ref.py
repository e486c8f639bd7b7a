"""Float64 restatement of the environment law (Scene.render_image with ``environment``; drt_amd/csrc/drt_image_env.h; test only).

Builds on ``image_ref``: sample rays, paths, classes and throughputs are that module's, unchanged -- the paths do not know what they will
look at.  The outer-surface reflection is ``paths_ref._reflect`` on the first interaction of ``oracle.intersect_ids``, with this package's
``image_ref.fresnel_R``, and one more ``intersect_ids`` for the occlusion verdict.  The lookup is written out as the law states it, with
elementwise torch operations in the stated association; ``torch.acos`` and
``torch.atan2`` are the two calls that are not correctly rounded on either side, so u and v agree with the header to the bound
``UV_ULPS`` below and everything computed from the SAME (u, v) agrees bit for bit."""
import math

import numpy as np
import torch

import image_loss_ref
import image_ref
import ior_ref
import paths_ref
import snell_ref
from oracle import diffrender_oracle as orc
from oracle.diffrender_oracle import _cross, _dot, fresnel_tir, moller_trumbore

F64 = torch.float64
FILL, SCREEN, ENV = 0, 1, 2          # where a sample's colour comes from (drt_image_env.h kImageBg*)
# |u_header - u_restatement| <= Ew * 2^-50 (v: Eh): phi (theta) is within 1 ulp(pi) = 2^-51 of the true value on each side (glibc's and
# SLEEF's stated bounds for acos / atan2 on identical inputs), so the two differ by at most 2^-50, times Ew / (2 pi) < Ew * 2^-52.6; the
# four roundings that follow (quotient, sum, product, difference; values at most Ew) add at most 4 * Ew * 2^-53 = Ew * 2^-51.
UV_ULPS = 2.0 ** -50


def rotation():
    """Rx(0.3) Ry(0.7): no row or column of it can be swapped unnoticed."""
    cx, sx, cy, sy = math.cos(0.3), math.sin(0.3), math.cos(0.7), math.sin(0.7)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def env_dir(R, d):
    R = torch.as_tensor(np.asarray(R), dtype=F64)
    return [(R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1]) + R[r, 2] * d[:, 2] for r in range(3)]


def env_uv(R, d, eh, ew):
    """(u, v, e_y): texel coordinates before the clamp of v, and the direction's height in the environment frame."""
    ex, ey, ez = env_dir(R, d)
    theta = torch.acos(ey.clamp(-1, 1))
    phi = torch.atan2(ex, -ez)
    u = ((phi / (2.0 * math.pi)) + 0.5) * float(ew) - 0.5
    v = (theta / math.pi) * float(eh) - 0.5
    return u, v, ey


def env_bilinear(env, u, v):
    """float64 [P, C]: v clamped to [0, Eh - 1], y0 = min(floor(v), Eh - 2), x0 = floor(u) with wrapped columns, image_bilinear's formula."""
    tex = torch.as_tensor(np.asarray(env), dtype=torch.float32)
    eh, ew = tex.shape[:2]
    vc = v.clamp(0, eh - 1)
    y0 = torch.floor(vc).clamp(max=eh - 2)
    x0 = torch.floor(u).clamp(-1, ew - 1)
    fx, fy = (u - x0).view(-1, 1), (vc - y0).view(-1, 1)
    yi, xa, xb = y0.detach().long(), (x0.detach().long() + ew) % ew, (x0.detach().long() + 1) % ew
    t00, t01, t10, t11 = (tex[yi, xa].to(F64), tex[yi, xb].to(F64), tex[yi + 1, xa].to(F64), tex[yi + 1, xb].to(F64))
    return ((t00 * (1 - fx) + t01 * fx) * (1 - fy)) + ((t10 * (1 - fx) + t11 * fx) * fy)


def lookup(env, R, d):
    """E(d) float64 [P, C]."""
    u, v, _ = env_uv(R, d, env.shape[0], env.shape[1])
    return env_bilinear(env, u, v)


def background(screen, texture, env, R, o, d):
    """The unweighted background of rays (o, d): dict(B float64 [P, C], on bool [P] (the screen caught the ray), u / v / ey of the
    environment lookup of every row, and su / sv / t / dn of image_ref.screen_uv when a screen is given)."""
    env = np.asarray(env)
    out = {}
    on = torch.zeros(len(o), dtype=torch.bool)
    u, v, ey = env_uv(R, d, env.shape[0], env.shape[1])
    B = env_bilinear(env, u, v)
    if screen is not None:
        tex = np.asarray(texture)
        on, su, sv, t, dn = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], o, d)
        idx = torch.nonzero(on).squeeze(1)
        B = B.index_put((idx,), image_ref.bilinear(tex, su[idx], sv[idx]))
        out.update(su=su, sv=sv, t=t, dn=dn)
    out.update(B=B, on=on, u=u, v=v, ey=ey)
    return out


def reflection(faces, V, o, d, ior_int, ior_ext):
    """The outer-surface reflection of camera rays (o, d): dict(face int64 [P] (-1: no interaction), qual bool [P] (the first interaction
    enters the object and has no TIR flag), ro / wr float64 [P, 3] and R1 [P] (zeros elsewhere), seen bool [P] (qual, and the any-hit
    query of the float32 cast of (ro, wr) found nothing)).  Both refraction laws give the same values: the first Bounce's t, n, ci and
    flags are bounce_forward's under either."""
    V = torch.as_tensor(np.asarray(V), dtype=F64)
    P = len(o)
    out = dict(face=torch.full((P,), -1, dtype=torch.long), qual=torch.zeros(P, dtype=torch.bool), ro=torch.zeros((P, 3), dtype=F64),
               wr=torch.zeros((P, 3), dtype=F64), R1=torch.zeros(P, dtype=F64), seen=torch.zeros(P, dtype=torch.bool))
    if len(faces) == 0:
        return out
    mesh = orc.Mesh(faces, V)
    ids, hitted = orc.intersect_ids(mesh, o, d)
    hi = torch.nonzero(hitted).squeeze(1)
    out["face"][hi] = ids[hi]
    tri = V[torch.as_tensor(np.asarray(faces), dtype=torch.long)[ids[hi]]]
    _, _, t, _ = moller_trumbore(o[hi], d[hi], tri)
    # the unit normal with the law's own root, (m_x^2 + m_y^2) + m_z^2 under a correctly rounded sqrt (image_ref._sqrt): torch's vector
    # norm, which moller_trumbore divides by, may be one unit in the last place off, and ro, wr, R1 are held to the header bit for bit
    m = _cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n = m / image_ref._sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).view(-1, 1)
    wo = -d[hi]
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, torch.full_like(t, ior_int), torch.full_like(t, ior_ext))
    eta_t = torch.where(leaving, torch.full_like(t, ior_ext), torch.full_like(t, ior_int))
    tir = fresnel_tir(cos_i * sgn, eta_i, eta_t)
    nf = n * sgn.view(-1, 1)
    ci = _dot(nf, wo)
    q = torch.logical_not(leaving) & torch.logical_not(tir)
    ro, wr = paths_ref._reflect(o[hi], d[hi], t, nf)
    qi = hi[q]
    out["qual"][qi] = True
    out["ro"][qi], out["wr"][qi] = ro[q], wr[q]
    out["R1"][qi] = image_ref.fresnel_R(ci[q], ior_ext, ior_int)
    _, blocked = orc.intersect_ids(mesh, ro[q], wr[q])
    out["seen"][qi] = torch.logical_not(blocked)
    return out


def sample_colours(screen, texture, env, R, cls, o, d, T, invalid):
    """dict(col float64 [P, C], src int64 [P] in FILL / SCREEN / ENV, u / v / ey of the environment lookup (of every row; meaningful where
    src == ENV), and the screen stage on / su / sv / t / dn of image_ref.screen_uv when a screen is given)."""
    env = np.asarray(env)
    C = env.shape[2]
    P = len(o)
    out = {}
    on = torch.zeros(P, dtype=torch.bool)
    if screen is not None:
        tex = np.asarray(texture)
        on, su, sv, t, dn = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], o, d)
        on = on & (cls != image_ref.INVALID)
        out.update(on=on, su=su, sv=sv, t=t, dn=dn)
    u, v, ey = env_uv(R, d, env.shape[0], env.shape[1])
    col = T.view(-1, 1) * env_bilinear(env, u, v)
    if screen is not None:
        idx = torch.nonzero(on).squeeze(1)
        col[idx] = T[idx].view(-1, 1) * image_ref.bilinear(tex, su[idx], sv[idx])
    bad = cls == image_ref.INVALID
    col[bad] = torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy())
    src = torch.where(bad, FILL, torch.where(on, SCREEN, ENV))
    out.update(col=col, src=src, u=u, v=v, ey=ey)
    return out


def render_from(stage, height, width, s, screen, texture, env, R, invalid, refl=None):
    """The image of per-sample results of ``image_ref.render`` (``stage``: its dict; classes, exit rays and throughputs are taken from it,
    they do not depend on the background): dict(image float32 [H, W, C], hit / through as they are, and sample_colours' dict).  ``refl``
    (``reflection``'s dict): c = T B(exit) + R1 B(ro, wr) on the through samples whose reflection was seen; then also added bool [P], the
    plane reflect float32 [H, W] and rb, ``background``'s dict of the reflected rays (all rows; meaningful where added)."""
    st = sample_colours(screen, texture, env, R, stage["cls"], stage["out_ori"], stage["out_dir"], stage["T"], invalid)
    if refl is not None:
        added = refl["seen"] & (stage["cls"] == image_ref.THROUGH)
        rb = background(screen, texture, env, R, refl["ro"], refl["wr"])
        ai = torch.nonzero(added).squeeze(1)
        st["col"][ai] = st["col"][ai] + refl["R1"][ai].view(-1, 1) * rb["B"][ai]
        s2 = s * s
        st.update(added=added, rb=rb, reflect=(added.view(-1, s2).sum(1).to(F64) / float(s2)).to(torch.float32).view(height, width))
    st.update(image=image_ref.pixel_mean(st["col"], s).view(height, width, -1), hit=stage["hit"], through=stage["through"], cls=stage["cls"])
    return st


# ---- the photometric loss, differentiable in the vertices and the two IORs by autograd ---------------------------------------------------
def loss_forward(faces, V, camera_M, height, width, screen, texture, env, R, s, law, invalid, ior_int, ior_ext, reflect=False, detach=None):
    """image_loss_ref.forward (Fresnel on) in front of an environment: dict(mean float64 [H * W, C], cls, T, bg (``background`` of the exit
    rays), through: the number of through samples, and with ``reflect`` added bool [P] and rb (``background`` of the reflected rays of
    the added rows, in their order)).  The path is image_loss_ref's, statement for statement (``snell_ref.trace`` for classes and tape,
    ``ior_ref.interact`` and ``image_loss_ref.interaction_factor`` on it); the reflection is recomputed from V on the faces and verdicts of
    ``reflection``.  ``detach``: "reflection" / "lookup" cut that term's gradient -- NOT the derivative of the law (negative controls)."""
    max_bounces, tir, refraction = law
    V = torch.as_tensor(np.asarray(V) if not isinstance(V, torch.Tensor) else V, dtype=F64)
    vi_int, vi_ext = ior_ref._value(ior_int), ior_ref._value(ior_ext)
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    P = o.shape[0]
    C = np.asarray(env).shape[2]
    F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    if len(faces) == 0:
        cls = torch.zeros(P, dtype=torch.long)
        out_o, out_d, T = o, d, torch.ones(P, dtype=F64)
        tape, hits = torch.full((max_bounces, P), -1, dtype=torch.long), torch.zeros(P, dtype=torch.long)
    else:
        aux = snell_ref.trace(faces, V.detach(), o, d, vi_int, vi_ext, max_bounces, tir, refraction)
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
    bg = background(screen, texture, env, R, out_o, out_d)
    B = bg["B"]
    if detach == "lookup":
        B = torch.where(bg["on"].view(-1, 1), B, B.detach())
    col = T.view(-1, 1) * B
    out = dict(cls=cls, T=T, bg=bg, through=int((cls == image_ref.THROUGH).sum()), tape=tape, hits=hits, seen=torch.zeros(P, dtype=torch.bool))
    if reflect and len(faces):
        r0 = reflection(faces, V.detach(), o, d, vi_int, vi_ext)
        added = r0["seen"] & (cls == image_ref.THROUGH)
        ai = torch.nonzero(added).squeeze(1)
        tri = V[F[r0["face"][ai]]]
        _, _, t, _ = moller_trumbore(o[ai], d[ai], tri)
        m = _cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n = m / torch.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).view(-1, 1)      # (entering: the normal is not flipped)
        ci = _dot(n, -d[ai])
        ro, wr = paths_ref._reflect(o[ai], d[ai], t, n)
        R1 = image_loss_ref.fresnel_R(ci, torch.ones_like(ci) * ior_ext, torch.ones_like(ci) * ior_int)
        rb = background(screen, texture, env, R, ro, wr)
        Br = torch.where(rb["on"].view(-1, 1), rb["B"], rb["B"].detach()) if detach == "lookup" else rb["B"]
        term = R1.view(-1, 1) * Br
        col = col.index_put((ai,), col[ai] + (term.detach() if detach == "reflection" else term))
        out.update(added=added, rb=rb, seen=r0["seen"])
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    out["mean"] = acc / float(s2)
    return out


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, env, R, target, s, law, invalid, ior_int, ior_ext, weight=None, reflect=False,
                   detach=None):
    """dict(loss, grad_V [nv, 3], g_int, g_ext, count (every through sample), image float32 [H, W, C], fwd)."""
    Vt = torch.as_tensor(np.asarray(V), dtype=F64).clone().requires_grad_(True)
    ii = torch.tensor(float(ior_int), dtype=F64, requires_grad=True)
    ie = torch.tensor(float(ior_ext), dtype=F64, requires_grad=True)
    fwd = loss_forward(faces, Vt, camera_M, height, width, screen, texture, env, R, s, law, invalid, ii, ie, reflect, detach)
    loss = image_loss_ref.loss_of(fwd["mean"], target, weight)
    gV, gi, ge = torch.autograd.grad(loss, (Vt, ii, ie), allow_unused=True) if loss.requires_grad else (None, None, None)
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    C = fwd["mean"].shape[1]
    return dict(loss=float(loss.detach()), grad_V=z(gV, Vt).numpy(), g_int=float(z(gi, ii)), g_ext=float(z(ge, ie)), count=fwd["through"],
                image=fwd["mean"].detach().to(torch.float32).view(height, width, C).numpy(), fwd=fwd)
