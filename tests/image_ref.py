"""Float64 restatement of the forward renderer's law (Scene.render_image; drt_amd/csrc/drt_image.h; test only).

Sample rays by the law's formula with elementwise operations (no matmul: every product and sum is one rounding, in the stated
association).  Paths come from ``snell_ref.trace`` (``paths_ref.trace`` under the reference refraction), so the face ids are the oracle
tracer's; the throughput is recomputed along the completed paths from the face tape with this module's own ``fresnel_R``.  Plane,
bilinear sample and pixel mean are written out as the law states them."""
import numpy as np
import torch

import snell_ref
from oracle.diffrender_oracle import _dot, fresnel_tir, moller_trumbore

F64 = torch.float64
DIRECT, THROUGH, INVALID = 0, 1, 2


def _sqrt(x):
    """Correctly rounded square root (numpy's: the hardware instruction).  torch.sqrt's vectorised float64 path may be one unit in the
    last place off, which the bit-for-bit comparisons of this law cannot take."""
    return torch.from_numpy(np.sqrt(x.detach().numpy()))


def sample_rays(Kinv, Rinv, height, width, s):
    """(origin, dir) float64 [height * width * s * s, 3]: pixel-major, sample-minor, sample j = b * s + a."""
    K, R = torch.as_tensor(np.asarray(Kinv), dtype=F64), torch.as_tensor(np.asarray(Rinv), dtype=F64)
    y, x, b, a = torch.meshgrid(torch.arange(height, dtype=F64), torch.arange(width, dtype=F64), torch.arange(s, dtype=F64),
                                torch.arange(s, dtype=F64), indexing="ij")
    px = ((x + (a + 0.5) / float(s)) - 0.5).reshape(-1)
    py = ((y + (b + 0.5) / float(s)) - 0.5).reshape(-1)
    p = [(K[r, 0] * px + K[r, 1] * py) + K[r, 2] for r in range(3)]
    w = [(R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2] for r in range(3)]
    length = _sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    d = torch.stack([w[0] / length, w[1] / length, w[2] / length], dim=1)
    o = R[:3, 3].view(1, 3).expand_as(d).contiguous()
    return o, d


def fresnel_R(ci, eta_i, eta_t):
    """The reference's FrDielectric (DiffRender.py:51-61), its R."""
    ci, eta_i, eta_t = (torch.as_tensor(v, dtype=F64) for v in (ci, eta_i, eta_t))
    sin_i = _sqrt((1 - ci * ci).clamp(0, 1))
    sin_t = sin_i * eta_i / eta_t
    cos_t = _sqrt((1 - sin_t * sin_t).clamp(min=0))
    r_parl = ((eta_t * ci) - (eta_i * cos_t)) / ((eta_t * ci) + (eta_i * cos_t))
    r_perp = ((eta_i * ci) - (eta_t * cos_t)) / ((eta_i * ci) + (eta_t * cos_t))
    return (r_parl * r_parl + r_perp * r_perp) / 2


def interaction_factor(o, d, tri, ior_int, ior_ext):
    """What one interaction of every row puts on the throughput: 1 - R with cos(theta_i) from the flipped normal and the eta_i, eta_t
    refract_ray assigns; 1 on rows whose TIR flag is set."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, torch.full_like(t, ior_int), torch.full_like(t, ior_ext))
    eta_t = torch.where(leaving, torch.full_like(t, ior_ext), torch.full_like(t, ior_int))
    tir = fresnel_tir(cos_i * sgn, eta_i, eta_t)
    ci = _dot(n * sgn.view(-1, 1), wo)
    return torch.where(tir, torch.ones_like(t), 1 - fresnel_R(ci, eta_i, eta_t))


def trace_samples(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction, fresnel):
    """dict(cls int64 [P], hit bool [P], out_ori / out_dir [P,3] (the camera ray on direct rows), T [P])."""
    V = torch.as_tensor(np.asarray(V), dtype=F64)
    P = origin.shape[0]
    if len(faces) == 0:
        return dict(cls=torch.zeros(P, dtype=torch.long), hit=torch.zeros(P, dtype=torch.bool), out_ori=origin.clone(), out_dir=ray_dir.clone(),
                    T=torch.ones(P, dtype=F64))
    aux = snell_ref.trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction)
    hit = aux["tape"][0] >= 0
    valid = aux["valid"]
    cls = torch.where(hit, torch.where(valid, THROUGH, INVALID), DIRECT)
    sel3 = valid.view(-1, 1)
    out_ori, out_dir = torch.where(sel3, aux["out_ori"], origin), torch.where(sel3, aux["out_dir"], ray_dir)
    T = torch.ones(P, dtype=F64)
    if fresnel:
        F = torch.as_tensor(np.asarray(faces), dtype=torch.long)
        vi = torch.nonzero(valid).squeeze(1)
        o, d, n_hits, Tv = origin[vi], ray_dir[vi], aux["hits"][vi], torch.ones(len(vi), dtype=F64)
        for k in range(max_bounces):
            sel = torch.nonzero(n_hits > k).squeeze(1)
            if len(sel) == 0:
                break
            tri = V[F[aux["tape"][k, vi[sel]]]]
            Tv[sel] = Tv[sel] * interaction_factor(o[sel], d[sel], tri, ior_int, ior_ext)
            no, nd, _ = snell_ref.interact(o[sel], d[sel], tri, ior_int, ior_ext, refraction)
            o = o.index_put((sel,), no)
            d = d.index_put((sel,), nd)
        assert len(vi) == 0 or max((o - aux["out_ori"][vi]).abs().max(), (d - aux["out_dir"][vi]).abs().max()) <= 1e-9      # the traced path
        T[vi] = Tv
    return dict(cls=cls, hit=hit, out_ori=out_ori, out_dir=out_dir, T=T)


def screen_uv(p0, eu, ev, tex_h, tex_w, o, d):
    """(on bool [P], u, v, t, dn) of exit rays on the screen plane; u, v are only meaningful where ``seen``; on = seen and inside."""
    p0, eu, ev = (torch.as_tensor(np.asarray(a), dtype=F64).view(1, 3).expand_as(o) for a in (p0, eu, ev))
    n = torch.stack([eu[:, 1] * ev[:, 2] - eu[:, 2] * ev[:, 1], eu[:, 2] * ev[:, 0] - eu[:, 0] * ev[:, 2], eu[:, 0] * ev[:, 1] - eu[:, 1] * ev[:, 0]], dim=1)
    dn = _dot(d, n)
    t = _dot(p0 - o, n) / dn
    seen = (dn != 0) & (t > 0)
    q = o + t.view(-1, 1) * d
    r = q - p0
    u = _dot(r, eu) / _dot(eu, eu)
    v = _dot(r, ev) / _dot(ev, ev)
    on = seen & (u >= 0) & (u <= tex_w - 1) & (v >= 0) & (v <= tex_h - 1)
    return on, u, v, t, dn


def bilinear(texture, u, v):
    """float64 [P, C]: the visual hull's bilinear formula on rows inside the texture."""
    tex = torch.as_tensor(np.asarray(texture), dtype=torch.float32)
    tex_h, tex_w = tex.shape[:2]
    x0 = torch.floor(u).clamp(max=tex_w - 2)
    y0 = torch.floor(v).clamp(max=tex_h - 2)
    fx, fy = (u - x0).view(-1, 1), (v - y0).view(-1, 1)
    xi, yi = x0.long(), y0.long()
    t00, t01, t10, t11 = (tex[yi + dy, xi + dx].to(F64) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    return ((t00 * (1 - fx) + t01 * fx) * (1 - fy)) + ((t10 * (1 - fx) + t11 * fx) * fy)


def sample_colours(screen, texture, cls, o, d, T, void, invalid):
    """(colour float64 [P, C], on bool [P], u, v, t, dn)."""
    tex = np.asarray(texture)
    tex = tex[:, :, None] if tex.ndim == 2 else tex
    C = tex.shape[2]
    on, u, v, t, dn = screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], o, d)
    on = on & (cls != INVALID)
    col = torch.as_tensor(np.broadcast_to(np.asarray(void, np.float64), (C,)).copy()).view(1, C).repeat(len(o), 1)
    idx = torch.nonzero(on).squeeze(1)
    col[idx] = T[idx].view(-1, 1) * bilinear(tex, u[idx], v[idx])
    col[cls == INVALID] = torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy())
    return col, on, u, v, t, dn


def pixel_mean(col, s):
    """float32 [n_pix, C]: (((c_0 + c_1) + c_2) + ...) / s^2 in float64, stored as float32."""
    s2 = s * s
    c = col.view(-1, s2, col.shape[1])
    acc = c[:, 0].clone()
    for j in range(1, s2):
        acc = acc + c[:, j]
    return (acc / float(s2)).to(torch.float32)


def render(faces, V, camera_M, height, width, screen, texture, s=1, max_bounces=2, tir="drop", refraction="reference", fresnel=True, void=0.0,
           invalid=0.0, ior_int=1.5, ior_ext=1.00029):
    """The whole law: dict(image float32 [H, W, C], hit / through float32 [H, W], and the per-sample stage: cls, on, u, v, t, dn, T)."""
    o, d = sample_rays(camera_M[3], camera_M[2], height, width, s)
    tr = trace_samples(faces, V, o, d, ior_int, ior_ext, max_bounces, tir, refraction, fresnel)
    col, on, u, v, t, dn = sample_colours(screen, texture, tr["cls"], tr["out_ori"], tr["out_dir"], tr["T"], void, invalid)
    s2 = s * s
    share = lambda flag: (flag.view(-1, s2).sum(1).to(F64) / float(s2)).to(torch.float32).view(height, width)      # noqa: E731
    return dict(image=pixel_mean(col, s).view(height, width, -1), hit=share(tr["hit"]), through=share(tr["cls"] == THROUGH), cls=tr["cls"], on=on,
                u=u, v=v, t=t, dn=dn, T=tr["T"], out_ori=tr["out_ori"], out_dir=tr["out_dir"])
