"""Float64 restatement of the K-interaction path law that is differentiable in the indices of refraction (Scene.paths_ray_loss_ior_fused,
drt_amd.calibrate; test only).

tests/snell_ref.py with ONE function restated: ``_frame`` builds eta_i / eta_t as ``ones_like(t) * ior`` where snell_ref's takes
``full_like(t, ior)`` (floats only), so an IOR may be a tensor that autograd tracks -- 0-dim, or one element per row, which is how
``loss_and_grads`` obtains the contribution of every single path.  Everything else is snell_ref's / paths_ref's / the oracle's own:
``snell_ref.trace`` (face ids from the oracle's tracer, float IORs), ``moller_trumbore``, ``fresnel_tir``, ``refract_dir`` /
``refract_dir_snell``, ``paths_ref._reflect``, ``oracle.ray_loss``.  The TIR flag and the entering / leaving branch carry no gradient,
as in torch."""
import torch

import paths_ref
import snell_ref
from oracle import diffrender_oracle as orc
from oracle.diffrender_oracle import _dot, fresnel_tir, moller_trumbore


def _frame(o, d, tri, ior_int, ior_ext):
    """snell_ref._frame with tensor IORs (0-dim or one per row): (t, flipped normal, wo, eta, tir flag)."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = _dot(wo, n).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    ii, ie = torch.ones_like(t) * ior_int, torch.ones_like(t) * ior_ext
    eta_i = torch.where(leaving, ii, ie)
    eta_t = torch.where(leaving, ie, ii)
    return t, n * sgn.view(-1, 1), wo, eta_i / eta_t, fresnel_tir(cos_i * sgn, eta_i, eta_t)


def refract_only(o, d, tri, ior_int, ior_ext, refraction="snell"):
    """The refract continuation of every row whatever its TIR flag says, differentiable in the IORs too: (new_o, wt, tir)."""
    t, n, wo, eta, tir = _frame(o, d, tri, ior_int, ior_ext)
    wt = snell_ref._refract(refraction)(wo, n, eta)
    return (o + t.view(-1, 1) * d) + 1e-5 * wt, wt, tir


def interact(o, d, tri, ior_int, ior_ext, refraction="reference"):
    """One interaction of every row: (new_o, new_d, tir).  Rows with the TIR flag continue mirrored (no IOR enters there)."""
    t, n, wo, eta, tir = _frame(o, d, tri, ior_int, ior_ext)
    wt = snell_ref._refract(refraction)(wo, n, eta)
    to = (o + t.view(-1, 1) * d) + 1e-5 * wt
    ro, wr = paths_ref._reflect(o, d, t, n)
    sel = tir.view(-1, 1)
    return torch.where(sel, ro, to), torch.where(sel, wr, wt), tir


def _value(ior):
    return float(ior.detach().reshape(-1)[0]) if isinstance(ior, torch.Tensor) else float(ior)


def render_paths(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction="reference", aux=None):
    """snell_ref.render_paths, differentiable in V, the rays AND the IORs: floats, 0-dim tensors, or tensors with one element per
    VALID path (in the order of ``nonzero(aux["valid"])``).  The tape is traced with the IORs' values."""
    if aux is None:
        aux = snell_ref.trace(faces, V, origin, ray_dir, _value(ior_int), _value(ior_ext), max_bounces, tir, refraction)
    F = torch.as_tensor(faces, dtype=torch.long)
    vi = torch.nonzero(aux["valid"]).squeeze(1)
    o, d = origin[vi], ray_dir[vi]
    n_hits = aux["hits"][vi]

    def rows(ior, sel):
        return ior[sel] if isinstance(ior, torch.Tensor) and ior.dim() > 0 else ior

    for k in range(max_bounces):
        sel = torch.nonzero(n_hits > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, flag = interact(o[sel], d[sel], V[F[aux["tape"][k, vi[sel]]]], rows(ior_int, sel), rows(ior_ext, sel), refraction)
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


def loss_and_grads(faces, V, origin, ray_dir, screen_pixel, valid, ior_int, ior_ext, max_bounces, tir, refraction="reference", aux=None,
                   want_vertices=False):
    """ray_loss of one view and its IOR partials by autograd, with a completed path's tape held fixed.  Every valid path is given its
    own pair of IOR leaves, so the gradient w.r.t. them is the list of per-path contributions.  dict(loss, g_int, g_ext: the sums;
    abs_int, abs_ext: the sums of the absolute per-path contributions -- what a tolerance on the sums is relative to; per_int, per_ext,
    rows: the contributions and the ray index of each; count: contributing rays; grad_V with ``want_vertices``; aux)."""
    ior_int, ior_ext = float(ior_int), float(ior_ext)
    if aux is None:
        aux = snell_ref.trace(faces, V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction)
    n = int(aux["valid"].sum())
    ii = torch.full((n,), ior_int, dtype=torch.float64, requires_grad=True)
    ie = torch.full((n,), ior_ext, dtype=torch.float64, requires_grad=True)
    Vt = V.detach().clone().requires_grad_(want_vertices)
    out_ori, out_dir, mask, _ = render_paths(faces, Vt, origin, ray_dir, ii, ie, max_bounces, tir, refraction, aux)
    loss = orc.ray_loss(out_ori, out_dir, mask, screen_pixel, valid)
    grads = torch.autograd.grad(loss, (ii, ie) + ((Vt,) if want_vertices else ()))
    rows = torch.nonzero(aux["valid"]).squeeze(1)
    return dict(loss=float(loss.detach()), g_int=float(grads[0].sum()), g_ext=float(grads[1].sum()), abs_int=float(grads[0].abs().sum()),
                abs_ext=float(grads[1].abs().sum()), per_int=grads[0].numpy(), per_ext=grads[1].numpy(), rows=rows.numpy(),
                count=int((aux["valid"] & valid).sum()), grad_V=grads[2].numpy() if want_vertices else None, aux=aux)


# ---------------------------------------------------------------------------------------------------- the fit on the CPU
class RefScene:
    """A stand-in for ``Scene`` with the one method ``drt_amd.calibrate.fit_ior`` calls, on this restatement: the CPU measurement the
    GPU fit's bounds come from (``python tests/ior_ref.py``)."""

    def __init__(self, mesh):
        self.faces, self.V = mesh.faces, torch.tensor(mesh.vertices, dtype=torch.float64)
        self.last_path_count = 0

    def paths_ray_loss_ior_fused(self, origin, ray_dir, screen_pixel, valid, ior_int, ior_ext=None, max_bounces=4, tir="reflect",
                                 refraction="reference", vertices=True):
        ior_ext = orc.EXT_IOR if ior_ext is None else ior_ext
        out_ori, out_dir, mask, aux = render_paths(self.faces, self.V, origin, ray_dir, ior_int, ior_ext, max_bounces, tir, refraction)
        self.last_path_count = int((aux["valid"] & valid).sum())
        return orc.ray_loss(out_ori, out_dir, mask, screen_pixel, valid)


class RefCapture:
    """Views of a 72-view turntable at res x res whose targets are traced on the mesh itself under ``law`` at ``ior``:
    screen_pixel = out_ori + 50 out_dir on the rays whose path completes."""

    def __init__(self, mesh, res, view_ids, law, ior, ior_ext=orc.EXT_IOR):
        from drt_amd import views
        center, extent = views.mesh_frame(mesh.vertices)
        cams = views.turntable_cameras(center, extent, 72, res, res)
        V = torch.tensor(mesh.vertices, dtype=torch.float64)
        self._views = {}
        for v in view_ids:
            R, K, Rinv, Kinv = cams[v]
            o, d = views.generate_ray(res, res, Kinv, Rinv)
            aux = snell_ref.trace(mesh.faces, V, o, d, ior, ior_ext, law[0], law[1], law[2])
            self._views[v] = (aux["out_ori"] + 50.0 * aux["out_dir"], aux["valid"].clone(), None, o, d, None)
        self._ids = list(view_ids)

    def get_view(self, v):
        return self._views[v]

    def ray_view_ids(self):
        return self._ids


if __name__ == "__main__":
    # the CPU figures of DESIGN.md 7.4: end error of the bisection per law, hand_vh at 64 x 64, views (5, 23, 41, 59), IOR 1.4723
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from drt_amd import calibrate, mesh_io
    mesh = mesh_io.read_ply(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "hand_vh.ply"))
    for law in [(2, "drop", "snell"), (6, "reflect", "snell"), (6, "reflect", "reference")]:
        t0 = time.time()
        fit = calibrate.fit_ior(RefScene(mesh), RefCapture(mesh, 64, (5, 23, 41, 59), law, 1.4723), law, (1.3, 1.7), 14)
        print(law, "fitted", fit["ior"], "error", fit["ior"] - 1.4723, "bracket", fit["bracket"], "seconds", round(time.time() - t0, 1), flush=True)
