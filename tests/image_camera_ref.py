"""Float64 restatement of the photometric loss of the refracted image as a function of the CAMERA -- the tensors Rinv (camera -> world,
its top 3 x 4) and Kinv [3, 3] -- differentiable in both by torch autograd (Scene.image_loss_fused with camera_param;
drt_amd/csrc/drt_image_camera.h; test only).

It is ``image_loss_ref.forward`` with the rays made differentiable: ``sample_rays`` restates ``image_ref.sample_rays`` on tensor
``Rinv`` / ``Kinv`` in the same operation order (the square root with the value of ``image_ref._sqrt`` and the derivative of
``torch.sqrt``, as ``image_loss_ref._guarded_sqrt`` has it); the classes and the face tape come from ``snell_ref.trace`` on the DETACHED
rays; the path (``ior_ref.interact``), the Fresnel factor (``image_loss_ref.interaction_factor``), the plane and the bilinear sample
(``image_ref.screen_uv`` / ``image_ref.bilinear``), the pixel mean and the loss (``image_loss_ref.loss_of``) are the existing
restatements, which are differentiable in the rays.  A sample's class, the tape, the TIR flags, the entering branch, ``floor``, the clamp
of the cell and the on-screen test carry no gradient, as in torch.  Three switches make the tests' negative controls."""
import functools

import numpy as np
import torch

import image_cases
import image_loss_cases
import image_loss_ref
import image_ref
import ior_ref
import snell_ref
from conftest import IOR

F64 = torch.float64
EXT = image_cases.EXT


def camera_tensors(camera_M):
    """(Rinv [4, 4], Kinv [3, 3]) float64 tensors of a camera_M 4-tuple."""
    return torch.tensor(np.asarray(camera_M[2], np.float64)), torch.tensor(np.asarray(camera_M[3], np.float64))


def sample_rays(Kinv, Rinv, height, width, s):
    """image_ref.sample_rays on tensors autograd may track: (origin, dir) float64 [height * width * s * s, 3]."""
    K, R = Kinv, Rinv
    y, x, b, a = torch.meshgrid(torch.arange(height, dtype=F64), torch.arange(width, dtype=F64), torch.arange(s, dtype=F64),
                                torch.arange(s, dtype=F64), indexing="ij")
    px = ((x + (a + 0.5) / float(s)) - 0.5).reshape(-1)
    py = ((y + (b + 0.5) / float(s)) - 0.5).reshape(-1)
    p = [(K[r, 0] * px + K[r, 1] * py) + K[r, 2] for r in range(3)]
    w = [(R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2] for r in range(3)]
    len2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    length = torch.sqrt(len2)
    length = length + (image_ref._sqrt(len2) - length).detach()
    d = torch.stack([w[0] / length, w[1] / length, w[2] / length], dim=1)
    o = R[:3, 3].view(1, 3).expand_as(d)
    return o, d


def forward(faces, V, Rinv, Kinv, height, width, screen, texture, s, law, fresnel, void, invalid, ior_int=IOR, ior_ext=EXT, detach_direct=False,
            detach_origin=False, detach_T=False):
    """dict(mean float64 [H * W, C], cls, on, u, v, through_on) -- image_loss_ref.forward with tensor Rinv / Kinv and a constant mesh.
    ``detach_direct``: the colours of the direct samples are detached (a pass over the through samples alone); ``detach_origin``: no
    gradient passes the ray origin, only the direction carries one; ``detach_T``: the throughput is detached (geometry only)."""
    max_bounces, tir, refraction = law
    V = torch.as_tensor(np.asarray(V), dtype=F64)
    o, d = sample_rays(Kinv, Rinv, height, width, s)
    if detach_origin:
        o = o.detach()
    P = o.shape[0]
    tex = np.asarray(texture)
    tex = tex[:, :, None] if tex.ndim == 2 else tex
    C = tex.shape[2]
    if len(faces) == 0:
        cls = torch.zeros(P, dtype=torch.long)
        out_o, out_d, T = o, d, torch.ones(P, dtype=F64)
    else:
        aux = snell_ref.trace(faces, V, o.detach().contiguous(), d.detach(), ior_int, ior_ext, max_bounces, tir, refraction)
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
                Tv = Tv.index_put((sel,), Tv[sel] * image_loss_ref.interaction_factor(po[sel], pd[sel], tri, ior_int, ior_ext))
            no, nd, _ = ior_ref.interact(po[sel], pd[sel], tri, ior_int, ior_ext, refraction)
            po = po.index_put((sel,), no)
            pd = pd.index_put((sel,), nd)
        out_o, out_d = o.index_put((vi,), po), d.index_put((vi,), pd)
        T = torch.ones(P, dtype=F64).index_put((vi,), Tv)
    if detach_T:
        T = T.detach()
    on, u, v, _, _ = image_ref.screen_uv(screen.p0, screen.eu, screen.ev, tex.shape[0], tex.shape[1], out_o, out_d)
    on = on & (cls != image_ref.INVALID)
    col = torch.as_tensor(np.broadcast_to(np.asarray(void, np.float64), (C,)).copy()).view(1, C).repeat(P, 1)
    idx = torch.nonzero(on).squeeze(1)
    lit = T[idx].view(-1, 1) * image_ref.bilinear(tex, u[idx], v[idx])
    if detach_direct:
        lit = torch.where((cls[idx] == image_ref.DIRECT).view(-1, 1), lit.detach(), lit)
    col = col.index_put((idx,), lit)
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    return dict(mean=acc / float(s2), cls=cls, on=on, u=u, v=v, through_on=int((on & (cls == image_ref.THROUGH)).sum()))


def margin(fwd, tex_h, tex_w):
    """The smallest distance, in texels, of a gradient-carrying sample (direct ones included) from a texel line or a screen border."""
    sel = fwd["on"].numpy()
    best = np.inf
    for w, top in ((fwd["u"].detach().numpy()[sel], tex_w - 1), (fwd["v"].detach().numpy()[sel], tex_h - 1)):
        best = min(best, np.abs(w - np.rint(w)).min(), w.min(), (top - w).min())
    return float(best)


def loss_and_grads(faces, V, camera_M, height, width, screen, texture, target, s, law, fresnel, void, invalid, ior_int=IOR, ior_ext=EXT, weight=None,
                   **controls):
    """dict(loss, g_rinv [3, 4], g_kinv [3, 3], on: gradient-carrying samples, through_on, margin, fwd) at the camera ``camera_M``."""
    Rinv, Kinv = (m.requires_grad_(True) for m in camera_tensors(camera_M))
    fwd = forward(faces, V, Rinv, Kinv, height, width, screen, texture, s, law, fresnel, void, invalid, ior_int, ior_ext, **controls)
    loss = image_loss_ref.loss_of(fwd["mean"], target, weight)
    gR, gK = torch.autograd.grad(loss, (Rinv, Kinv), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    tex_h, tex_w = np.asarray(texture).shape[:2]
    return dict(loss=float(loss.detach()), g_rinv=z(gR, Rinv).numpy()[:3].copy(), g_kinv=z(gK, Kinv).numpy(), on=int(fwd["on"].sum()),
                through_on=fwd["through_on"], margin=margin(fwd, tex_h, tex_w), fwd=fwd)


def groups(g_rinv, g_kinv):
    """The three groups the 21 partials are compared in -- they differ by orders of magnitude: rinv[:, :3], rinv[:, 3], kinv."""
    g_rinv, g_kinv = np.asarray(g_rinv, np.float64), np.asarray(g_kinv, np.float64)
    return {"rinv[:, :3]": g_rinv[:3, :3], "rinv[:, 3]": g_rinv[:3, 3], "kinv": g_kinv}


# ---- the cases of the host and GPU tests ---------------------------------------------------------------------------------------------------
SCENES = ("v5", "wide")
LAWS = image_loss_cases.LAWS


@functools.lru_cache(maxsize=None)
def reference(name, law, fresnel, control=None):
    """loss_and_grads of a case at the fixture's own camera with image_loss_cases.target; ``control``: one of detach_direct,
    detach_origin, detach_T, or None.  Computed once per process and never modified."""
    sc = image_cases.scene(name)
    return loss_and_grads(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], sc["texture"],
                          image_loss_cases.target(name, law, fresnel), sc["s"], law, fresnel, sc["void"], sc["invalid"], **({control: True} if control else {}))


# ---- the camera fit (drt_amd.calibrate.fit_camera) -------------------------------------------------------------------------------------------
FIT_VIEW, FIT_RES, FIT_S, FIT_LAW, FIT_TEX = 5, 32, 2, image_loss_cases.LAWS[2], 64
FIT_STEPS, FIT_LR = 150, 0.02
# The start: along the camera's x, and about the view axis.  Half of the half pixel and 0.3 degrees first planned for this fit: from that
# start the restatement's own fit did not converge (pose error 0.5227 -> 0.3948 pixels, loss 16.55 -> 7.35 in 150 steps) -- at 32 x 32
# the loss of a camera moved by a fraction of a pixel is mostly samples that change class at the silhouette, which carry no gradient --
# so the displacement was halved, where it does.
FIT_SIDEWAYS_PIXELS, FIT_ROLL_DEGREES = 0.25, 0.15


def start_six(camera_M, centre, extent):
    """The six numbers of calibrate.camera_pose that displace ``camera_M`` by FIT_SIDEWAYS_PIXELS and FIT_ROLL_DEGREES."""
    f = float(np.asarray(camera_M[1])[0, 0])
    rinv = np.asarray(camera_M[2], np.float64)
    z = float((np.asarray(centre) - rinv[:3, 3]) @ rinv[:3, 2])
    return np.array([FIT_SIDEWAYS_PIXELS, 0.0, 0.0, 0.0, 0.0, np.radians(FIT_ROLL_DEGREES) * f * extent / z])


@functools.lru_cache(maxsize=None)
def fit_case():
    """The hand from view 5 at 32 x 32, s = 2, (6, reflect, snell) with Fresnel, in front of image_screen_ref's smooth 64 x 64 texture; the
    photograph is rendered by this restatement at the true camera; the start camera is off by FIT_SIDEWAYS_PIXELS sideways and
    FIT_ROLL_DEGREES about the view axis: dict(true / start: camera_M 4-tuples, photo float32 [H, W, 3], texture, screen, void, invalid,
    centre, extent, mesh)."""
    import image_screen_ref
    from drt_amd import calibrate, render
    centre, extent = image_cases.frame()
    mesh = image_cases.hand()
    true = image_cases.camera(FIT_VIEW, FIT_RES, FIT_RES)
    screen = render.Screen.behind(true, centre, extent, FIT_TEX, FIT_TEX, span=image_cases.SPAN)
    tex = image_screen_ref.smooth_texture(FIT_TEX, FIT_TEX)
    void, invalid = 0.25, 0.75
    Rinv, Kinv = camera_tensors(true)
    fwd = forward(mesh.faces, mesh.vertices, Rinv, Kinv, FIT_RES, FIT_RES, screen, tex, FIT_S, FIT_LAW, True, void, invalid)
    photo = np.ascontiguousarray(fwd["mean"].to(torch.float32).view(FIT_RES, FIT_RES, 3).numpy())
    rinv, kinv = (m.numpy() for m in calibrate.camera_pose(true, torch.tensor(start_six(true, centre, extent)), centre, extent))
    start = (np.linalg.inv(rinv), np.asarray(true[1], np.float64), rinv, kinv)
    return dict(true=true, start=start, photo=photo, texture=tex, screen=screen, void=void, invalid=invalid, centre=centre, extent=extent, mesh=mesh)


def project(camera_M, point):
    """Pixel coordinates (x, y) of a world point: K (R point)."""
    q = np.asarray(camera_M[0], np.float64) @ np.append(np.asarray(point, np.float64), 1.0)
    p = np.asarray(camera_M[1], np.float64) @ q[:3]
    return p[:2] / p[2]


def pose_error(camera_M, true, centre, extent):
    """The larger projected displacement, in pixels, of the object's centre and of a point one extent to its side (along the true
    camera's x axis) between ``camera_M`` and ``true``."""
    side = np.asarray(centre) + extent * np.asarray(true[2], np.float64)[:3, 0]
    return float(max(np.linalg.norm(project(camera_M, p) - project(true, p)) for p in (np.asarray(centre), side)))


def fit_on_the_restatement(steps=FIT_STEPS, lr=FIT_LR):
    """calibrate.fit_camera's loop over this restatement's loss of fit_case(), re-traced at every step (classes and tape follow the
    camera).  Returns (fitted camera_M, loss history).  Regenerates CPU_FIT below: python -c "import image_camera_ref as m;
    print(m.measure_fit())" from tests/ (a quarter of a minute)."""
    from drt_amd import calibrate
    case = fit_case()
    mesh = case["mesh"]

    def loss_of(six):
        Rinv, Kinv = calibrate.camera_pose(case["start"], six, case["centre"], case["extent"])
        fwd = forward(mesh.faces, mesh.vertices, Rinv, Kinv, FIT_RES, FIT_RES, case["screen"], case["texture"], FIT_S, FIT_LAW, True, case["void"], case["invalid"])
        return image_loss_ref.loss_of(fwd["mean"], case["photo"])

    six, history = calibrate._adam_from_zero(loss_of, steps, lr)
    rinv, kinv = (m.numpy() for m in calibrate.camera_pose(case["start"], six, case["centre"], case["extent"]))
    return (np.linalg.inv(rinv), np.asarray(case["start"][1]), rinv, kinv), history


def measure_fit():
    """dict(start_error, error, first ten losses, smallest loss): what CPU_FIT records."""
    case = fit_case()
    fitted, history = fit_on_the_restatement()
    return dict(start_error=pose_error(case["start"], case["true"], case["centre"], case["extent"]),
                error=pose_error(fitted, case["true"], case["centre"], case["extent"]), first=history[:10], best=min(history))


# measure_fit() as run once on the CPU (the whole fit re-traces 150 times): the pose errors in pixels, the first ten losses of the
# history and the smallest loss seen -- the loss falls by 0.548 decades, the pose error by 0.735
CPU_FIT = dict(start_error=0.26143283656261423, error=0.04814295120913581, best=2.9795411030163286,
               first=[10.534742497360515, 9.653087556467852, 9.781854927435239, 9.431417869529373, 10.430510270955558, 10.313047495755344,
                      10.554040808004757, 10.459541912343736, 10.273417161454244, 9.593810023448867])
