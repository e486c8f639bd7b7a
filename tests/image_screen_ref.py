"""Float64 restatement of the photometric loss of the refracted image as a function of the END of the light path -- the screen's pose
(rows p0, eu, ev) and the texture -- differentiable in both by torch autograd (Scene.image_loss_fused with screen_param / texture_param;
drt_amd/csrc/drt_image_screen.h; test only).

Built from what the other restatements state: ``image_ref.sample_rays`` and ``image_ref.trace_samples`` give every sample's class, its
ray -- the camera ray of a direct sample, the exit ray of a through one -- and its throughput T.  A fixed mesh and fixed IORs make these
CONSTANTS of the screen and the texture, so they are computed once per scene, detached.  After them ``screen_uv`` and ``bilinear`` are
restated with a tensor pose and a tensor texture in the operation order of ``image_ref``; the colours, the pixel mean and the loss are
``image_loss_ref.forward``'s tail and ``image_loss_ref.loss_of``.  The class of a sample, the on-screen test, ``floor`` and the clamp of
the cell carry no gradient, as in torch."""
import functools

import numpy as np
import torch

import image_cases
import image_loss_cases
import image_loss_ref
import image_ref
from conftest import IOR
from oracle.diffrender_oracle import _dot

F64 = torch.float64
EXT = image_cases.EXT


def rows_of(screen):
    """float64 [3, 3]: p0, eu, ev of a render.Screen."""
    return torch.tensor(np.stack([screen.p0, screen.eu, screen.ev]), dtype=F64)


def shifted(screen, du, dv):
    """rows_of(screen) moved by (du, dv) texels within its plane."""
    P = rows_of(screen)
    return torch.stack([P[0] + du * P[1] + dv * P[2], P[1], P[2]])


def trace(faces, V, camera_M, height, width, s, law, fresnel, ior_int=IOR, ior_ext=EXT):
    """The constants of a view: dict(cls, o, d, T) per sample, detached."""
    o, d = image_ref.sample_rays(camera_M[3], camera_M[2], height, width, s)
    tr = image_ref.trace_samples(faces, V, o, d, ior_int, ior_ext, law[0], law[1], law[2], fresnel)
    return dict(cls=tr["cls"], o=tr["out_ori"].detach(), d=tr["out_dir"].detach(), T=tr["T"].detach())


@functools.lru_cache(maxsize=None)
def constants(name, law, fresnel):
    """trace() of a scene of tests/image_cases.py at conftest.IOR; shared, never modified."""
    sc = image_cases.scene(name)
    return trace(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["s"], law, fresnel)


def screen_uv(P, tex_h, tex_w, o, d):
    """image_ref.screen_uv with the tensor pose P [3, 3]: (on, u, v)."""
    p0, eu, ev = (P[k].view(1, 3).expand_as(o) for k in range(3))
    n = torch.stack([eu[:, 1] * ev[:, 2] - eu[:, 2] * ev[:, 1], eu[:, 2] * ev[:, 0] - eu[:, 0] * ev[:, 2], eu[:, 0] * ev[:, 1] - eu[:, 1] * ev[:, 0]], dim=1)
    dn = _dot(d, n)
    t = _dot(p0 - o, n) / dn
    seen = (dn != 0) & (t > 0)
    q = o + t.view(-1, 1) * d
    r = q - p0
    u = _dot(r, eu) / _dot(eu, eu)
    v = _dot(r, ev) / _dot(ev, ev)
    on = seen & (u >= 0) & (u <= tex_w - 1) & (v >= 0) & (v <= tex_h - 1)
    return on, u, v


def bilinear(tex, u, v):
    """image_ref.bilinear with the float64 tensor texture [Th, Tw, C] (the values of the float32 texels)."""
    tex_h, tex_w = tex.shape[:2]
    x0 = torch.floor(u).clamp(max=tex_w - 2).detach()
    y0 = torch.floor(v).clamp(max=tex_h - 2).detach()
    fx, fy = (u - x0).view(-1, 1), (v - y0).view(-1, 1)
    xi, yi = x0.long(), y0.long()
    t00, t01, t10, t11 = (tex[yi + dy, xi + dx] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    return ((t00 * (1 - fx) + t01 * fx) * (1 - fy)) + ((t10 * (1 - fx) + t11 * fx) * fy)


def forward(const, P, tex, s, void, invalid, detach_direct=False):
    """dict(mean float64 [n_pix, C], on, u, v): image_loss_ref.forward's tail on the constants of a view.  ``detach_direct``: the colours
    of the direct samples are detached -- what a pass over the through samples alone would differentiate (the tests' negative control)."""
    cls, o, d, T = const["cls"], const["o"], const["d"], const["T"]
    P_n, C = len(cls), tex.shape[2]
    on, u, v = screen_uv(P, tex.shape[0], tex.shape[1], o, d)
    on = on & (cls != image_ref.INVALID)
    col = torch.as_tensor(np.broadcast_to(np.asarray(void, np.float64), (C,)).copy()).view(1, C).repeat(P_n, 1)
    idx = torch.nonzero(on).squeeze(1)
    lit = T[idx].view(-1, 1) * bilinear(tex, u[idx], v[idx])
    if detach_direct:
        lit = torch.where((cls[idx] == image_ref.DIRECT).view(-1, 1), lit.detach(), lit)
    col = col.index_put((idx,), lit)
    col = torch.where((cls == image_ref.INVALID).view(-1, 1), torch.as_tensor(np.broadcast_to(np.asarray(invalid, np.float64), (C,)).copy()).view(1, C), col)
    s2 = s * s
    c = col.view(-1, s2, C)
    acc = c[:, 0]
    for j in range(1, s2):
        acc = acc + c[:, j]
    return dict(mean=acc / float(s2), on=on, u=u, v=v)


def margin(fwd, tex_h, tex_w):
    """The smallest distance, in texels, of a gradient-carrying sample (direct ones included) from a texel line or a screen border."""
    sel = fwd["on"].numpy()
    best = np.inf
    for w, top in ((fwd["u"].detach().numpy()[sel], tex_w - 1), (fwd["v"].detach().numpy()[sel], tex_h - 1)):
        best = min(best, np.abs(w - np.rint(w)).min(), w.min(), (top - w).min())
    return float(best)


def loss_and_grads(const, P, texture, target, s, void, invalid, weight=None, detach_direct=False):
    """dict(loss, g_screen [3, 3], g_texture [Th, Tw, C], on: gradient-carrying samples, margin, fwd) at the pose P (rows p0, eu, ev) and
    the float32 texture."""
    tex32 = np.asarray(texture, np.float32)
    tex32 = tex32[:, :, None] if tex32.ndim == 2 else tex32
    Pt = torch.as_tensor(np.asarray(P), dtype=F64).clone().requires_grad_(True)
    tex = torch.tensor(tex32).to(F64).requires_grad_(True)
    fwd = forward(const, Pt, tex, s, void, invalid, detach_direct)
    loss = image_loss_ref.loss_of(fwd["mean"], target, weight)
    gP, gT = torch.autograd.grad(loss, (Pt, tex), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    return dict(loss=float(loss.detach()), g_screen=z(gP, Pt).numpy(), g_texture=z(gT, tex).numpy(), on=int(fwd["on"].sum()),
                margin=margin(fwd, tex32.shape[0], tex32.shape[1]), fwd=fwd)


# ---- the cases of the host and GPU tests ---------------------------------------------------------------------------------------------------
SCENES = ("v5", "wide")
LAWS = image_loss_cases.LAWS


def pose(name):
    """float64 [3, 3]: the pose a case is evaluated at -- the fixture's own screen.  Every gradient-carrying sample of every case, direct
    ones included, keeps TEXEL_MARGIN from the texel lines and the borders there (tests/test_image_screen_host.py checks it: the smallest
    margin is 8.9e-5 texels), so no case needs its screen shifted; one that did would be moved with ``shifted``, never thinned out."""
    return rows_of(image_cases.scene(name)["screen"])


@functools.lru_cache(maxsize=None)
def reference(name, law, fresnel, detach_direct=False):
    """loss_and_grads of a case with image_loss_cases.target; computed once per process and never modified."""
    sc = image_cases.scene(name)
    return loss_and_grads(constants(name, law, fresnel), pose(name), sc["texture"], image_loss_cases.target(name, law, fresnel), sc["s"], sc["void"],
                          sc["invalid"], detach_direct=detach_direct)


# ---- the pose fit (drt_amd.calibrate.fit_screen) -------------------------------------------------------------------------------------------
FIT_VIEWS, FIT_RES, FIT_S, FIT_LAW, FIT_TEX = (3, 5, 7), 32, 2, image_loss_cases.LAWS[2], 64
FIT_STEPS, FIT_LR = 150, 0.02
FIT_OFFSET_TEXELS, FIT_TWIST_DEGREES = 0.5, 0.5      # the start pose: along eu, and about the screen's normal through its centre


def smooth_texture(tex_h, tex_w):
    """float32 [tex_h, tex_w, 3]: a low-frequency pattern, one and a half to two periods across the screen per channel."""
    y, x = np.meshgrid(np.arange(tex_h) / tex_h, np.arange(tex_w) / tex_w, indexing="ij")
    two_pi = 2.0 * np.pi
    return np.stack([0.5 + 0.4 * np.sin(two_pi * 2.0 * x) * np.cos(two_pi * 1.5 * y), 0.5 + 0.4 * np.cos(two_pi * 1.5 * x + 1.0) * np.sin(two_pi * 2.0 * y),
                     0.5 + 0.4 * np.sin(two_pi * (x + y))], axis=2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_case():
    """Three views of the hand around view 5 in front of ONE screen (behind view 5) with a smooth texture, photographs rendered by this
    restatement at the true pose, and a start pose off by FIT_OFFSET_TEXELS of the pitch along eu and FIT_TWIST_DEGREES about the normal:
    dict(cams, consts, photos float32 [H, W, 3], texture, true / start: render.Screen, void, invalid)."""
    from drt_amd import calibrate, render
    center, extent = image_cases.frame()
    mesh = image_cases.hand()
    cams = [image_cases.camera(v, FIT_RES, FIT_RES) for v in FIT_VIEWS]
    true = render.Screen.behind(cams[1], center, extent, FIT_TEX, FIT_TEX, span=image_cases.SPAN)
    tex = smooth_texture(FIT_TEX, FIT_TEX)
    void, invalid = 0.25, 0.75
    consts = [trace(mesh.faces, mesh.vertices, cam, FIT_RES, FIT_RES, FIT_S, FIT_LAW, True) for cam in cams]
    tex64 = torch.tensor(tex).to(F64)
    photos = [np.ascontiguousarray(forward(c, rows_of(true), tex64, FIT_S, void, invalid)["mean"].to(torch.float32).view(FIT_RES, FIT_RES, 3).numpy())
              for c in consts]
    normal = np.cross(true.eu, true.ev)
    half = (FIT_TEX - 1) / 2.0
    six = np.concatenate([FIT_OFFSET_TEXELS * true.eu / np.linalg.norm(true.eu),
                          np.radians(FIT_TWIST_DEGREES) * normal / np.linalg.norm(normal) * np.sqrt(2.0 * half * half)])
    rows = calibrate.screen_pose(true, FIT_TEX, FIT_TEX, torch.tensor(six, dtype=F64)).numpy()
    return dict(cams=cams, consts=consts, photos=photos, texture=tex, true=true, start=render.Screen(rows[0], rows[1], rows[2]), void=void, invalid=invalid)


def corner_error(screen, true, tex_h, tex_w):
    """The largest distance of a corner of ``screen`` from the same corner of ``true``, in texel pitches of ``true``."""
    def corners(sc):
        return np.stack([sc.p0 + a * (tex_w - 1) * sc.eu + b * (tex_h - 1) * sc.ev for a in (0, 1) for b in (0, 1)])
    return float(np.linalg.norm(corners(screen) - corners(true), axis=1).max() / np.linalg.norm(true.eu))


def fit_on_the_restatement(steps=FIT_STEPS, lr=FIT_LR):
    """calibrate.fit_pose -- fit_screen's optimiser -- over this restatement's loss of fit_case(): exit rays are constants of a fixed mesh,
    so the screen stage alone is the whole dependence.  Returns (fitted render.Screen, loss history)."""
    from drt_amd import calibrate, render
    case = fit_case()
    tex64 = torch.tensor(case["texture"]).to(F64)

    def loss_of(rows):
        total = None
        for const, photo in zip(case["consts"], case["photos"]):
            term = image_loss_ref.loss_of(forward(const, rows, tex64, FIT_S, case["void"], case["invalid"])["mean"], photo)
            total = term if total is None else total + term
        return total

    six, history = calibrate.fit_pose(loss_of, case["start"], FIT_TEX, FIT_TEX, steps, lr)
    rows = calibrate.screen_pose(case["start"], FIT_TEX, FIT_TEX, six).numpy()
    return render.Screen(rows[0], rows[1], rows[2]), history
