"""Calibration of a capture: fit the interior index of refraction of a FIXED mesh.

    python -m drt_amd.calibrate --name horse --max-bounces 6 --tir reflect --refraction snell --bracket 1.3 1.7

A capture comes with a nominal IOR, not a known one.  ``fit_ior`` finds the IOR at which the refraction loss of the given mesh against
the capture's targets is smallest, under any K-interaction law -- Snell's included -- from the exact derivative d loss / d IOR of
``Scene.paths_ray_loss_ior_fused(..., vertices=False)`` summed over the refraction views.  The loss as a function of the IOR is only
piecewise smooth (paths change face and validity), so a fixed-step optimiser rings around the minimum; the SIGN of the summed
derivative is right well away from it, and the fit bisects a bracket on that sign.

``fit_screen`` fits the POSE of the textured screen behind the object -- placed by hand, calibrated separately -- to plain photographs:
a rigid motion of the initial screen under the photometric loss of ``Scene.image_loss_fused(..., screen_param=)``,
mesh and IORs fixed.  ``fit_camera`` does the same for the POSE of the camera of one photograph -- a rotation about the camera's own
centre and a translation of the calibrated camera -- through ``Scene.image_loss_fused(..., camera_param=)``.
``fit_absorption`` fits the Beer-Lambert absorption coefficients of the glass through ``Scene.image_loss_fused(..., absorption=)``
(DESIGN.md 10.7).  None of the three has a command line.
"""
from __future__ import annotations

import argparse
import json
import os

import torch

from . import optim


def _law(path_law):
    """(K, tir, refraction) by the rules of ``optim.path_law_keyword``; (2, "drop") under the reference formula -- no law to the loops
    -- is a law here: the IOR is fitted under today's formula."""
    law = optim.path_law_keyword(path_law, {}, "fit_ior")
    if law is None:
        return (2, "drop", "reference")
    return law if len(law) > 2 else (law[0], law[1], "reference")


def evaluate_views(scene, data, ior, law, view_ids, ior_ext=None):
    """(loss, d loss / d ior, contributing rays) summed over ``view_ids`` at the interior IOR ``ior``, as Python numbers."""
    x = torch.tensor(float(ior), dtype=torch.float64, requires_grad=True)
    total, rays = None, []
    for v in view_ids:
        screen_pixel, valid, _, origin, ray_dir, _ = data.get_view(v)
        loss = scene.paths_ray_loss_ior_fused(origin, ray_dir, screen_pixel, valid, x, ior_ext, *law, vertices=False)
        total = loss if total is None else total + loss
        rays.append(scene.last_path_count)
    if total is None:
        raise ValueError("fit_ior: no views to evaluate")
    g, = torch.autograd.grad(total, x)
    return float(total.detach()), float(g), int(sum(int(r) for r in rays))


def fit_ior(scene, data, path_law=(2, "drop", "snell"), bracket=(1.2, 1.8), halvings=14, view_ids=None, ior_ext=None):
    """The interior IOR of the fixed mesh of ``scene`` against the capture ``data``: bisection of ``bracket`` on the sign of
    d loss / d IOR, the refraction loss of ``path_law`` summed over ``view_ids`` (default: ``data.ray_view_ids()``).
    Returns dict(ior: the middle of the final bracket, bracket: the final one, evaluations, history: [(ior, loss, derivative,
    contributing rays)] per evaluation).  The bracket must hold a minimum -- derivative negative at its lower end, positive at its
    upper end -- else RuntimeError."""
    law = _law(path_law)
    lo, hi = (float(b) for b in bracket)
    if not (0.0 < lo < hi):
        raise ValueError(f"bracket must be (lo, hi) with 0 < lo < hi, got {bracket!r}")
    if isinstance(halvings, bool) or int(halvings) != halvings or int(halvings) < 0:
        raise ValueError(f"halvings must be a non-negative integer, got {halvings!r}")
    ids = list(data.ray_view_ids() if view_ids is None else view_ids)
    history = []

    def derivative(x):
        loss, g, rays = evaluate_views(scene, data, x, law, ids, ior_ext)
        history.append((x, loss, g, rays))
        return g

    g_lo, g_hi = derivative(lo), derivative(hi)
    if not (g_lo < 0.0 < g_hi):
        raise RuntimeError(f"fit_ior: the bracket ({lo}, {hi}) does not hold a minimum of the loss: d loss / d IOR is {g_lo:.6g} at its lower "
                           f"end and {g_hi:.6g} at its upper end (wanted: negative, positive)")
    for _ in range(int(halvings)):
        mid = 0.5 * (lo + hi)
        if derivative(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return {"ior": 0.5 * (lo + hi), "bracket": (lo, hi), "evaluations": len(history), "history": history}


def screen_pose(screen, tex_h, tex_w, six):
    """float64 [3, 3], rows p0, eu, ev: ``screen`` (a ``render.Screen`` under a texture of ``tex_h`` x ``tex_w`` texels) moved rigidly by
    the six numbers ``six`` (a float64 tensor; differentiable): rotated about its centre by the rotation vector ``six[3:] / h`` and then
    translated by ``pitch * six[:3]``, with pitch = |eu| and h = the half diagonal of the screen in texels -- so that one unit of any of
    the six moves a corner of the screen by about one texel.  The pitch is untouched and the axes stay orthogonal: both are rotated by
    the same orthogonal matrix (the matrix exponential of the rotation vector's cross-product matrix)."""
    p0, eu, ev = (torch.as_tensor(a, dtype=torch.float64) for a in (screen.p0, screen.eu, screen.ev))
    half_u, half_v = (tex_w - 1) / 2.0, (tex_h - 1) / 2.0
    centre = p0 + eu * half_u + ev * half_v
    w = six[3:] / float((half_u * half_u + half_v * half_v) ** 0.5)
    zero = torch.zeros((), dtype=torch.float64)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    R = torch.linalg.matrix_exp(K)
    shift = six[:3] * float(torch.linalg.norm(eu))
    return torch.stack([centre + R @ (p0 - centre) + shift, R @ eu, R @ ev])


def _adam_from_zero(loss_of_six, steps, lr, n=6):
    """Adam with step ``lr`` on six numbers (``n`` of them) from zero over ``loss_of_six(six)`` (six: a float64 tensor that requires grad;
    returns a scalar tensor).  Returns (the numbers of the smallest loss seen, the loss history: one float per step, evaluated BEFORE that
    step's update)."""
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"steps must be a positive integer, got {steps!r}")
    if not (float(lr) > 0.0):
        raise ValueError(f"lr must be positive, got {lr!r}")
    six = torch.zeros(int(n), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([six], lr=float(lr))
    history, best = [], (None, None)
    for _ in range(int(steps)):
        opt.zero_grad()
        loss = loss_of_six(six)
        value = float(loss.detach())
        if best[0] is None or value < best[0]:
            best = (value, six.detach().clone())
        history.append(value)
        loss.backward()
        opt.step()
    return best[1], history


def fit_pose(loss_of, screen, tex_h, tex_w, steps, lr):
    """The optimiser of ``fit_screen`` over any ``loss_of(rows)`` (rows: ``screen_pose``'s tensor, which requires grad; returns a scalar
    tensor): Adam with step ``lr`` (in texels, see ``screen_pose``) on the six numbers from zero.  Returns (the six numbers of the smallest
    loss seen, the loss history: one float per step, evaluated BEFORE that step's update)."""
    return _adam_from_zero(lambda six: loss_of(screen_pose(screen, tex_h, tex_w, six)), steps, lr)


def fit_screen(scene, views, screen, texture, *, steps, lr, **law):
    """The pose of the screen behind the fixed mesh of ``scene`` from photographs: a rigid motion of the initial ``screen`` (a
    ``render.Screen``; ``screen_pose`` builds the pose from six numbers in torch) that minimises the photometric loss summed over
    ``views`` = [(camera_M, photograph[, weight]), ...] -- ``Scene.image_loss_fused(camera_M, H, W, None, texture, photograph,
    screen_param=pose, vertices=False, **law)`` with H, W the photograph's.  The kernel hands back the nine partials of the pose; the
    chain from them to the six numbers is torch autograd.  ``steps`` Adam steps of ``lr`` texels.  ``law``: the law, IOR and band
    keywords of ``image_loss_fused``.  Returns (the fitted ``Screen``: the pose of the smallest loss seen, the loss history)."""
    from . import render
    if not isinstance(screen, render.Screen):
        raise ValueError(f"screen must be a drt_amd.render.Screen, got {type(screen).__name__}")
    views = [tuple(v) for v in views]
    if not views or any(len(v) not in (2, 3) for v in views):
        raise ValueError("views must be a non-empty list of (camera_M, photograph) or (camera_M, photograph, weight)")
    for bad in ("screen_param", "texture_param", "vertices", "want_image"):
        if bad in law:
            raise ValueError(f"fit_screen sets {bad} itself")
    tex = render.check_texture(texture)
    tex_h, tex_w = int(tex.shape[0]), int(tex.shape[1])

    def loss_of(rows):
        total = None
        for v in views:
            photo = v[1]
            term = scene.image_loss_fused(v[0], int(photo.shape[0]), int(photo.shape[1]), None, tex, photo, weight=v[2] if len(v) == 3 else None,
                                          vertices=False, screen_param=rows, **law)
            term = term.to(rows.device)
            total = term if total is None else total + term
        return total

    six, history = fit_pose(loss_of, screen, tex_h, tex_w, steps, lr)
    rows = screen_pose(screen, tex_h, tex_w, six).numpy()
    return render.Screen(rows[0], rows[1], rows[2]), history


def fit_absorption(scene, views, screen, texture, *, steps, lr, **law):
    """The absorption coefficients of the glass of ``scene`` (mesh and IOR fixed) from photographs: C numbers ``sigma >= 0`` per unit of
    mesh length that minimise the photometric loss summed over ``views`` = [(camera_M, photograph[, weight]), ...] --
    ``Scene.image_loss_fused(camera_M, H, W, screen, texture, photograph, absorption=sigma, vertices=False, **law)`` with H, W the
    photograph's; the resolve kernel hands back the C partials, no path is recomputed.  ``steps`` Adam steps of ``lr`` (in units of sigma)
    from 0, each followed by the projection onto ``sigma >= 0``.  ``law``: the law, IOR and band keywords of ``image_loss_fused``.  Returns (sigma float64 numpy [C]: that of the smallest loss seen, the loss history: one float
    per step, evaluated BEFORE that step's update)."""
    from . import render
    if not isinstance(screen, render.Screen):
        raise ValueError(f"screen must be a drt_amd.render.Screen, got {type(screen).__name__}")
    views = [tuple(v) for v in views]
    if not views or any(len(v) not in (2, 3) for v in views):
        raise ValueError("views must be a non-empty list of (camera_M, photograph) or (camera_M, photograph, weight)")
    for bad in ("absorption", "screen_param", "texture_param", "camera_param", "vertices", "want_image"):
        if bad in law:
            raise ValueError(f"fit_absorption sets {bad} itself")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"steps must be a positive integer, got {steps!r}")
    if not (float(lr) > 0.0):
        raise ValueError(f"lr must be positive, got {lr!r}")
    tex = render.check_texture(texture)
    sigma = torch.zeros(int(tex.shape[2]), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([sigma], lr=float(lr))
    history, best = [], (None, None)
    for _ in range(int(steps)):
        opt.zero_grad()
        total = None
        for v in views:
            photo = v[1]
            term = scene.image_loss_fused(v[0], int(photo.shape[0]), int(photo.shape[1]), screen, tex, photo, weight=v[2] if len(v) == 3 else None,
                                          vertices=False, absorption=sigma, **law).to(sigma.device)
            total = term if total is None else total + term
        value = float(total.detach())
        if best[0] is None or value < best[0]:
            best = (value, sigma.detach().clone())
        history.append(value)
        total.backward()
        opt.step()
        with torch.no_grad():
            sigma.clamp_(min=0.0)
    return best[1].numpy(), history


def environment_pose(environment, three):
    """float64 [3, 3] -- an ``env_rotation_param`` -- of ``environment`` (a ``render.Environment`` with rotation R0) turned by the three
    numbers ``three`` (a float64 tensor; differentiable): ``R = expm(hat(three * 2 pi / Ew)) @ R0``, a rotation of the environment FRAME
    by the rotation vector ``three`` in units of one texel's angle at the equator -- so that one unit of any of the three moves the
    panorama by about one texel there (``three[1]``, about the frame's y axis, is a yaw: it moves u of every direction by exactly that
    many texels, towards smaller u), and zero, which gives R0 itself, is no special point.  The matrix exponential of a skew matrix is orthogonal, so R
    keeps R0's orthonormality to rounding -- which the call's check needs to 1e-12, and which ``torch.linalg.matrix_exp`` does not give:
    around 0.05 rad, half a texel of a 64-column map, its result was measured 8.6e-12 off orthonormal.  So the exponential is taken here,
    by its Taylor series to degree 14 of K / 32 (remainder below 1e-25 for turns of up to four radians) and five squarings: torch
    float64 throughout, no branch on the angle, measured at most 9e-15 off orthonormal from 1e-9 to 40 texels."""
    import math
    R0 = torch.as_tensor(environment.rotation, dtype=torch.float64)
    w = three * (2.0 * math.pi / float(environment.texels.shape[1]))
    zero = torch.zeros((), dtype=torch.float64)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])]) / 32.0
    eye = torch.eye(3, dtype=torch.float64)
    E = eye
    for k in range(14, 0, -1):          # Horner: I + K (I + K / 2 (I + K / 3 (...)))
        E = eye + (K @ E) / float(k)
    for _ in range(5):
        E = E @ E
    return E @ R0


def fit_environment(scene, views, environment, screen=None, texture=None, *, steps, lr, reflection=False, **law):
    """The rotation of the environment around the fixed mesh of ``scene`` from photographs: a turn of the initial ``environment`` (a
    ``render.Environment``; ``environment_pose`` builds the rotation from three numbers in torch) that minimises the photometric loss summed
    over ``views`` = [(camera_M, photograph[, weight]), ...] -- ``Scene.image_loss_fused(camera_M, H, W, screen, texture, photograph,
    environment=environment, env_rotation_param=R, reflection=reflection, vertices=False, **law)`` with H, W the photograph's; ``screen``
    and ``texture`` may both be None.  The kernel hands back the nine partials of the rotation; the chain from them to the three numbers
    is torch autograd.  ``steps`` Adam steps of ``lr`` texels (``fit_screen``'s loop).  The texels are not fitted.  ``law``: the law, IOR
    and band keywords of ``image_loss_fused``.  Returns (the ``Environment`` of the smallest loss seen, the loss history)."""
    from . import render
    if not isinstance(environment, render.Environment):
        raise ValueError(f"environment must be a drt_amd.render.Environment, got {type(environment).__name__}")
    views = [tuple(v) for v in views]
    if not views or any(len(v) not in (2, 3) for v in views):
        raise ValueError("views must be a non-empty list of (camera_M, photograph) or (camera_M, photograph, weight)")
    for bad in ("environment", "env_texels_param", "env_rotation_param", "absorption", "screen_param", "texture_param", "camera_param", "vertices", "want_image"):
        if bad in law:
            raise ValueError(f"fit_environment sets {bad} itself")

    def loss_of(three):
        R = environment_pose(environment, three)
        total = None
        for v in views:
            photo = v[1]
            term = scene.image_loss_fused(v[0], int(photo.shape[0]), int(photo.shape[1]), screen, texture, photo, weight=v[2] if len(v) == 3 else None,
                                          vertices=False, environment=environment, reflection=reflection, env_rotation_param=R, **law).to(three.device)
            total = term if total is None else total + term
        return total

    three, history = _adam_from_zero(loss_of, steps, lr, 3)
    return render.Environment(environment.texels, environment_pose(environment, three).numpy()), history


def camera_pose(camera_M, six, centre=None, extent=1.0):
    """(Rinv float64 [4, 4], Kinv float64 [3, 3]) -- a ``camera_param`` -- of ``camera_M`` = (R, K, R^-1, K^-1) moved rigidly by the six
    numbers ``six`` (a float64 tensor; differentiable): turned about its OWN centre by the rotation vector ``six[3:]`` (in the camera's
    axes, by the matrix exponential of its cross-product matrix) and moved by the translation ``six[:3]`` (in the camera's axes of the
    input camera).  Both are scaled to pixels with the object's ``centre`` (default: the world origin) at depth z along the view axis,
    its ``extent`` e and the focal length f = K[0, 0]: a unit of ``six[0]``, ``six[1]`` (z / f along the image axes) or ``six[3]``,
    ``six[4]`` (1 / f radians about them) moves the image of the centre by about one pixel; the two motions along and about the view axis
    leave the image of a centre on that axis where it is, so a unit of ``six[2]`` (z^2 / (f e)) or ``six[5]`` (z / (f e) radians) moves the
    image of a point one extent to the centre's side by about one pixel.  ``Kinv`` passes through untouched; zero gives the camera
    itself."""
    import numpy as np
    rinv0 = torch.as_tensor(np.asarray(camera_M[2], dtype=np.float64))
    kinv = torch.as_tensor(np.asarray(camera_M[3], dtype=np.float64))
    f = float(np.asarray(camera_M[1], dtype=np.float64)[0, 0])
    axes, position = rinv0[:3, :3], rinv0[:3, 3]
    c = torch.zeros(3, dtype=torch.float64) if centre is None else torch.as_tensor(np.asarray(centre, dtype=np.float64))
    z = float(torch.dot(c - position, axes[:, 2]))
    e = float(extent)
    if not (f > 0.0 and z > 0.0 and e > 0.0):
        raise ValueError(f"camera_pose: focal length {f!r}, depth of the centre {z!r} and extent {e!r} must be positive")
    shift = six[:3] * torch.tensor([z / f, z / f, z * z / (f * e)], dtype=torch.float64)
    w = six[3:] * torch.tensor([1.0 / f, 1.0 / f, z / (f * e)], dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    top = torch.cat([axes @ torch.linalg.matrix_exp(K), (position + axes @ shift).view(3, 1)], dim=1)
    return torch.cat([top, rinv0[3:4, :]]), kinv


def fit_camera(scene, camera_M, photograph, screen, texture, *, weight=None, steps, lr, **law):
    """The pose of the camera of one ``photograph`` of the fixed mesh of ``scene`` in front of ``screen`` (a ``render.Screen``) and
    ``texture``: the rigid motion of the calibrated ``camera_M`` (``camera_pose`` builds ``(Rinv, Kinv)`` from six numbers in torch, scaled
    with ``views.mesh_frame`` of the scene's mesh) that minimises ``Scene.image_loss_fused(None, H, W, screen, texture, photograph,
    weight=weight, camera_param=pose, vertices=False, **law)`` with H, W the photograph's.  The kernel hands back the 21 partials of the
    camera; the chain from them to the six numbers is torch autograd.  ``steps`` Adam steps of ``lr`` pixels (``fit_screen``'s loop).
    The intrinsics are not fitted.  ``law``: the law, IOR and band keywords of ``image_loss_fused``.  Returns (the ``camera_M`` 4-tuple
    (R, K, R^-1, K^-1) of the smallest loss seen, as numpy arrays; the loss history)."""
    import numpy as np
    from . import views
    for bad in ("camera_param", "screen_param", "texture_param", "vertices", "want_image"):
        if bad in law:
            raise ValueError(f"fit_camera sets {bad} itself")
    centre, extent = views.mesh_frame(scene.mesh.vertices)
    H, W = int(photograph.shape[0]), int(photograph.shape[1])

    def loss_of(six):
        pose = camera_pose(camera_M, six, centre, extent)
        return scene.image_loss_fused(None, H, W, screen, texture, photograph, weight=weight, vertices=False, camera_param=pose, **law).to(six.device)

    six, history = _adam_from_zero(loss_of, steps, lr)
    rinv, kinv = (m.numpy() for m in camera_pose(camera_M, six, centre, extent))
    return (np.linalg.inv(rinv), np.asarray(camera_M[1], dtype=np.float64), rinv, kinv), history


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fit the interior IOR of a fixed mesh against a capture (bisection on d loss / d IOR).")
    ap.add_argument("--name", default=optim.HyperParams["name"])
    ap.add_argument("--data-path", default="./data/")
    ap.add_argument("--capture", default=None, help=".npz / .h5 capture with the reference's datasets (default: a synthetic capture of "
                    "<name>_scan.ply, or of the hull without a scan, traced under the same law at --ior)")
    ap.add_argument("--mesh", default=None, help="the mesh to calibrate against (default: the mesh the synthetic capture was traced on; "
                    "required with --capture)")
    ap.add_argument("--ior", type=float, default=optim.HyperParams["IOR"], help="the IOR the synthetic capture is traced with")
    ap.add_argument("--bracket", type=float, nargs=2, default=(1.2, 1.8), metavar=("LO", "HI"))
    ap.add_argument("--halvings", type=int, default=14)
    ap.add_argument("--max-bounces", type=int, default=2, metavar="K")
    ap.add_argument("--tir", choices=("drop", "reflect"), default="drop")
    ap.add_argument("--refraction", choices=("reference", "snell"), default="snell")
    ap.add_argument("--res", type=int, default=256, help="resolution of the synthetic capture")
    ap.add_argument("--views", type=int, default=72, help="views of the synthetic capture")
    ap.add_argument("--num-view", type=int, default=optim.HyperParams["num_view"], help="views the refraction loss cycles through")
    args = ap.parse_args(argv)
    from . import captured_data, diffrender as Render, views
    law = (args.max_bounces, args.tir, args.refraction)
    if args.capture is not None:
        if args.mesh is None:
            ap.error("--capture needs --mesh: the mesh the IOR is fitted on")
        data = captured_data.get_data(dict(optim.HyperParams, name=args.name, num_view=args.num_view), path=args.capture)
        scene = Render.Scene(args.mesh, 0)
    else:
        scan = os.path.join(args.data_path, f"{args.name}_scan.ply")
        scene = Render.Scene(args.mesh or (scan if os.path.exists(scan) else os.path.join(args.data_path, f"{args.name}_vh.ply")), 0)
        Render.intIOR = args.ior
        Render.resx = Render.resy = args.res
        center, extent = views.mesh_frame(scene.mesh.vertices)
        data = captured_data.SyntheticData(scene, center, extent, args.res, args.res, num_view=min(args.num_view, args.views), n_total=args.views,
                                           name=args.name, path_law=law)
    fit = fit_ior(scene, data, law, tuple(args.bracket), args.halvings)
    report = {"name": args.name, "max_bounces": law[0], "tir": law[1], "refraction": law[2], "ior": fit["ior"], "bracket": list(fit["bracket"]),
              "evaluations": fit["evaluations"]}
    if args.capture is None:
        report["ior_true"] = args.ior
        report["error"] = fit["ior"] - args.ior
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
