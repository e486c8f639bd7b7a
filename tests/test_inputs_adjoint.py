"""CPU: the adjoints of the refraction path w.r.t. the camera ray and the indices of refraction (drt_shade.h bounce_backward_eta +
eta_to_ior, drt_path.h path_recompute_backward_inputs), compiled for the host by g++ (tests/hostsim/inputs_adjoint.cpp) and held
against torch autograd of a float64 restatement built from the oracle's moller_trumbore / refract_dir with eta as a tensor."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle.diffrender_oracle import moller_trumbore, refract_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
IOR_INT, IOR_EXT = 1.4723, 1.00029


@pytest.fixture(scope="module")
def hi():
    src = os.path.join(ROOT, "tests", "hostsim", "inputs_adjoint.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libinputs_adjoint.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hi_bounce.argtypes = [_P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P]
    lib.hi_path.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P]
    return lib


def _p(a):
    return a.ctypes.data_as(_P)


def _bounce_torch(o, d, tri, ior_int, ior_ext):
    """One bounce of the reference's refract_ray (DiffRender.py:503-535) with the IORs as tensors: (new_o, new_d)."""
    _, _, t, n = moller_trumbore(o, d, tri)
    wo = -d
    cos_i = (wo * n).sum(1).clamp(-1, 1)
    leaving = torch.logical_not(cos_i > 0)
    sgn = torch.where(leaving, -torch.ones_like(t), torch.ones_like(t))
    eta_i = torch.where(leaving, ior_int, ior_ext)
    eta_t = torch.where(leaving, ior_ext, ior_int)
    n = n * sgn.view(-1, 1)
    wt = refract_dir(wo, n, eta_i / eta_t)
    return o + t.view(-1, 1) * d + 1e-5 * wt, wt


def _rays(rng, n, flip):
    """n rays that hit a random triangle at a moderate angle; flip[i]: the triangle faces away (the ray leaves the object)."""
    tri = rng.standard_normal((n, 3, 3)) * 5.0
    w = rng.dirichlet((2.0, 2.0, 2.0), n)
    p = np.einsum("nk,nkc->nc", w, tri)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = -nrm + 0.6 * rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cos = -(d * nrm).sum(1)
    d[cos < 0] *= -1.0                                # every ray enters through the front face ...
    tri[flip] = tri[flip][:, [0, 2, 1]]               # ... unless the winding is reversed
    o = p - d * rng.uniform(5.0, 50.0, (n, 1))
    return o, d, tri


def _keep(d, tri, lo=0.25):
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.abs((d * nrm).sum(1)) > lo


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("leaving", [False, True])
def test_bounce_adjoint_matches_autograd(hi, leaving):
    rng = np.random.default_rng(11 + leaving)
    n = 400
    o, d, tri = _rays(rng, n, np.full(n, leaving))
    k = _keep(d, tri)
    o, d, tri = o[k].copy(), d[k].copy(), tri[k].copy()
    n = len(o)
    g_new_o, g_wt = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    new_o, wt, sg = np.empty((n, 3)), np.empty((n, 3)), np.empty(n)
    g_tri, g_o, g_d, g_ior = np.empty((n, 3, 3)), np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))
    hi.hi_bounce(_p(o), _p(d), _p(tri), n, IOR_INT, IOR_EXT, _p(g_new_o), _p(g_wt), _p(new_o), _p(wt), _p(sg), _p(g_tri), _p(g_o), _p(g_d), _p(g_ior))
    assert (sg < 0).all() if leaving else (sg > 0).all()

    to, td, tt = (torch.tensor(a, requires_grad=True) for a in (o, d, tri))
    ti = torch.tensor(IOR_INT, dtype=torch.float64, requires_grad=True)
    te = torch.tensor(IOR_EXT, dtype=torch.float64, requires_grad=True)
    n_o, n_d = _bounce_torch(to, td, tt, ti, te)
    assert _rel(new_o, n_o.detach()) < 1e-13 and _rel(wt, n_d.detach()) < 1e-13
    # per-row IOR partials: one functional per row (the rows are independent), summed by autograd row by row through a batch of IORs
    ti_rows = torch.full((n,), IOR_INT, dtype=torch.float64, requires_grad=True)
    te_rows = torch.full((n,), IOR_EXT, dtype=torch.float64, requires_grad=True)
    n_o2, n_d2 = _bounce_torch(to, td, tt, ti_rows, te_rows)
    f = (n_o2 * torch.tensor(g_new_o)).sum() + (n_d2 * torch.tensor(g_wt)).sum()
    go_ref, gd_ref, gt_ref, gi_ref, ge_ref = torch.autograd.grad(f, (to, td, tt, ti_rows, te_rows))
    assert _rel(g_o, go_ref) < 1e-12
    assert _rel(g_d, gd_ref) < 1e-12
    assert _rel(g_tri, gt_ref) < 1e-12
    assert _rel(g_ior[:, 0], gi_ref) < 1e-12
    assert _rel(g_ior[:, 1], ge_ref) < 1e-12
    # the scalar IOR of the reference: the sum over rows
    f1 = (n_o * torch.tensor(g_new_o)).sum() + (n_d * torch.tensor(g_wt)).sum()
    gi1, ge1 = torch.autograd.grad(f1, (ti, te))
    assert abs(g_ior[:, 0].sum() - gi1.item()) <= 1e-12 * np.abs(g_ior[:, 0]).sum()
    assert abs(g_ior[:, 1].sum() - ge1.item()) <= 1e-12 * np.abs(g_ior[:, 1]).sum()


def _path_torch(o, d, tri1, tri2, ior_int, ior_ext):
    o2, d2 = _bounce_torch(o, d, tri1, ior_int, ior_ext)
    return _bounce_torch(o2, d2, tri2, ior_int, ior_ext)


def _paths(rng, n):
    """Two-bounce paths: the ray enters through tri1, and tri2 is placed across its refracted direction (so it leaves through tri2)."""
    o, d, tri1 = _rays(rng, n, np.zeros(n, bool))
    with torch.no_grad():
        o2, d2 = _bounce_torch(torch.tensor(o), torch.tensor(d), torch.tensor(tri1), torch.tensor(IOR_INT, dtype=torch.float64),
                               torch.tensor(IOR_EXT, dtype=torch.float64))
    o2, d2 = o2.numpy(), d2.numpy()
    p2 = o2 + d2 * rng.uniform(2.0, 10.0, (n, 1))
    # a triangle around p2 whose normal points along d2 (front face hit from inside: leaving), tilted at random
    nrm = d2 + 0.5 * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = np.cross(nrm, rng.standard_normal((n, 3)))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(nrm, a)
    ang = np.array([0.0, 2.1, 4.2]) + rng.uniform(0, 1, (n, 1))
    tri2 = p2[:, None, :] + 4.0 * (np.cos(ang)[..., None] * a[:, None, :] + np.sin(ang)[..., None] * b[:, None, :])
    keep = _keep(d, tri1) & _keep(d2, tri2, 0.5)
    return o[keep].copy(), d[keep].copy(), tri1[keep].copy(), np.ascontiguousarray(tri2[keep])


def test_path_adjoint_matches_autograd_and_fd(hi):
    rng = np.random.default_rng(5)
    o, d, tri1, tri2 = _paths(rng, 500)
    n = len(o)
    assert n > 100
    g_ori, g_dir = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    out_o, out_d = np.empty((n, 3)), np.empty((n, 3))
    g_tri, g_tri_plain, g_o, g_d, g_ior = np.empty((n, 6, 3)), np.empty((n, 6, 3)), np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))
    hi.hi_path(_p(o), _p(d), _p(tri1), _p(tri2), n, IOR_INT, IOR_EXT, _p(g_ori), _p(g_dir), _p(out_o), _p(out_d), _p(g_tri), _p(g_tri_plain),
               _p(g_o), _p(g_d), _p(g_ior))
    # the vertex gradients are path_recompute_backward's, bit for bit
    assert np.array_equal(g_tri, g_tri_plain)

    to, td, t1, t2 = (torch.tensor(a, requires_grad=True) for a in (o, d, tri1, tri2))
    ti_rows = torch.full((n,), IOR_INT, dtype=torch.float64, requires_grad=True)
    te_rows = torch.full((n,), IOR_EXT, dtype=torch.float64, requires_grad=True)
    oo, od = _path_torch(to, td, t1, t2, ti_rows, te_rows)
    assert _rel(out_o, oo.detach()) < 1e-13 and _rel(out_d, od.detach()) < 1e-13
    f = (oo * torch.tensor(g_ori)).sum() + (od * torch.tensor(g_dir)).sum()
    go_ref, gd_ref, g1_ref, g2_ref, gi_ref, ge_ref = torch.autograd.grad(f, (to, td, t1, t2, ti_rows, te_rows))
    assert _rel(g_o, go_ref) < 1e-12
    assert _rel(g_d, gd_ref) < 1e-12
    assert _rel(g_tri[:, :3], g1_ref) < 1e-12 and _rel(g_tri[:, 3:], g2_ref) < 1e-12
    assert _rel(g_ior[:, 0], gi_ref) < 1e-12
    assert _rel(g_ior[:, 1], ge_ref) < 1e-12

    # central finite differences of the whole functional in each IOR
    def F(ior_int, ior_ext):
        with torch.no_grad():
            a, b = _path_torch(torch.tensor(o), torch.tensor(d), torch.tensor(tri1), torch.tensor(tri2),
                               torch.tensor(ior_int, dtype=torch.float64), torch.tensor(ior_ext, dtype=torch.float64))
            return float((a * torch.tensor(g_ori)).sum() + (b * torch.tensor(g_dir)).sum())
    h = 1e-6
    fd_int = (F(IOR_INT + h, IOR_EXT) - F(IOR_INT - h, IOR_EXT)) / (2 * h)
    fd_ext = (F(IOR_INT, IOR_EXT + h) - F(IOR_INT, IOR_EXT - h)) / (2 * h)
    assert abs(g_ior[:, 0].sum() - fd_int) <= 1e-6 * abs(fd_int)
    assert abs(g_ior[:, 1].sum() - fd_ext) <= 1e-6 * abs(fd_ext)


def test_exit_direction_does_not_depend_on_origin(hi):
    """With only d / d out_dir seeded, the origin adjoint is exactly zero (flat faces): why ray_loss leaves origin.grad None."""
    rng = np.random.default_rng(9)
    o, d, tri1, tri2 = _paths(rng, 64)
    n = len(o)
    g_ori, g_dir = np.zeros((n, 3)), rng.standard_normal((n, 3))
    bufs = [np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 6, 3)), np.empty((n, 6, 3)), np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))]
    hi.hi_path(_p(o), _p(d), _p(tri1), _p(tri2), n, IOR_INT, IOR_EXT, _p(g_ori), _p(g_dir), *[_p(b) for b in bufs])
    assert not bufs[4].any()
    assert np.abs(bufs[5]).max() > 0
