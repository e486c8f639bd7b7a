"""CPU: refraction paths of up to K interactions with internal reflection (drt_shade.h bounce_reflect / bounce_reflect_backward,
drt_paths.h trace_path_k / path_recompute_backward_k), compiled for the host by g++ (tests/hostsim/paths_adjoint.cpp) and held against
torch autograd of the same expressions, central finite differences and the float64 restatement tests/paths_ref.py.

Depth-8 gradient disagreement, host harness against paths_ref's autograd, measured here on the fixture views (test_depth8_gradient_*
prints it): see MEASURED_DEPTH8_REL below."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import paths_ref
from conftest import IOR, data_path, fixture_mesh, fixture_view, golden
from drt_amd import mesh_io, views
from oracle import diffrender_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
IOR_INT, IOR_EXT = IOR, 1.00029
KMAX = 8

# max |host - autograd| / max |autograd| of d ray_loss / d vertices and d lin / d vertices at (K = 8, reflect), the largest of the views
# of test_depth8_gradient_disagreement_is_far_inside_the_tolerance (hand 64 x 64 view 5: 4.8e-16 and 4.7e-16; horse x4 256 x 256 view 11:
# 7.2e-16 and 5.7e-16; absolute: at most 9.1e-13).  Far below a tenth of the project's 1e-9, so the GPU tests keep the project's tolerances (1e-9 relative, 1e-5 absolute).
MEASURED_DEPTH8_REL = 7.2e-16
GRAD_REL, GRAD_ABS, RAY_ABS = 1e-9, 1e-5, 1e-10


@pytest.fixture(scope="module")
def hp():
    src = os.path.join(ROOT, "tests", "hostsim", "paths_adjoint.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libpaths_adjoint.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hs_create.restype = _P
    lib.hs_create.argtypes = [_P, _I64, _P, _I64]
    lib.hs_destroy.argtypes = [_P]
    lib.hp_reflect.argtypes = [_P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P, _P, _P]
    lib.hp_path.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P, _P]
    lib.hp_trace.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I, _I, _P, _P, _P, _P, _P]
    lib.hp_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P]
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _triangle_across(rng, o, d, inside, theta):
    """A triangle per row across the ray (o, d) at a moderate distance, hit at the incidence angle theta; `inside`: the ray travels inside
    the object (the geometric normal points along it, so bounce_forward sees it leaving)."""
    n = len(o)
    dh = _unit(d)
    a = _unit(np.cross(dh, rng.standard_normal((n, 3))))
    nrm = np.cos(theta)[:, None] * dh + np.sin(theta)[:, None] * a
    n0 = np.where(inside[:, None], nrm, -nrm)
    p = o + d * rng.uniform(3.0, 12.0, (n, 1))
    a2 = _unit(np.cross(n0, rng.standard_normal((n, 3))))
    b2 = np.cross(n0, a2)
    ang = np.array([0.0, 2.1, 4.2]) + rng.uniform(0, 1, (n, 1))
    return p[:, None, :] + 6.0 * (np.cos(ang)[..., None] * a2[:, None, :] + np.sin(ang)[..., None] * b2[:, None, :])


def _interact_torch(o, d, tri):
    return paths_ref.interact(o, d, tri, IOR_INT, IOR_EXT)


def test_reflect_adjoint_matches_autograd_and_fd(hp):
    rng = np.random.default_rng(21)
    n = 600
    o = rng.standard_normal((n, 3)) * 20.0
    d = _unit(rng.standard_normal((n, 3)))
    inside = rng.random(n) < 0.7
    theta = np.where(inside, rng.uniform(np.radians(48), np.radians(75), n), rng.uniform(np.radians(5), np.radians(60), n))
    tri = np.ascontiguousarray(_triangle_across(rng, o, d, inside, theta))
    g_new_o, g_wr = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    new_o, wr, tir = np.empty((n, 3)), np.empty((n, 3)), np.empty(n, np.uint8)
    g_tri, g_o, g_d = np.empty((n, 3, 3)), np.empty((n, 3)), np.empty((n, 3))
    hp.hp_reflect(_p(o), _p(d), _p(tri), n, IOR_INT, IOR_EXT, _p(g_new_o), _p(g_wr), _p(new_o), _p(wr), _p(tir), _p(g_tri), _p(g_o), _p(g_d))
    assert (tir[inside] == 1).all() and (tir[~inside] == 0).all()          # beyond the critical angle (42.8 degrees) from inside only

    def reflect_torch(to, td, tt):
        _, _, t, nn = orc.moller_trumbore(to, td, tt)
        leaving = torch.logical_not(orc._dot(-td, nn).clamp(-1, 1) > 0)
        nn = nn * torch.where(leaving, -torch.ones_like(t), torch.ones_like(t)).view(-1, 1)
        return paths_ref._reflect(to, td, t, nn)

    to, td, tt = (torch.tensor(a, requires_grad=True) for a in (o, d, tri))
    n_o, n_d = reflect_torch(to, td, tt)
    assert _rel(new_o, n_o.detach()) < 1e-13 and _rel(wr, n_d.detach()) < 1e-13
    f = (n_o * torch.tensor(g_new_o)).sum() + (n_d * torch.tensor(g_wr)).sum()
    go_ref, gd_ref, gt_ref = torch.autograd.grad(f, (to, td, tt))
    assert _rel(g_o, go_ref) < 1e-12
    assert _rel(g_d, gd_ref) < 1e-12
    assert _rel(g_tri, gt_ref) < 1e-12

    # central finite differences of the whole functional along random directions of the three inputs
    def F(oo, dd, tt_):
        with torch.no_grad():
            a, b = reflect_torch(torch.tensor(oo), torch.tensor(dd), torch.tensor(tt_))
            return float((a * torch.tensor(g_new_o)).sum() + (b * torch.tensor(g_wr)).sum())
    h = 1e-6
    for seed in range(3):
        r = np.random.default_rng(100 + seed)
        do, dd, dt = r.standard_normal(o.shape), r.standard_normal(d.shape), r.standard_normal(tri.shape)
        fd = (F(o + h * do, d + h * dd, tri + h * dt) - F(o - h * do, d - h * dd, tri - h * dt)) / (2 * h)
        an = float((g_o * do).sum() + (g_d * dd).sum() + (g_tri * dt).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)


def _mixed_paths(rng, n):
    """n paths of 2..8 interactions through their own triangles: enter, then inside the object every hit is either a total internal
    reflection (incidence beyond the critical angle) or a refraction out, after which the ray may enter again.  Returns
    (o, d, tris [n,8,3,3], n_hits [n], planned TIR flags [n,8])."""
    o = rng.standard_normal((n, 3)) * 30.0
    d = _unit(rng.standard_normal((n, 3)))
    n_hits = rng.integers(2, KMAX + 1, n).astype(np.int32)
    n_hits[:40] = KMAX
    tris = np.zeros((n, KMAX, 3, 3))
    flags = np.zeros((n, KMAX), np.uint8)
    inside = np.zeros(n, bool)
    co, cd = o.copy(), d.copy()
    for k in range(KMAX):
        want_reflect = inside & (rng.random(n) < 0.6)
        want_reflect[:40] = inside[:40] & (k < KMAX - 1)               # enter, six reflections in a row, leave
        theta = np.where(want_reflect, rng.uniform(np.radians(50), np.radians(72), n),
                         np.where(inside, rng.uniform(np.radians(4), np.radians(32), n), rng.uniform(np.radians(5), np.radians(55), n)))
        tris[:, k] = _triangle_across(rng, co, cd, inside, theta)
        with torch.no_grad():
            no, nd, tir = _interact_torch(torch.tensor(co), torch.tensor(cd), torch.tensor(tris[:, k]))
        assert (tir.numpy() == want_reflect).all()
        flags[:, k] = want_reflect
        live = k < n_hits
        flags[~live, k] = 0
        co, cd = no.numpy(), nd.numpy()
        inside = np.where(want_reflect, inside, ~inside)
    return o, d, np.ascontiguousarray(tris), n_hits, flags


def _path_torch(to, td, ttris, n_hits):
    o, d = to, td
    hits = torch.tensor(n_hits.astype(np.int64))
    for k in range(KMAX):
        sel = torch.nonzero(hits > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, _ = _interact_torch(o[sel], d[sel], ttris[sel, k])
        o, d = o.index_put((sel,), no), d.index_put((sel,), nd)
    return o, d


def test_path_k_adjoint_matches_autograd_and_fd(hp):
    rng = np.random.default_rng(31)
    n = 500
    o, d, tris, n_hits, flags = _mixed_paths(rng, n)
    assert set(np.unique(n_hits)) == set(range(2, KMAX + 1))
    assert (flags[:40, 1:KMAX - 1] == 1).all()                          # several consecutive reflections
    g_ori, g_dir = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))     # gradients on both out_ori and out_dir
    out_o, out_d = np.empty((n, 3)), np.empty((n, 3))
    got_flags, n_refr, g_tri = np.empty((n, KMAX), np.uint8), np.empty(n, np.int32), np.empty((n, KMAX, 3, 3))
    hp.hp_path(_p(o), _p(d), _p(tris), _p(n_hits), n, IOR_INT, IOR_EXT, _p(g_ori), _p(g_dir), _p(out_o), _p(out_d), _p(got_flags), _p(n_refr), _p(g_tri))
    assert np.array_equal(got_flags, flags)
    assert np.array_equal(n_refr, n_hits - flags.sum(1))

    to, td, tt = (torch.tensor(a, requires_grad=True) for a in (o, d, tris))
    oo, od = _path_torch(to, td, tt, n_hits)
    assert _rel(out_o, oo.detach()) < 1e-13 and _rel(out_d, od.detach()) < 1e-13
    f = (oo * torch.tensor(g_ori)).sum() + (od * torch.tensor(g_dir)).sum()
    gt_ref, = torch.autograd.grad(f, (tt,))
    live = np.arange(KMAX)[None, :] < n_hits[:, None]
    assert not g_tri[~live].any() and not gt_ref.numpy()[~live].any()
    # per row: each path is its own functional, so a deep path is judged on its own scale
    err = np.abs(g_tri - gt_ref.numpy()).reshape(n, -1).max(1) / np.abs(gt_ref.numpy()).reshape(n, -1).max(1)
    print("path_k adjoint vs autograd: worst relative error per path", err.max(), "at", int(n_hits[err.argmax()]), "interactions")
    assert err.max() < 1e-11

    def F(tris_):
        with torch.no_grad():
            a, b = _path_torch(torch.tensor(o), torch.tensor(d), torch.tensor(tris_), n_hits)
            return float((a * torch.tensor(g_ori)).sum() + (b * torch.tensor(g_dir)).sum())
    h = 1e-6
    for seed in range(3):
        dt = np.random.default_rng(300 + seed).standard_normal(tris.shape) * live[:, :, None, None]
        fd = (F(tris + h * dt) - F(tris - h * dt)) / (2 * h)
        an = float((g_tri * dt).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)


# ---------------------------------------------------------------------------------------------------- camera rays through the host BVH
def _view(mesh, res, view_id):
    center, extent = views.mesh_frame(mesh.vertices)
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, 72, res, res)[view_id]
    return views.generate_ray(res, res, Kinv, Rinv)


def _host_trace(hp, mesh, o, d, max_bounces, tir):
    F = np.ascontiguousarray(mesh.faces, np.int32)
    V = np.ascontiguousarray(mesh.vertices, np.float64)
    V32 = np.ascontiguousarray(V.astype(np.float32))
    h = hp.hs_create(_p(F), len(F), _p(V32), len(V))
    n = o.shape[0]
    on, dn = np.ascontiguousarray(o.numpy()), np.ascontiguousarray(d.numpy())
    out = dict(out_ori=np.empty((n, 3)), out_dir=np.empty((n, 3)), mask=np.empty(n, np.uint8), tape=np.empty((max_bounces, n), np.int32),
               hits=np.empty(n, np.uint8))
    hp.hp_trace(h, _p(V), _p(on), _p(dn), n, IOR_INT, IOR_EXT, max_bounces, int(tir == "reflect"), _p(out["out_ori"]), _p(out["out_dir"]),
                _p(out["mask"]), _p(out["tape"]), _p(out["hits"]))
    return h, F, V, on, dn, out


def _meshes():
    return {"hand": lambda: mesh_io.read_ply(data_path("hand_vh.ply")), "horse": lambda: fixture_mesh(golden("horse50k_r256_v11"))}


@pytest.mark.parametrize("name,res,view_id", [("hand", 128, 5), ("horse", 256, 11)])
@pytest.mark.parametrize("max_bounces,tir", [(8, "reflect"), (4, "drop")])
def test_trace_path_k_agrees_with_the_restatement_on_every_ray(hp, name, res, view_id, max_bounces, tir):
    mesh = _meshes()[name]()
    o, d = _view(mesh, res, view_id)
    h, F, V, on, dn, got = _host_trace(hp, mesh, o, d, max_bounces, tir)
    hp.hs_destroy(h)
    ref = paths_ref.trace(mesh.faces, torch.tensor(V), o, d, IOR_INT, IOR_EXT, max_bounces, tir)
    # nothing is excluded: validity, hit count and tape of EVERY ray
    assert np.array_equal(got["mask"].astype(bool), ref["valid"].numpy())
    assert np.array_equal(got["hits"].astype(np.int64), ref["hits"].numpy())
    assert np.array_equal(got["tape"].astype(np.int64), ref["tape"].numpy())
    assert int(ref["valid"].sum()) > 500
    assert np.abs(got["out_ori"] - ref["out_ori"].numpy()).max() <= RAY_ABS
    assert np.abs(got["out_dir"] - ref["out_dir"].numpy()).max() <= RAY_ABS
    print(name, res, view_id, max_bounces, tir, "valid", int(ref["valid"].sum()), "max hits", int(ref["hits"].max()),
          "d out_ori", np.abs(got["out_ori"] - ref["out_ori"].numpy()).max(), "d out_dir", np.abs(got["out_dir"] - ref["out_dir"].numpy()).max())


@pytest.mark.parametrize("name,fixture", [("hand", "hand_r64_v5"), ("horse", "horse50k_r256_v11")])
def test_depth8_gradient_disagreement_is_far_inside_the_tolerance(hp, name, fixture):
    """The figure the GPU tolerances rest on: host harness (the kernels' own code) against paths_ref's autograd at (K = 8, reflect) on the
    fixture views, for d ray_loss / d vertices and d lin / d vertices."""
    g = golden(fixture)
    mesh = _meshes()[name]()
    o, d, sp, valid = fixture_view(g)
    h, F, V, on, dn, got = _host_trace(hp, mesh, o, d, 8, "reflect")
    Vt = torch.tensor(V, requires_grad=True)
    out_ori, out_dir, mask, aux = paths_ref.render_paths(mesh.faces, Vt, o, d, IOR_INT, IOR_EXT, 8, "reflect")
    assert np.array_equal(got["mask"].astype(bool), aux["valid"].numpy()) and np.array_equal(got["tape"].astype(np.int64), aux["tape"].numpy())
    assert int(aux["hits"].max()) >= 6
    loss = orc.ray_loss(out_ori, out_dir, mask, sp, valid)
    g_ray, = torch.autograd.grad(loss, Vt, retain_graph=True)
    rng = np.random.default_rng(int(g["lin_seed"]))
    P = o.shape[0]
    w_ori, w_dir = rng.standard_normal((P, 3)), rng.standard_normal((P, 3))
    lin = (out_ori * torch.tensor(w_ori)).sum() + (out_dir * torch.tensor(w_dir)).sum()
    g_lin, = torch.autograd.grad(lin, Vt)

    # d ray_loss / d out_dir as the loss defines it (out_ori detached), from the host's own exit rays
    tgt = sp.numpy() - got["out_ori"]
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    vm = valid.numpy() & got["mask"].astype(bool)
    gd = np.where(vm[:, None], 2.0 * (got["out_dir"] - tgt), 0.0)
    worst = 0.0
    for g_o, g_d, ref in ((np.zeros((P, 3)), np.ascontiguousarray(gd), g_ray.numpy()), (w_ori, w_dir, g_lin.numpy())):
        acc = np.zeros_like(V)
        hp.hp_backward(h, _p(V), _p(on), _p(dn), P, IOR_INT, IOR_EXT, _p(got["mask"]), _p(got["tape"]), _p(got["hits"]), _p(g_o), _p(g_d), _p(acc))
        diff = np.abs(acc - ref).max()
        print(fixture, "depth-8 gradient: max abs diff", diff, "relative to max |ref|", diff / np.abs(ref).max())
        assert diff <= GRAD_ABS and diff <= GRAD_REL * np.abs(ref).max()
        worst = max(worst, diff / np.abs(ref).max())
    hp.hs_destroy(h)
    assert worst <= 0.1 * GRAD_REL, "the depth-8 disagreement is no longer far inside the tolerance: see MEASURED_DEPTH8_REL"
