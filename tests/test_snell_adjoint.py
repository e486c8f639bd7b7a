"""CPU: the Snell element of the K-interaction path law (drt_shade.h bounce_forward_snell / bounce_backward_snell, drt_paths.h
trace_path_k<true> / path_recompute_backward_k<true> / path_loss_backward_k<true>), compiled for the host by g++
(tests/hostsim/snell_adjoint.cpp) and held against the law of sines itself, torch autograd of the float64 restatement
tests/snell_ref.py, central finite differences and time reversal.

Depth-8 gradient disagreement, host harness against snell_ref's autograd, measured here (test_depth8_gradient_* prints it): see
MEASURED_DEPTH8_REL below."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import snell_ref
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import mesh_io, views
from oracle import diffrender_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
IOR_INT, IOR_EXT = IOR, 1.00029
CRITICAL = float(np.arcsin(IOR_EXT / IOR_INT))           # 42.8 degrees, from inside

# max |host - autograd| / max |autograd| of d ray_loss / d vertices and d lin / d vertices at (K = 8, reflect, snell) on hand 64 x 64
# view 5: 1.5e-15 and 7.7e-16 (absolute: at most 1.7e-13).  Far below a tenth of the project's 1e-9, so the GPU tests keep the
# project's tolerances (1e-9 relative, 1e-5 absolute).
MEASURED_DEPTH8_REL = 1.5e-15
GRAD_REL, GRAD_ABS, RAY_ABS = 1e-9, 1e-5, 1e-10


@pytest.fixture(scope="module")
def sn():
    src = os.path.join(ROOT, "tests", "hostsim", "snell_adjoint.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libsnell_adjoint.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hs_create.restype = _P
    lib.hs_create.argtypes = [_P, _I64, _P, _I64]
    lib.hs_destroy.argtypes = [_P]
    lib.sn_bounce.argtypes = [_P, _P, _P, _I64, _D, _D, _I] + [_P] * 11
    lib.sn_trace.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I, _I, _P, _P, _P, _P, _P]
    lib.sn_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P]
    lib.sn_loss_backward.restype = _D
    lib.sn_loss_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D] + [_P] * 8
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _triangle_across(rng, o, d, inside, theta):
    """A triangle per row across the ray (o, d) at a moderate distance, hit at the incidence angle theta; `inside`: the ray travels inside
    the object (the geometric normal points along it, so the bounce sees it leaving)."""
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


def _bounce(sn, o, d, tri, snell, g_new_o=None, g_wt=None):
    n = len(o)
    g_new_o = np.zeros((n, 3)) if g_new_o is None else g_new_o
    g_wt = np.zeros((n, 3)) if g_wt is None else g_wt
    r = dict(new_o=np.empty((n, 3)), wt=np.empty((n, 3)), tir=np.empty(n, np.uint8), ct=np.empty(n), n=np.empty((n, 3)), eta=np.empty(n),
             g_tri=np.empty((n, 3, 3)), g_o=np.empty((n, 3)), g_d=np.empty((n, 3)))
    sn.sn_bounce(_p(o), _p(d), _p(tri), n, IOR_INT, IOR_EXT, int(snell), _p(g_new_o), _p(g_wt), _p(r["new_o"]), _p(r["wt"]), _p(r["tir"]),
                 _p(r["ct"]), _p(r["n"]), _p(r["eta"]), _p(r["g_tri"]), _p(r["g_o"]), _p(r["g_d"]))
    return r


def _refracting_rows(seed, n, n_critical=0, theta_min=0.0):
    """n (ray, triangle) pairs that refract: half entering at theta_min .. 85 degrees, half leaving at theta_min .. 1e-3 rad below the
    critical angle; the first n_critical leaving rows sit exactly 1e-3 rad below it."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((n, 3)) * 20.0
    d = _unit(rng.standard_normal((n, 3)))
    inside = np.arange(n) < n // 2
    theta = np.where(inside, rng.uniform(theta_min, CRITICAL - 1e-3, n), rng.uniform(theta_min, np.radians(85), n))
    theta[:n_critical] = CRITICAL - 1e-3
    return o, d, inside, theta, np.ascontiguousarray(_triangle_across(rng, o, d, inside, theta)), rng


def test_snell_bounce_obeys_the_law_of_sines_and_the_reference_bounce_does_not(sn):
    """sin(theta_t) = eta sin(theta_i) to 1e-14 under Snell, entering and leaving, with wt in the plane of d and n (the triple product wt . (d x n) is 0
    exactly; wt is a normalised combination of d and n, about 5 roundings per component, and forming the product here takes 9 products
    and 6 sums of numbers below 1: under 20 roundings of 2^-53 in all); the
    reference's Refract misses the relation by more than 1e-3 wherever the incidence exceeds 10 degrees (measured on these rows: at least
    1.09e-3.  The miss grows like theta_i^3; for ENTERING rays it is 9.7e-4 at exactly 10 degrees and passes 1e-3 at 10.12 degrees, so a
    row drawn inside that tenth of a degree would fail this assertion through no fault of the code; none of these 2 000 is)."""
    o, d, inside, theta, tri, _ = _refracting_rows(7, 2000, n_critical=50)
    got, ref = _bounce(sn, o, d, tri, True), _bounce(sn, o, d, tri, False)
    assert not got["tir"].any() and np.array_equal(got["tir"], ref["tir"])
    assert inside.sum() == 1000 and np.array_equal(got["eta"] > 1, inside)
    sin_i = np.linalg.norm(np.cross(d, got["n"]), axis=1)
    assert np.abs(np.arcsin(sin_i) - theta).max() < 1e-9
    for r in (got, ref):                 # everything but the direction is shared: the same tape
        assert np.array_equal(r["n"], got["n"]) and np.array_equal(r["eta"], got["eta"])
    resid = np.abs(np.linalg.norm(np.cross(got["wt"], got["n"]), axis=1) - got["eta"] * sin_i)
    print("snell: max |sin t - eta sin i|", resid.max())
    assert resid.max() <= 1e-14
    off = np.abs((got["wt"] * np.cross(d, got["n"])).sum(1))
    print("snell: max |wt . (d x n)|", off.max())
    assert off.max() <= 20 * 2.0 ** -53
    assert (got["wt"] * got["n"]).sum(1).max() < 0          # through the surface
    assert np.abs(np.linalg.norm(got["wt"], axis=1) - 1).max() <= 1e-15
    # the reference's formula on the same inputs
    resid_ref = np.abs(np.linalg.norm(np.cross(ref["wt"], ref["n"]), axis=1) - ref["eta"] * sin_i)
    wide = theta > np.radians(10)
    print("reference: min |sin t - eta sin i| beyond 10 degrees", resid_ref[wide].min(), "over", int(wide.sum()), "rows")
    assert wide.sum() > 1500 and resid_ref[wide].min() > 1e-3


def _autograd_rows(o, d, tri, g_new_o, g_wt):
    to, td, tt = (torch.tensor(a, requires_grad=True) for a in (o, d, tri))
    n_o, n_d, tir = snell_ref.refract_only(to, td, tt, IOR_INT, IOR_EXT, "snell")
    f = (n_o * torch.tensor(g_new_o)).sum() + (n_d * torch.tensor(g_wt)).sum()
    go, gd, gt = torch.autograd.grad(f, (to, td, tt))
    return n_o.detach().numpy(), n_d.detach().numpy(), tir.numpy(), go.numpy(), gd.numpy(), gt.numpy()


def _row_err(got, ref_o, ref_d, ref_t):
    n = len(ref_o)
    a = np.concatenate([got["g_o"], got["g_d"], got["g_tri"].reshape(n, 9)], axis=1)
    b = np.concatenate([ref_o, ref_d, ref_t.reshape(n, 9)], axis=1)
    return np.abs(a - b).max(1) / np.abs(b).max(1)


def test_snell_bounce_adjoint_matches_autograd_and_fd(sn):
    # from 2 degrees: the finite differences below move d off unit length by 1e-6, and within 0.1 degrees of normal incidence that takes
    # 1 - cos_i^2 across the clamp at 0 -- a kink of the reference's own expression, shared by both laws
    o, d, inside, theta, tri, rng = _refracting_rows(11, 600, n_critical=60, theta_min=np.radians(2))
    n = len(o)
    g_new_o, g_wt = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got = _bounce(sn, o, d, tri, True, g_new_o, g_wt)
    ref_no, ref_wt, ref_tir, go, gd, gt = _autograd_rows(o, d, tri, g_new_o, g_wt)
    assert not got["tir"].any() and not ref_tir.any()
    assert np.abs(got["new_o"] - ref_no).max() <= 1e-13 * np.abs(ref_no).max() and np.abs(got["wt"] - ref_wt).max() <= 1e-13
    err = _row_err(got, go, gd, gt)
    print("snell bounce adjoint vs autograd: worst relative error per row", err.max(), "; rows 1e-3 rad below the critical angle", err[:60].max(),
          "(their ct:", got["ct"][:60].min(), ")")
    assert err.max() < 1e-11

    # central finite differences (h = 1e-6) of the functional along random directions of the three inputs, over every row -- a tenth of them
    # 1e-3 rad below the critical angle, where they carry the largest gradients.  Then those rows alone: there ct = sqrt(u) with u = 2.2e-3,
    # and the h^2 term of a central difference, (h du/dh)^2 / (8 u^2) relative, is itself 1e-6 at h = 1e-6 (measured: 1.1e-6, falling
    # fourfold per halving of h), so that run removes it by Richardson extrapolation from h and h / 2.
    def F(oo, dd, tt_, rows):
        with torch.no_grad():
            a, b, _ = snell_ref.refract_only(torch.tensor(oo[rows]), torch.tensor(dd[rows]), torch.tensor(tt_[rows]), IOR_INT, IOR_EXT, "snell")
            return float((a * torch.tensor(g_new_o[rows])).sum() + (b * torch.tensor(g_wt[rows])).sum())

    def central(h, do, dd, dt, rows):
        return (F(o + h * do, d + h * dd, tri + h * dt, rows) - F(o - h * do, d - h * dd, tri - h * dt, rows)) / (2 * h)
    h = 1e-6
    for rows in (slice(None), slice(0, 60)):
        for seed in range(3):
            r = np.random.default_rng(100 + seed)
            do, dd, dt = r.standard_normal(o.shape), r.standard_normal(d.shape), r.standard_normal(tri.shape)
            fd = central(h, do, dd, dt, rows)
            if rows != slice(None):
                fd = (4.0 * central(h / 2, do, dd, dt, rows) - fd) / 3.0
            an = float((got["g_o"][rows] * do[rows]).sum() + (got["g_d"][rows] * dd[rows]).sum() + (got["g_tri"][rows] * dt[rows]).sum())
            print("fd", fd, "adjoint", an)
            assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)


def test_a_refracting_flag_over_a_non_positive_argument_gives_finite_gradients(sn):
    """Rows beyond the critical angle: 1 - eta^2 sin2 < 0, so ct = 0.  The harness runs bounce_backward_snell on them as if their flag said
    "refracts" (a flag and an argument that disagree by a rounding look just like this to the adjoint): no gradient passes through ct,
    nothing is NaN or inf, and the result is autograd's of the restatement with the same guard."""
    rng = np.random.default_rng(13)
    n = 200
    o = rng.standard_normal((n, 3)) * 20.0
    d = _unit(rng.standard_normal((n, 3)))
    inside = np.ones(n, bool)
    theta = rng.uniform(CRITICAL + 1e-9, np.radians(80), n)
    theta[:20] = CRITICAL + 1e-9
    tri = np.ascontiguousarray(_triangle_across(rng, o, d, inside, theta))
    g_new_o, g_wt = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got = _bounce(sn, o, d, tri, True, g_new_o, g_wt)
    assert got["tir"].all() and (got["ct"] == 0).all()
    for k in ("new_o", "wt", "g_o", "g_d", "g_tri"):
        assert np.isfinite(got[k]).all(), k
    _, _, ref_tir, go, gd, gt = _autograd_rows(o, d, tri, g_new_o, g_wt)
    assert ref_tir.all() and np.isfinite(gt).all()
    assert _row_err(got, go, gd, gt).max() < 1e-11


# ---------------------------------------------------------------------------------------------------- camera rays through the host BVH
def _view(mesh, res, view_id):
    center, extent = views.mesh_frame(mesh.vertices)
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, 72, res, res)[view_id]
    return views.generate_ray(res, res, Kinv, Rinv)


class _Host:
    """The hand hull in the host BVH."""

    def __init__(self, sn):
        self.sn = sn
        self.mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
        self.F = np.ascontiguousarray(self.mesh.faces, np.int32)
        self.V = np.ascontiguousarray(self.mesh.vertices, np.float64)
        self.V32 = np.ascontiguousarray(self.V.astype(np.float32))
        self.h = sn.hs_create(_p(self.F), len(self.F), _p(self.V32), len(self.V))

    def trace(self, o, d, max_bounces, tir):
        n = o.shape[0]
        on, dn = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
        out = dict(out_ori=np.empty((n, 3)), out_dir=np.empty((n, 3)), mask=np.empty(n, np.uint8), tape=np.empty((max_bounces, n), np.int32),
                   hits=np.empty(n, np.uint8), origin=on, dir=dn)
        self.sn.sn_trace(self.h, _p(self.V), _p(on), _p(dn), n, IOR_INT, IOR_EXT, max_bounces, int(tir == "reflect"), _p(out["out_ori"]),
                         _p(out["out_dir"]), _p(out["mask"]), _p(out["tape"]), _p(out["hits"]))
        return out


@pytest.fixture(scope="module")
def host(sn):
    hst = _Host(sn)
    yield hst
    sn.hs_destroy(hst.h)


CASES = [(128, 8, "reflect", 1428), (64, 2, "drop", 226), (64, 6, "reflect", 342)]
_traced = {}


def _case(host, res, max_bounces, tir):
    """(host trace, restatement trace) of hand view 5, computed once per case and shared (read-only)."""
    key = (res, max_bounces, tir)
    if key not in _traced:
        o, d = _view(host.mesh, res, 5)
        got = host.trace(o.numpy(), d.numpy(), max_bounces, tir)
        ref = snell_ref.trace(host.mesh.faces, torch.tensor(host.V), o, d, IOR_INT, IOR_EXT, max_bounces, tir, "snell")
        _traced[key] = (got, ref)
    return _traced[key]


@pytest.mark.parametrize("res,max_bounces,tir,n_valid", CASES)
def test_trace_path_k_snell_agrees_with_the_restatement_on_every_ray(host, res, max_bounces, tir, n_valid):
    got, ref = _case(host, res, max_bounces, tir)
    # nothing is excluded: validity, hit count and tape of EVERY ray
    assert np.array_equal(got["mask"].astype(bool), ref["valid"].numpy())
    assert np.array_equal(got["hits"].astype(np.int64), ref["hits"].numpy())
    assert np.array_equal(got["tape"].astype(np.int64), ref["tape"].numpy())
    assert np.abs(got["out_ori"] - ref["out_ori"].numpy()).max() <= RAY_ABS
    assert np.abs(got["out_dir"] - ref["out_dir"].numpy()).max() <= RAY_ABS
    hist = np.bincount(got["hits"], minlength=max_bounces + 1).tolist()
    print(res, max_bounces, tir, "valid", int(got["mask"].sum()), "hit histogram", hist)
    assert int(got["mask"].sum()) == n_valid
    if (res, max_bounces) == (64, 6):
        assert hist == [3754, 0, 226, 61, 37, 10, 8]


@pytest.mark.parametrize("res,max_bounces,tir,n_valid", CASES)
def test_snell_paths_retrace_themselves_backwards(host, res, max_bounces, tir, n_valid):
    """Independent of the restatement: refraction by Snell's law and mirror reflection are time-reversible.  The exit ray of every valid
    path, sent back from two mesh extents out, must -- where it meets the same faces in reverse order -- leave along the camera ray; the
    1e-5 offsets move a path sideways by less than that per interaction, so nearly all of them do meet the same faces.  (Under the
    reference's formula a fifth of the paths does not come back this way: this fails if the flag is ignored.)"""
    got, _ = _case(host, res, max_bounces, tir)
    vi = np.nonzero(got["mask"])[0]
    _, extent = views.mesh_frame(host.mesh.vertices)
    back_o = got["out_ori"][vi] + 2.0 * float(np.max(extent)) * got["out_dir"][vi]
    back = host.trace(back_o, -got["out_dir"][vi], max_bounces, tir)
    K = np.arange(max_bounces)[:, None]
    hits = got["hits"][vi].astype(np.int64)
    fwd = got["tape"][:, vi]
    rev_idx = np.clip(hits[None, :] - 1 - K, 0, max_bounces - 1)
    reversed_tape = np.where(K < hits[None, :], np.take_along_axis(fwd, rev_idx, axis=0), -1)
    retraced = back["mask"].astype(bool) & (back["hits"] == got["hits"][vi]) & (back["tape"] == reversed_tape).all(0)
    err = np.linalg.norm(back["out_dir"][retraced] + got["dir"][vi][retraced], axis=1)
    print(res, max_bounces, tir, "retraced", int(retraced.sum()), "of", len(vi), "max |out_dir + camera dir|", err.max())
    assert len(vi) == n_valid
    assert err.max() <= 1e-10
    assert retraced.sum() >= 0.99 * len(vi)


def test_depth8_gradient_disagreement_is_far_inside_the_tolerance(host, sn):
    """The figure the GPU tolerances rest on: host harness (the kernels' own code) against snell_ref's autograd at (K = 8, reflect, snell) on
    hand 64 x 64 view 5, for d ray_loss / d vertices (path_loss_backward_k<true>) and d lin / d vertices (path_recompute_backward_k<true>)."""
    g = golden("hand_r64_v5")
    o, d, sp, valid = fixture_view(g)
    got = host.trace(o.numpy(), d.numpy(), 8, "reflect")
    Vt = torch.tensor(host.V, requires_grad=True)
    out_ori, out_dir, mask, aux = snell_ref.render_paths(host.mesh.faces, Vt, o, d, IOR_INT, IOR_EXT, 8, "reflect", "snell")
    assert np.array_equal(got["mask"].astype(bool), aux["valid"].numpy()) and np.array_equal(got["tape"].astype(np.int64), aux["tape"].numpy())
    assert int(aux["hits"].max()) >= 6
    loss = orc.ray_loss(out_ori, out_dir, mask, sp, valid)
    g_ray, = torch.autograd.grad(loss, Vt, retain_graph=True)
    rng = np.random.default_rng(int(g["lin_seed"]))
    P = o.shape[0]
    w_ori, w_dir = rng.standard_normal((P, 3)), rng.standard_normal((P, 3))
    lin = (out_ori * torch.tensor(w_ori)).sum() + (out_dir * torch.tensor(w_dir)).sum()
    g_lin, = torch.autograd.grad(lin, Vt)

    spn = np.ascontiguousarray(sp.numpy(), np.float64)
    va = np.ascontiguousarray(valid.numpy().astype(np.uint8))
    acc_ray = np.zeros_like(host.V)
    host_loss = sn.sn_loss_backward(host.h, _p(host.V), _p(got["origin"]), _p(got["dir"]), P, IOR_INT, IOR_EXT, _p(got["mask"]), _p(got["tape"]),
                                    _p(got["hits"]), _p(got["out_ori"]), _p(got["out_dir"]), _p(spn), _p(va), _p(acc_ray))
    assert abs(host_loss - loss.item()) <= 1e-12 * abs(loss.item())
    acc_lin = np.zeros_like(host.V)
    sn.sn_backward(host.h, _p(host.V), _p(got["origin"]), _p(got["dir"]), P, IOR_INT, IOR_EXT, _p(got["mask"]), _p(got["tape"]), _p(got["hits"]),
                   _p(w_ori), _p(w_dir), _p(acc_lin))
    worst = 0.0
    for what, acc, ref in (("ray_loss", acc_ray, g_ray.numpy()), ("lin", acc_lin, g_lin.numpy())):
        diff = np.abs(acc - ref).max()
        print("hand_r64_v5 depth-8 snell gradient of", what, ": max abs diff", diff, "relative to max |ref|", diff / np.abs(ref).max())
        assert diff <= GRAD_ABS and diff <= GRAD_REL * np.abs(ref).max()
        worst = max(worst, diff / np.abs(ref).max())
    assert worst <= 0.1 * GRAD_REL, "the depth-8 disagreement is no longer far inside the tolerance: see MEASURED_DEPTH8_REL"
