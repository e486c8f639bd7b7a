"""CPU: the IOR adjoint of the K-interaction path law (drt_shade.h bounce_backward_snell_eta / bounce_backward_eta / eta_to_ior,
drt_paths.h path_recompute_backward_ior_k / path_loss_backward_ior_k), compiled for the host by g++ (tests/hostsim/paths_ior.cpp) and
held against torch autograd of the float64 restatement tests/ior_ref.py, against path_loss_backward_k (the vertex gradients: bit for
bit) and against the two-bounce route of drt_path.h (path_recompute_backward_inputs: the same terms by another route).

Tolerance of the summed IOR partials: 1e-9 relative to the sum of the absolute per-path contributions.  Measured here (printed by
test_path_ior_partials_*): see MEASURED below."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import ior_ref
from conftest import IOR, data_path, fixture_view, golden
from drt_amd import mesh_io
from test_snell_adjoint import CRITICAL, _refracting_rows, _triangle_across, _unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
IOR_INT, IOR_EXT = IOR, 1.00029
IOR_REL = 1e-9
# |host sum - autograd sum| / sum |per-path autograd| of (d / d ior_int, d / d ior_ext) on hand 64 x 64 view 5, worst of the four laws
# of LAWS (the worst single path, relative to the largest: 1.7e-15); DESIGN.md 7.4 quotes them
MEASURED = {"g_int": 1.5e-16, "g_ext": 1.4e-16}
LAWS = [(2, "drop", "snell", 226), (6, "reflect", "snell", 342), (6, "reflect", "reference", 346), (2, "drop", "reference", 257)]


@pytest.fixture(scope="module")
def pi():
    src = os.path.join(ROOT, "tests", "hostsim", "paths_ior.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libpaths_ior.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hs_create.restype = _P
    lib.hs_create.argtypes = [_P, _I64, _P, _I64]
    lib.hs_destroy.argtypes = [_P]
    lib.pi_bounce.restype = _I64
    lib.pi_bounce.argtypes = [_P, _P, _P, _I64, _D, _D, _I] + [_P] * 7
    lib.pi_interaction.argtypes = [_P, _P, _P, _I64, _D, _D, _I] + [_P] * 6
    lib.pi_trace.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I, _I, _I, _P, _P, _P, _P, _P]
    lib.pi_loss_backward.restype = _D
    lib.pi_loss_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I] + [_P] * 12
    lib.pi_two_bounce.argtypes = [_P, _P, _P, _P, _I64, _D, _D] + [_P] * 8
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


def _bounce(pi, o, d, tri, snell, g_new_o, g_wt):
    n = len(o)
    r = dict(tir=np.empty(n, np.uint8), ct=np.empty(n), g_eta=np.empty(n), g_int=np.empty(n), g_ext=np.empty(n))
    r["differ"] = pi.pi_bounce(_p(o), _p(d), _p(tri), n, IOR_INT, IOR_EXT, int(snell), _p(g_new_o), _p(g_wt), _p(r["tir"]), _p(r["ct"]),
                               _p(r["g_eta"]), _p(r["g_int"]), _p(r["g_ext"]))
    return r


def _autograd_rows(o, d, tri, g_new_o, g_wt, refraction):
    """Per-row (d / d ior_int, d / d ior_ext) of the functional <new_o, g_new_o> + <wt, g_wt>: every row has its own IOR leaves."""
    n = len(o)
    ii = torch.full((n,), IOR_INT, dtype=torch.float64, requires_grad=True)
    ie = torch.full((n,), IOR_EXT, dtype=torch.float64, requires_grad=True)
    n_o, n_d, tir = ior_ref.refract_only(torch.tensor(o), torch.tensor(d), torch.tensor(tri), ii, ie, refraction)
    f = (n_o * torch.tensor(g_new_o)).sum() + (n_d * torch.tensor(g_wt)).sum()
    gi, ge = torch.autograd.grad(f, (ii, ie))
    return gi.numpy(), ge.numpy(), tir.numpy()


@pytest.mark.parametrize("refraction", ["snell", "reference"])
def test_single_bounce_eta_adjoint_matches_autograd(pi, refraction):
    """2 000 random refracting bounces, entering and leaving, 100 of them 1e-3 rad below the critical angle (where, under Snell, the
    ct chain carries the largest term: ct = 0.047 there and d ct / d eta goes like 1 / ct)."""
    o, d, inside, theta, tri, rng = _refracting_rows(21, 2000, n_critical=100)
    n = len(o)
    g_new_o, g_wt = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got = _bounce(pi, o, d, tri, refraction == "snell", g_new_o, g_wt)
    gi, ge, tir = _autograd_rows(o, d, tri, g_new_o, g_wt, refraction)
    assert not got["tir"].any() and not tir.any()
    assert got["differ"] == 0              # the vertex and ray adjoints are those of the pair without eta, bit for bit
    assert np.isfinite(got["g_int"]).all() and np.isfinite(got["g_ext"]).all()
    err_i = np.abs(got["g_int"] - gi) / np.abs(gi)
    err_e = np.abs(got["g_ext"] - ge) / np.abs(ge)
    print(refraction, "g_int / g_ext per row against autograd: worst relative error", err_i.max(), err_e.max(), "; critical rows", err_i[:100].max(),
          "(their ct:", got["ct"][:100].min(), ")")
    assert err_i.max() < 1e-11 and err_e.max() < 1e-11
    # the IORs enter through their quotient only: eta is homogeneous of degree 0 in (ior_int, ior_ext)
    assert np.abs(got["g_int"] * IOR_INT + got["g_ext"] * IOR_EXT).max() <= 1e-12 * np.abs(got["g_int"] * IOR_INT).max()


def test_the_ct_guard_row_gives_finite_values(pi):
    """Rows beyond the critical angle, run through bounce_backward_snell_eta as if their flag said "refracts": ct = 0, nothing passes
    through it, g_eta is finite and is autograd's of the restatement with the same guard."""
    rng = np.random.default_rng(23)
    n = 200
    o = rng.standard_normal((n, 3)) * 20.0
    d = _unit(rng.standard_normal((n, 3)))
    theta = rng.uniform(CRITICAL + 1e-9, np.radians(80), n)
    theta[:20] = CRITICAL + 1e-9
    tri = np.ascontiguousarray(_triangle_across(rng, o, d, np.ones(n, bool), theta))
    g_new_o, g_wt = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got = _bounce(pi, o, d, tri, True, g_new_o, g_wt)
    assert got["tir"].all() and (got["ct"] == 0).all() and got["differ"] == 0
    for k in ("g_eta", "g_int", "g_ext"):
        assert np.isfinite(got[k]).all(), k
    gi, ge, tir = _autograd_rows(o, d, tri, g_new_o, g_wt, "snell")
    assert tir.all()
    # with ct the constant 0, w = eta * (d + ci * n): its direction does not depend on eta, so the true partials are 0 and both sides hold
    # rounding residue of the O(1) terms that cancel (measured: at most 3e-16) -- an absolute bound, 100 roundings of those terms
    print("guard rows: max |g_int|, |g_ext|", np.abs(got["g_int"]).max(), np.abs(got["g_ext"]).max(), "autograd", np.abs(gi).max(), np.abs(ge).max())
    for a, b in ((got["g_int"], gi), (got["g_ext"], ge)):
        assert np.abs(a).max() <= 100 * 2.0 ** -53 * 4 and np.abs(a - b).max() <= 100 * 2.0 ** -53 * 4


@pytest.mark.parametrize("snell", [True, False])
def test_a_mirrored_interaction_contributes_exactly_zero(pi, snell):
    """path_recompute_backward_ior_k on one-interaction paths: rows beyond the critical angle are mirrored and add exactly 0 to both
    partials (while their vertex gradient is not zero); rows that refract on the same call add something."""
    rng = np.random.default_rng(29)
    n = 400
    o = rng.standard_normal((n, 3)) * 20.0
    d = _unit(rng.standard_normal((n, 3)))
    theta = np.where(np.arange(n) < 200, rng.uniform(CRITICAL + 1e-6, np.radians(80), n), rng.uniform(0.05, CRITICAL - 1e-3, n))
    tri = np.ascontiguousarray(_triangle_across(rng, o, d, np.ones(n, bool), theta))
    g_o, g_d = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    tir, gi, ge, g_tri = np.empty(n, np.uint8), np.full(n, np.nan), np.full(n, np.nan), np.empty((n, 3, 3))
    pi.pi_interaction(_p(o), _p(d), _p(tri), n, IOR_INT, IOR_EXT, int(snell), _p(g_o), _p(g_d), _p(tir), _p(gi), _p(ge), _p(g_tri))
    assert tir[:200].all() and not tir[200:].any()
    assert (gi[:200] == 0).all() and (ge[:200] == 0).all()
    assert np.abs(g_tri[:200]).reshape(200, -1).max(1).min() > 0
    assert (gi[200:] != 0).all() and (ge[200:] != 0).all()
    # and the refracting rows are autograd's
    ii = torch.full((200,), IOR_INT, dtype=torch.float64, requires_grad=True)
    ie = torch.full((200,), IOR_EXT, dtype=torch.float64, requires_grad=True)
    n_o, n_d, _ = ior_ref.interact(torch.tensor(o[200:]), torch.tensor(d[200:]), torch.tensor(tri[200:]), ii, ie, "snell" if snell else "reference")
    ri, re_ = torch.autograd.grad((n_o * torch.tensor(g_o[200:])).sum() + (n_d * torch.tensor(g_d[200:])).sum(), (ii, ie))
    assert (np.abs(gi[200:] - ri.numpy()) / np.abs(ri.numpy())).max() < 1e-11 and (np.abs(ge[200:] - re_.numpy()) / np.abs(re_.numpy())).max() < 1e-11


# ---------------------------------------------------------------------------------------------------- camera rays through the host BVH
class _Host:
    """The hand hull in the host BVH, and view 5 of the 64 x 64 fixture with a target on every ray."""

    def __init__(self, pi):
        self.pi = pi
        self.mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
        self.F = np.ascontiguousarray(self.mesh.faces, np.int32)
        self.V = np.ascontiguousarray(self.mesh.vertices, np.float64)
        self.V32 = np.ascontiguousarray(self.V.astype(np.float32))
        self.h = pi.hs_create(_p(self.F), len(self.F), _p(self.V32), len(self.V))
        o, d, sp, _ = fixture_view(golden("hand_r64_v5"))
        self.o, self.d, self.sp = o, d, sp
        self.valid = torch.ones(o.shape[0], dtype=torch.bool)
        self.on, self.dn = np.ascontiguousarray(o.numpy(), np.float64), np.ascontiguousarray(d.numpy(), np.float64)
        self.spn = np.ascontiguousarray(sp.numpy(), np.float64)
        self.va = np.ones(o.shape[0], np.uint8)
        self._cases = {}

    def case(self, k, tir, refraction):
        """(host trace, host adjoints, restatement) of one law: computed once, shared read-only."""
        key = (k, tir, refraction)
        if key not in self._cases:
            n, snell = self.on.shape[0], int(refraction == "snell")
            t = dict(out_ori=np.empty((n, 3)), out_dir=np.empty((n, 3)), mask=np.empty(n, np.uint8), tape=np.empty((k, n), np.int32), hits=np.empty(n, np.uint8))
            self.pi.pi_trace(self.h, _p(self.V), _p(self.on), _p(self.dn), n, IOR_INT, IOR_EXT, k, int(tir == "reflect"), snell, _p(t["out_ori"]),
                             _p(t["out_dir"]), _p(t["mask"]), _p(t["tape"]), _p(t["hits"]))
            a = dict(per_int=np.empty(n), per_ext=np.empty(n), grad=np.zeros_like(self.V), grad_plain=np.zeros_like(self.V), loss_plain=np.zeros(1))
            a["loss"] = self.pi.pi_loss_backward(self.h, _p(self.V), _p(self.on), _p(self.dn), n, IOR_INT, IOR_EXT, snell, _p(t["mask"]), _p(t["tape"]),
                                                 _p(t["hits"]), _p(t["out_ori"]), _p(t["out_dir"]), _p(self.spn), _p(self.va), _p(a["per_int"]),
                                                 _p(a["per_ext"]), _p(a["grad"]), _p(a["grad_plain"]), _p(a["loss_plain"]))
            ref = ior_ref.loss_and_grads(self.mesh.faces, torch.tensor(self.V), self.o, self.d, self.sp, self.valid, IOR_INT, IOR_EXT, k, tir, refraction,
                                         want_vertices=True)
            self._cases[key] = (t, a, ref)
        return self._cases[key]


@pytest.fixture(scope="module")
def host(pi):
    hst = _Host(pi)
    yield hst
    pi.hs_destroy(hst.h)


@pytest.mark.parametrize("k,tir,refraction,n_valid", LAWS)
def test_path_ior_partials_match_autograd_and_leave_the_vertex_gradient_alone(host, k, tir, refraction, n_valid):
    t, a, ref = host.case(k, tir, refraction)
    aux = ref["aux"]
    assert np.array_equal(t["mask"].astype(bool), aux["valid"].numpy()) and np.array_equal(t["tape"].astype(np.int64), aux["tape"].numpy())
    assert int(t["mask"].sum()) == n_valid == ref["count"]
    if tir == "reflect":
        assert int(t["hits"].max()) >= 5          # paths with mirrored interactions are among them
    assert abs(a["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    # the vertex gradient and the loss are path_loss_backward_k's, bit for bit
    assert a["loss"] == a["loss_plain"][0]
    assert np.array_equal(a["grad"].view(np.int64), a["grad_plain"].view(np.int64)) and np.abs(a["grad"]).max() > 0
    assert np.abs(a["grad"] - ref["grad_V"]).max() <= 1e-9 * np.abs(ref["grad_V"]).max()
    # the summed partials, relative to the sum of the absolute per-path contributions
    rows = ref["rows"]
    for name, per, key in (("g_int", a["per_int"], "int"), ("g_ext", a["per_ext"], "ext")):
        got, want, scale = per.sum(), ref["g_" + key], ref["abs_" + key]
        rel = abs(got - want) / scale
        worst_path = np.abs(per[rows] - ref["per_" + key]).max() / np.abs(ref["per_" + key]).max()
        print(f"({k}, {tir}, {refraction}) {name}: host {got:.12e} autograd {want:.12e} sum |per path| {scale:.6e} disagreement {rel:.3e} "
              f"(worst single path, relative to the largest: {worst_path:.3e})")
        assert np.isfinite(per).all() and scale > 0
        assert rel <= IOR_REL
        assert np.abs(per[rows] - ref["per_" + key]).max() <= IOR_REL * np.abs(ref["per_" + key]).max()
        assert (per[np.setdiff1d(np.arange(len(per)), rows)] == 0).all()
        assert rel <= 0.01 * IOR_REL, "the disagreement is no longer far inside the tolerance: see MEASURED"


def test_two_bounce_route_gives_the_same_partials_per_path(host):
    """(2, drop) under the reference formula is the two-bounce path: path_recompute_backward_inputs (drt_path.h), which reverses b2 then b1
    with bounce_backward_eta / eta_to_ior, gives the partials of every path -- the same statements in the same order, so the same bits."""
    t, a, _ = host.case(2, "drop", "reference")
    n = host.on.shape[0]
    per_int, per_ext = np.empty(n), np.empty(n)
    host.pi.pi_two_bounce(host.h, _p(host.V), _p(host.on), _p(host.dn), n, IOR_INT, IOR_EXT, _p(t["mask"]), _p(t["tape"]), _p(t["out_ori"]),
                          _p(t["out_dir"]), _p(host.spn), _p(host.va), _p(per_int), _p(per_ext))
    assert np.count_nonzero(per_int) == 257
    assert np.array_equal(per_int.view(np.int64), a["per_int"].view(np.int64))
    assert np.array_equal(per_ext.view(np.int64), a["per_ext"].view(np.int64))
