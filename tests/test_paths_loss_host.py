"""CPU: the one-pass form of the K-interaction law, drt_paths.h path_loss_backward_k (the ray_loss term of a completed path on its parked
exit ray + the adjoint with a unit seed), compiled for the host by g++ (tests/hostsim/paths_loss.cpp) and run over the recorded face tapes
of tests/golden/hand_r64_v5_paths.npz.  The summed loss and the vertex gradient must match the golden chain of the reference's own pieces
(`*_ray_loss`, `*_grad_ray_loss`) at the project's tolerances: loss 1e-10 relative, gradient 1e-9 relative to the largest reference entry and
1e-5 absolute."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import IOR, data_path, fixture_view, golden
from drt_amd import mesh_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
IOR_INT, IOR_EXT = IOR, 1.00029
LOSS_REL, GRAD_REL, GRAD_ABS = 1e-10, 1e-9, 1e-5


@pytest.fixture(scope="module")
def hl():
    src = os.path.join(ROOT, "tests", "hostsim", "paths_loss.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libpaths_loss.so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hl_loss_backward.restype = _I64
    lib.hl_loss_backward.argtypes = [_P, _P, _P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P]
    return lib


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


@pytest.mark.parametrize("tag", ["k6_reflect", "k4_drop"])
def test_loss_and_gradient_over_the_golden_tapes(hl, tag):
    g = golden("hand_r64_v5_paths")
    o, d, sp, valid = fixture_view(golden("hand_r64_v5"))
    mesh = mesh_io.read_ply(data_path("hand_vh.ply"))
    F = np.ascontiguousarray(mesh.faces, np.int32)
    V = np.ascontiguousarray(mesh.vertices, np.float64)
    on, dn, spn = (np.ascontiguousarray(t.numpy(), np.float64) for t in (o, d, sp))
    va = np.ascontiguousarray(valid.numpy().astype(np.uint8))
    mask = np.ascontiguousarray(g[f"{tag}_mask"].astype(np.uint8))
    tape = np.ascontiguousarray(g[f"{tag}_tape"], np.int32)
    hits = np.ascontiguousarray(g[f"{tag}_hits"], np.uint8)
    n = on.shape[0]
    assert tape.shape == (int(g[f"{tag}_max_bounces"]), n)
    loss = ctypes.c_double(0.0)
    grad = np.zeros_like(V)
    cnt = hl.hl_loss_backward(_p(F), _p(V), _p(on), _p(dn), _p(spn), _p(va), n, IOR_INT, IOR_EXT, _p(mask), _p(tape), _p(hits),
                              ctypes.byref(loss), _p(grad))
    assert cnt == int((mask.astype(bool) & va.astype(bool)).sum()) and cnt > 200
    ref_loss, ref_grad = float(g[f"{tag}_ray_loss"]), g[f"{tag}_grad_ray_loss"]
    diff = np.abs(grad - ref_grad).max()
    print(tag, "rays", cnt, "loss", loss.value, "rel", abs(loss.value - ref_loss) / abs(ref_loss), "gradient: max abs diff", diff,
          "relative to max |ref|", diff / np.abs(ref_grad).max())
    assert loss.value == pytest.approx(ref_loss, rel=LOSS_REL)
    assert np.isfinite(grad).all()
    assert diff <= GRAD_ABS and diff <= GRAD_REL * np.abs(ref_grad).max()
