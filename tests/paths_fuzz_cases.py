"""Random cases of the K-interaction path kernels' fuzz tests (tests/test_paths_fuzz_host.py on the CPU, tests/test_gpu_paths_fuzz.py on
the device; modelled on tests/image_fuzz_cases.py): ``case(seed)`` is a dict with a random closed shape of ``test_gpu_fuzz._shape`` (one
body, two shells or two lobes), its own pair of IORs, a law (K, tir, refraction), the rays of a turntable camera far from, close to or
inside the body on a non-square image, targets for about 80 % of the rays and two weight planes of a linear functional of the exit rays.
Everything is deterministic from the seed.  ``CASES`` is the literal list of admitted seeds; admission and coverage are computed from the
float64 restatements alone (tests/test_paths_fuzz_host.py), never from what a device returns.

The draws of ``case(seed, variant)``, in this order: (1) from ``default_rng(BASE + seed)`` the body, ``_shape(rng)``; then, from the same
generator when ``variant == 0`` and from ``default_rng(BASE + VARIANT_STRIDE * variant + seed)`` otherwise (the same mesh under other rays
and another law), (2) ``ior_int`` of IORS_INT, (3) ``ior_ext`` of IORS_EXT, (4) K in 2..8, (5) ``tir`` of TIRS, (6) ``refraction`` of
REFRACTIONS, (7) the image size of SIZES, (8) the camera's distance factor of DISTANCES, (9) its view of the 72-view turntable,
(10) the targets ``sp`` -- standard normal * 40 around the mesh's centre, [P, 3] --, (11) ``valid`` -- uniform [P] > 0.2 --, (12) the
weight planes ``w_ori`` then ``w_dir``, standard normal [P, 3] each."""
import functools

import numpy as np
import torch

import ior_ref
import snell_ref
from conftest import IOR
from drt_amd import views
from test_gpu_fuzz import _shape

BASE = 13000                 # the generator of seed k is numpy's default_rng(BASE + k)
VARIANT_STRIDE = 100000
N_VIEWS = 72
IORS_INT, IORS_EXT = (IOR, 1.1, 1.33, 2.4), (1.00029, 1.0, 1.2)
TIRS, REFRACTIONS = ("drop", "reflect"), ("reference", "snell")
DISTANCES = (2.5, 1.2, 0.8, 0.3)          # 0.3: the camera is inside the object or at its rim
SIZES = ((48, 40), (33, 57), (64, 31), (1, 1), (31, 64), (57, 43), (40, 60))          # (H, W): at most 2 451 rays

# The admitted seeds, chosen for the coverage tests/test_paths_fuzz_host.py asserts (its table is printed with -s).  A seed that fails
# admission there is replaced by the next one that serves the same purpose and noted here with its figure.  Rejected: none -- on all of
# the first 72 seeds the host build of the kernels' headers and the restatement give the same tape, hit count and mask on every ray.
CASES = [0, 3, 8, 9, 12, 16, 22, 26, 30, 34, 38, 43, 44, 52, 57, 64]
# (seed, variant a, variant b): one mesh under two sets of rays and laws, for the one-scene-many-calls test of the device
PAIRS = [(43, 0, 2), (30, 0, 2), (9, 0, 2)]


@functools.lru_cache(maxsize=None)
def case(seed, variant=0):
    """The case of a seed (``variant``: the same body under other rays and another law); shared by the tests and left unchanged."""
    rng = np.random.default_rng(BASE + seed)
    mesh = _shape(rng)
    if variant:
        rng = np.random.default_rng(BASE + VARIANT_STRIDE * variant + seed)
    ior_int, ior_ext = float(rng.choice(IORS_INT)), float(rng.choice(IORS_EXT))
    k = int(rng.integers(2, 9))
    tir, refraction = TIRS[int(rng.integers(2))], REFRACTIONS[int(rng.integers(2))]
    height, width = SIZES[int(rng.integers(len(SIZES)))]
    distance, view = float(rng.choice(DISTANCES)), int(rng.integers(N_VIEWS))
    center, extent = views.mesh_frame(mesh.vertices)
    R, K, Rinv, Kinv = views.turntable_cameras(center, extent, N_VIEWS, width, height, distance_factor=distance)[view]
    o, d = views.generate_ray(height, width, Kinv, Rinv)
    n = o.shape[0]
    sp = torch.tensor(rng.standard_normal((n, 3)) * 40.0 + np.asarray(center))
    valid = torch.tensor(rng.random(n) > 0.2)
    w_ori, w_dir = torch.tensor(rng.standard_normal((n, 3))), torch.tensor(rng.standard_normal((n, 3)))
    return dict(name=f"fuzz{seed}" + (f"/{variant}" if variant else ""), seed=seed, variant=variant, mesh=mesh, center=center, extent=extent,
                ior_int=ior_int, ior_ext=ior_ext, k=k, tir=tir, refraction=refraction, law=(k, tir, refraction), height=height, width=width,
                distance=distance, view=view, eye=np.asarray(Rinv)[:3, 3].copy(), o=o, d=d, n=n, sp=sp, valid=valid, w_ori=w_ori, w_dir=w_dir)


def two_components(sc):
    """Whether the mesh is two bodies (no vertex of one is in a face of the other): ``_shape`` appends the second body's vertices."""
    F = np.asarray(sc["mesh"].faces)
    for cut in range(1, len(sc["mesh"].vertices)):
        lo = (F < cut).all(1)
        if lo.any() and not lo.all() and ((F < cut).any(1) == lo).all():
            return True
    return False


def vertices(sc):
    return torch.tensor(sc["mesh"].vertices, dtype=torch.float64)


# ---- the restatements' results, computed once per process and never modified ---------------------------------------------------------------
def trace_of(sc, law=None, iors=None):
    """snell_ref.trace of a case's rays (``law`` / ``iors``: others than the case's own, for the negative controls)."""
    k, tir, refraction = sc["law"] if law is None else law
    ior_int, ior_ext = (sc["ior_int"], sc["ior_ext"]) if iors is None else iors
    return snell_ref.trace(sc["mesh"].faces, vertices(sc), sc["o"], sc["d"], ior_int, ior_ext, k, tir, refraction)


@functools.lru_cache(maxsize=None)
def trace(seed, variant=0):
    return trace_of(case(seed, variant))


def loss_and_grads(sc, valid=None, law=None, iors=None, aux=None):
    """``ior_ref.loss_and_grads`` of a case with the vertex gradient -- and, where the restatement's trace has NO contributing path (none
    completes, or none that completes has a target), what the law gives there: loss 0, zero gradients, count 0.  ``ior_ref`` raises on
    those, because autograd has nothing to differentiate: a limit of the restatement's domain, not of the law."""
    k, tir, refraction = sc["law"] if law is None else law
    ior_int, ior_ext = (sc["ior_int"], sc["ior_ext"]) if iors is None else iors
    valid = sc["valid"] if valid is None else valid
    V = vertices(sc)
    if aux is None:
        aux = snell_ref.trace(sc["mesh"].faces, V, sc["o"], sc["d"], ior_int, ior_ext, k, tir, refraction)
    if not bool((aux["valid"] & valid).any()):
        none = np.zeros(0)
        return dict(loss=0.0, g_int=0.0, g_ext=0.0, abs_int=0.0, abs_ext=0.0, per_int=none, per_ext=none, rows=np.zeros(0, np.int64), count=0,
                    grad_V=np.zeros(tuple(V.shape)), aux=aux)
    return ior_ref.loss_and_grads(sc["mesh"].faces, V, sc["o"], sc["d"], sc["sp"], valid, ior_int, ior_ext, k, tir, refraction, aux=aux,
                                  want_vertices=True)


@functools.lru_cache(maxsize=None)
def reference(seed, variant=0):
    return loss_and_grads(case(seed, variant), aux=trace(seed, variant))


def exit_rays(sc, law=None, iors=None, aux=None):
    """The restatement's exit rays, the linear functional <out_ori, w_ori> + <out_dir, w_dir> and its vertex gradient by autograd:
    dict(out_ori, out_dir [P, 3] with zeros on the rows without a completed path, lin, grad_lin, aux)."""
    k, tir, refraction = sc["law"] if law is None else law
    ior_int, ior_ext = (sc["ior_int"], sc["ior_ext"]) if iors is None else iors
    V = vertices(sc).requires_grad_(True)
    oo, od, _, aux = snell_ref.render_paths(sc["mesh"].faces, V, sc["o"], sc["d"], ior_int, ior_ext, k, tir, refraction, aux=aux)
    lin = (oo * sc["w_ori"]).sum() + (od * sc["w_dir"]).sum()
    grad = torch.autograd.grad(lin, V)[0].numpy() if bool(aux["valid"].any()) else np.zeros(tuple(V.shape))
    return dict(out_ori=oo.detach().numpy(), out_dir=od.detach().numpy(), lin=float(lin.detach()), grad_lin=grad, aux=aux)


@functools.lru_cache(maxsize=None)
def exit_reference(seed, variant=0):
    return exit_rays(case(seed, variant), aux=trace(seed, variant))


def mirrored(sc, aux):
    """int64 [P]: interactions of each completed path that were mirrored (hits minus refractions; 0 on the other rows).  Recomputed
    from the tape with the restatement's own ``interact``."""
    V, F = vertices(sc), torch.as_tensor(sc["mesh"].faces, dtype=torch.long)
    vi = torch.nonzero(aux["valid"]).squeeze(1)
    o, d, n_hits = sc["o"][vi], sc["d"][vi], aux["hits"][vi]
    count = torch.zeros(len(vi), dtype=torch.long)
    for k in range(sc["k"]):
        sel = torch.nonzero(n_hits > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, flag = snell_ref.interact(o[sel], d[sel], V[F[aux["tape"][k, vi[sel]]]], sc["ior_int"], sc["ior_ext"], sc["refraction"])
        o, d = o.index_put((sel,), no), d.index_put((sel,), nd)
        count[sel] += flag.long()
    out = torch.zeros(sc["n"], dtype=torch.long)
    out[vi] = count
    return out


def coverage(sc, aux, ref):
    """What a case contributes to the list's coverage, from the restatement's trace alone."""
    P, k = sc["n"], sc["k"]
    recorded = (aux["tape"] >= 0).sum(0)                       # interactions on the tape, completed or not
    dead = torch.logical_not(aux["valid"])
    # a ray whose path was ended by TIR under drop: its last recorded interaction is a TIR hit (the path stops there, nothing follows it)
    # -- told from exhaustion (K recorded, the continuation still hits) and from a leave after an odd count by recomputing that last hit
    tir_ended = 0
    if sc["tir"] == "drop":
        cand = torch.nonzero(dead & (recorded > 0)).squeeze(1)
        tir_ended = int(_ends_in_tir(sc, aux, cand, recorded).sum())
    exhausted = int(_exhausted(sc, aux, recorded).sum())
    inside = _camera_inside(sc)
    mir = mirrored(sc, aux) if sc["tir"] == "reflect" else torch.zeros(P, dtype=torch.long)
    return dict(seed=sc["seed"], faces=len(sc["mesh"].faces), two=two_components(sc), ior_int=sc["ior_int"], ior_ext=sc["ior_ext"], k=k, tir=sc["tir"],
                refraction=sc["refraction"], size=(sc["height"], sc["width"]), distance=sc["distance"], inside=inside, rays=P,
                valid=int(aux["valid"].sum()), count=ref["count"], max_hits=int(aux["hits"].max()) if P else 0,
                full_k=int((aux["hits"] == k).sum()), max_mirrored=int(mir.max()), tir_ended=tir_ended, exhausted=exhausted)


def _replay(sc, aux, rows, upto):
    """(o, d) of ``rows`` after ``upto[r]`` interactions of their tape, under the case's law (mirrored where the flag says so)."""
    V, F = vertices(sc), torch.as_tensor(sc["mesh"].faces, dtype=torch.long)
    o, d = sc["o"][rows].clone(), sc["d"][rows].clone()
    for k in range(sc["k"]):
        sel = torch.nonzero(upto > k).squeeze(1)
        if len(sel) == 0:
            break
        no, nd, _ = snell_ref.interact(o[sel], d[sel], V[F[aux["tape"][k, rows[sel]]]], sc["ior_int"], sc["ior_ext"], sc["refraction"])
        o[sel], d[sel] = no, nd
    return o, d


def _ends_in_tir(sc, aux, rows, recorded):
    """bool [len(rows)]: the last recorded interaction of each row carries the TIR flag."""
    if len(rows) == 0:
        return torch.zeros(0, dtype=torch.bool)
    V, F = vertices(sc), torch.as_tensor(sc["mesh"].faces, dtype=torch.long)
    last = recorded[rows] - 1
    o, d = _replay(sc, aux, rows, last)
    _, _, _, _, flag = snell_ref._frame(o, d, V[F[aux["tape"][last, rows]]], sc["ior_int"], sc["ior_ext"])
    return flag


def _exhausted(sc, aux, recorded):
    """bool [P]: K interactions recorded, none ended the path, and the continuation still hits (invalid by exhaustion)."""
    from oracle import diffrender_oracle as orc
    out = torch.zeros(sc["n"], dtype=torch.bool)
    rows = torch.nonzero(torch.logical_not(aux["valid"]) & (recorded == sc["k"])).squeeze(1)
    if len(rows) == 0:
        return out
    if sc["tir"] == "drop":
        rows = rows[torch.logical_not(_ends_in_tir(sc, aux, rows, recorded))]
        if len(rows) == 0:
            return out
    o, d = _replay(sc, aux, rows, recorded[rows])
    _, hitted = orc.intersect_ids(orc.Mesh(sc["mesh"].faces, vertices(sc)), o, d)
    out[rows[hitted]] = True
    return out


def _camera_inside(sc):
    """Whether the camera's eye is inside the body: a ray from it along +x crosses the surface an odd number of times (chained
    ``intersect_ids``; closed shapes)."""
    from oracle import diffrender_oracle as orc
    mesh = orc.Mesh(sc["mesh"].faces, vertices(sc))
    votes = 0
    for axis in np.eye(3):
        o, d, n = torch.tensor(sc["eye"]).view(1, 3), torch.tensor(axis).view(1, 3), 0
        for _ in range(64):
            ids, hitted = orc.intersect_ids(mesh, o, d)
            if not bool(hitted[0]):
                break
            tri = mesh.vertices[mesh.faces[ids[hitted]]]
            _, _, t, _ = orc.moller_trumbore(o, d, tri)
            o, n = o + (t.view(-1, 1) + 1e-6) * d, n + 1
        votes += n % 2
    return votes >= 2
