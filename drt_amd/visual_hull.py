"""The visual hull of a capture's silhouette masks, built on the device: what ``data/<name>_vh.ply`` is for a capture of one's own.

    python -m drt_amd.visual_hull --name horse [--capture FILE] [--resolution N] [--level X] [--target-len L] [--keep largest|all] [-o PATH] [--force]

The reference ships nine precomputed hulls and no code that made them.  Here the capture's own datasets (``mask``, ``cam_proj``,
``cam_k``) give one:

    silhouette_field   every corner of a dense grid is projected into every view with P = K R[:3, :]; its value is the minimum over the
                       views of the bilinear sample of the binary mask (k_hull_field)
    extract_surface    marching tetrahedra on the Kuhn subdivision of the cells: a closed oriented manifold by construction
                       (k_hull_mark, two prefix sums, k_hull_emit; no sort, no atomics: bit-reproducible)
    visual_hull        field -> surface -> component selection -> isotropic remesh to the edge length the loop expects

The law is stated once, in csrc/drt_hull.h (and DESIGN.md section 10); tests/hull_ref.py restates it in numpy and the device agrees
with it bit for bit.  There is no CPU fallback: the kernels are the implementation."""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from . import _lib, mesh_io

MIN_DIM, MAX_DIM = 3, 1024
EMPTY_HINT = ("nothing is inside the hull: check the bounds (does the box contain the object?), the mask polarity (nonzero = object) and the "
              "projection convention (P = K @ R[:3, :], world -> camera R, pixel centres at integer coordinates)")


# ---- argument checks (before anything touches the device) ----------------------------------------------------------------------------
def _check_grid(lo, cell, dims):
    lo = np.asarray(lo, dtype=np.float64)
    if lo.shape != (3,) or not np.isfinite(lo).all():
        raise ValueError(f"lo must be three finite numbers, got {lo!r}")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite, got {cell!r}")
    try:
        dims = tuple(int(d) for d in dims)
    except TypeError:
        raise ValueError(f"dims must be three corner counts, got {dims!r}") from None
    if len(dims) != 3 or not all(MIN_DIM <= d <= MAX_DIM for d in dims):
        raise ValueError(f"dims must be three corner counts in [{MIN_DIM}, {MAX_DIM}], got {dims!r}")
    return lo, cell, dims


def _check_level(level):
    level = float(np.float32(level))
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie inside (0, 1), got {level!r}")
    return level


def _check_outside(outside):
    if outside not in ("carve", "keep"):
        raise ValueError(f"outside must be 'carve' or 'keep', got {outside!r}")
    return int(outside == "keep")


def _check_views(masks, P):
    if not (isinstance(masks, (np.ndarray, torch.Tensor)) and masks.ndim == 3 and str(masks.dtype).endswith("uint8")):
        raise ValueError(f"masks must be a uint8 array [n, H, W], got {getattr(masks, 'dtype', type(masks))} {tuple(getattr(masks, 'shape', ()))}")
    n, H, W = (int(s) for s in masks.shape)
    if n < 1 or H < 2 or W < 2:
        raise ValueError(f"masks must hold at least one view of at least 2 x 2 pixels, got {(n, H, W)}")
    P = np.ascontiguousarray(P.detach().cpu().numpy() if isinstance(P, torch.Tensor) else P, dtype=np.float64)
    if P.shape != (n, 3, 4):
        raise ValueError(f"P must be float64 [{n}, 3, 4] (K @ R[:3, :] of every view), got {P.shape}")
    return P


def _device(t=None):
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    from .optix_mesh import _stream as s
    return s()


# ---- the two device stages -----------------------------------------------------------------------------------------------------------
def silhouette_field(masks, P, lo, cell, dims, outside="carve"):
    """float32 [nx, ny, nz] on the device.  ``masks`` uint8 [n, H, W] (nonzero = object; numpy or a device tensor), ``P`` float64
    [n, 3, 4] = K @ R[:3, :] formed on the host, corner (i, j, k) at ``lo + cell * (i, j, k)``.  Per corner: the minimum over the views
    of the bilinear mask sample at its projection; a view that does not see the corner contributes 0 (``outside="carve"``) or is
    skipped (``"keep"``); corners on the grid's boundary planes are 0."""
    P = _check_views(masks, P)
    lo, cell, dims = _check_grid(lo, cell, dims)
    keep = _check_outside(outside)
    dev = _device(masks)
    with torch.cuda.device(dev):
        m = torch.as_tensor(masks, device=dev).contiguous()
        proj = torch.as_tensor(P, device=dev)
        field = torch.empty(dims, dtype=torch.float32, device=dev)
        n, H, W = m.shape
        _lib.check(_lib.lib().drt_hull_field(m.data_ptr(), n, H, W, proj.data_ptr(), lo[0], lo[1], lo[2], cell, dims[0], dims[1], dims[2], keep,
                                             field.data_ptr(), _stream()))
    return field


def extract_surface(field, lo, cell, level=0.5):
    """(V float64 [nv, 3], F int32 [nf, 3]) on the device: marching tetrahedra of ``field > level`` on the Kuhn subdivision, normals
    outward.  Raises ValueError when nothing is inside."""
    if not (isinstance(field, (np.ndarray, torch.Tensor)) and field.ndim == 3 and str(field.dtype).endswith("float32")):
        raise ValueError(f"field must be a float32 array [nx, ny, nz], got {getattr(field, 'dtype', type(field))} {tuple(getattr(field, 'shape', ()))}")
    lo, cell, dims = _check_grid(lo, cell, field.shape)
    level = _check_level(level)
    dev = _device(field)
    with torch.cuda.device(dev):
        f = torch.as_tensor(field, device=dev).contiguous()
        n = f.numel()
        edge_mask, n_vert, n_tri = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
        lib = _lib.lib()
        _lib.check(lib.drt_hull_mark(f.data_ptr(), dims[0], dims[1], dims[2], level, edge_mask.data_ptr(), n_vert.data_ptr(), n_tri.data_ptr(), _stream()))
        v_inc = torch.cumsum(n_vert, 0, dtype=torch.int32)
        t_inc = torch.cumsum(n_tri, 0, dtype=torch.int32)
        del n_vert, n_tri
        nv, nf = torch.stack([v_inc[-1], t_inc[-1]]).tolist()                 # the one read-back: the sizes of the two outputs
        if nv < 0 or nf < 0:
            raise ValueError("field: the surface has more than 2^31 vertices or triangles")
        if nf == 0:
            raise ValueError("field: " + EMPTY_HINT)
        V = torch.empty((nv, 3), dtype=torch.float64, device=dev)
        F = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.drt_hull_emit(f.data_ptr(), dims[0], dims[1], dims[2], lo[0], lo[1], lo[2], cell, level, edge_mask.data_ptr(), v_inc.data_ptr(),
                                     t_inc.data_ptr(), nv, nf, V.data_ptr(), F.data_ptr(), _stream()))
    return V, F


# ---- from a capture --------------------------------------------------------------------------------------------------------------
def _view_ids(data, view_ids):
    if view_ids is None:
        return sorted(data.Views.keys()) if isinstance(data.Views, dict) else list(range(len(data.Views)))
    return [int(v) for v in view_ids]


def capture_masks(data, view_ids=None):
    """(masks uint8 [n, resy, resx] on the device, P float64 numpy [n, 3, 4]) of a capture's views, from ``Data.get_view``.

    The data classes keep only the SOFT mask of ``views.process_mask``, whose values are exactly 1 inside the object, 0.5 on the
    one-pixel ring just outside it and on the image's last row, and 0 beyond.  The binary mask is ``soft > 0.75``: the object's own
    pixels (so the last row is never object).  ``P = K @ R[:3, :]`` from ``camera_M``'s R and K, formed on the host in float64."""
    ids = _view_ids(data, view_ids)
    masks, P = [], []
    for k in ids:
        view = data.get_view(k)
        soft, (R, K) = view[2], view[5][:2]
        masks.append((soft.reshape(data.resy, data.resx) > 0.75).to(torch.uint8))
        P.append(K.detach().cpu().numpy().astype(np.float64) @ R.detach().cpu().numpy().astype(np.float64)[:3, :])
    return torch.stack(masks).contiguous(), np.stack(P)


def auto_bounds(masks, P, level=0.5, outside="carve"):
    """(lo, hi) of a box around the hull.  Centre: the point closest (least squares) to the rays through the mask centroids.  Radius:
    the farthest corner of a mask's bounding box, back-projected to the centre's depth in its view.  Then one 32^3 pass of the field
    kernel over that cube; the box of its occupied corners, padded by two coarse cells, is the answer."""
    P = _check_views(masks, P)
    m = torch.as_tensor(masks)
    n, H, W = m.shape
    rows = (m != 0).any(2).cpu().numpy()
    cols = (m != 0).any(1).cpu().numpy()
    ys = torch.arange(H, dtype=torch.float64, device=m.device)
    xs = torch.arange(W, dtype=torch.float64, device=m.device)
    cnt = (m != 0).sum((1, 2)).to(torch.float64)
    cu = (((m != 0).sum(1).to(torch.float64) * xs).sum(1) / cnt.clamp(min=1)).cpu().numpy()
    cw = (((m != 0).sum(2).to(torch.float64) * ys).sum(1) / cnt.clamp(min=1)).cpu().numpy()
    used = np.nonzero(cnt.cpu().numpy() > 0)[0]
    if len(used) == 0:
        raise ValueError("masks: every mask is empty; " + EMPTY_HINT)
    A, b, Minv, eye = np.zeros((3, 3)), np.zeros(3), {}, {}
    for v in used:
        Minv[v] = np.linalg.inv(P[v][:, :3])
        eye[v] = -Minv[v] @ P[v][:, 3]
        d = Minv[v] @ np.array([cu[v], cw[v], 1.0])
        d /= np.linalg.norm(d)
        T = np.eye(3) - np.outer(d, d)
        A += T
        b += T @ eye[v]
    centre = np.linalg.lstsq(A, b, rcond=None)[0]
    radius = 0.0
    for v in used:
        depth = float(P[v][2] @ np.append(centre, 1.0))
        if depth <= 0:
            continue
        r, c = np.nonzero(rows[v])[0], np.nonzero(cols[v])[0]
        for pw in (r[0], r[-1]):
            for pu in (c[0], c[-1]):
                X = Minv[v] @ (depth * np.array([pu, pw, 1.0]) - P[v][:, 3])
                radius = max(radius, float(np.linalg.norm(X - centre)))
    if not radius > 0:
        raise ValueError("masks: no view sees the point its centroid rays meet at; " + EMPTY_HINT)
    coarse = 32
    cell = 2.0 * radius / (coarse - 1)
    lo = centre - radius
    occ = silhouette_field(masks, P, lo, cell, (coarse,) * 3, outside) > _check_level(level)
    if not bool(occ.any()):
        raise ValueError("masks: " + EMPTY_HINT)
    idx = torch.nonzero(occ)
    i0, i1 = idx.min(0).values.cpu().numpy(), idx.max(0).values.cpu().numpy()
    return lo + cell * (i0 - 2.0), lo + cell * (i1 + 2.0)


def hull_grid(bounds, resolution):
    """(lo, cell, dims) of the grid ``visual_hull`` lays over ``bounds = (lo, hi)``: cubic cells, ``resolution`` corners along the longest side."""
    try:
        lo, hi = (np.asarray(b, dtype=np.float64) for b in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be (lo, hi), two points, got {bounds!r}") from None
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"bounds must be (lo, hi) with hi > lo on every axis, got {bounds!r}")
    cell = float((hi - lo).max()) / (resolution - 1)
    dims = tuple(int(min(resolution, max(MIN_DIM, np.ceil(s / cell - 1e-9) + 1))) for s in (hi - lo))
    return lo, cell, dims


def _components(F, n_vertices):
    """Component label of every face (host; scipy is already what views.process_mask uses)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a, b = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n_vertices, n_vertices))
    n, label = connected_components(g, directed=False)
    return n, label[F[:, 0]]


def _signed_volumes(V, F, label, n):
    t = V[F]
    six = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2]))
    return np.bincount(label, weights=six, minlength=n) / 6.0


def _check_keywords(resolution, level, target_len, keep, bounds, view_ids, outside):
    if not (isinstance(resolution, (int, np.integer)) and MIN_DIM <= resolution <= MAX_DIM):
        raise ValueError(f"resolution must be an integer in [{MIN_DIM}, {MAX_DIM}], got {resolution!r}")
    try:
        _check_level(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must lie inside (0, 1), got {level!r}") from None
    if target_len is not None and not (isinstance(target_len, (int, float)) and target_len > 0 and np.isfinite(target_len)):
        raise ValueError(f"target_len must be a positive length or None, got {target_len!r}")
    if keep not in ("largest", "all"):
        raise ValueError(f"keep must be 'largest' or 'all', got {keep!r}")
    _check_outside(outside)
    if bounds is not None:
        hull_grid(bounds, resolution)
    if view_ids is not None and len(list(view_ids)) == 0:
        raise ValueError("view_ids must name at least one view")


def visual_hull(data, resolution=256, level=0.5, target_len=None, keep="largest", bounds=None, view_ids=None, outside="carve", return_raw=False,
                report=None):
    """The visual hull of a capture (``captured_data.Data``) as a ``mesh_io.TriMesh`` ready for ``Scene``.

    ``resolution``: corners along the longest side of ``bounds`` (default ``auto_bounds``), cubic cells.  ``keep="largest"`` keeps the
    component of the largest |signed volume| (``"all"``: every one).  The surface is remeshed on the device (``isotropic_remesh_gpu``
    against the raw hull) to ``target_len`` (default: longest side / 32) and the positions are rounded through float32, as
    ``GpuMeshlabserver`` does.  ``return_raw=True``: ``(mesh, V_raw, F_raw)`` with the extraction's output (device tensors) as well.
    ``report``: a dict that receives sizes, bounds and seconds per stage."""
    _check_keywords(resolution, level, target_len, keep, bounds, view_ids, outside)
    from .optix_mesh import optix_mesh
    from .remesh_gpu import isotropic_remesh_gpu
    rep = {} if report is None else report
    clock = _Clock(rep)
    masks, P = capture_masks(data, view_ids)
    if bounds is None:
        bounds = auto_bounds(masks, P, level, outside)
    lo, cell, dims = hull_grid(bounds, int(resolution))
    clock("bounds")
    field = silhouette_field(masks, P, lo, cell, dims, outside)
    clock("field")
    V_raw, F_raw = extract_surface(field, lo, cell, level)
    del field
    clock("surface")
    Vh, Fh = V_raw.cpu().numpy(), F_raw.cpu().numpy().astype(np.int64)
    n_comp, label = _components(Fh, len(Vh))
    vol = _signed_volumes(Vh, Fh, label, n_comp)
    if keep == "largest" and n_comp > 1:
        sel = label == int(np.argmax(np.abs(vol)))
        used = np.unique(Fh[sel])
        remap = np.full(len(Vh), -1, np.int64)
        remap[used] = np.arange(len(used))
        Vh, Fh, kept = Vh[used], remap[Fh[sel]], 1
    else:
        kept = n_comp
    clock("components")
    dev = V_raw.device
    side = float(max(np.asarray(bounds[1], np.float64) - np.asarray(bounds[0], np.float64)))
    L = float(target_len) if target_len is not None else side / 32.0
    with torch.cuda.device(dev):
        Vd, Fd = torch.as_tensor(Vh, device=dev), torch.as_tensor(Fh, device=dev)
        surface = optix_mesh(dev.index)
        surface.update_mesh(Fd.to(torch.int32), Vd.to(torch.float32))
        Vr, Fr = isotropic_remesh_gpu(Vd, Fd, L, surface=surface)
        Vr = Vr.to(torch.float32).to(torch.float64)
    mesh = mesh_io.TriMesh(Vr.cpu().numpy(), Fr.cpu().numpy())
    clock("remesh")
    chi = len(mesh.vertices) - 3 * len(mesh.faces) // 2 + len(mesh.faces)
    rep.update(faces=int(len(mesh.faces)), vertices=int(len(mesh.vertices)), raw_faces=int(F_raw.shape[0]), raw_vertices=int(V_raw.shape[0]),
               components_kept=int(kept), components_dropped=int(n_comp - kept), genus=int((2 * kept - chi) // 2),
               volume=float(_signed_volumes(mesh.vertices, mesh.faces, np.zeros(len(mesh.faces), np.int64), 1)[0]),
               bounds=[np.asarray(bounds[0], np.float64).tolist(), np.asarray(bounds[1], np.float64).tolist()], cell=cell, dims=list(dims),
               target_len=L, views=int(masks.shape[0]))
    return (mesh, V_raw, F_raw) if return_raw else mesh


class _Clock:
    """Seconds per stage into report["seconds"] (the device is synchronised at every mark)."""

    def __init__(self, report):
        self.seconds = report.setdefault("seconds", {})
        self.t = time.perf_counter()

    def __call__(self, stage):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.seconds[stage] = now - self.t
        self.t = now


def silhouette_iou(mesh, data, view_ids=None, device=0):
    """(IoU, share of the hull's pixels that lie outside the mask) per view: ``Scene.render_mask`` of ``mesh`` through the capture's own
    rays against the binary masks of ``capture_masks``."""
    from . import diffrender as Render
    scene = mesh if isinstance(mesh, Render.Scene) else Render.Scene(mesh, device)
    ids = _view_ids(data, view_ids)
    masks, _ = capture_masks(data, ids)
    iou, extra = [], []
    for m, k in zip(masks, ids):
        view = data.get_view(k)
        hit = scene.render_mask(view[3], view[4]).reshape(m.shape) > 0
        ref = m != 0
        inter, union = (hit & ref).sum(), (hit | ref).sum()
        iou.append(float(inter) / max(1.0, float(union)))
        extra.append(float((hit & ~ref).sum()) / max(1.0, float(ref.sum())))
    return np.array(iou), np.array(extra)


# ---- command line --------------------------------------------------------------------------------------------------------------------
def default_output(name, data_path):
    """Where the CLI writes without -o: never one of the shipped ``<name>_vh.ply``."""
    return os.path.join(data_path, f"{name}_hull.ply")


def main(argv=None):
    from . import optim
    ap = argparse.ArgumentParser(description="Build the visual hull of a capture's silhouette masks on the device and write it as a PLY.")
    ap.add_argument("--name", default=optim.HyperParams["name"])
    ap.add_argument("--data-path", default="./data/")
    ap.add_argument("--capture", default=None, help=".npz / .h5 capture with the reference's datasets (default: a synthetic capture of "
                    "<name>_scan.ply, or of the shipped hull without a scan)")
    ap.add_argument("--resolution", type=int, default=256, help="grid corners along the longest side of the bounds")
    ap.add_argument("--level", type=float, default=0.5)
    ap.add_argument("--target-len", type=float, default=None, help="edge length of the remeshed hull (default: longest side / 32)")
    ap.add_argument("--keep", choices=("largest", "all"), default="largest")
    ap.add_argument("--outside", choices=("carve", "keep"), default="carve", help="what a view that does not see a grid corner does to it")
    ap.add_argument("--res", type=int, default=256, help="resolution of the synthetic capture")
    ap.add_argument("--views", type=int, default=72, help="views of the synthetic capture")
    ap.add_argument("-o", "--output", default=None, help="default: <data-path>/<name>_hull.ply (never the shipped <name>_vh.ply)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    a = ap.parse_args(argv)
    out = a.output or default_output(a.name, a.data_path)
    if os.path.exists(out) and not a.force:
        raise SystemExit(f"{out} exists: pass --force to overwrite it")
    from . import captured_data, diffrender as Render, views
    if a.capture is not None:
        data = captured_data.get_data(dict(optim.HyperParams, name=a.name), path=a.capture)
    else:
        scan = os.path.join(a.data_path, f"{a.name}_scan.ply")
        gt = Render.Scene(scan if os.path.exists(scan) else os.path.join(a.data_path, f"{a.name}_vh.ply"), 0)
        Render.resx = Render.resy = a.res
        center, extent = views.mesh_frame(gt.mesh.vertices)
        data = captured_data.SyntheticData(gt, center, extent, a.res, a.res, num_view=a.views, n_total=a.views, name=a.name)
    report = {"name": a.name}
    mesh = visual_hull(data, a.resolution, a.level, a.target_len, a.keep, outside=a.outside, report=report)
    t0 = time.perf_counter()
    iou, extra = silhouette_iou(mesh, data)
    report["seconds"]["iou"] = time.perf_counter() - t0
    report.update(iou_min=float(iou.min()), iou_mean=float(iou.mean()), outside_share_max=float(extra.max()), output=out)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    mesh_io.write_ply(out, mesh.vertices, mesh.faces)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
