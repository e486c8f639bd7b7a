"""GPU: the visual hull (drt_amd/csrc/drt_hull.hip: k_hull_field, k_hull_mark, k_hull_emit; drt_amd/visual_hull.py).

The three C-ABI stages against the numpy restatement tests/hull_ref.py with tolerance 0 -- derived, not measured: the kernels and the
restatement perform the same correctly rounded IEEE-754 operations in the same order (the library is built with -ffp-contract=off; the
division and the conversions of gfx950 are correctly rounded), the prefix sums are integer, nothing is accumulated atomically.

End to end on a synthetic capture of hand_vh.ply (128 x 128, 72 views, 64^3 grid over centre +- 0.6 extent).  The raw hull traced with
Scene.render_mask through the capture's own rays checks the projection convention against generate_ray.  Measured on the CPU with
hull_ref and the oracle's tracer on the same cameras (DESIGN.md section 10 quotes the figures): min IoU CPU_MIN_IOU, largest share of hull
pixels outside a mask CPU_MAX_OUTSIDE."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hull_cases
import hull_ref
from conftest import ROOT, data_path
from drt_amd import _lib
from oracle import remesh_oracle

pytestmark = pytest.mark.gpu

CPU_MIN_IOU = 0.9390        # hull_ref + the oracle tracer, 72 views of 128 x 128, 64^3: min over the views (mean 0.9547; at most 83 of ~1260 mask pixels missed)
CPU_MAX_OUTSIDE = 0.0       # no hull pixel outside its mask in any view

CASES = hull_cases.host_cases() + [("hand70", lambda: hull_cases.hand(70))]         # 70 views: more than one LDS chunk of 64


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def abi_hull(case):
    """The three stages through the C ABI, with torch's cumsum between the second and the third."""
    lib = _lib.lib()
    dev = torch.device("cuda")
    masks, P = torch.tensor(case["masks"], device=dev), torch.tensor(case["P"], device=dev)
    lo, h, (nx, ny, nz), level = case["lo"], float(case["h"]), case["dims"], case["level"]
    n, H, W = masks.shape
    field = torch.full(case["dims"], float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.drt_hull_field(masks.data_ptr(), n, H, W, P.data_ptr(), lo[0], lo[1], lo[2], h, nx, ny, nz, int(case["outside"] == "keep"),
                                  field.data_ptr(), _stream()))
    N = nx * ny * nz
    emask, n_vert, n_tri = (torch.full((N,), 255, dtype=torch.uint8, device=dev) for _ in range(3))
    _lib.check(lib.drt_hull_mark(field.data_ptr(), nx, ny, nz, level, emask.data_ptr(), n_vert.data_ptr(), n_tri.data_ptr(), _stream()))
    v_inc, t_inc = torch.cumsum(n_vert, 0, dtype=torch.int32), torch.cumsum(n_tri, 0, dtype=torch.int32)
    nv, nf = int(v_inc[-1]), int(t_inc[-1])
    V = torch.full((nv + 1, 3), float("nan"), dtype=torch.float64, device=dev)          # one guard row each: nothing is written beyond the totals
    F = torch.full((nf + 1, 3), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.drt_hull_emit(field.data_ptr(), nx, ny, nz, lo[0], lo[1], lo[2], h, level, emask.data_ptr(), v_inc.data_ptr(), t_inc.data_ptr(),
                                 nv, nf, V.data_ptr(), F.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(V[nv]).all() and (F[nf] == -7).all()
    assert int((emask != 0).sum()) > 0 and int(n_vert.max()) <= 7 and int(n_tri.max()) <= 12
    return field, V[:nv], F[:nf]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,make", CASES, ids=[n for n, _ in CASES])
def test_abi_stages_equal_the_restatement(name, make):
    case = make()
    field, V, F = abi_hull(case)
    assert np.array_equal(field.cpu().numpy(), case["field"])
    assert len(case["F"]) > 0 and np.array_equal(F.cpu().numpy(), case["F"])
    assert same_bits(V.cpu().numpy(), case["V"])


def test_python_layer_equals_the_abi_and_two_runs_agree():
    from drt_amd import visual_hull
    case = hull_cases.hand()
    runs = []
    for _ in range(2):
        f = visual_hull.silhouette_field(case["masks"], case["P"], case["lo"], case["h"], case["dims"])
        V, F = visual_hull.extract_surface(f, case["lo"], case["h"], case["level"])
        runs.append((f, V, F))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], abi_hull(case)))
    assert runs[0][2].dtype == torch.int32 and runs[0][1].dtype == torch.float64 and runs[0][0].dtype == torch.float32


def test_empty_hull_is_an_error_that_names_the_causes():
    from drt_amd import visual_hull
    case = hull_cases.hand()
    f = visual_hull.silhouette_field(np.zeros_like(case["masks"]), case["P"], case["lo"], case["h"], case["dims"])
    assert float(f.max()) == 0.0
    with pytest.raises(ValueError, match="bounds.*polarity.*projection"):
        visual_hull.extract_surface(f, case["lo"], case["h"])


def test_abi_argument_checks():
    lib = _lib.lib()
    dev = torch.device("cuda")
    m = torch.ones((2, 8, 8), dtype=torch.uint8, device=dev)
    P = torch.zeros((2, 3, 4), dtype=torch.float64, device=dev)
    f = torch.zeros((5, 5, 5), dtype=torch.float32, device=dev)
    b = torch.zeros(125, dtype=torch.uint8, device=dev)
    i32 = torch.zeros(125, dtype=torch.int32, device=dev)
    V = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    F = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    s = _stream()

    def field(**kw):
        a = dict(masks=m.data_ptr(), n=2, H=8, W=8, P=P.data_ptr(), lx=0.0, ly=0.0, lz=0.0, cell=1.0, nx=5, ny=5, nz=5, keep=0, out=f.data_ptr())
        a.update(kw)
        return lib.drt_hull_field(*a.values(), s)

    def mark(**kw):
        a = dict(f=f.data_ptr(), nx=5, ny=5, nz=5, level=0.5, em=b.data_ptr(), nv=b.data_ptr(), nt=b.data_ptr())
        a.update(kw)
        return lib.drt_hull_mark(*a.values(), s)

    def emit(**kw):
        a = dict(f=f.data_ptr(), nx=5, ny=5, nz=5, lx=0.0, ly=0.0, lz=0.0, cell=1.0, level=0.5, em=b.data_ptr(), vi=i32.data_ptr(), ti=i32.data_ptr(),
                 n_verts=4, n_faces=4, V=V.data_ptr(), F=F.data_ptr())
        a.update(kw)
        return lib.drt_hull_emit(*a.values(), s)

    def rejected(rc, word):
        assert rc == -1, (rc, word)
        assert word in lib.drt_last_error().decode(), (word, lib.drt_last_error())

    assert field() == 0 and mark() == 0 and emit() == 0
    rejected(field(masks=None), "d_masks")
    rejected(field(P=None), "d_proj")
    rejected(field(out=None), "d_field")
    rejected(field(n=0), "n_views")
    rejected(field(H=1), "height")
    rejected(field(W=1), "width")
    rejected(field(cell=0.0), "cell")
    rejected(field(cell=float("nan")), "cell")
    rejected(field(lx=float("inf")), "lo")
    rejected(field(nx=2), "nx")
    rejected(field(ny=1025), "ny")
    rejected(field(nz=0), "nz")
    rejected(field(keep=2), "keep_outside")
    rejected(mark(f=None), "d_field")
    rejected(mark(em=None), "d_edge_mask")
    rejected(mark(nv=None), "d_n_vert")
    rejected(mark(nt=None), "d_n_tri")
    rejected(mark(level=0.0), "level")
    rejected(mark(level=1.0), "level")
    rejected(mark(nx=2), "nx")
    rejected(emit(f=None), "d_field")
    rejected(emit(em=None), "d_edge_mask")
    rejected(emit(vi=None), "d_v_inc")
    rejected(emit(ti=None), "d_t_inc")
    rejected(emit(V=None), "d_verts")
    rejected(emit(F=None), "d_faces")
    rejected(emit(n_verts=-1), "n_verts")
    rejected(emit(n_faces=1 << 31), "n_faces")
    rejected(emit(level=float("nan")), "level")
    rejected(emit(cell=-1.0), "cell")
    torch.cuda.synchronize()
    assert lib.drt_version() >= 7


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
RES, N_VIEWS, GRID = 128, 72, 64


@pytest.fixture(scope="module")
def capture():
    from drt_amd import captured_data, diffrender as Render, views, visual_hull
    Render.resx = Render.resy = RES
    gt = Render.Scene(data_path("hand_vh.ply"), 0)
    center, extent = views.mesh_frame(gt.mesh.vertices)
    data = captured_data.SyntheticData(gt, center, extent, RES, RES, num_view=N_VIEWS, n_total=N_VIEWS, name="hand")
    bounds = (center - 0.6 * extent, center + 0.6 * extent)
    report = {}
    mesh, V_raw, F_raw = visual_hull.visual_hull(data, resolution=GRID, bounds=bounds, return_raw=True, report=report)
    return dict(data=data, bounds=bounds, mesh=mesh, V_raw=V_raw, F_raw=F_raw, report=report, extent=extent)


def test_end_to_end_raw_hull_equals_the_restatement(capture):
    from drt_amd import visual_hull
    masks, P = visual_hull.capture_masks(capture["data"])
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N_VIEWS, RES, RES) and P.shape == (N_VIEWS, 3, 4)
    lo, hi = capture["bounds"]
    cell = float((hi - lo).max()) / (GRID - 1)
    glo, gcell, gdims = visual_hull.hull_grid(capture["bounds"], GRID)
    assert gdims == (GRID,) * 3 and gcell == cell and np.array_equal(glo, lo)
    f = hull_ref.field(masks.cpu().numpy(), P, lo, cell, gdims)
    V, F = hull_ref.surface(f, lo, cell, 0.5)
    assert np.array_equal(capture["F_raw"].cpu().numpy(), F) and same_bits(capture["V_raw"].cpu().numpy(), V)


def test_end_to_end_result_is_a_remeshed_manifold(capture):
    mesh, rep = capture["mesh"], capture["report"]
    topo = remesh_oracle.topology(mesh.vertices, mesh.faces)
    assert topo["ok"] and topo["components"] == 1, {k: v for k, v in topo.items() if k != "valence"}
    L = 1.2 * capture["extent"] / 32
    assert abs(rep["target_len"] - L) <= 1e-12 * L
    assert np.array_equal(mesh.vertices, mesh.vertices.astype(np.float32).astype(np.float64))
    r, bad = remesh_oracle.check(capture["V_raw"].cpu().numpy(), capture["F_raw"].cpu().numpy(), mesh.vertices, mesh.faces, L, max_samples=300)
    print(json.dumps({k: v for k, v in r.items() if k != "topology"}))
    assert not bad, bad
    assert rep["faces"] == len(mesh.faces) and rep["components_kept"] == 1 and rep["genus"] == topo["genus_sum"]
    assert set(rep["seconds"]) >= {"bounds", "field", "surface", "components", "remesh"}


def test_end_to_end_silhouettes_match_the_capture(capture):
    from drt_amd import mesh_io, visual_hull
    raw = mesh_io.TriMesh(capture["V_raw"].cpu().numpy(), capture["F_raw"].cpu().numpy())
    iou, outside = visual_hull.silhouette_iou(raw, capture["data"])
    print(f"raw hull: IoU min {iou.min():.4f} mean {iou.mean():.4f}; largest share of hull pixels outside a mask {outside.max():.5f}")
    assert len(iou) == N_VIEWS
    assert iou.min() >= CPU_MIN_IOU - 0.005
    assert iou.min() >= 0.92
    assert outside.max() <= 0.01


def test_auto_bounds_contain_the_object(capture):
    from drt_amd import visual_hull
    masks, P = visual_hull.capture_masks(capture["data"])
    lo, hi = visual_hull.auto_bounds(masks, P)
    V = capture["V_raw"].cpu().numpy()
    assert (lo <= V.min(0)).all() and (hi >= V.max(0)).all()
    assert (hi - lo).max() <= 2.0 * capture["extent"]              # and the box is not the whole scene


def test_reconstruct_hull_from_capture(tmp_path):
    cmd = [sys.executable, "-m", "drt_amd.reconstruct", "--name", "hand", "--res", "128", "--views", "72", "--num-view", "8", "--passes", "2",
           "--iters", "5", "--hull-from-capture", "64", "--data-path", data_path(""), "--result-path", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rep = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")][-1]
    assert rep["hull_source"] == "capture" and rep["iterations"] == 10
    assert rep["hull"]["dims"] and max(rep["hull"]["dims"]) == 64 and rep["hull"]["faces"] == rep["hull_faces"] > 500 and rep["hull"]["views"] == 72
    assert os.path.exists(rep["result"])


def test_cli_writes_a_hull_and_reports_it(tmp_path, capsys):
    from drt_amd import mesh_io, visual_hull
    out = tmp_path / "hand_hull.ply"
    rep = visual_hull.main(["--name", "hand", "--data-path", data_path(""), "--res", "64", "--views", "24", "--resolution", "48", "-o", str(out)])
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1]
    assert line["faces"] == rep["faces"] > 100 and line["output"] == str(out)
    for key in ("faces", "vertices", "components_kept", "components_dropped", "genus", "volume", "bounds", "cell", "iou_min", "iou_mean", "seconds"):
        assert key in line, key
    assert set(line["seconds"]) >= {"bounds", "field", "surface", "components", "remesh", "iou"}
    assert 0.5 < line["iou_min"] <= line["iou_mean"] <= 1.0 and line["volume"] > 0            # auto bounds found the object
    mesh = mesh_io.read_ply(str(out))
    assert len(mesh.faces) == line["faces"] and mesh.is_watertight
    with pytest.raises(SystemExit, match="--force"):
        visual_hull.main(["--name", "hand", "--data-path", data_path(""), "-o", str(out)])
