"""Every kernel of the device remesher (drt_amd/csrc/drt_remesh_gpu.hip) against tests/remesh_ref.py, the float64 host restatement of its
rules: the vertex -> face lists and normals, the split plan, the collapse and flip evaluations, the surface-distance filters, the
closest-point projection, the relaxation target, the roll-back check and the round control -- exactly, bit for bit where the reference
mirrors the operation order.  Then the claim / apply passes: the collapses (flips) one round applies are a set whose sequential
application, in either order, gives the device's mesh, and each of which still passes the evaluation on the mesh just before it.  Then
the input check of isotropic_remesh_gpu and its DEBUG size checks."""
import numpy as np
import pytest
import torch

import remesh_ref as R
from conftest import data_path
from test_remesh_ref import octahedron, padded_quad, valence3_pair

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT_I, SENT_D = -7, -7.25


def _lib():
    from drt_amd import _lib
    return _lib.lib()


def _st():
    from drt_amd.optix_mesh import _stream
    return _stream()


def _ck(rc):
    from drt_amd import _lib
    _lib.check(rc)


def _p(t):
    return None if t is None else t.data_ptr()


_KEEP = []        # every device copy a test makes lives until the test is over: the kernels that read it run asynchronously


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _d(a, dtype=torch.float64):
    t = torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)
    _KEEP.append(t)
    return t


def _bits_equal(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.fixture(scope="module")
def hand():
    from drt_amd import mesh_io
    m = mesh_io.read_ply(data_path("hand_vh.ply"))
    return m.faces.astype(np.int64), m.vertices.astype(np.float64)


@pytest.fixture(scope="module")
def hand_split(hand):
    """hand_vh after one refine pass at L = 4: many edges shorter than 0.8 L, irregular valences."""
    F, V = hand
    _, mid, _ = R.split_plan(F, V, 4.0 * 4.0 / 3.0)
    return R.split_apply(F, V, mid)


def gpu_csr(F, nv, V=None, live=None):
    """drt_rm_vertex_faces -> (vf_start, vf_face, vn or None) as numpy; outputs pre-filled with sentinels."""
    nf = len(F)
    Fd = _d(F, torch.long) if nf else torch.empty((0, 3), dtype=torch.long, device=DEV)
    start = torch.full((nv + 1,), SENT_I, dtype=torch.long, device=DEV)
    vf = torch.full((max(3 * nf, 1),), SENT_I, dtype=torch.long, device=DEV)
    count = torch.empty(nv, dtype=torch.int32, device=DEV)
    Vd = _d(V) if V is not None else None
    vn = torch.full((nv, 3), SENT_D, dtype=torch.float64, device=DEV) if V is not None else None
    _KEEP.extend([Fd, start, vf, count, vn])
    _ck(_lib().drt_rm_vertex_faces(_p(Fd) if nf else None, nf, nv, count.data_ptr(), start.data_ptr(), vf.data_ptr(), _p(Vd), _p(vn), _p(live), _st()))
    out_vf = vf.cpu().numpy()
    return start.cpu().numpy(), out_vf, (vn.cpu().numpy() if vn is not None else None)


def gpu_vertex_normals(F, V, start, vf):
    vn = torch.full((len(V), 3), SENT_D, dtype=torch.float64, device=DEV)
    _ck(_lib().drt_rm_vertex_normals(_d(F, torch.long).data_ptr(), _d(V).data_ptr(), _d(start, torch.long).data_ptr(), _d(vf, torch.long).data_ptr(),
                                     len(V), vn.data_ptr(), _st()))
    return vn.cpu().numpy()


def random_faces(rng, nv, nf, hub=None, n_dead=3):
    """nf random triangles over the first 90 % of nv vertices (the rest unused), three distinct corners each; `hub` takes the first
    corner of 320 faces (~320 faces around it); n_dead rows of -1."""
    used = max(3, int(0.9 * nv))
    a = rng.integers(0, used, nf)
    d1 = rng.integers(1, used - 1, nf)
    d2 = d1 + rng.integers(1, used - d1)                                     # 1 <= d1 < d2 <= used - 1: three distinct corners
    F = np.stack([a, (a + d1) % used, (a + d2) % used], 1)
    if hub is not None:
        F[:320, 0] = hub
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 0] != F[:, 2]) & (F[:, 1] != F[:, 2])]
    F[rng.choice(len(F), min(n_dead, len(F)), replace=False)] = -1
    return F.astype(np.int64)


# ---- vertex -> face lists and normals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 7, 8191, 8192, 8193, 2 * 8192 + 3])
def test_vertex_faces_and_normals(nv):
    rng = np.random.default_rng(nv)
    V = rng.standard_normal((nv, 3)) * 10.0
    if nv == 1:
        F = np.array([[0, 0, 0], [-1, -1, -1]], dtype=np.int64)
    else:
        F = random_faces(rng, nv, 2 * nv, hub=nv // 3 if nv > 1000 else None)
    start, vf = R.vertex_faces(F, nv)
    g_start, g_vf, g_vn = gpu_csr(F, nv, V)
    np.testing.assert_array_equal(g_start, start)
    np.testing.assert_array_equal(g_vf[:len(vf)], vf)
    if nv > 1000:
        assert np.diff(start).max() >= 300                                   # the hub
        assert (np.diff(start) == 0).sum() >= nv // 20                       # unused vertices
    ref = R.vertex_normals(F, V, start, vf)
    assert _bits_equal(g_vn, ref)
    assert _bits_equal(gpu_vertex_normals(F, V, start, vf), ref)


def test_vertex_faces_and_normals_of_monkey_twelve_tiles():
    from drt_amd import mesh_io
    m = mesh_io.read_ply(data_path("monkey_vh.ply"))
    F, V = m.faces.astype(np.int64), m.vertices.astype(np.float64)
    assert len(V) == 92047                                                   # 12 scan tiles of 8192
    F = F.copy()
    F[::997] = -1
    start, vf = R.vertex_faces(F, len(V))
    g_start, g_vf, g_vn = gpu_csr(F, len(V), V)
    np.testing.assert_array_equal(g_start, start)
    np.testing.assert_array_equal(g_vf[:len(vf)], vf)
    assert _bits_equal(g_vn, R.vertex_normals(F, V, start, vf))


def test_vertex_faces_without_faces_and_when_not_live():
    g_start, _, g_vn = gpu_csr(np.zeros((0, 3), dtype=np.int64), 9, np.ones((9, 3)))
    assert (g_start == 0).all() and (g_vn == 0).all()
    F, V = octahedron()
    dead = torch.zeros(8, dtype=torch.int32, device=DEV)                     # ctl[0] = 0: the step's rounds are over
    g_start, g_vf, g_vn = gpu_csr(F, 6, V, live=dead)
    assert (g_start == SENT_I).all() and (g_vf == SENT_I).all() and (g_vn == SENT_D).all()


# ---- split ---------------------------------------------------------------------------------------------------------------------------
def gpu_split(F, V, max_len):
    lib, st = _lib(), _st()
    nf, nv = len(F), len(V)
    Fd, Vd = _d(F, torch.long), _d(V)
    start, vf, _ = gpu_csr(F, nv)
    flag = torch.empty(3 * nf, dtype=torch.uint8, device=DEV)
    _ck(lib.drt_rm_split_mark(Fd.data_ptr(), nf, Vd.data_ptr(), float(max_len), flag.data_ptr(), st))
    rank = torch.cumsum(flag, 0)
    mid = torch.full((3 * nf,), -1, dtype=torch.long, device=DEV)
    count = torch.empty(nf, dtype=torch.long, device=DEV)
    _ck(lib.drt_rm_split_plan(Fd.data_ptr(), nf, _d(start, torch.long).data_ptr(), _d(vf, torch.long).data_ptr(), flag.data_ptr(), rank.data_ptr(), nv,
                              mid.data_ptr(), count.data_ptr(), st))
    offset = torch.cumsum(count, 0) - count
    n_split, n_out = int(rank[-1]), int(count.sum())
    newV = torch.full((nv + n_split, 3), SENT_D, dtype=torch.float64, device=DEV)
    newV[:nv] = Vd
    out = torch.full((n_out, 3), SENT_I, dtype=torch.long, device=DEV)
    _ck(lib.drt_rm_split_faces(Fd.data_ptr(), nf, mid.data_ptr(), newV.data_ptr(), offset.data_ptr(), out.data_ptr(), st))
    return flag.cpu().numpy(), mid.cpu().numpy(), count.cpu().numpy(), out.cpu().numpy(), newV.cpu().numpy()


def _split_cases():
    from drt_amd import mesh_io
    m = mesh_io.read_ply(data_path("hand_vh.ply"))
    iso = ([[0, 1, 2], [0, 2, 1]], [[-1, 0, 0], [0, 2, 0], [1, 0, 0]])          # isosceles: the two diagonals tie
    return [("hand L=4", m.faces, m.vertices, 4.0 * 4 / 3), ("hand L=2", m.faces, m.vertices, 2.0 * 4 / 3),
            ("all three long", iso[0], iso[1], 1.9), ("diagonal tie", iso[0], iso[1], 2.1)]


@pytest.mark.parametrize("case", range(4))
def test_split_plan_and_faces(case):
    name, F, V, max_len = _split_cases()[case]
    F, V = np.asarray(F, dtype=np.int64), np.asarray(V, dtype=np.float64)
    flag, mid, count = R.split_plan(F, V, max_len)
    g_flag, g_mid, g_count, g_out, g_V = gpu_split(F, V, max_len)
    np.testing.assert_array_equal(g_flag, flag, err_msg=name)
    np.testing.assert_array_equal(g_mid, mid, err_msg=name)
    np.testing.assert_array_equal(g_count, count, err_msg=name)
    out, newV = R.split_apply(F, V, mid)
    np.testing.assert_array_equal(g_out, out, err_msg=name)
    assert _bits_equal(g_V, newV), name
    if name == "diagonal tie":
        assert count.tolist() == [3, 3] and out[:3].tolist() == [[3, 1, 4], [0, 3, 4], [0, 4, 2]]
    if name == "all three long":
        assert count.tolist() == [4, 4]


# ---- collapse evaluation -------------------------------------------------------------------------------------------------------------
MAX_Q = 24


def gpu_collapse_eval(F, V, vn, min_len, max_len, max_q=MAX_Q, ql_cap=None):
    nf, nv = len(F), len(V)
    start, vf, _ = gpu_csr(F, nv)
    Fd, Vd = _d(F, torch.long), _d(V)
    E = torch.full((3 * nf, 2), SENT_I, dtype=torch.long, device=DEV)
    length = torch.full((3 * nf,), SENT_D, dtype=torch.float64, device=DEV)
    ok = torch.full((3 * nf,), 9, dtype=torch.uint8, device=DEV)
    nq = torch.full((3 * nf,), SENT_I, dtype=torch.int32, device=DEV)
    q = torch.full((3 * nf, max_q, 3), SENT_D, dtype=torch.float64, device=DEV)
    cap = ql_cap if ql_cap is not None else 3 * nf * max_q                 # (room for every query point: nothing is left to a next round)
    item = torch.full((cap,), SENT_I, dtype=torch.int32, device=DEV)
    point = torch.full((cap, 3), SENT_D, dtype=torch.float64, device=DEV)
    qcount = torch.zeros(1, dtype=torch.int32, device=DEV)
    live = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    _ck(_lib().drt_rm_collapse_eval_all(Fd.data_ptr(), nf, Vd.data_ptr(), _d(vn).data_ptr(), _d(start, torch.long).data_ptr(), _d(vf, torch.long).data_ptr(),
                                        float(min_len), float(max_len), max_q, E.data_ptr(), length.data_ptr(), ok.data_ptr(), nq.data_ptr(), q.data_ptr(),
                                        item.data_ptr(), point.data_ptr(), qcount.data_ptr(), cap, live.data_ptr(), _st()))
    return dict(ok=ok.cpu().numpy(), nq=nq.cpu().numpy(), q=q.cpu().numpy(), E=E.cpu().numpy(), length=length.cpu().numpy(),
                item=item.cpu().numpy(), point=point.cpu().numpy(), count=int(qcount.item()), cap=cap)


def bicone(n, h=0.3, r=1.0):
    """A ring of n vertices and two apexes (valence n each) at +-h: a closed double cone."""
    ang = np.arange(n) * 2 * np.pi / n
    V = np.concatenate([np.stack([r * np.cos(ang), r * np.sin(ang), 0 * ang], 1), [[0, 0, h], [0, 0, -h]]])
    F = [[n, i, (i + 1) % n] for i in range(n)] + [[n + 1, (i + 1) % n, i] for i in range(n)]
    return np.array(F, dtype=np.int64), V


def dented_sphere():
    from drt_amd import mesh_io
    s = mesh_io.icosphere(3, radius=50.0)
    V = s.vertices.copy()
    rng = np.random.default_rng(5)
    dent = rng.choice(len(V), 60, replace=False)
    V[dent] *= rng.uniform(0.7, 1.15, (60, 1))                               # pits and bumps: folded neighbourhoods
    return s.faces.astype(np.int64), V


def _collapse_cases(hand_split):
    F, V = hand_split
    L = 4.0
    m = R.Mesh(F, V)
    ok, _, _, E, _ = R.collapse_eval_all(m, None, m.normals(), 0.8 * L, 4 / 3 * L, MAX_Q)
    c = np.nonzero(ok)[0]
    Fk, Vk = R.collapse_apply(F, V, [tuple(E[c[0]]), tuple(E[c[len(c) // 2]])])       # two collapses applied: rows of -1 in the face array
    Fs, Vs = dented_sphere()
    cases = [("hand split", F, V, None, 0.8 * L, 4 / 3 * L, MAX_Q), ("hand split, killed rows", Fk, Vk, None, 0.8 * L, 4 / 3 * L, MAX_Q),
             ("dented sphere", Fs, Vs, None, 9.0, 12.0, MAX_Q)]
    for n in (31, 33):
        Fb, Vb = bicone(n)
        cases.append((f"bicone {n}", Fb, Vb, None, 1.2, 3.0, 48))              # (room for every query point of an apex edge)
    for pad in (0, 1):
        Fv, Vv = valence3_pair(pad)
        cases.append((f"valence-3 pair, pad {pad}", Fv, Vv, np.zeros_like(Vv), 10.0, 200.0, MAX_Q))
    return cases


@pytest.fixture(scope="module")
def collapse_cases(hand_split):
    return _collapse_cases(hand_split)


@pytest.mark.parametrize("case", range(7))
def test_collapse_eval_all(collapse_cases, case):
    name, F, V, vn, min_len, max_len, max_q = collapse_cases[case]
    m = R.Mesh(F, V)
    vn = m.normals() if vn is None else vn
    ok, nq, q, E, length = R.collapse_eval_all(m, None, vn, min_len, max_len, max_q)
    g = gpu_collapse_eval(F, V, vn, min_len, max_len, max_q)
    np.testing.assert_array_equal(g["E"], E, err_msg=name)
    assert _bits_equal(g["length"], length), name
    np.testing.assert_array_equal(g["ok"], ok, err_msg=name)
    np.testing.assert_array_equal(g["nq"], nq, err_msg=name)
    for c, pts in q.items():
        assert _bits_equal(g["q"][c, :len(pts)], pts), (name, c)
    # the compact list (generous cap): the multiset of (item, point) is the reference's
    n = g["count"]
    assert n == int(nq.sum()) <= g["cap"]
    got = sorted((int(i), tuple(p)) for i, p in zip(g["item"][:n], g["point"][:n]))
    want = sorted((c, tuple(p)) for c, pts in q.items() for p in pts)
    assert got == want, name
    if name.startswith("hand split"):
        assert ok.sum() > 200
    if name.startswith("bicone"):
        apex = (E[:, 0] >= len(V) - 2) | (E[:, 1] >= len(V) - 2)
        assert ok[apex].any() == (name == "bicone 31")                        # a valence above 32 is left alone
    if name == "valence-3 pair, pad 0":
        assert not ok.any()
    if name == "valence-3 pair, pad 1":
        assert ok.sum() >= 1


def test_collapse_eval_tight_list(hand_split):
    F, V = hand_split
    m = R.Mesh(F, V)
    vn = m.normals()
    ok, nq, q, E, length = R.collapse_eval_all(m, None, vn, 3.2, 16 / 3, MAX_Q)
    cap = 37
    g = gpu_collapse_eval(F, V, vn, 3.2, 16 / 3, ql_cap=cap)
    n = min(g["count"], cap)
    items, pts = g["item"][:n], g["point"][:n]
    listed = set(int(i) for i in items if i >= 0)
    assert listed and g["count"] > cap                                       # the cap did bind
    for c in listed:                                                         # no item partly listed, in order, with its points
        sel = np.nonzero(items == c)[0]
        assert len(sel) == nq[c] and (np.diff(sel) == 1).all()
        assert _bits_equal(pts[sel], q[c])
    assert all(g["ok"][c] for c in listed)
    assert set(np.nonzero(g["ok"])[0].tolist()) == listed                     # every `ok` that stays is listed ...
    assert listed <= set(np.nonzero(ok)[0].tolist())                         # ... and is a reference `ok`
    assert (items[~np.isin(items, list(listed))] == -1).all()                # what it skipped is -1


# ---- surface distance and closest point ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand_surface(hand):
    from drt_amd.optix_mesh import optix_mesh
    F, V = hand
    s = optix_mesh(0)
    s.update_mesh(_d(F, torch.int32), _d(V, torch.float32))
    return s, F, V.astype(np.float32).astype(np.float64)


def brute_distance(P, F, V):
    from oracle.remesh_oracle import point_triangle_distance
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    out = np.empty(len(P))
    for i, p in enumerate(P):
        out[i] = point_triangle_distance(np.broadcast_to(p, A.shape), A, B, C).min()
    return out


def surface_points(F, V, D, rng):
    """Points at D (1 +- 1e-6) along face normals, on vertices, on edge midpoints, far away."""
    f = rng.choice(len(F), 120, replace=False)
    a, b, c = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cen = (a + b + c) / 3
    near = np.concatenate([cen + n * D * (1 + 1e-6), cen + n * D * (1 - 1e-6)])
    return np.concatenate([near, V[F[f[:20], 0]], (a[:20] + b[:20]) / 2, cen[:10] + 1e3])


def test_surface_filters(hand_surface):
    s, F, V32 = hand_surface
    rng = np.random.default_rng(7)
    D = 0.5
    P = surface_points(F, V32, D, rng)
    d = brute_distance(P, F, V32)
    within = d <= D
    assert within.sum() > 50 and (~within).sum() > 50
    lib, st = _lib(), _st()
    # drt_rm_surface_filter: items of up to max_q points
    max_q, n_items = 4, len(P) // 2
    q = np.full((n_items, max_q, 3), 1e9)
    nq = rng.integers(1, max_q + 1, n_items).astype(np.int32)
    order = rng.permutation(len(P))
    k = 0
    for i in range(n_items):
        for j in range(nq[i]):
            q[i, j] = P[order[k % len(P)]]
            k += 1
    ok0 = (rng.random(n_items) < 0.9).astype(np.uint8)
    want = ok0.copy()
    k = 0
    for i in range(n_items):
        for j in range(nq[i]):
            want[i] &= within[order[k % len(P)]]
            k += 1
    ok = _d(ok0, torch.uint8)
    _ck(lib.drt_rm_surface_filter(s._h, ok.data_ptr(), _d(nq, torch.int32).data_ptr(), _d(q).data_ptr(), n_items, max_q, D, None, st))
    np.testing.assert_array_equal(ok.cpu().numpy(), want)
    ok1 = _d(np.ones(len(P), np.uint8), torch.uint8)                          # no n_query: one point per item
    _ck(lib.drt_rm_surface_filter(s._h, ok1.data_ptr(), None, _d(P[:, None, :]).data_ptr(), len(P), 1, D, None, st))
    np.testing.assert_array_equal(ok1.cpu().numpy(), within.astype(np.uint8))
    # drt_rm_surface_filter_list: item / point pairs, skipped entries (-1), entries past the count not read
    n_it = 40
    item = rng.integers(0, n_it, len(P)).astype(np.int32)
    item[::11] = -1
    cnt = len(P) - 5
    ok0 = np.ones(n_it, np.uint8)
    ok0[3] = 0
    want = ok0.copy()
    for i in range(cnt):
        if item[i] >= 0:
            want[item[i]] &= within[i]
    okl = _d(ok0, torch.uint8)
    _ck(lib.drt_rm_surface_filter_list(s._h, okl.data_ptr(), _d(item, torch.int32).data_ptr(), _d(P).data_ptr(),
                                        _d(np.array([cnt]), torch.int32).data_ptr(), len(P), D, None, st))
    np.testing.assert_array_equal(okl.cpu().numpy(), want)


@pytest.mark.parametrize("hint", ["target", "tiny", 0.0, -1.0, float("nan")])
def test_closest_near(hand_surface, hint):
    s, F, V32 = hand_surface
    rng = np.random.default_rng(11)
    P = V32[rng.choice(len(V32), 300, replace=False)] + rng.standard_normal((300, 3)) * 1.5
    P = np.concatenate([P, V32[:5] + 40.0])                                  # a few far out: beyond any hint
    h = {"target": 4.0, "tiny": 1e-9}.get(hint, hint)
    out = torch.full((len(P), 3), SENT_D, dtype=torch.float64, device=DEV)
    Pd = _d(P)
    _ck(_lib().drt_rm_closest_near(s._h, Pd.data_ptr(), len(P), float(h), out.data_ptr(), _st()))
    got = out.cpu().numpy()
    d = brute_distance(P, F, V32)
    np.testing.assert_allclose(np.linalg.norm(got - P, axis=1), d, rtol=1e-12, atol=0)
    assert brute_distance(got[::15], F, V32).max() < 1e-9                     # the point is ON the surface
    ref = s.closest_point(Pd, want_face=False, want_point=True)[2].cpu().numpy()
    assert _bits_equal(got, ref)


# ---- flip evaluation -----------------------------------------------------------------------------------------------------------------
def gpu_flip_eval(F, V, vn, max_len):
    nf, nv = len(F), len(V)
    start, vf, _ = gpu_csr(F, nv)
    ok = torch.full((3 * nf,), 9, dtype=torch.uint8, device=DEV)
    quad = torch.full((3 * nf, 6), SENT_I, dtype=torch.long, device=DEV)
    q = torch.full((3 * nf, 3), SENT_D, dtype=torch.float64, device=DEV)
    _ck(_lib().drt_rm_flip_eval(_d(F, torch.long).data_ptr(), nf, _d(V).data_ptr(), _d(vn).data_ptr(), _d(start, torch.long).data_ptr(),
                                _d(vf, torch.long).data_ptr(), float(max_len), ok.data_ptr(), quad.data_ptr(), q.data_ptr(), None, _st()))
    return ok.cpu().numpy(), quad.cpu().numpy(), q.cpu().numpy()


def _flip_cases(hand_split):
    F, V = hand_split
    up = lambda V: np.tile([0.0, 0.0, 1.0], (len(V), 1))
    cases = [("hand split", F, V, None, 16 / 3)]
    Fs, Vs = dented_sphere()
    cases.append(("dented sphere", Fs, Vs, None, 12.0))
    Ff, Vf = padded_quad((1.0, 0.5, 0.0), pads=(2, 2, 0, 0))
    cases.append(("folded pair", Ff, Vf, up(Vf), 10.0))
    Fe, Ve = padded_quad((1.0, -1.0, 0.0), pads=(5, 5, 3, 3))
    Fe = np.concatenate([Fe, [[2, 3, len(Ve)]]])
    Ve = np.concatenate([Ve, [[1.0, 0.0, 5.0]]])
    cases.append(("flip edge exists", Fe, Ve, up(Ve), 10.0))
    for cos in (0.9445, 0.9405, 0.9395):
        h = np.sqrt(1.0 / cos ** 2 - 1.0)
        Fc, Vc = padded_quad((1.0, -1.0, -h), pads=(5, 5, 4, 4))
        cases.append((f"flatness {cos}", Fc, Vc, up(Vc), 10.0))
    return cases


@pytest.mark.parametrize("case", range(7))
def test_flip_eval(hand_split, case):
    name, F, V, vn, max_len = _flip_cases(hand_split)[case]
    m = R.Mesh(F, V)
    vn = m.normals() if vn is None else vn
    ok, quads, mids = R.flip_eval_all(m, None, vn, max_len)
    g_ok, g_quad, g_q = gpu_flip_eval(F, V, vn, max_len)
    np.testing.assert_array_equal(g_ok, ok, err_msg=name)
    for c, qd in quads.items():
        assert tuple(g_quad[c]) == qd, (name, c)
        assert _bits_equal(g_q[c], mids[c]), (name, c)
    if name == "hand split":
        assert ok.sum() > 100
    if name == "folded pair":
        assert ok[0] == 1
    if name == "flip edge exists":
        assert not ok.any()
    if name.startswith("flatness"):
        assert ok[0] == (float(name.split()[1]) >= 0.94)


# ---- relaxation target, agreement, roll-back ----------------------------------------------------------------------------------------
def gpu_smooth_target(F, V):
    start, vf, _ = gpu_csr(F, len(V))
    t = torch.full((len(V), 3), SENT_D, dtype=torch.float64, device=DEV)
    _ck(_lib().drt_rm_smooth_target(_d(F, torch.long).data_ptr(), _d(V).data_ptr(), _d(start, torch.long).data_ptr(), _d(vf, torch.long).data_ptr(),
                                    len(V), t.data_ptr(), _st()))
    return t.cpu().numpy()


def test_smooth_target(hand_split):
    F, V = hand_split
    assert _bits_equal(gpu_smooth_target(F, V), R.smooth_target(R.Mesh(F, V)))
    # float32-born positions sum exactly in float64 in any order; jittered ones do not: the ring's ascending order is then visible
    Vj = V + np.random.default_rng(2).standard_normal(V.shape) * 1e-3
    assert _bits_equal(gpu_smooth_target(F, Vj), R.smooth_target(R.Mesh(F, Vj)))
    Fb, Vb = bicone(33)                                                      # apexes: 33 neighbours, more than a ring holds
    Vb = np.concatenate([Vb, [[5.0, 5.0, 5.0]]])                              # an isolated vertex
    Fz = np.array([[36, 37, 38], [36, 38, 37]])                              # a face and its reverse: a zero normal
    Vz = np.concatenate([Vb, [[0.5, 0, 2], [1.5, 0, 2], [0.5, 1, 2]]])
    Fa = np.concatenate([Fb, Fz])
    ref = R.smooth_target(R.Mesh(Fa, Vz))
    got = gpu_smooth_target(Fa, Vz)
    assert _bits_equal(got, ref)
    assert _bits_equal(got[33:], Vz[33:])  # apexes, isolated, zero normal: in place
    assert not _bits_equal(got[:33], Vz[:33])


def test_face_agreement_and_move_check(hand_split):
    F, V = hand_split
    lib, st = _lib(), _st()
    vn = R.Mesh(F, V).normals()
    nf, nv = len(F), len(V)
    Fd, vnd = _d(F, torch.long), _d(vn)
    a0 = torch.full((nf,), SENT_D, dtype=torch.float64, device=DEV)
    _ck(lib.drt_rm_face_agreement(Fd.data_ptr(), _d(V).data_ptr(), vnd.data_ptr(), nf, a0.data_ptr(), st))
    ref_a0 = R.face_agreement(F, V, vn)
    assert _bits_equal(a0.cpu().numpy(), ref_a0)
    rng = np.random.default_rng(3)
    moved = V.copy()
    sel = rng.random(nv) < 0.3
    moved[sel] += rng.standard_normal((sel.sum(), 3)) * 2.5                 # large moves: some faces fold
    moved[F[0, 0]] = V[F[0, 1]]                                               # a vertex onto its neighbour: two faces lose their area
    Vd = _d(moved)
    revert = torch.full((nv,), 9, dtype=torch.uint8, device=DEV)
    n_bad = torch.full((1,), SENT_I, dtype=torch.int32, device=DEV)
    _ck(lib.drt_rm_move_check(Fd.data_ptr(), Vd.data_ptr(), _d(V).data_ptr(), vnd.data_ptr(), a0.data_ptr(), nf, nv, revert.data_ptr(), n_bad.data_ptr(), st))
    r_rev, r_bad, r_V = R.move_check(F, moved, V, vn, ref_a0)
    assert r_bad > 100 and r_rev[F[0, 0]] == 1
    np.testing.assert_array_equal(revert.cpu().numpy(), r_rev)
    assert int(n_bad.item()) == r_bad
    assert _bits_equal(Vd.cpu().numpy(), r_V)


# ---- round control -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail_cut", [1, 4, 32])
def test_round_end(tail_cut):
    rng = np.random.default_rng(tail_cut)
    seqs = [[10], [0], [64, 2], [64, 1], [64, 0], [31, 31, 1, 0], [32, 1, 1], [4 * tail_cut, tail_cut - 1 if tail_cut > 1 else 0]]
    seqs += [list(rng.integers(0, 200, rng.integers(1, 9))) for _ in range(20)]
    for seq in seqs:
        ctl = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        ref = [1, 0, 0, 0, 0, 0, 0, 0]
        for n in seq:
            ctl[1] += int(n)                                                 # what the apply kernels add up
            ref[1] += int(n)
            _ck(_lib().drt_rm_round_end(ctl.data_ptr(), tail_cut, _st()))
            ref = R.round_end(ref, tail_cut)
            assert ctl.tolist() == ref, (seq, tail_cut)


# ---- claim / apply: the commutation claim --------------------------------------------------------------------------------------------
def _faces_of(F, v):
    return set(np.nonzero((F == v).any(1))[0].tolist())


@pytest.mark.parametrize("sub_rounds", [1, 3])
def test_collapse_round_is_a_sequential_set(hand_split, sub_rounds):
    F, V = hand_split
    L = 4.0
    min_len, max_len = 0.8 * L, 4 / 3 * L
    lib, st = _lib(), _st()
    nf, nv = len(F), len(V)
    m0 = R.Mesh(F, V)
    vn = m0.normals()
    ok_ref, _, _, E, length = R.collapse_eval_all(m0, None, vn, min_len, max_len, MAX_Q)
    start, vf, g_vn = gpu_csr(F, nv, V)
    assert _bits_equal(g_vn, vn)
    g = gpu_collapse_eval(F, V, vn, min_len, max_len)
    np.testing.assert_array_equal(g["ok"], ok_ref)
    Fd, Vd = _d(F, torch.long), _d(V)
    ctl = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    lock = torch.empty(nv, dtype=torch.int64, device=DEV)
    dirty = torch.empty(nv, dtype=torch.uint8, device=DEV)
    f_alive = torch.ones(nf, dtype=torch.uint8, device=DEV)
    v_alive = torch.ones(nv, dtype=torch.uint8, device=DEV)
    _ck(lib.drt_rm_collapse_apply(None, 3 * nf, _d(g["ok"], torch.uint8).data_ptr(), _d(g["E"], torch.long).data_ptr(), Fd.data_ptr(), Vd.data_ptr(),
                                  _d(start, torch.long).data_ptr(), _d(vf, torch.long).data_ptr(), nv, float(min_len), 0x9E3779B9, 0, _d(g["length"]).data_ptr(),
                                  lock.data_ptr(), f_alive.data_ptr(), v_alive.data_ptr(), dirty.data_ptr(), sub_rounds, ctl.data_ptr() + 4, ctl.data_ptr(), st))
    _ck(lib.drt_rm_kill_faces(Fd.data_ptr(), f_alive.data_ptr(), nf, ctl.data_ptr(), st))
    F1, V1, alive, n_done = Fd.cpu().numpy(), Vd.cpu().numpy(), v_alive.cpu().numpy(), int(ctl[1])
    # the applied set: b died and a sits on the midpoint, bit for bit
    applied = []
    for c in np.nonzero((E[:, 0] >= 0) & (E[:, 0] < E[:, 1]))[0]:
        a, b = int(E[c, 0]), int(E[c, 1])
        if alive[b] == 0 and _bits_equal(V1[a], (V[a] + V[b]) * 0.5):
            applied.append(int(c))
    assert len(applied) == n_done > 20
    assert all(ok_ref[c] for c in applied)
    pairs = {c: (int(E[c, 0]), int(E[c, 1])) for c in applied}
    touched = {c: _faces_of(F, b) for c, (a, b) in pairs.items()}           # the faces a collapse rewrote or killed
    for c, (a, b) in pairs.items():
        near = _faces_of(F, a) | _faces_of(F, b)
        for c2 in applied:
            if c2 != c:
                assert not (touched[c2] & near), (c, c2)
    for seq in (applied, applied[::-1]):
        Fs, Vs = R.collapse_apply(F, V, [pairs[c] for c in seq])
        np.testing.assert_array_equal(F1, Fs)
        assert _bits_equal(V1, Vs)
    Fc, Vc = F.copy(), V.copy()                                               # each one's premises still hold just before it
    for c in applied:
        ok, _ = R.collapse_eval(R.Mesh(Fc, Vc), vn, *pairs[c], min_len, max_len, MAX_Q)
        assert ok, c
        Fc, Vc = R.collapse_apply(Fc, Vc, [pairs[c]])


@pytest.mark.parametrize("sub_rounds", [1, 3])
def test_flip_round_is_a_sequential_set(hand_split, sub_rounds):
    F, V = hand_split
    max_len = 16 / 3
    lib, st = _lib(), _st()
    nf, nv = len(F), len(V)
    m0 = R.Mesh(F, V)
    vn = m0.normals()
    ok_ref, quads, _ = R.flip_eval_all(m0, None, vn, max_len)
    g_ok, g_quad, _ = gpu_flip_eval(F, V, vn, max_len)
    np.testing.assert_array_equal(g_ok, ok_ref)
    Fd = _d(F, torch.long)
    ctl = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    lock = torch.empty(nv, dtype=torch.int64, device=DEV)
    dirty = torch.empty(nv, dtype=torch.uint8, device=DEV)
    _ck(lib.drt_rm_flip_apply(3 * nf, _d(g_ok, torch.uint8).data_ptr(), _d(g_quad, torch.long).data_ptr(), Fd.data_ptr(), nv, 0, lock.data_ptr(),
                              dirty.data_ptr(), sub_rounds, ctl.data_ptr() + 4, ctl.data_ptr(), st))
    F1, n_done = Fd.cpu().numpy(), int(ctl[1])
    applied = [c for c, (a, b, cc, d, f1, f2) in quads.items() if tuple(F1[f1]) == (cc, a, d) and tuple(F1[f2]) == (d, b, cc)]
    assert len(applied) == n_done > 20
    verts = [v for c in applied for v in quads[c][:4]]
    assert len(verts) == len(set(verts))                                     # no two applied flips share a vertex
    for seq in (applied, applied[::-1]):
        np.testing.assert_array_equal(F1, R.flip_apply(F, [quads[c] for c in seq]))
    Fc = F.copy()
    for c in applied:
        assert R.flip_eval(R.Mesh(Fc, V), vn, c // 3, c % 3, max_len) == quads[c], c
        Fc = R.flip_apply(Fc, [quads[c]])


# ---- the input check and the DEBUG size checks of isotropic_remesh_gpu -----------------------------------------------------------------
def _malformed(F, V):
    two_tets = (np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [0, 4, 1], [0, 1, 5], [0, 5, 4], [1, 4, 5]]), np.random.default_rng(0).random((6, 3)))
    flipped = F.copy()
    flipped[7] = flipped[7, ::-1]
    high = F.copy()
    high[3, 1] = len(V)
    return [("one face missing", F[1:], V), ("two faces missing", np.delete(F, [5, 900], 0), V), ("one face flipped", flipped, V),
            ("two tetrahedra sharing an edge", *two_tets), ("an index >= V", high, V)]


@pytest.mark.parametrize("case", range(5))
def test_remesh_rejects_what_is_not_a_closed_oriented_manifold(hand, case):
    from drt_amd import remesh_gpu
    name, F, V = _malformed(*hand)[case]
    with pytest.raises(ValueError):
        remesh_gpu.isotropic_remesh_gpu(_d(V), _d(F, torch.long), 4.0)
    torch.cuda.synchronize()


def _remesh(F, V, L):
    from drt_amd import remesh_gpu
    from drt_amd.optix_mesh import optix_mesh
    s = optix_mesh(0)
    s.update_mesh(_d(F, torch.int32), _d(V, torch.float32))
    return remesh_gpu.isotropic_remesh_gpu(_d(V), _d(F, torch.long), L, surface=s)


def test_debug_size_checks_on_whole_remeshes(hand, monkeypatch):
    from drt_amd import mesh_io, remesh_gpu
    horse = mesh_io.subdivide_midpoint(mesh_io.read_ply(data_path("horse_vh.ply")))
    monkeypatch.setattr(remesh_gpu, "DEBUG", True)
    for F, V, L in ((hand[0], hand[1], 4.0), (horse.faces.astype(np.int64), horse.vertices, 2.0)):
        Vo, Fo = _remesh(F, V, L)
        assert int(Fo.max()) == len(Vo) - 1 and len(torch.unique(Fo)) == len(Vo)
    monkeypatch.undo()
    assert remesh_gpu.DEBUG is False
