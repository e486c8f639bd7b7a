"""tests/remesh_ref.py -- the float64 host reference of the device remesher's stages -- pinned on tiny meshes whose answers are worked out
by hand (no GPU: the reference must be right before the kernels are held against it in tests/test_gpu_remesh_kernels.py)."""
import numpy as np
import pytest

import remesh_ref as R


def octahedron():
    """Vertices +x -x +y -y +z -z (ids 0..5), eight outward faces: every vertex has valence 4, every face normal is (+-1, +-1, +-1)."""
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    F = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                sign = (1 if sx == 0 else -1) * (1 if sy == 2 else -1) * (1 if sz == 4 else -1)
                F.append([sx, sy, sz] if sign > 0 else [sx, sz, sy])
    return np.array(F, dtype=np.int64), V


def tetrahedron():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    return F, V


def hexagon_fan(centre=(0.5, 0.25, 0.0)):
    """Centre 0 and a flat hexagon 1..6 whose corners sum to zero exactly (area 12): six faces around the centre."""
    ring = [[2, 0, 0], [1, 2, 0], [-1, 2, 0], [-2, 0, 0], [-1, -2, 0], [1, -2, 0]]
    V = np.array([list(centre)] + ring, dtype=np.float64)
    F = np.array([[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)], dtype=np.int64)
    return F, V


def padded_quad(d, pads, extra=()):
    """Faces f1 = (a, b, c) = (0, 1, 2) and f2 = (b, a, d) = (1, 0, 3) around edge a-b, plus `pads` faces per vertex (vertex, p, p + 1)
    far away that only raise its valence (the rules read valence as the number of faces), plus `extra` faces."""
    V = [[0, 0, 0], [2, 0, 0], [1, 1, 0], list(d)]
    F = [[0, 1, 2], [1, 0, 3]]
    for v, n in enumerate(pads):
        for _ in range(n):
            p = len(V)
            V += [[100 + p, 0, 0], [100 + p, 1, 0]]
            F.append([v, p, p + 1])
    F += [list(f) for f in extra]
    return np.array(F, dtype=np.int64), np.array(V, dtype=np.float64)


def test_csr_and_normals_of_the_octahedron():
    F, V = octahedron()
    start, vf = R.vertex_faces(F, 6)
    assert start.tolist() == [0, 4, 8, 12, 16, 20, 24]
    for v in range(6):
        run = vf[start[v]:start[v + 1]].tolist()
        assert run == sorted(run) and run == [f for f in range(8) if v in F[f]]
    vn = R.vertex_normals(F, V, start, vf)
    np.testing.assert_array_equal(vn, 4.0 * V)                 # four unit-cube normals (+-1, +-1, +-1): the off-axis parts cancel


def test_csr_skips_killed_faces_and_unused_vertices():
    F, V = octahedron()
    F[[2, 5]] = -1
    start, vf = R.vertex_faces(F, 8)                             # vertices 6 and 7: no face
    assert len(vf) == 18 and 2 not in vf and 5 not in vf
    assert np.diff(start)[6:].tolist() == [0, 0]
    vn = R.vertex_normals(F, np.concatenate([V, np.ones((2, 3))]), start, vf)
    assert (vn[6:] == 0).all()


def test_normals_of_the_fan_and_its_smoothing_target():
    F, V = hexagon_fan()
    m = R.Mesh(F, V)
    np.testing.assert_array_equal(m.normals()[0], [0.0, 0.0, 24.0])           # twice the hexagon's area, wherever the centre sits inside
    t = R.smooth_target(m)
    np.testing.assert_array_equal(t[0], [0.0, 0.0, 0.0])                       # the ring centroid, nothing along the normal (flat)
    F2, V2 = hexagon_fan(centre=(0.0, 0.0, 0.5))
    np.testing.assert_array_equal(R.smooth_target(R.Mesh(F2, V2))[0], [0.0, 0.0, 0.5])   # the height along the normal is kept


def test_smoothing_leaves_isolated_zero_normal_and_crowded_vertices():
    F, V = hexagon_fan()
    V = np.concatenate([V, [[9.0, 9.0, 9.0]]])                                 # 7: isolated
    assert np.array_equal(R.smooth_target(R.Mesh(F, V))[7], V[7])
    Fz = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)                      # the normals of a face and its reverse cancel: zero normal
    Vz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64)
    assert np.array_equal(R.smooth_target(R.Mesh(Fz, Vz)), Vz)
    n = 33                                                                     # a fan of 33 faces: 33 neighbours, more than a ring holds
    ang = np.arange(n) * 2 * np.pi / n
    Vc = np.concatenate([[[0.3, 0.1, 0.0]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)])
    Fc = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], dtype=np.int64)
    assert np.array_equal(R.smooth_target(R.Mesh(Fc, Vc))[0], Vc[0])
    Fc2, Vc2 = Fc[:32], Vc                                                     # 32 faces: 33 neighbours still (an open fan)
    assert np.array_equal(R.smooth_target(R.Mesh(Fc2, Vc2))[0], Vc2[0])
    Vd = Vc[:33].copy()                                                        # 32 neighbours: it moves
    Fd = np.array([[0, 1 + i, 1 + (i + 1) % 32] for i in range(32)], dtype=np.int64)
    assert not np.array_equal(R.smooth_target(R.Mesh(Fd, Vd))[0], Vd[0])


def test_octahedron_collapses_pass_with_five_query_points():
    F, V = octahedron()
    m = R.Mesh(F, V)
    vn = m.normals()
    ok, nq, q, E, length = R.collapse_eval_all(m, None, vn, min_len=2.0, max_len=10.0, max_q=24)
    own = (E[:, 0] < E[:, 1])
    assert own.sum() == 12 and ok[own].all() and not ok[~own].any()            # every edge: two common neighbours of valence 4, 4 + 4 - 4 >= 3
    np.testing.assert_array_equal(length[own], np.sqrt(2.0))
    assert (nq[own] == 5).all()                                                # midpoint + the two surviving faces of each end
    c = int(np.nonzero((E[:, 0] == 0) & (E[:, 1] == 2))[0][0])                 # +x -> +y
    assert q[c][0] == (0.5, 0.5, 0.0)
    # a's surviving faces (+x +z -y) and (+x -y -z) after the move, then b's (+y -x +z) and (+y -z -x)
    want = [(1 / 6, -1 / 6, 1 / 3), (1 / 6, -1 / 6, -1 / 3), (-1 / 6, 1 / 6, 1 / 3), (-1 / 6, 1 / 6, -1 / 3)]
    assert sorted(q[c][1:]) == pytest.approx(sorted(want), abs=1e-15)
    assert not R.collapse_eval_all(m, None, vn, 2.0, 10.0, max_q=4)[0].any()   # five points do not fit in four
    assert not R.collapse_eval_all(m, None, vn, 1.4, 10.0, 24)[0].any()        # sqrt(2) is not shorter than 1.4
    assert not R.collapse_eval_all(m, None, vn, 2.0, 1.0, 24)[0].any()         # a new edge from the midpoint would be longer than max_len


def test_octahedron_collapse_applied():
    F, V = octahedron()
    F2, V2 = R.collapse_apply(F, V, [(0, 2)])
    assert ((F2 == -1).all(1)).sum() == 2 and not (F2 == 2).any()
    np.testing.assert_array_equal(V2[0], [0.5, 0.5, 0.0])
    live = F2[F2[:, 0] >= 0]
    assert len(live) == 6 and sorted(np.unique(live).tolist()) == [0, 1, 3, 4, 5]


def test_tetrahedron_refuses_every_collapse_and_flip():
    F, V = tetrahedron()
    m = R.Mesh(F, V)
    vn = m.normals()
    assert not R.collapse_eval_all(m, None, vn, 10.0, 100.0, 24)[0].any()     # the opposite vertices have valence 3
    assert not R.flip_eval_all(m, None, vn, 100.0)[0].any()                   # so do the edge's ends


def valence3_pair(pad_ab):
    """Two adjacent vertices a = 0, b = 1 with common neighbours o1 = 2, o2 = 3 (a closed tetrahedron a b o1 o2) and one far pad face on
    o1 and on o2 (valence 4), and `pad_ab` pad faces on a and on b."""
    V = [[0, 1, 0.3], [0, 1, -0.3], [1, 0, 0], [-1, 0, 0]]
    F = [[0, 1, 2], [1, 0, 3], [0, 2, 3], [1, 3, 2]]
    for v in [2, 3] + [0, 1] * pad_ab:
        p = len(V)
        V += [[50 + p, 0, 0], [50 + p, 1, 0]]
        F.append([v, p, p + 1])
    return np.array(F, dtype=np.int64), np.array(V, dtype=np.float64)


def test_the_valence_sum_rule_alone():
    """Valences 3 + 3 - 4 = 2 < 3 refuse a-b; a pad face on each end (4 + 4 - 4 = 4) and the same collapse passes: no other rule
    refused it (a zero consensus accepts every face)."""
    F, V = valence3_pair(0)
    assert R.collapse_eval(R.Mesh(F, V), np.zeros_like(V), 0, 1, 10.0, 200.0, 24) == (False, [])
    F, V = valence3_pair(1)
    ok, q = R.collapse_eval(R.Mesh(F, V), np.zeros_like(V), 0, 1, 10.0, 200.0, 24)
    assert ok and len(q) == 5 and q[0] == (0.0, 1.0, 0.0)


def test_fold_repair_flip_and_the_valence_rule():
    vn = lambda F, V: np.tile([0.0, 0.0, 1.0], (len(V), 1))
    # d = (1, 0.5, 0) lies on c's side of a-b: f2 = (b, a, d) faces down, the pair is folded -> repaired whatever the valences
    F, V = padded_quad((1.0, 0.5, 0.0), pads=(2, 2, 0, 0))
    m = R.Mesh(F, V)
    assert R.flip_eval(m, vn(F, V), 0, 0, 10.0) == (0, 1, 2, 3, 0, 1)
    assert R.flip_eval(m, -vn(F, V), 0, 0, 10.0) is None                       # the new faces would disagree with the consensus
    np.testing.assert_array_equal(R.flip_apply(F, [(0, 1, 2, 3, 0, 1)])[:2], [[2, 0, 3], [3, 1, 2]])
    # d = (1, -1, 0): a flat convex quad; valences a = b = 4, c = d = 1: |4-6|*2 + |1-6|*2 = 14 -> |4-7|*2 + |1-5|*2 = 14, no gain
    F, V = padded_quad((1.0, -1.0, 0.0), pads=(2, 2, 0, 0))
    assert R.flip_eval(R.Mesh(F, V), vn(F, V), 0, 0, 10.0) is None
    # valences 7 7 5 5 (pads 5 5 4 4): deviation 4 -> 0, the flip passes; and a < 4 at either end refuses it
    F, V = padded_quad((1.0, -1.0, 0.0), pads=(5, 5, 4, 4))
    assert R.flip_eval(R.Mesh(F, V), vn(F, V), 0, 0, 10.0) == (0, 1, 2, 3, 0, 1)
    assert R.flip_eval(R.Mesh(F, V), vn(F, V), 0, 0, 1.9) is None              # |c - d| = 2 > max_len
    F, V = padded_quad((1.0, -1.0, 0.0), pads=(1, 5, 4, 4))
    assert R.flip_eval(R.Mesh(F, V), vn(F, V), 0, 0, 10.0) is None


@pytest.mark.parametrize("cos, ok", [(0.945, True), (0.935, False)])
def test_flip_flatness_rule(cos, ok):
    """f1 = (a, b, c) in z = 0, d lowered by h: the pair's cosine is 1 / sqrt(1 + h^2) -- flips only above 0.94."""
    h = np.sqrt(1.0 / cos ** 2 - 1.0)
    F, V = padded_quad((1.0, -1.0, -h), pads=(5, 5, 4, 4))
    m = R.Mesh(F, V)
    n1, n2 = R.tri_normal(*map(tuple, V[F[0]])), R.tri_normal(*map(tuple, V[F[1]]))
    assert R._dot(n1, n2) / (R._len(n1) * R._len(n2)) == pytest.approx(cos, abs=1e-12)
    assert (R.flip_eval(m, np.tile([0.0, 0.0, 1.0], (len(V), 1)), 0, 0, 10.0) is not None) == ok


def test_flip_refused_when_the_new_edge_exists():
    F, V = padded_quad((1.0, -1.0, 0.0), pads=(5, 5, 3, 3))
    n = len(V)
    F = np.concatenate([F, [[2, 3, n]]])                                      # a face that holds c and d: c-d is an edge already
    V = np.concatenate([V, [[1.0, 0.0, 5.0]]])
    m = R.Mesh(F, V)
    assert m.valence(2) == 5 and m.valence(3) == 5
    assert R.flip_eval(m, np.tile([0.0, 0.0, 1.0], (len(V), 1)), 0, 0, 10.0) is None
    F2 = F.copy()
    F2[-1] = [2, n, 4]                                                         # same valences, no c-d edge: passes
    assert R.flip_eval(R.Mesh(F2, V), np.tile([0.0, 0.0, 1.0], (len(V), 1)), 0, 0, 10.0) is not None


def test_split_plan_patterns_and_the_diagonal_tie():
    # one face (0, 1, 2) and its reverse (0, 2, 1): a closed two-face "pillow", edges 0-1 = 4, 1-2 = 5, 2-0 = 3
    # slots: 0: 0->1, 1: 1->2, 2: 2->0 | 3: 0->2, 4: 2->1, 5: 1->0
    V = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], dtype=np.float64)
    F = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)
    flag, mid, count = R.split_plan(F, V, max_len=3.5)
    assert flag.tolist() == [1, 1, 0, 0, 0, 0]                                # the lo -> hi slots of the two long edges
    assert mid.tolist() == [3, 4, -1, -1, 4, 3] and count.tolist() == [3, 3]   # numbered in slot order, the same id on both sides
    F2, V2 = R.split_apply(F, V, mid)
    np.testing.assert_array_equal(V2[3:], [[2.0, 0.0, 0.0], [2.0, 1.5, 0.0]])
    # face 0: a = 0, b = 1, c = 2, |a - mbc| = 2.5 > |mab - c| = sqrt 13 ? no: 2.5 < 3.6 -> a-mbc
    assert F2.tolist()[:3] == [[3, 1, 4], [0, 3, 4], [0, 4, 2]]
    flag, mid, count = R.split_plan(F, V, max_len=2.0)                        # all three: 1 -> 4
    assert flag.sum() == 3 and count.tolist() == [4, 4]
    F4, _ = R.split_apply(F, V, mid)
    assert len(F4) == 8 and F4[3].tolist() == [mid[0], mid[1], mid[2]]
    # the diagonal tie: |a - mbc| = |(0,0) - (2,1)| = sqrt 5 = |mab - c| = |(1,0) - (2,2)|: a-mbc
    Vs = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0]], dtype=np.float64)
    out, Vo = R.split_apply(np.array([[0, 1, 2]]), Vs, np.array([3, 4, -1]))
    np.testing.assert_array_equal(Vo[3:], [[1.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
    assert out.tolist() == [[3, 1, 4], [0, 3, 4], [0, 4, 2]]
    Vs[2] = [1.0, 1.0, 0.0]                                                   # |a - mbc| = sqrt 2.5 > |mab - c| = 1 now: mab-c
    out, _ = R.split_apply(np.array([[0, 1, 2]]), Vs, np.array([3, 4, -1]))
    assert out.tolist() == [[3, 1, 4], [0, 3, 2], [3, 4, 2]]


def test_face_agreement_and_move_check():
    F, V = octahedron()
    m = R.Mesh(F, V)
    vn = m.normals()
    a0 = R.face_agreement(F, V, vn)
    np.testing.assert_allclose(a0, 1.0, rtol=0, atol=1e-15)                  # every face agrees with its corners' consensus
    moved = V.copy()
    moved[4] = [0.0, 0.0, -0.5]                                               # +z pushed through: its four faces fold
    revert, n_bad, V2 = R.move_check(F, moved, V, vn, a0)
    assert n_bad == 4 and revert.tolist() == [1, 1, 1, 1, 1, 0]
    np.testing.assert_array_equal(V2, V)
    moved[4] = V[0]                                                           # onto its neighbour +x: two faces lose their area
    revert, n_bad, _ = R.move_check(F, moved, V, vn, a0)
    assert n_bad >= 2 and revert[0] == 1 and revert[4] == 1


@pytest.mark.parametrize("seq, tail_cut, want", [
    # ctl = [live, applied, previous, first, rounds]
    ([(10, [1, 10, 0, 0, 0])], 32, [1, 10, 10, 10, 1]),                      # a first round below tail_cut: goes on (10 // 32 = 0)
    ([(0, [1, 0, 0, 0, 0])], 32, [0, 0, 0, 0, 1]),                            # a first round that applied nothing: over
    ([(64, [1, 64, 0, 0, 0]), (66, [None, 66])], 32, [1, 66, 66, 64, 2]),    # 2 == 64 // 32 exactly: still live
    ([(64, [1, 64, 0, 0, 0]), (65, [None, 65])], 32, [0, 65, 65, 64, 2]),    # 1 < 2: over
    ([(64, [1, 64, 0, 0, 0]), (64, [None, 64])], 32, [0, 64, 64, 64, 2]),    # a zero round: over
])
def test_round_end_state_machine(seq, tail_cut, want):
    ctl = None
    for _, c in seq:
        ctl = list(c) + [0, 0, 0] if ctl is None else ctl
        ctl[1] = c[1]
        ctl = R.round_end(ctl, tail_cut)
    assert ctl[:5] == want
    dead = R.round_end([0, 5, 1, 2, 3, 0, 0, 0], tail_cut)
    assert dead == [0, 5, 1, 2, 3, 0, 0, 0]                                   # a dead step is left alone
