"""TEST CODE ONLY -- a float64 host reference of every stage of the device remesher (drt_amd/csrc/drt_remesh_gpu.hip).

Each function restates one rule of drt_amd/csrc/drt_remesh.cpp / the contract comments of the device kernels in plain numpy and Python
floats: sets where the rule speaks of sets, explicit loops where it speaks of an order.  It is held against hand-worked answers in
tests/test_remesh_ref.py and the device kernels are held against it in tests/test_gpu_remesh_kernels.py.

Arithmetic that decides bits is written one rounding per operation, in the order the library evaluates it (the library is built with
-ffp-contract=off): cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z,
|u| = sqrt(dot(u, u)), sums left to right.  Python floats and numpy float64 element-wise operations are IEEE double with one rounding
each, so where the kernel and this module evaluate the same expression in the same order, they agree bit for bit.

Meshes: V float64 [nv, 3], F int64 [nf, 3]; a face a collapse round killed holds -1 in all three places and belongs to nobody.
"""
from __future__ import annotations

import math

import numpy as np

MAX_RING = 32               # a vertex with more faces than this is left alone by the collapse and the relaxation


# ---- vector arithmetic on 3-tuples of Python floats (one rounding per operation) -----------------------------------------------------
def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _add(u, v):
    return (u[0] + v[0], u[1] + v[1], u[2] + v[2])


def _scale(u, s):
    return (u[0] * s, u[1] * s, u[2] * s)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _len(u):
    return math.sqrt(_dot(u, u))


def _p(V, i):
    return (float(V[i, 0]), float(V[i, 1]), float(V[i, 2]))


def tri_normal(a, b, c):
    """Twice the area vector of triangle abc: (b - a) x (c - a)."""
    return _cross(_sub(b, a), _sub(c, a))


def agreement(n, vn, a, b, c):
    """Cosine between face normal n and the consensus (vn[a] + vn[b]) + vn[c]; 1 without a consensus, -1 for a face without area."""
    r = _add(_add(_p(vn, a), _p(vn, b)), _p(vn, c))
    ln, lr = _len(n), _len(r)
    if ln > 0 and lr > 0:
        return _dot(n, r) / (ln * lr)
    return 1.0 if ln > 0 else -1.0


def acceptable(before, after):
    """A changed face is acceptable when it agrees with the consensus (cosine >= 0.3), or at least no less than it did before."""
    return after >= 0.3 or after >= before


# ---- vertex -> face lists and vertex normals -----------------------------------------------------------------------------------------
def vertex_faces(F, nv):
    """CSR (start int64 [nv+1], faces int64 [3 nf']) of the faces around each vertex, ascending inside a vertex; rows of -1 in no list."""
    F = np.asarray(F, dtype=np.int64)
    corner = F.reshape(-1)
    face = np.repeat(np.arange(len(F), dtype=np.int64), 3)
    keep = corner >= 0
    corner, face = corner[keep], face[keep]
    order = np.lexsort((face, corner))
    start = np.zeros(nv + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(corner, minlength=nv))
    return start, face[order]


def face_normals(F, V):
    """tri_normal of every face, vectorised (same operations as tri_normal); rows of -1 give garbage and must not be read."""
    Fc = np.where(F >= 0, F, 0)
    a, b, c = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
    u, w = b - a, c - a
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def vertex_normals(F, V, start, vf):
    """Area-weighted vertex normals: the sum of the face normals of a vertex in ascending face order, starting from 0."""
    F, V = np.asarray(F, dtype=np.int64), np.asarray(V, dtype=np.float64)
    fn = face_normals(F, V)
    nv = len(start) - 1
    val = np.diff(start)
    s = np.zeros((nv, 3))
    for k in range(int(val.max()) if nv else 0):           # k-th face of every vertex that has one: the sums run in list order
        vs = np.nonzero(val > k)[0]
        s[vs] = s[vs] + fn[vf[start[vs] + k]]
    return s


class Mesh:
    """A mesh with its vertex -> face lists: the view every evaluation rule reads."""

    def __init__(self, F, V):
        self.F = np.array(F, dtype=np.int64).reshape(-1, 3)
        self.V = np.array(V, dtype=np.float64).reshape(-1, 3)
        self.start, self.vf = vertex_faces(self.F, len(self.V))

    def faces(self, v):
        return [int(f) for f in self.vf[self.start[v]:self.start[v + 1]]]

    def valence(self, v):
        return int(self.start[v + 1] - self.start[v])

    def neighbours(self, v):
        return {int(u) for f in self.faces(v) for u in self.F[f] if u != v}

    def tri(self, f):
        return tuple(int(x) for x in self.F[f])

    def normals(self):
        return vertex_normals(self.F, self.V, self.start, self.vf)


# ---- split -------------------------------------------------------------------------------------------------------------------------
def split_plan(F, V, max_len):
    """The refine step's plan over directed-edge slots c = 3 f + k (edge F[f,k] -> F[f,k+1]).

    flag[c]: the slot is the lo -> hi side of an edge longer than max_len.  The flagged slots, in slot order, number the new vertices
    nv, nv + 1, ...; mid[c] is that number on BOTH slots of a flagged edge, -1 everywhere else.  count[f] = 1 + split edges of f."""
    F, V = np.asarray(F, dtype=np.int64), np.asarray(V, dtype=np.float64)
    nf, nv = len(F), len(V)
    flag = np.zeros(3 * nf, dtype=np.uint8)
    slot_of = {}
    for f in range(nf):
        for k in range(3):
            a, b = int(F[f, k]), int(F[f, (k + 1) % 3])
            if a >= 0:
                slot_of[(a, b)] = 3 * f + k
                flag[3 * f + k] = a < b and _len(_sub(_p(V, a), _p(V, b))) > max_len
    mid = np.full(3 * nf, -1, dtype=np.int64)
    n_split = 0
    for c in np.nonzero(flag)[0]:
        f, k = divmod(int(c), 3)
        a, b = int(F[f, k]), int(F[f, (k + 1) % 3])
        mid[c] = nv + n_split
        if (b, a) in slot_of:
            mid[slot_of[(b, a)]] = nv + n_split
        n_split += 1
    count = 1 + (mid.reshape(nf, 3) >= 0).sum(1)
    return flag, mid, count


def split_apply(F, V, mid):
    """New vertices (V, then the midpoints (V[lo] + V[hi]) * 0.5 in number order) and faces (each face's pattern in face order):
    one split edge (a, b) -> (a, m, c), (m, b, c); two, (a, b) and (b, c) with (c, a) whole -> (mab, b, mbc) and the shorter diagonal,
    a-mbc when |a - mbc| <= |mab - c| (a tie takes a-mbc), else mab-c; three -> the four-face pattern."""
    F, V = np.asarray(F, dtype=np.int64), np.asarray(V, dtype=np.float64)
    nv = len(V)
    n_new = int(mid.max()) + 1 - nv if (mid >= 0).any() else 0
    newV = np.empty((nv + n_new, 3))
    newV[:nv] = V
    for c in np.nonzero(mid >= 0)[0]:
        f, k = divmod(int(c), 3)
        a, b = int(F[f, k]), int(F[f, (k + 1) % 3])
        if a < b:
            newV[mid[c]] = _scale(_add(_p(V, a), _p(V, b)), 0.5)
    out = []
    for f in range(len(F)):
        v = [int(x) for x in F[f]]
        m = [int(x) for x in mid[3 * f:3 * f + 3]]
        n = sum(x >= 0 for x in m)
        if n == 0:
            out.append(v)
        elif n == 3:
            out += [[v[0], m[0], m[2]], [m[0], v[1], m[1]], [m[2], m[1], v[2]], [m[0], m[1], m[2]]]
        elif n == 1:
            r = [x >= 0 for x in m].index(True)
            a, b, c = v[r], v[(r + 1) % 3], v[(r + 2) % 3]
            out += [[a, m[r], c], [m[r], b, c]]
        else:
            r = ([x < 0 for x in m].index(True) + 1) % 3            # the whole edge is (c, a)
            a, b, c = v[r], v[(r + 1) % 3], v[(r + 2) % 3]
            mab, mbc = m[r], m[(r + 1) % 3]
            out.append([mab, b, mbc])
            if _len(_sub(_p(newV, a), _p(newV, mbc))) <= _len(_sub(_p(newV, mab), _p(newV, c))):
                out += [[a, mab, mbc], [a, mbc, c]]
            else:
                out += [[a, mab, c], [mab, mbc, c]]
    return np.array(out, dtype=np.int64).reshape(-1, 3), newV


# ---- collapse ----------------------------------------------------------------------------------------------------------------------
def collapse_eval(mesh, vn, a, b, min_len, max_len, max_q):
    """Whether edge (a, b) may collapse into its midpoint, and its surface-distance query points: (ok, [points]).

    Rules: |a - b| < min_len; neither end has more than MAX_RING faces; a and b have exactly two common neighbours (link condition);
    both have valence >= 4; valence(a) + valence(b) - 4 >= 3; every face around a or b that does not hold both (those die), with a
    or b moved to the midpoint m, keeps an area above 1e-12 (1 + its old area), is acceptable to the consensus normals vn, and has no
    edge to m longer than max_len.  Query points: m, then the centroid ((p0 + p1) + p2) / 3 of every surviving face after the move, a's
    faces then b's, ascending; more than max_q of them and the edge is left alone."""
    pa, pb = _p(mesh.V, a), _p(mesh.V, b)
    if not _len(_sub(pa, pb)) < min_len:
        return False, []
    if mesh.valence(a) > MAX_RING or mesh.valence(b) > MAX_RING:
        return False, []
    common = (mesh.neighbours(a) & mesh.neighbours(b)) - {a, b}
    if len(common) != 2:
        return False, []
    if any(mesh.valence(u) < 4 for u in common):
        return False, []
    if mesh.valence(a) + mesh.valence(b) - 4 < 3:
        return False, []
    m = _scale(_add(pa, pb), 0.5)
    q = [m]
    for v in (a, b):
        for f in mesh.faces(v):
            t = mesh.tri(f)
            if a in t and b in t:
                continue
            p = [_p(mesh.V, x) for x in t]
            n0 = tri_normal(*p)
            p = [m if x == v else pk for x, pk in zip(t, p)]
            n1 = tri_normal(*p)
            if not _len(n1) > 1e-12 * (1.0 + _len(n0)):
                return False, []
            if not acceptable(agreement(n0, vn, *t), agreement(n1, vn, *t)):
                return False, []
            if any(x != v and _len(_sub(pk, m)) > max_len for x, pk in zip(t, p)):
                return False, []
            q.append(_scale(_add(_add(p[0], p[1]), p[2]), 1.0 / 3.0))
    if len(q) > max_q:
        return False, []
    return True, q


def collapse_eval_all(F, V, vn, min_len, max_len, max_q):
    """collapse_eval over every directed-edge slot c = 3 f + k: the lo -> hi slot of an edge speaks for it, every other slot (and those
    of killed faces) reports not ok.  Returns (ok uint8 [3F], n_query int32 [3F], q {slot: points}, E_snap int64 [3F,2], length [3F])."""
    mesh = F if isinstance(F, Mesh) else Mesh(F, V)
    F, V = mesh.F, mesh.V
    nf = len(F)
    a = F.reshape(-1)
    b = F[:, [1, 2, 0]].reshape(-1)
    E_snap = np.stack([a, b], 1)
    own = (a >= 0) & (a < b)
    length = np.zeros(3 * nf)
    d = V[np.where(own, a, 0)] - V[np.where(own, b, 0)]
    length[own] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[own]
    ok = np.zeros(3 * nf, dtype=np.uint8)
    n_query = np.zeros(3 * nf, dtype=np.int32)
    q = {}
    for c in np.nonzero(own & (length < min_len))[0]:
        good, pts = collapse_eval(mesh, vn, int(a[c]), int(b[c]), min_len, max_len, max_q)
        if good:
            ok[c], n_query[c], q[int(c)] = 1, len(pts), pts
    return ok, n_query, q, E_snap, length


def collapse_apply(F, V, pairs):
    """The collapses (a, b) applied one after the other: a moves to the midpoint of a and b as they are at that moment, the faces that
    hold both a and b die (rows of -1), b becomes a in every other face."""
    F, V = np.array(F, dtype=np.int64), np.array(V, dtype=np.float64)
    for a, b in pairs:
        m = _scale(_add(_p(V, a), _p(V, b)), 0.5)
        has_a, has_b = (F == a).any(1), (F == b).any(1)
        F[has_a & has_b] = -1
        F[F == b] = a
        V[a] = m
    return F, V


# ---- flip --------------------------------------------------------------------------------------------------------------------------
def flip_eval(mesh, vn, f1, k1, max_len):
    """The flip of the edge of slot 3 f1 + k1 -- a -> b in face f1 = (a, b, c), b -> a in its neighbour f2 = (b, a, d) -- into the edge
    (c, d), faces (c, a, d) and (d, b, c).  Returns (a, b, c, d, f1, f2) when it passes, else None.

    Rules: the slot is the lo -> hi side (a < b); f2 exists; c, d distinct and distinct from a, b; valence(a), valence(b) >= 4; both new
    faces keep an area above 1e-12 (1 + old area); then, when the pair is folded (n1 . n2 < -0.5 |n1| |n2|), the new pair must not be
    (m1 . m2 >= 0.5 |m1| |m2|) and each new face must agree with the consensus (cosine >= 0.3); otherwise the valence deviation from 6
    must drop, the pair must be nearly flat (n1 . n2 >= 0.94 |n1| |n2|) and each new face within 60 degrees of each old one.  Last: the
    edge (c, d) must not exist already and be no longer than max_len."""
    t1 = mesh.tri(f1)
    a, b, c = t1[k1], t1[(k1 + 1) % 3], t1[(k1 + 2) % 3]
    if a < 0 or not a < b:
        return None
    f2 = d = -1
    for f in mesh.faces(b):
        t = mesh.tri(f)
        for k in range(3):
            if t[k] == b and t[(k + 1) % 3] == a:
                f2, d = f, t[(k + 2) % 3]
    if f2 < 0 or c == d or c in (a, b) or d in (a, b):
        return None
    va, vb, vc, vd = (mesh.valence(x) for x in (a, b, c, d))
    if va < 4 or vb < 4:
        return None
    pa, pb, pc, pd = (_p(mesh.V, x) for x in (a, b, c, d))
    n1 = tri_normal(*(_p(mesh.V, x) for x in mesh.tri(f1)))
    n2 = tri_normal(*(_p(mesh.V, x) for x in mesh.tri(f2)))
    m1, m2 = tri_normal(pc, pa, pd), tri_normal(pd, pb, pc)
    l1, l2, k1n, k2n = _len(n1), _len(n2), _len(m1), _len(m2)
    if not k1n > 1e-12 * (1.0 + l1) or not k2n > 1e-12 * (1.0 + l2):
        return None
    if _dot(n1, n2) < -0.5 * l1 * l2:                                 # folded pair: repair
        if _dot(m1, m2) < 0.5 * k1n * k2n:
            return None
        if agreement(m1, vn, c, a, d) < 0.3 or agreement(m2, vn, d, b, c) < 0.3:
            return None
    else:
        before = abs(va - 6) + abs(vb - 6) + abs(vc - 6) + abs(vd - 6)
        after = abs(va - 7) + abs(vb - 7) + abs(vc - 5) + abs(vd - 5)
        if after >= before:
            return None
        if _dot(n1, n2) < 0.94 * l1 * l2:
            return None
        if (_dot(m1, n1) < 0.5 * k1n * l1 or _dot(m1, n2) < 0.5 * k1n * l2 or _dot(m2, n1) < 0.5 * k2n * l1
                or _dot(m2, n2) < 0.5 * k2n * l2):
            return None
    if d in mesh.neighbours(c):
        return None
    if _len(_sub(pc, pd)) > max_len:
        return None
    return (a, b, c, d, f1, f2)


def flip_eval_all(F, V, vn, max_len):
    """flip_eval over every slot: (ok uint8 [3F], quads {slot: (a, b, c, d, f1, f2)}, midpoints {slot: (pc + pd) * 0.5})."""
    mesh = F if isinstance(F, Mesh) else Mesh(F, V)
    nf = len(mesh.F)
    ok = np.zeros(3 * nf, dtype=np.uint8)
    quads, mids = {}, {}
    for c in range(3 * nf):
        r = flip_eval(mesh, vn, c // 3, c % 3, max_len)
        if r is not None:
            ok[c], quads[c] = 1, r
            mids[c] = _scale(_add(_p(mesh.V, r[2]), _p(mesh.V, r[3])), 0.5)
    return ok, quads, mids


def flip_apply(F, quads):
    """The flips applied one after the other: f1 = (c, a, d), f2 = (d, b, c)."""
    F = np.array(F, dtype=np.int64)
    for a, b, c, d, f1, f2 in quads:
        F[f1] = (c, a, d)
        F[f2] = (d, b, c)
    return F


# ---- relaxation and roll-back ------------------------------------------------------------------------------------------------------
def smooth_target(mesh):
    """Tangential relaxation target of every vertex: the centroid g of its neighbours (summed in ascending id order, scaled by 1 / n),
    moved back along the unit area-weighted normal: g + n (n . (p - g)).  A vertex without faces, with a zero normal or with more than
    MAX_RING neighbours stays where it is."""
    out = mesh.V.copy()
    for v in range(len(mesh.V)):
        fs = mesh.faces(v)
        if not fs:
            continue
        n = (0.0, 0.0, 0.0)
        for f in fs:
            n = _add(n, tri_normal(*(_p(mesh.V, x) for x in mesh.tri(f))))
        ln = _len(n)
        if not ln > 0:
            continue
        n = _scale(n, 1.0 / ln)
        ring = sorted(mesh.neighbours(v))
        if len(ring) > MAX_RING or not ring:
            continue
        g = (0.0, 0.0, 0.0)
        for u in ring:
            g = _add(g, _p(mesh.V, u))
        g = _scale(g, 1.0 / len(ring))
        pv = _p(mesh.V, v)
        out[v] = _add(g, _scale(n, _dot(n, _sub(pv, g))))
    return out


def face_agreement(F, V, vn):
    """a0 [F]: agreement of every face with the consensus, vectorised with the operations of agreement()."""
    F, V, vn = np.asarray(F), np.asarray(V, dtype=np.float64), np.asarray(vn, dtype=np.float64)
    n = face_normals(F, V)
    r = (vn[F[:, 0]] + vn[F[:, 1]]) + vn[F[:, 2]]
    dot = lambda u, w: (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
    ln, lr = np.sqrt(dot(n, n)), np.sqrt(dot(r, r))
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot(n, r) / (ln * lr)
    return np.where((ln > 0) & (lr > 0), cos, np.where(ln > 0, 1.0, -1.0))


def move_check(F, V, old, vn, a0):
    """One roll-back round: a face whose normal vanished or that is no longer acceptable against a0 flags its three vertices; the flagged
    vertices go back to `old`.  Returns (revert uint8 [V], n_bad, V after the roll-back)."""
    a1 = face_agreement(F, V, vn)
    n = face_normals(F, V)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    bad = ~(ln > 0) | ~((a1 >= 0.3) | (a1 >= a0))
    revert = np.zeros(len(V), dtype=np.uint8)
    revert[F[bad].reshape(-1)] = 1
    V2 = np.where(revert[:, None] == 1, old, V)
    return revert, int(bad.sum()), V2


# ---- the end of a round ------------------------------------------------------------------------------------------------------------
def round_end(ctl, tail_cut):
    """ctl [8]: [0] live, [1] applied so far, [2] that count at the previous round's end, [3] the first round's count, [4] rounds run.
    A live step records the round (n = [1] - [2]) and stays live while n > 0 and n >= first // tail_cut; a dead step is left alone."""
    ctl = list(ctl)
    if not ctl[0]:
        return ctl
    n = ctl[1] - ctl[2]
    ctl[2] = ctl[1]
    if ctl[4] == 0:
        ctl[3] = n
    ctl[4] += 1
    ctl[0] = int(n > 0 and n >= ctl[3] // tail_cut)
    return ctl
