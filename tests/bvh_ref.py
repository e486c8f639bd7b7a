"""A restatement of the device BVH build in numpy, written from the definition of every stage and from no project header.

What the build is (float32 throughout, one rounding per operation):

* scene box: min / max over ALL vertices; ``inv = 1 / extent`` (0 for a flat axis); leaf padding ``pad = largest extent / 8192``;
* plan: 30 key bits, most significant first; each halves the axis along which the cells are longest (ties x, y, z; at most 20 per axis);
* key of a triangle: the centre of its bounding box, per axis quantised to ``bits[a]`` bits (clamped), the bits interleaved by the plan,
  the low ``drop`` bits cleared (6 for meshes of at most 128 sort tiles of 2048 faces, else 0);
* order: the stable sort of the keys;
* hierarchy: the radix tree over the composites ``(key << 32) | slot``, built top-down; an inner node is numbered by the slot it splits at;
* refit: leaf box = min / max of the three vertices -/+ pad, inner boxes = unions;
* records: ``v0, b - a, c - a``, face id, ``margin = pad / 2``;
* wide nodes: the two children of a binary node, then twice the open-able slot of largest surface area opened;
* quantised bounds: stated as properties (conservative, inverted when unused, not looser than measured), not re-implemented.

Arrays are the ones ``optix_mesh.tree_arrays()`` and hostsim's ``hs_export`` return, with the same names and dtypes."""
import numpy as np

F32 = np.float32
NODE = np.dtype([(k, "<f4") for k in ("c0lox", "c0hix", "c0loy", "c0hiy", "c1lox", "c1hix", "c1loy", "c1hiy", "c0loz", "c0hiz", "c1loz", "c1hiz")]
                + [(k, "<i4") for k in ("child0", "child1", "pad0", "pad1")])
NODE4Q = np.dtype([(k, "<f4") for k in ("ox", "oy", "oz", "sx", "sy", "sz")]
                  + [(k, "u1", (4,)) for k in ("qlox", "qloy", "qloz", "qhix", "qhiy", "qhiz")] + [("child", "<i4", (4,))])
TRIREC = np.dtype([("v0", "<f4", (3,)), ("face", "<i4"), ("e1", "<f4", (3,)), ("margin", "<f4"), ("e2", "<f4", (3,)), ("pad1", "<f4")])
PARAMS = np.dtype(dict(names=["lo", "inv", "pad", "reserved", "axis", "pos", "bits", "plan_pad"], offsets=[0, 12, 24, 28, 32, 62, 92, 95], itemsize=100,
                       formats=[("<f4", (3,)), ("<f4", (3,)), "<f4", "<i4", ("u1", (30,)), ("u1", (30,)), ("u1", (3,)), ("u1", (3,))]))   # two bytes of padding follow
ARRAYS = ("keys", "order", "nodes", "parent_inner", "parent_leaf", "range_lo", "range_hi", "wide", "tris", "tris_flat", "slot_of_face", "params")
DTYPES = dict(keys=np.uint32, order=np.uint32, nodes=NODE, parent_inner=np.int32, parent_leaf=np.int32, range_lo=np.int32, range_hi=np.int32,
              wide=NODE4Q, tris=TRIREC, tris_flat=TRIREC, slot_of_face=np.int32, params=PARAMS)
EMPTY_CHILD = -2 ** 31
SORT_TILE, FUSED_TILES = 2048, 128


def drop_bits(n):
    """Low key bits the device clears: 6 while the mesh fits the fused sort (at most 128 tiles of 2048 faces)."""
    return 6 if -(-n // SORT_TILE) <= FUSED_TILES else 0


# ---- scene box, plan, keys, order ---------------------------------------------------------------------------------------------------
def params(verts):
    v = np.asarray(verts, F32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext = hi - lo
    with np.errstate(divide="ignore"):
        inv = np.where(ext > 0, F32(1) / ext, F32(0)).astype(F32)
    p = np.zeros((), PARAMS)
    p["lo"], p["inv"], p["pad"] = lo, inv, ext.max() / F32(8192)
    p["axis"], p["pos"], p["bits"] = plan(ext)
    return p


def plan(ext):
    cell = [max(float(e), 0.0) for e in ext]
    axis, bits = [], [0, 0, 0]
    for _ in range(30):
        a = max((c for c in range(3) if bits[c] < 20), key=lambda c: (cell[c], -c))      # the longest cell axis, ties x, y, z
        axis.append(a)
        bits[a] += 1
        cell[a] /= 2
    used, pos = [0, 0, 0], []
    for a in axis:                       # an axis' bits are handed out most significant first
        used[a] += 1
        pos.append(bits[a] - used[a])
    return axis, pos, bits


def keys(faces, verts, p, drop):
    v = np.asarray(verts, F32).reshape(-1, 3)[np.asarray(faces).reshape(-1, 3)]          # [n, 3 corners, 3 axes]
    centre = F32(0.5) * (v.min(1) + v.max(1))
    t = (centre - p["lo"]) * p["inv"]
    scale = np.ldexp(F32(1), p["bits"].astype(np.int32)).astype(F32)
    q = np.minimum(np.maximum(t * scale, F32(0)), scale - F32(1)).astype(np.uint32)      # truncation of a value in [0, 2^bits - 1]
    key = np.zeros(len(v), np.uint32)
    for k in range(30):
        key |= ((q[:, p["axis"][k]] >> np.uint32(p["pos"][k])) & np.uint32(1)) << np.uint32(29 - k)
    return key & ~np.uint32((1 << drop) - 1)


def order_of(key):
    return np.argsort(key, kind="stable").astype(np.uint32)


# ---- hierarchy ----------------------------------------------------------------------------------------------------------------------
def _top_bit(x):
    """Index of the highest set bit of every (non-zero) uint64."""
    hi, lo = (x >> np.uint64(32)).astype(np.float64), (x & np.uint64(0xFFFFFFFF)).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(hi > 0, 32 + np.floor(np.log2(np.maximum(hi, 1))), np.floor(np.log2(np.maximum(lo, 1)))).astype(np.uint64)


def hierarchy(sorted_keys):
    """nodes (links only), parent_inner, parent_leaf, range_lo, range_hi of the radix tree over (key << 32) | slot, top-down from the root."""
    n = len(sorted_keys)
    inner = max(n - 1, 1)
    nodes = np.zeros(inner, NODE)
    parent_inner, parent_leaf = np.full(inner, -1, np.int32), np.full(n, -1, np.int32)
    range_lo, range_hi = np.zeros(inner, np.int32), np.zeros(inner, np.int32)
    if n == 1:      # the documented special case: both children are the one leaf, which hangs in slot 0
        nodes["child0"] = nodes["child1"] = ~0
        parent_leaf[0] = 0
        return nodes, parent_inner, parent_leaf, range_lo, range_hi
    comp = (np.asarray(sorted_keys).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    node, lo, hi = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, n - 1, np.int64)
    while len(node):
        range_lo[node], range_hi[node] = lo, hi
        b = _top_bit(comp[lo] ^ comp[hi])
        first_one = (comp[hi] >> b) << b                            # the smallest composite of this node that has bit b set
        g = np.searchsorted(comp, first_one, side="left") - 1       # the last slot with a 0 in bit b
        assert np.all((g >= lo) & (g < hi))
        nxt = []
        for slot, (clo, chi, idx) in enumerate(((lo, g, g), (g + 1, hi, g + 1))):
            leaf = clo == chi
            nodes["child%d" % slot][node] = np.where(leaf, ~clo, idx)
            link = (2 * node + slot).astype(np.int32)
            parent_leaf[clo[leaf]] = link[leaf]
            parent_inner[idx[~leaf]] = link[~leaf]
            nxt.append((idx[~leaf], clo[~leaf], chi[~leaf]))
        node, lo, hi = (np.concatenate([a[k] for a in nxt]) for k in range(3))
    return nodes, parent_inner, parent_leaf, range_lo, range_hi


# ---- refit, records -----------------------------------------------------------------------------------------------------------------
def leaf_boxes(faces, verts, order, pad):
    """[n, 6] = lo xyz, hi xyz of every slot's triangle, grown by pad."""
    v = np.asarray(verts, F32).reshape(-1, 3)[np.asarray(faces).reshape(-1, 3)[np.asarray(order).astype(np.int64)]]
    return np.concatenate([v.min(1) - F32(pad), v.max(1) + F32(pad)], 1).astype(F32)


def range_boxes(leaf, lo, hi):
    """Union of the leaf boxes of the slots lo..hi (inclusive) for every pair: exact, min and max do not round.  (Two overlapping
    power-of-two windows per query from a table of them.)"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    signed = np.concatenate([leaf[:, :3], -leaf[:, 3:]], 1)        # min of the negated upper bounds
    level = np.frexp(hi - lo + 1)[1] - 1                            # floor(log2(length))
    out = np.empty((len(lo), 6), F32)
    table, width = signed, 1
    for k in range(int(level.max()) + 1 if len(lo) else 0):
        if k:
            table, width = np.minimum(table[:-width], table[width:]), 2 * width
        m = level == k
        out[m] = np.minimum(table[lo[m]], table[hi[m] - width + 1])
    out[:, 3:] = -out[:, 3:]
    return out


def child_ranges(nodes, range_lo, range_hi, slot):
    c = nodes["child%d" % slot].astype(np.int64)
    leaf = c < 0
    ci = np.where(leaf, 0, c)
    return np.where(leaf, ~c, range_lo[ci]), np.where(leaf, ~c, range_hi[ci])


_BOX_FIELDS = ("c%dlox", "c%dloy", "c%dloz", "c%dhix", "c%dhiy", "c%dhiz")


def refit(nodes, range_lo, range_hi, leaf):
    """The binary nodes with both child boxes filled in (a copy)."""
    out = nodes.copy()
    n = len(leaf)
    if n == 1:      # the leaf's box arrives in slot 0; nothing ever writes slot 1
        boxes = [leaf, np.array([[np.inf] * 3 + [-np.inf] * 3], F32)]
    else:
        boxes = [range_boxes(leaf, *child_ranges(nodes, range_lo, range_hi, s)) for s in (0, 1)]
    for s in (0, 1):
        for k, f in enumerate(_BOX_FIELDS):
            out[f % s] = boxes[s][:, k]
    return out


def node_boxes(nodes, slot):
    return np.stack([nodes[f % slot] for f in _BOX_FIELDS], 1)


def records(faces, verts, order, pad):
    f = np.asarray(order).astype(np.int64)
    v = np.asarray(verts, F32).reshape(-1, 3)[np.asarray(faces).reshape(-1, 3)[f]]
    r = np.zeros(len(f), TRIREC)
    r["v0"], r["e1"], r["e2"] = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    r["face"], r["margin"] = f, F32(0.5) * F32(pad)
    return r


def inverse(order):
    inv = np.empty(len(order), np.int32)
    inv[np.asarray(order).astype(np.int64)] = np.arange(len(order), dtype=np.int32)
    return inv


# ---- wide nodes ---------------------------------------------------------------------------------------------------------------------
def _area(b):
    d = b[..., 3:] - b[..., :3]
    return (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]


def collapse(nodes, range_lo, range_hi, n, leaf_bits=0):
    """(child [I, 4] int32, box [I, 4, 6] float32, written [I] bool) of the wide node rooted at every binary node."""
    inner = len(nodes)
    leaf_max = 1 << leaf_bits
    child = np.full((inner, 4), EMPTY_CHILD, np.int64)
    box = np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, F32), (inner, 4, 1))
    count = range_hi.astype(np.int64) - range_lo + 1
    written = count > leaf_max
    written[0] = True
    if n <= leaf_max:       # the whole mesh is one leaf under the root
        box[0, 0] = np.concatenate([np.minimum(node_boxes(nodes, 0)[0, :3], node_boxes(nodes, 1)[0, :3]), np.maximum(node_boxes(nodes, 0)[0, 3:], node_boxes(nodes, 1)[0, 3:])])
        child[0, 0] = ~(n - 1)
        return child.astype(np.int32), box, written

    def entries(of):        # the two children of the binary nodes `of` as (reference, open-able, box)
        res = []
        for s in (0, 1):
            c = nodes["child%d" % s][of].astype(np.int64)
            ci = np.where(c < 0, 0, c)
            first, cnt = np.where(c < 0, ~c, range_lo[ci]), np.where(c < 0, 1, count[ci])
            is_leaf = cnt <= leaf_max
            res.append((np.where(is_leaf, ~((first << leaf_bits) | (cnt - 1)), c), ~is_leaf, node_boxes(nodes, s)[of]))
        return res

    rows = np.arange(inner)
    is_open = np.zeros((inner, 4), bool)
    for s, (r, o, b) in enumerate(entries(rows)):
        child[:, s], is_open[:, s], box[:, s] = r, o, b
    for used in (2, 3):
        with np.errstate(invalid="ignore", over="ignore"):
            area = np.where(is_open, _area(box), -np.inf)
        pick = np.argmax(area, 1)                                   # the first of the largest
        go = area[rows, pick] > -1
        g, p = rows[go], pick[go]
        k = np.sum(child[g] != EMPTY_CHILD, 1)                       # the next free slot
        (r0, o0, b0), (r1, o1, b1) = entries(child[g, p])
        child[g, p], is_open[g, p], box[g, p] = r0, o0, b0
        child[g, k], is_open[g, k], box[g, k] = r1, o1, b1
    return child.astype(np.int32), box, written


# ---- quantised bounds as properties -------------------------------------------------------------------------------------------------
def fma32(q, s, o):
    """float32(o + q * s) with ONE rounding (q an integer below 2^8, s and o float32), as a fused multiply-add gives it."""
    a = np.asarray(q, np.float64) * np.asarray(s, np.float64)       # exact: 8 x 24 bits
    o = np.broadcast_to(np.asarray(o, np.float64), a.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        total = o + a
        z = total - o
        err = (o - (total - z)) + (a - z)                           # two-sum: o + a == total + err exactly
        r = total.astype(F32)
        d = total - r.astype(np.float64)
        toward = np.where(d > 0, np.inf, -np.inf).astype(F32)
        other = np.nextafter(r, toward)
        tie = (d != 0) & np.isfinite(other) & (2 * d == other.astype(np.float64) - r.astype(np.float64))
        beyond = tie & (err * d > 0)                                # the exact sum lies past the midpoint the float64 sum sits on
    return np.where(beyond, other, r).astype(F32)


def wide_slot_boxes(wide, range_lo, range_hi, leaf, leaf_bits=0):
    """[I, 4, 6] float32 box of what every used slot of a wide node covers (a binary node's slots, or a leaf's run of slots)."""
    c = wide["child"].astype(np.int64)
    used = c != EMPTY_CHILD
    enc = ~c
    is_leaf = c < 0
    ci = np.where(is_leaf | ~used, 0, c)
    lo = np.where(is_leaf, enc >> leaf_bits, range_lo[ci])
    hi = np.where(is_leaf, (enc >> leaf_bits) + (enc & ((1 << leaf_bits) - 1)), range_hi[ci])
    lo, hi = np.where(used, lo, 0), np.where(used, hi, 0)
    return range_boxes(leaf, lo.ravel(), hi.ravel()).reshape(len(wide), 4, 6), used


def _ordinal(f):
    """float32 -> integers in the same order, consecutive for neighbouring floats."""
    b = np.asarray(f, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def quant_report(wide, slot_box, used, written):
    """(violations, worst slack) of the byte bounds of the written wide nodes against the float32 boxes of their slots.

    violations: used slots whose decoded interval ``fma32(q, scale, origin)`` does not contain the box on some axis, plus unused slots
    that are not the inverted interval (255, 0) on all axes.
    slack of a byte: how many grid steps it could move inwards and stay conservative -- counted in float32 values where the grid is finer
    than float32 is there (a node a few ulps across: many bytes decode to the same bound, and moving between them tightens nothing)."""
    w = np.asarray(written)
    bad, slack = 0, 0
    u = used[w]
    for a, ax in enumerate("xyz"):
        o = wide["o" + ax][w][:, None]
        s = (wide["s" + ax][w] * F32(2.0 ** -24))[:, None]         # exact: a power of two
        qlo, qhi = wide["qlo" + ax][w].astype(np.int64), wide["qhi" + ax][w].astype(np.int64)
        lo, hi = slot_box[w][:, :, a], slot_box[w][:, :, 3 + a]
        ok = (fma32(qlo, s, o) <= lo) & (fma32(qhi, s, o) >= hi)
        bad += int(np.sum(u & ~ok)) + int(np.sum(~u & ~((qlo == 255) & (qhi == 0))))
        # the tightest conservative bytes, by bisection (the decoded bound does not decrease with the byte)
        L, R = qlo.copy(), np.full_like(qlo, 255)
        for _ in range(8):
            mid = (L + R + 1) // 2
            fits = fma32(mid, s, o) <= lo
            L, R = np.where(fits, mid, L), np.where(fits, R, mid - 1)
        tight_lo = L
        L, R = np.zeros_like(qhi), qhi.copy()
        for _ in range(8):
            mid = (L + R) // 2
            fits = fma32(mid, s, o) >= hi
            L, R = np.where(fits, L, mid + 1), np.where(fits, mid, R)
        tight_hi = R
        steps_lo = np.minimum(tight_lo - qlo, _ordinal(fma32(tight_lo, s, o)) - _ordinal(fma32(qlo, s, o)))
        steps_hi = np.minimum(qhi - tight_hi, _ordinal(fma32(qhi, s, o)) - _ordinal(fma32(tight_hi, s, o)))
        both = np.where(u & ok, np.maximum(steps_lo, steps_hi), 0)
        slack = max(slack, int(both.max()) if both.size else 0)
    return bad, slack


# ---- whole builds -------------------------------------------------------------------------------------------------------------------
def refit_on(topology, faces, verts, flat_order=None, leaf_bits=0):
    """Boxes, records and wide children of a KEPT topology (order, links, ranges of `topology`) for new vertices."""
    out = dict(topology)
    n = len(out["order"])
    p = params(verts)
    out["params"] = p
    leaf = leaf_boxes(faces, verts, out["order"], p["pad"])
    out["nodes"] = refit(out["nodes"], out["range_lo"], out["range_hi"], leaf)
    out["tris"] = records(faces, verts, out["order"], p["pad"])
    out["tris_flat"] = records(faces, verts, np.arange(n) if flat_order is None else flat_order, p["pad"])
    out["slot_of_face"] = inverse(out["order"])
    out["leaf"] = leaf
    out["wide_child"], out["wide_box"], out["wide_written"] = collapse(out["nodes"], out["range_lo"], out["range_hi"], n, leaf_bits)
    return out


def build(faces, verts, drop=None, flat_order=None, leaf_bits=0, upto="all"):
    """Every array of a full build.  ``flat_order``: the order the previous build left (None: face order, as after update_mesh).
    ``upto="order"`` stops after params, keys and order (large cases)."""
    faces = np.asarray(faces).reshape(-1, 3)
    n = len(faces)
    p = params(verts)
    key = keys(faces, verts, p, drop_bits(n) if drop is None else drop)
    order = order_of(key)
    out = dict(params=p, keys=key[order], order=order)
    if upto == "order":
        return out
    out["nodes"], out["parent_inner"], out["parent_leaf"], out["range_lo"], out["range_hi"] = hierarchy(out["keys"])
    return refit_on(out, faces, verts, flat_order, leaf_bits)


# ---- properties of any topology -----------------------------------------------------------------------------------------------------
def check_topology(arrays, n):
    """The reasons (strings; none when sound) why order / nodes / parents / ranges are not a binary tree over the n leaf slots."""
    errs = []
    order = np.asarray(arrays["order"]).astype(np.int64)
    if len(order) != n or not np.array_equal(np.sort(order), np.arange(n)):
        errs.append("order is not a permutation")
    nodes, pi, pl, rlo, rhi = (arrays[k] for k in ("nodes", "parent_inner", "parent_leaf", "range_lo", "range_hi"))
    inner = max(n - 1, 1)
    if not (len(nodes) == len(pi) == len(rlo) == len(rhi) == inner and len(pl) == n):
        return errs + ["array sizes"]
    c = np.stack([nodes["child0"], nodes["child1"]], 1).astype(np.int64)
    if n == 1:
        if not (np.all(c == ~0) and pl[0] == 0 and pi[0] == -1 and rlo[0] == 0 and rhi[0] == 0):
            errs.append("single-triangle tree is not the documented special case")
        return errs
    link = 2 * np.arange(inner)[:, None] + np.arange(2)[None, :]
    leaf = c < 0
    if np.any(c[~leaf] >= inner) or np.any(~c[leaf] >= n):
        return errs + ["child reference out of range"]
    if not np.array_equal(np.bincount(c[~leaf], minlength=inner), np.r_[0, np.ones(inner - 1, np.int64)]):
        errs.append("an inner node has no or several parents (or the root has one)")
    if not np.array_equal(np.bincount(~c[leaf], minlength=n), np.ones(n, np.int64)):
        errs.append("a leaf slot is referenced never or several times")
    if pi[0] != -1 or np.any(pi[c[~leaf]] != link[~leaf]) or np.any(pl[~c[leaf]] != link[leaf]):
        errs.append("parent links do not mirror the child links")
    clo = np.where(leaf, ~c, rlo[np.where(leaf, 0, c)])
    chi = np.where(leaf, ~c, rhi[np.where(leaf, 0, c)])
    if np.any(clo[:, 0] != rlo) or np.any(chi[:, 0] + 1 != clo[:, 1]) or np.any(chi[:, 1] != rhi) or np.any(clo > chi):
        errs.append("a node's range is not its children's ranges one after the other")
    if rlo[0] != 0 or rhi[0] != n - 1:
        errs.append("the root does not cover every slot")
    # walk down from the root: every inner node and every leaf slot is reached, once
    seen_inner, seen_leaf = np.zeros(inner, np.int64), np.zeros(n, np.int64)
    front, steps = np.zeros(1, np.int64), 0
    while len(front) and steps <= n:
        np.add.at(seen_inner, front, 1)
        cc = c[front].ravel()
        np.add.at(seen_leaf, ~cc[cc < 0], 1)
        front, steps = cc[cc >= 0], steps + 1
    if np.any(seen_inner != 1) or np.any(seen_leaf != 1):
        errs.append("the walk from the root does not reach every node and leaf slot exactly once")
    return errs


# ---- comparing two sets of arrays ---------------------------------------------------------------------------------------------------
def same(a, b):
    """Equal entry by entry: integers bit for bit, floats by value (so -0.0 == +0.0) and never NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.names:
        return a.dtype.names == b.dtype.names and all(same(a[f], b[f]) for f in a.dtype.names)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return not np.isnan(a).any() and not np.isnan(b).any() and bool(np.all(a == b))
    return bool(np.array_equal(a, b))


def differing(got, want, names=None, wide="struct"):
    """Names of the arrays of `got` that are not those of `want` (a build of this module or another export).  Wide nodes are compared
    where the build writes them (``want["wide_written"]`` or, for an export, every node of more than one triangle and the root):
    their whole 64 bytes against another export, their child references against this module's collapse."""
    out = []
    for name in (names or [k for k in ARRAYS if k in want or (k == "wide" and "wide_child" in want)]):
        if name == "wide":
            written = want["wide_written"] if "wide_written" in want else np.r_[True, (got["range_hi"] > got["range_lo"])[1:]]
            ok = same(got["wide"]["child"][written], want["wide_child"][written]) if "wide_child" in want else same(got["wide"][written], want["wide"][written])
        else:
            ok = same(got[name], want[name])
        if not ok:
            out.append(name)
    return out
