"""The deterministic mode's claim -- every gradient and loss is the EXACT integer sum of its contributions, truncated at 2^-80, rounded once to
nearest-even, the same bits on any rank count below 2^20 (drt_amd/csrc/drt_fixed.h) -- held against Python integers
on the device: the gfx950 compilation of the conversions, the carry ownership of the two 64-bit atomics under contention, the LDS table of
the path kernels with its probe stride, its overflow to memory and its flush, LossAcc<true>, and the exchange format at its stated range.
tests/devsim/fx_device.hip launches the production structs unchanged; tests/fx_cases.py is the reference (q, the flags, the one rounding)
and the edge lists that tests/test_fixed_point.py runs against the host compilation of the same header.  Cells are compared word for word
and values bit for bit: there is no tolerance in the fixed-point tests.  The one allowance: where a flag is set, LossAcc drops the partial
sum of the wave that saw it (a flagged value does not enter the sum), so a flagged LOSS cell is compared by flags and value only.
The float64 table (HashAdd3 / hash_flush) is compared with math.fsum within the textbook bound of m - 1 rounded additions in any order."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

import fx_cases as fx

pytestmark = pytest.mark.gpu

_P, _I64, _INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
FX_HASH_SIZE, HASH_SIZE, PROBES, BWD_BATCH = 1024, 2048, 24, 1024       # drt_pathsink.h: kFxHashSize, kHashSize, the probe limit, kBwdBatch
BATCHES = (256, BWD_BATCH, 4096)


@pytest.fixture(scope="module")
def dev():
    lib = ctypes.CDLL(fx.build_devsim())
    for name, args in (("dv_direct", [_P, _P, _P, _I64, _INT, _P]), ("dv_sink_det", [_P, _P, _P, _I64, _I64, _INT, _P]),
                       ("dv_sink_f64", [_P, _P, _P, _I64, _I64, _INT, _P]), ("dv_loss", [_P, _P, _I64, _INT, _P])):
        getattr(lib, name).restype = _INT
        getattr(lib, name).argtypes = args
    return lib


# ---- launches: every index is checked HERE, against the size of the target, before anything reaches the device ------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _checked(idx, x, target, words_per_value):
    n_values = target.numel() // words_per_value
    assert target.numel() == n_values * words_per_value and n_values % 3 == 0
    for t in (idx, x, target):
        assert t.is_cuda and t.is_contiguous()
    assert idx.dtype == torch.int32 and x.dtype == torch.float64 and idx.dim() == 1 and x.numel() == 3 * idx.numel()
    if idx.numel():
        assert 0 <= int(idx.min()) and int(idx.max()) < n_values // 3
    return idx.numel()


def _direct(dev, idx, x, n_vert, grid):
    cells = torch.zeros(9 * n_vert, dtype=torch.int64, device="cuda")
    n = _checked(idx, x, cells, 3)
    assert dev.dv_direct(cells.data_ptr(), idx.data_ptr(), x.data_ptr(), n, grid, _stream()) == 0
    return cells


def _sink(dev, idx, x, n_vert, batch, grid):
    cells = torch.zeros(9 * n_vert, dtype=torch.int64, device="cuda")
    n = _checked(idx, x, cells, 3)
    assert dev.dv_sink_det(cells.data_ptr(), idx.data_ptr(), x.data_ptr(), n, batch, grid, _stream()) == 0
    return cells


def _sink_f64(dev, idx, x, n_vert, batch, grid):
    g = torch.zeros(3 * n_vert, dtype=torch.float64, device="cuda")
    n = _checked(idx, x, g, 1)
    assert dev.dv_sink_f64(g.data_ptr(), idx.data_ptr(), x.data_ptr(), n, batch, grid, _stream()) == 0
    return g


def _loss(dev, x, grid):
    cell = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float64 and x.dim() == 1
    assert dev.dv_loss(cell.data_ptr(), x.data_ptr(), x.numel(), grid, _stream()) == 0
    return cell


def _finalize(cells, accumulate=0, out=None):
    from drt_amd import _lib
    assert cells.is_cuda and cells.is_contiguous() and cells.dtype == torch.int64 and cells.numel() % 3 == 0
    n = cells.numel() // 3
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device="cuda")
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and out.numel() == n
    _lib.check(_lib.lib().drt_fx_finalize(cells.data_ptr(), n, out.data_ptr(), accumulate, _stream()))
    return out


def _dev(idx, x):
    return torch.tensor(np.asarray(idx, dtype=np.int32), device="cuda"), torch.tensor(np.asarray(x, dtype=np.float64).reshape(-1), device="cuda")


# ---- the reference: Python integers ---------------------------------------------------------------------------------------------------------
class Ref:
    """Per cell of a target of `n_cells` values: the exact sum of q(x) mod 2^128 as (hi, lo), the OR of the flags, the bits of the value."""

    def __init__(self, idx, x, n_cells):
        sums, flags = {}, {}
        x = np.asarray(x, dtype=np.float64).reshape(-1).tolist()
        for i, v in enumerate(np.asarray(idx).tolist()):
            for c in range(3):
                cell, xv = 3 * v + c, x[3 * i + c]
                f = fx.flags_of(xv)
                if f:
                    flags[cell] = flags.get(cell, 0) | f
                else:
                    sums[cell] = sums.get(cell, 0) + fx.q(xv)
        self.hi, self.lo, self.flags, self.bits = (np.zeros(n_cells, dtype=np.int64) for _ in range(4))
        for cell in set(sums) | set(flags):
            s, f = sums.get(cell, 0), flags.get(cell, 0)
            assert abs(s) < 1 << (47 + fx.FRAC)                         # the range the header states for a sum: the inputs keep it
            self.hi[cell], self.lo[cell] = fx.split(s)
            self.flags[cell] = f
            self.bits[cell] = fx.value_bits(s, f)


def _units(hi, lo):
    return fx.signed128((int(hi) << 64) | (int(lo) & fx.M64))


def check_cells(cells, ref, values=None, flagged_words=True):
    """cells: int64 [n_cells * 3] as the device left them.  Word for word; a mismatch reports the difference in units (2^64: a carry; q(x):
    a whole contribution).  flagged_words=False: a cell with flags is compared by flags (and value) only."""
    got = np.asarray(cells.cpu() if isinstance(cells, torch.Tensor) else cells).reshape(-1, 3)
    assert got.shape[0] == ref.flags.shape[0]
    bad = np.nonzero(got[:, 2] != ref.flags)[0]
    assert bad.size == 0, f"flags of cell {bad[0]}: {got[bad[0], 2]} != {ref.flags[bad[0]]} ({bad.size} cells differ)"
    keep = np.ones(len(ref.flags), dtype=bool) if flagged_words else ref.flags == 0
    bad = np.nonzero(keep & ((got[:, 0] != ref.hi) | (got[:, 1] != ref.lo)))[0]
    if bad.size:
        k = bad[0]
        diff = fx.signed128(_units(got[k, 0], got[k, 1]) - _units(ref.hi[k], ref.lo[k]))
        raise AssertionError(f"cell {k}: (hi, lo) = ({got[k, 0]}, {got[k, 1]}) != ({ref.hi[k]}, {ref.lo[k]}): off by {diff} units "
                             f"= {diff / 2.0 ** 64:.6g} x 2^64 ({bad.size} cells differ)")
    if values is not None:
        v = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values).view(np.int64)
        bad = np.nonzero(v != ref.bits)[0]
        assert bad.size == 0, f"value of cell {bad[0]}: {v[bad[0]]:#x} != {ref.bits[bad[0]]:#x} ({bad.size} cells differ)"


def check(cells, ref, flagged_words=True):
    check_cells(cells, ref, _finalize(cells), flagged_words)


def must_fail(*args, **kw):
    with pytest.raises(AssertionError):
        check_cells(*args, **kw)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
CARRY = 2.0 ** -16 - 2.0 ** -69            # 2^64 - 2^11 units: with its negative, every addition wraps or unwraps the low word
UNIT = 2.0 ** -80


def random_values(rng, n, lo=-90, hi=40):
    """[n, 3] of random sign x 2^U(lo, hi)."""
    return rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.uniform(lo, hi, (n, 3))


def carry_values(rng, n):
    """[n, 3], n a multiple of 4: equal counts of +-CARRY and +-UNIT in every column, shuffled -- each column sums to 0."""
    assert n % 4 == 0
    base = np.tile([CARRY, -CARRY, UNIT, -UNIT], n // 4)
    return np.stack([rng.permutation(base) for _ in range(3)], axis=1)


def swing_values(rng, n):
    """[n, 3]: pairs +-c, c in [2^45, 2^46), shuffled within each column, so that a cell's upper word moves through both signs while the sum
    stays in range; and a tail of unpaired small values, so that the expected sum is not simply zero."""
    pairs = (n - n // 32) // 2
    c = 2.0 ** 45 * (1.0 + rng.random((pairs, 3)))
    x = np.concatenate([c, -c, random_values(rng, n - 2 * pairs, -90, 30)])
    return np.stack([rng.permutation(x[:, k]) for k in range(3)], axis=1)


def per_vertex(rng, ids, counts, values):
    """(idx, x): values(rng, count) for each id on its own -- so that what cancels, cancels within a cell --, the rows shuffled together."""
    counts = [counts] * len(ids) if isinstance(counts, int) else counts
    idx = np.repeat(np.asarray(ids, dtype=np.int32), counts)
    x = np.concatenate([values(rng, c) for c in counts])
    p = rng.permutation(len(idx))
    return idx[p], x[p]


def with_flags(rng, x, every=97):
    """Some single components of x become +-inf, NaN or +-2^46: flags in x only, y only or z only, the other two keep their values."""
    x = x.copy()
    bad = [math.inf, -math.inf, math.nan, fx.HUGE, -fx.HUGE, fx.from_bits(0xFFF8000000000ABC)]
    for j, i in enumerate(range(3, len(x), every)):
        x[i, j % 3] = bad[j % len(bad)]
    return x


# ---- 1. conversion as compiled for the device -----------------------------------------------------------------------------------------------
def test_conversion_on_the_device_one_contribution_per_cell(dev):
    vals = fx.conversion_values()
    flagged = [[math.nan, 1.5, -2.5e-7], [3.0e-12, math.inf, 7.0], [-1e9, 2.0 ** -30, -math.inf],          # flags in x, y, z only:
               [fx.HUGE, 1.0, 1.0], [1.0, -fx.HUGE, 1.0], [1.0, 1.0, fx.from_bits(0xFFF0000000000001)]]   # the other two cells keep theirs
    vals = vals + [0.0] * (-len(vals) % 3) + [v for row in flagged for v in row]
    n_vert = len(vals) // 3
    idx, x = _dev(np.arange(n_vert), vals)
    ref = Ref(np.arange(n_vert), vals, len(vals))
    assert int((ref.flags != 0).sum()) > 500 and int((ref.lo != 0).sum()) > 20000
    for grid in (1, 64):
        cells = _direct(dev, idx, x, n_vert, grid)
        check(cells, ref)
    # the same through the LDS table (flags bypass it while the vertex's other components go through it)
    check(_sink(dev, idx, x, n_vert, BWD_BATCH, 16), ref)


# ---- 2. rounding as compiled for the device -------------------------------------------------------------------------------------------------
N_BIG = 1024 * 256 + 7                     # one trip past drt_fx_finalize's grid cap: the grid-stride loop runs twice


@pytest.fixture(scope="module")
def finalize_table():
    cases = fx.finalize_values(N_BIG)
    assert 769 < len(fx.finalize_edges())                               # every edge is in one of the small sizes below, and in the big one
    return fx.cells_array(cases), np.array([fx.value_bits(v, f) for v, f in cases], dtype=np.int64)


@pytest.mark.parametrize("n,first", [(1, 0), (255, 1), (256, 256), (257, 512), (N_BIG, 0)])
def test_rounding_on_the_device(finalize_table, n, first):
    cells, bits = finalize_table
    assert first + n <= len(bits)
    c = torch.tensor(cells[first:first + n].reshape(-1), device="cuda")
    got = _finalize(c).cpu().numpy().view(np.int64)
    bad = np.nonzero(got != bits[first:first + n])[0]
    assert bad.size == 0, f"cell {first + bad[0]} = {cells[first + bad[0]]}: {got[bad[0]]:#x} != {bits[first + bad[0]]:#x} ({bad.size} differ)"
    # accumulate: out += value is ONE IEEE addition
    rng = np.random.default_rng(n)
    prior = rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 15, n)
    with np.errstate(invalid="ignore", over="ignore"):
        want = prior + bits[first:first + n].view(np.float64)
    acc = _finalize(c, 1, torch.tensor(prior, device="cuda")).cpu().numpy()
    assert np.array_equal(acc.view(np.int64), want.view(np.int64))


# ---- 3. contention and carries --------------------------------------------------------------------------------------------------------------
N_CONTEND = 65536


def _contended(kind, n_ids):
    rng = np.random.default_rng(100 + 10 * n_ids + len(kind))
    counts = [N_CONTEND] if n_ids == 1 else [13108] * 4 + [13104]       # (multiples of 4)
    return per_vertex(rng, range(n_ids), counts, {"random": random_values, "carry": carry_values, "swing": swing_values}[kind])


@pytest.mark.parametrize("n_ids", [1, 5])
@pytest.mark.parametrize("kind", ["random", "carry", "swing"])
def test_contended_cells_hold_the_exact_sum(dev, kind, n_ids):
    idx, x = _contended(kind, n_ids)
    assert len(idx) == N_CONTEND
    ref = Ref(idx, x, 15)
    if kind == "carry":
        assert not ref.hi.any() and not ref.lo.any() and not ref.bits.any()          # (0, 0, 0) and +0.0
    else:
        assert np.count_nonzero(ref.lo[:3 * n_ids]) == 3 * n_ids
    rng = np.random.default_rng(7)
    results = []
    for perm in range(3):
        p = np.arange(N_CONTEND) if perm == 0 else rng.permutation(N_CONTEND)
        di, dx = _dev(idx[p], x[p])
        for grid in (1, 7, 256):
            cells = _direct(dev, di, dx, 5, grid)
            check(cells, ref)
            results.append(cells)
    for c in results[1:]:
        assert torch.equal(c, results[0])
    # negative controls (host only): the comparison resolves one unit, on either side
    got = results[-1].cpu().numpy().copy()
    got[1] ^= 1                                                         # lo of cell 0
    must_fail(got, ref)
    if kind == "carry":
        k = int(np.nonzero((x[:, 0] == UNIT) & (idx == 0))[0][0])       # one 2^-80 contribution less in the reference's input
        must_fail(results[0], Ref(np.delete(idx, k), np.delete(x, k, axis=0), 15))


# ---- 4. the deterministic LDS table ---------------------------------------------------------------------------------------------------------
def _runs(rng, n, n_vert, longest=8):
    """ids in runs of neighbours (a patch of a mesh), spread over [0, n_vert)."""
    out = []
    while len(out) < n:
        s, m = int(rng.integers(0, n_vert - longest)), int(rng.integers(1, longest + 1))
        out += list(range(s, s + m)) * int(rng.integers(1, 3))
    return np.array(out[:n], dtype=np.int32)


def _table_case(name):
    """(idx, x [n, 3], n_vert)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one_id":
        n = 20000
        return np.full(n, 5, dtype=np.int32), with_flags(rng, random_values(rng, n)), 8
    if name == "one_id_carry":
        return per_vertex(rng, [5], 16384, carry_values) + (8,)
    if name in ("stride40", "stride40_carry"):
        ids = 7 + FX_HASH_SIZE * np.arange(40)                          # the same low 10 bits: one home slot, 40 strides
        if name == "stride40_carry":
            return per_vertex(rng, ids, 400, carry_values) + (int(ids.max()) + 1,)
        idx = rng.permutation(np.repeat(ids, 200)).astype(np.int32)
        return idx, with_flags(rng, random_values(rng, len(idx))), int(ids.max()) + 1
    if name == "stride40_f64":                                          # the same low 11 bits: the float64 table has 2048 slots
        ids = 7 + HASH_SIZE * np.arange(40)
        idx = rng.permutation(np.repeat(ids, 200)).astype(np.int32)
        return idx, random_values(rng, len(idx)), int(ids.max()) + 1
    if name == "crowded":
        # 3000 distinct ids in ONE batch of 4096: the table has 1024 slots, so at least 1976 ids (pigeonhole) leave it after 24 probes
        ids = rng.permutation(9000)[:3000]
        idx = rng.permutation(np.concatenate([ids, rng.choice(ids, 1096)])).astype(np.int32)
        return idx, with_flags(rng, random_values(rng, 4096)), 9000
    if name == "wide":
        n_vert = 200000                                                 # 14 MB of cells
        idx = _runs(rng, 30000, n_vert)
        idx[:3] = [0, n_vert - 1, n_vert - 2]
        return idx, with_flags(rng, random_values(rng, len(idx))), n_vert
    if name == "wide_carry":
        return per_vertex(rng, np.unique(_runs(rng, 2000, 200000)), 16, carry_values) + (200000,)
    raise KeyError(name)


TABLE_CASES = ["one_id", "one_id_carry", "stride40", "stride40_carry", "crowded", "wide", "wide_carry"]


@pytest.mark.parametrize("name", TABLE_CASES)
def test_the_lds_table_holds_the_exact_sums(dev, name):
    idx, x, n_vert = _table_case(name)
    ref = Ref(idx, x, 3 * n_vert)
    if name.endswith("carry"):
        assert not ref.hi.any() and not ref.lo.any() and not ref.bits.any() and not ref.flags.any()
    if name == "crowded":
        assert len(np.unique(idx)) == 3000 > FX_HASH_SIZE + 1976 - 1 and len(idx) == 4096
    di, dx = _dev(idx, x)
    direct = _direct(dev, di, dx, n_vert, 64)
    check(direct, ref)
    for batch in BATCHES:
        for grid in (1, 64) if batch != 4096 or name != "crowded" else (1,):        # (the same id in many blocks; crowded: ONE batch)
            cells = _sink(dev, di, dx, n_vert, batch, grid)
            assert torch.equal(cells, direct), (batch, grid)
            check(cells, ref)
    if name in ("stride40", "one_id_carry"):                            # negative controls (host only)
        got = cells.cpu().numpy().copy()
        got[3 * 3 * int(idx[0]) + 1] ^= 1
        must_fail(got, ref)
    if name == "one_id_carry":
        k = int(np.nonzero(x[:, 2] == UNIT)[0][0])
        must_fail(cells, Ref(np.delete(idx, k), np.delete(x, k, axis=0), 3 * n_vert))


@pytest.mark.parametrize("batch,grid", [(256, 3), (BWD_BATCH, 2), (4096, 1)])
def test_the_lds_table_at_the_ends_of_a_batch(dev, batch, grid):
    """n of 0, 1, 255, 257 and one past a whole round of batches: empty launches, a last batch of one item, a block without work."""
    rng = np.random.default_rng(batch)
    n_max = batch * grid + 1
    n_vert = 700
    idx_all = np.concatenate([_runs(rng, n_max - 1, n_vert), [n_vert - 1]]).astype(np.int32)
    x_all = with_flags(rng, random_values(rng, n_max), 61)
    for n in (0, 1, 255, 257, n_max):
        idx, x = idx_all[n_max - n:], x_all[n_max - n:]                 # (the tail: the item beyond the round is always there)
        ref = Ref(idx, x, 3 * n_vert)
        di, dx = _dev(idx, x)
        cells = _sink(dev, di, dx, n_vert, batch, grid)
        check(cells, ref)
        assert torch.equal(cells, _direct(dev, di, dx, n_vert, grid))
        assert n or not cells.any()


# ---- 5. LossAcc<true> -----------------------------------------------------------------------------------------------------------------------
class LossRef:
    """The one cell of a scalar loss over the terms x."""

    def __init__(self, x):
        s = f = 0
        for v in np.asarray(x, dtype=np.float64).tolist():
            if fx.flags_of(v):
                f |= fx.flags_of(v)
            else:
                s += fx.q(v)
        assert abs(s) < 1 << (47 + fx.FRAC)
        self.hi, self.lo, self.flags, self.bits = (np.array([v], dtype=np.int64) for v in (*fx.split(s), f, fx.value_bits(s, f)))


@pytest.mark.parametrize("grid", [1, 64])
def test_loss_acc_holds_the_exact_sum(dev, grid):
    rng = np.random.default_rng(5 + grid)
    last = None
    for n in (1, 63, 64, 65, 255, 256, 256 * grid + 1):
        x = random_values(rng, n)[:, 0].copy()
        ref = LossRef(x)
        last = _loss(dev, torch.tensor(x, device="cuda"), grid)
        check(last, ref, flagged_words=False)
    got = last.cpu().numpy().copy()                                     # negative control (host only)
    got[1] ^= 1
    must_fail(got, ref, flagged_words=False)
    for n in (256, 16384):                                              # the carry stress: every addition wraps or unwraps the low word
        x = rng.permutation(np.tile([CARRY, -CARRY, UNIT, -UNIT], n // 4))
        ref = LossRef(x)
        assert not ref.hi.any() and not ref.lo.any() and not ref.bits.any()
        cell = _loss(dev, torch.tensor(x, device="cuda"), grid)
        check(cell, ref, flagged_words=False)
        k = int(np.nonzero(x == UNIT)[0][0])
        must_fail(cell.cpu().numpy(), LossRef(np.delete(x, k)), None, False)
    x = swing_values(rng, 4096)[:, 1].copy()
    check(_loss(dev, torch.tensor(x, device="cuda"), grid), LossRef(x), flagged_words=False)
    assert not _loss(dev, torch.empty(0, dtype=torch.float64, device="cuda"), grid).any()


@pytest.mark.parametrize("grid", [1, 64])
def test_loss_acc_flags(dev, grid):
    rng = np.random.default_rng(15 + grid)
    n = 256 * grid + 1
    base = random_values(rng, n)[:, 0].copy()
    one_nan = base.copy()
    one_nan[100] = math.nan                                             # one lane of the second wave, in its upper half
    both = base.copy()
    both[3], both[170] = 2.0 ** 50, -2.0 ** 50                          # +huge in one wave, -huge in another: NaN
    for x, flags, value in ((one_nan, fx.NAN, math.nan), (both, fx.POS | fx.NEG, math.nan),
                            (np.full(300, math.inf), fx.POS, math.inf), (np.concatenate([base[:200], [-math.inf]]), fx.NEG, -math.inf)):
        ref = LossRef(x)
        assert int(ref.flags[0]) == flags and int(ref.bits[0]) == fx.bits_of(value)
        cell = _loss(dev, torch.tensor(x, device="cuda"), grid)
        check(cell, ref, flagged_words=False)
        assert int(cell[2]) == flags


# ---- 6. the exchange format at range --------------------------------------------------------------------------------------------------------
def _to_limbs(cells):
    from drt_amd import _lib
    assert cells.is_cuda and cells.is_contiguous() and cells.dtype == torch.int64 and cells.numel() % 3 == 0
    limbs = torch.empty(cells.numel() // 3 * 4, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().drt_fx_to_limbs(cells.data_ptr(), cells.numel() // 3, limbs.data_ptr(), _stream()))
    return limbs


def _from_limbs(limbs):
    from drt_amd import _lib
    assert limbs.is_cuda and limbs.is_contiguous() and limbs.dtype == torch.int64 and limbs.numel() % 4 == 0
    cells = torch.empty(limbs.numel() // 4 * 3, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().drt_fx_from_limbs(limbs.data_ptr(), limbs.numel() // 4, cells.data_ptr(), _stream()))
    return cells


def _range_cells(rnd, n):
    """Random 127-bit cells of either sign, the extreme ones, and flags on every eighth."""
    out = [(-(1 << 127), 0), ((1 << 127) - 1, 0), (-1, 0), (1, 0), (0, 0), (0, fx.NAN), (-(1 << 86), 7), ((1 << 86) - 1, 2), (-(1 << 43), 4), (1 << 43, 0)]
    while len(out) < n:
        out.append((rnd.getrandbits(127) * rnd.choice([-1, 1]), rnd.randint(1, 7) if len(out) % 8 == 0 else 0))
    return out[:n]


def test_limbs_round_trip_and_a_thousand_ranks(dev):
    rnd = random.Random(6)
    n, R = 200, 1000
    ranks = [_range_cells(rnd, n) if r == 0 else [(rnd.getrandbits(127) * rnd.choice([-1, 1]), rnd.choice([0] * 12 + [1, 2, 4, 7])) for _ in range(n)]
             for r in range(R)]
    cells = torch.tensor(np.concatenate([fx.cells_array(c) for c in ranks]).reshape(-1), device="cuda")
    limbs = _to_limbs(cells)
    assert torch.equal(_from_limbs(limbs), cells)                       # the identity, at every magnitude and sign
    l = limbs.view(R, n, 4)
    assert int(l[..., :2].min()) >= 0 and int(l[..., :2].max()) < 1 << 43 and int(l[..., 2].min()) == -(1 << 41) and int(l[..., 2].max()) < 1 << 41
    summed = _from_limbs(l.sum(dim=0).contiguous().view(-1)).cpu().numpy().reshape(n, 3)       # what an all-reduce(SUM) over R ranks delivers
    want = np.empty((n, 3), dtype=np.int64)
    for i in range(n):
        f = 0
        for r in range(R):
            f |= ranks[r][i][1]
        want[i] = (*fx.split(sum(ranks[r][i][0] for r in range(R))), f)
    assert np.array_equal(summed, want)
    bad = want.copy()
    bad[n // 2, 1] ^= 1
    assert not np.array_equal(summed, bad)


def test_limbs_of_the_largest_rank_count(dev):
    """Every word times 2^20 - 1 stands for that many identical ranks: no word leaves int64 (the header's claim, checked here in Python
    first and then by reading back what the device made of it), the sum is (2^20 - 1) v mod 2^128 and the flags are the same flags."""
    rnd = random.Random(7)
    K = (1 << 20) - 1
    cases = _range_cells(rnd, 4096)
    limbs = _to_limbs(torch.tensor(fx.cells_array(cases).reshape(-1), device="cuda"))
    host = limbs.cpu().numpy().astype(object)
    assert all(-(1 << 63) <= int(w) * K < 1 << 63 for w in host)
    back = _from_limbs(limbs * K).cpu().numpy().reshape(-1, 3)
    want = np.array([(*fx.split(v * K), f) for v, f in cases], dtype=np.int64)
    assert np.array_equal(back, want)
    assert cases[5] == (0, fx.NAN) and tuple(back[5]) == (0, 0, fx.NAN)  # a NaN counter of 2^20 - 1 does not spill into the +inf counter
    got = _finalize(torch.tensor(back.reshape(-1), device="cuda")).cpu().numpy().view(np.int64)
    assert np.array_equal(got, np.array([fx.value_bits(v * K, f) for v, f in cases], dtype=np.int64))


# ---- 7. the float64 table -------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def f64_ref(idx, x, n_cells, drop=None):
    """(fsum, bound) per cell; bound = gamma_(m-1) sum|x_i|, gamma_k = k u / (1 - k u): the textbook bound of m - 1 rounded additions in ANY
    order, so it covers the table, its flush and the overflow to memory together.  drop: leave that contribution out of the reference."""
    parts = {}
    for i, v in enumerate(idx.tolist()):
        if i == drop:
            continue
        for c in range(3):
            parts.setdefault(3 * v + c, []).append(float(x[i, c]))
    want, bound = np.zeros(n_cells), np.zeros(n_cells)
    for cell, p in parts.items():
        m = len(p)
        assert m <= 64
        want[cell] = math.fsum(p)
        bound[cell] = (m - 1) * U / (1 - (m - 1) * U) * math.fsum(map(abs, p))
    assert bound.max() <= 2e-12
    return want, bound


def check_f64(g, ref):
    want, bound = ref
    got = g.cpu().numpy()
    err = np.abs(got - want)
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, f"cell {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}, off by {err[bad[0]]:.3e} > {bound[bad[0]]:.3e} ({bad.size} cells differ)"


@pytest.mark.parametrize("name", ["one_id", "stride40", "stride40_f64", "crowded", "wide"])
def test_the_float64_table_loses_and_doubles_nothing(dev, name):
    idx, _, n_vert = _table_case(name)
    rng = np.random.default_rng(70 + len(name))
    # at most 64 contributions per cell: thin the ids that occur more often
    keep, seen = [], {}
    for i, v in enumerate(idx.tolist()):
        seen[v] = seen.get(v, 0) + 1
        if seen[v] <= 64:
            keep.append(i)
    idx = idx[keep]
    x = rng.choice([-1.0, 1.0], (len(idx), 3)) * (1.0 + rng.random((len(idx), 3)))
    di, dx = _dev(idx, x)
    ref = f64_ref(idx, x, 3 * n_vert)
    for batch in BATCHES:
        for grid in (1, 64):
            g = _sink_f64(dev, di, dx, n_vert, batch, grid)
            check_f64(g, ref)
    with pytest.raises(AssertionError):                                 # negative control (host only): one contribution less in the reference
        check_f64(g, f64_ref(idx, x, 3 * n_vert, drop=len(idx) // 2))
    assert not _sink_f64(dev, di[:0], dx[:0], n_vert, BWD_BATCH, 4).any()
