"""CPU: the deal of k_raster's runs by the previous call's test counts (drt_amd/csrc/drt_raster.h: raster_deal_boundary,
raster_deal_end, raster_deal_slice), compiled for the host by g++ (tests/hostsim/raster_deal.cpp), which replays every wave's loop the
way k_raster<true> runs it.

What is held, for every cost array below and V = 1, 7, 64 and 8 192 waves:
* the table by the definition (prefix sums, one bisection per boundary) is the table raster_deal_place writes run by run, which is the
  call every thread of k_raster_deal makes;
* the boundaries B[0 .. V] are non-decreasing in the order of (run, item), B[0] = (0, 0), B[V] = (n_runs, 0);
* replayed against ACTUAL totals that are not the predicted ones (the same, halved, doubled, zero where there was work, work where there
  was none, unrelated), every (run, item) with item < total is worked exactly once: the non-empty slices of a run start where the one
  before ended, and the last ends at the total;
* every run has exactly one owner -- the wave that lists the run's large triangles, demotes its image and records its count.  (The
  bit-for-bit GPU tests cannot hold this rule: a triangle listed twice is rasterised twice into the same atomic minimum.)
* no wave's predicted cost -- c_fixed per run it visits plus its items -- exceeds C / V + c_fixed + 1: a boundary that falls into a run's
  fixed part moves to the run's start (less than c_fixed more for the wave behind it), one among the tests makes the wave behind it
  project the run again (c_fixed), and floor(v C / V) rounds by less than 1.

The same source with its own main runs under -fsanitize=address,undefined as a program of its own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "raster_deal.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "hostsim", "_build")
HEADER = os.path.join(ROOT, "drt_amd", "csrc", "drt_raster.h")
C_FIXED = 64
_P, _U32 = ctypes.c_void_p, ctypes.c_uint32


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (SRC, HEADER))


@pytest.fixture(scope="module")
def hs():
    so = os.path.join(OUT_DIR, "libraster_deal.so")
    os.makedirs(OUT_DIR, exist_ok=True)
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.rd_boundaries.argtypes = [_P, _U32, _U32, _U32, _P]
    lib.rd_boundaries.restype = None
    lib.rd_boundaries_by_run.argtypes = [_P, _U32, _U32, _U32, _P]
    lib.rd_boundaries_by_run.restype = None
    lib.rd_replay.argtypes = [_P, _U32, _U32, _P, _U32, _P, _P, _P]
    lib.rd_replay.restype = ctypes.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _boundaries(hs, cost, V):
    B = np.zeros((V + 1, 2), np.uint32)
    hs.rd_boundaries(_p(cost), len(cost), V, C_FIXED, _p(B))
    by_run = np.zeros((V + 1, 2), np.uint32)               # the device's way to the same table: every run places the boundaries inside it
    hs.rd_boundaries_by_run(_p(cost), len(cost), V, C_FIXED, _p(by_run))
    assert np.array_equal(B, by_run)
    return B


def _replay(hs, B, V, actual):
    n = len(actual)
    owners, nxt, wave = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32), np.zeros(V, np.uint64)
    bad = hs.rd_replay(_p(B), n, V, _p(actual), C_FIXED, _p(owners), _p(nxt), _p(wave))
    return bad, owners[:n], nxt[:n], wave


def _costs(kind, n, rng):
    if kind == "random":                                   # half the runs of a pass hold nothing, the others up to 64 * 48 tests
        return np.where(rng.random(n) < 0.5, 0, rng.integers(0, 3073, n)).astype(np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "giant":                                    # one run among zeros: cut between many waves
        c = np.zeros(n, np.uint32)
        if n:
            c[n // 3] = 3072
        return c
    if kind == "huge":                                     # sums near 2^32: the running sums are 64-bit
        return (np.uint64(0xFFFFFFFF) // np.uint64(max(n, 1)) - rng.integers(0, 3, n).astype(np.uint64)).astype(np.uint32)
    raise KeyError(kind)


def _actuals(cost, rng):
    n = len(cost)
    half, double = cost // 2, (np.minimum(cost.astype(np.uint64) * 2, 0xFFFFFFFF)).astype(np.uint32)
    gone = np.where(rng.random(n) < 0.5, 0, cost).astype(np.uint32)
    new = np.where(cost == 0, rng.integers(1, 3073, n), cost).astype(np.uint32)
    other = rng.integers(0, 5000, n).astype(np.uint32)
    return {"same": cost, "halved": half, "doubled": double, "zero where there was work": gone, "work where there was none": new, "unrelated": other}


SIZES = ("0", "1", "V-1", "V", "V+1", "4V")


def _n(size, V):
    return {"0": 0, "1": 1, "V-1": V - 1, "V": V, "V+1": V + 1, "4V": 4 * V}[size]


@pytest.mark.parametrize("kind", ["random", "zeros", "giant", "huge"])
@pytest.mark.parametrize("V", [1, 7, 64, 8192])
def test_boundaries_cover_every_item_once_with_one_owner_and_balanced_cost(hs, V, kind):
    rng = np.random.default_rng(17 + V)
    for size in SIZES:
        n = _n(size, V)
        cost = _costs(kind, n, rng)
        B = _boundaries(hs, cost, V)
        # non-decreasing, with the two fixed ends
        assert tuple(B[0]) == (0, 0) and tuple(B[V]) == (n, 0), (size, B[0], B[V])
        key = B[:, 0].astype(np.uint64) << np.uint64(32) | B[:, 1].astype(np.uint64)
        assert (np.diff(key.astype(np.int64)) >= 0).all(), size
        inside = B[:, 0] < n
        assert (B[inside, 1] < np.maximum(cost[B[inside, 0]], 1)).all() and not B[~inside, 1].any(), size      # a cut lies inside its run
        # exactly once, one owner: whatever the runs actually hold
        for name, actual in _actuals(cost, rng).items():
            bad, owners, nxt, _ = _replay(hs, B, V, actual)
            assert bad == 0, (size, name)
            assert np.array_equal(nxt, actual), (size, name)
            assert (owners == 1).all(), (size, name)
        # balance of the predicted cost
        _, _, _, wave = _replay(hs, B, V, cost)
        C = int(cost.astype(np.uint64).sum()) + C_FIXED * n
        assert int(wave.max()) * V <= C + V * (C_FIXED + 1), (size, int(wave.max()), C / V)
        assert int(wave.sum()) >= C                                                                         # (shared runs are projected again)


def test_a_table_of_another_launch_still_covers_every_item_once(hs):
    """Boundaries made for MORE runs than the launch has (a captured launch replayed behind a call of another shape on the same
    workspace): clamped to the end, the ranges still tile the runs."""
    rng = np.random.default_rng(5)
    V, n_table, n = 64, 300, 120
    B = _boundaries(hs, _costs("random", n_table, rng), V)
    actual = rng.integers(0, 3073, n).astype(np.uint32)
    bad, owners, nxt, _ = _replay(hs, B, V, actual)
    assert bad == 0 and np.array_equal(nxt, actual) and (owners == 1).all()


def test_a_giant_run_is_cut_between_many_waves(hs):
    V, n = 64, 16
    cost = _costs("giant", n, np.random.default_rng(0))
    B = _boundaries(hs, cost, V)
    in_giant = (B[:, 0] == n // 3) & (B[:, 1] > 0)
    assert in_giant.sum() >= V // 2                          # 3 072 tests against 16 * 64 of fixed cost: most waves share the one run


def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "raster_deal_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRASTER_DEAL_MAIN", "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
