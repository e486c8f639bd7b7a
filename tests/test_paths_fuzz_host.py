"""CPU: admission, coverage, measured figures and negative controls of the K-interaction path kernels' fuzz cases
(tests/paths_fuzz_cases.py; the device side is tests/test_gpu_paths_fuzz.py).

On every admitted case the host builds of the kernels' own headers -- tests/hostsim/paths_ior.cpp (``pi_trace``: trace_path_k<SNELL>;
``pi_loss_backward``: path_loss_backward_ior_k) and tests/hostsim/paths_adjoint.cpp (``hp_backward``: path_recompute_backward_k, which
knows the reference formula only, so the linear functional's gradient under snell is checked on the device alone) -- are held against
the float64 restatements tests/snell_ref.py and tests/ior_ref.py.  Tape, hit count and mask must be EQUAL ON EVERY RAY (no ray is left
out); a ray on which they were not would be a finding to look at -- a tie in t or a TIR discriminant at rounding replaces the seed, anything
else is a bug in the headers.

The device tolerances are the family's own (tests/test_gpu_paths.py, test_gpu_paths_ior.py): RAY_ABS 1e-10, GRAD_REL 1e-9 of the
reference's largest entry and GRAD_ABS 1e-5, LOSS_REL 1e-10, IOR_REL 1e-9 of the sum of the absolute per-path contributions.  Each CPU
figure must be at most a tenth of its tolerance; a quantity that were not would get ten times its largest CPU figure as its device
tolerance on these cases (ten times: the device contracts to FMA, the host build does not) -- none needed it, see FUZZ_TOLERANCES.

MEASURED (the largest disagreement over the 16 admitted cases and the 3 variants of the pairs, printed by test_zz_figures with -s):
    tape / hits / mask    equal on every ray of every case (32 038 rays of the 16 cases; no ray left out)
    out_ori               5.4e-13 absolute (fuzz9/2)          out_dir          5.3e-15 absolute
    loss                  2.0e-15 relative
    grad_V (ray_loss)     3.8e-14 of the largest entry, 3.7e-13 absolute
    grad_V (linear)       8.0e-15 of the largest entry, 1.1e-12 absolute          (reference-formula cases)
    g_int, g_ext          1.3e-14 of sum |per path|
Every figure is below a tenth of its tolerance (out_ori, the candidate, by a factor of 18), so no device tolerance is widened.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import paths_fuzz_cases as fz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I64, _D, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
RAY_ABS, GRAD_REL, GRAD_ABS, LOSS_REL, IOR_REL = 1e-10, 1e-9, 1e-5, 1e-10, 1e-9
# what the device test asserts on these cases: the family's tolerances, every CPU figure being below a tenth of its own
FUZZ_TOLERANCES = dict(ray_ori=RAY_ABS, ray_dir=RAY_ABS, loss=LOSS_REL, grad_rel=GRAD_REL, grad_abs=GRAD_ABS, ior=IOR_REL)
FIGURES = {}          # name -> (largest figure, case): filled by the tests below, printed by test_zz_figures


def _build(name):
    src = os.path.join(ROOT, "tests", "hostsim", name + ".cpp")
    out_dir = os.path.join(ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "lib" + name + ".so")
    os.makedirs(out_dir, exist_ok=True)
    csrc = os.path.join(ROOT, "drt_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.hs_create.restype = _P
    lib.hs_create.argtypes = [_P, _I64, _P, _I64]
    lib.hs_destroy.argtypes = [_P]
    return lib


def build_libs():
    """(paths_ior, paths_adjoint): built as tests/test_paths_ior_host.py and tests/test_paths_adjoint.py build them."""
    pi, hp = _build("paths_ior"), _build("paths_adjoint")
    pi.pi_trace.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I, _I, _I, _P, _P, _P, _P, _P]
    pi.pi_loss_backward.restype = _D
    pi.pi_loss_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _I] + [_P] * 12
    hp.hp_backward.argtypes = [_P, _P, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P]
    return pi, hp


@pytest.fixture(scope="module")
def libs():
    return build_libs()


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


_host = {}


def host(libs, seed, variant=0):
    """The host build's results on a case: dict(out_ori, out_dir, mask, tape, hits; loss, per_int, per_ext, grad; grad_lin or None under
    snell).  Computed once, shared read-only."""
    if (seed, variant) in _host:
        return _host[(seed, variant)]
    pi, hp = libs
    sc = fz.case(seed, variant)
    k, tir, refraction = sc["law"]
    F = np.ascontiguousarray(sc["mesh"].faces, np.int32)
    V = np.ascontiguousarray(sc["mesh"].vertices, np.float64)
    V32 = np.ascontiguousarray(V.astype(np.float32))
    n, snell = sc["n"], int(refraction == "snell")
    on, dn, spn = (np.ascontiguousarray(sc[key].numpy(), np.float64) for key in ("o", "d", "sp"))
    va = np.ascontiguousarray(sc["valid"].numpy().astype(np.uint8))
    h = pi.hs_create(_p(F), len(F), _p(V32), len(V))
    r = dict(out_ori=np.empty((n, 3)), out_dir=np.empty((n, 3)), mask=np.empty(n, np.uint8), tape=np.empty((k, n), np.int32), hits=np.empty(n, np.uint8),
             per_int=np.empty(n), per_ext=np.empty(n), grad=np.zeros_like(V), grad_lin=None)
    pi.pi_trace(h, _p(V), _p(on), _p(dn), n, sc["ior_int"], sc["ior_ext"], k, int(tir == "reflect"), snell, _p(r["out_ori"]), _p(r["out_dir"]),
                _p(r["mask"]), _p(r["tape"]), _p(r["hits"]))
    plain, loss_plain = np.zeros_like(V), np.zeros(1)
    r["loss"] = pi.pi_loss_backward(h, _p(V), _p(on), _p(dn), n, sc["ior_int"], sc["ior_ext"], snell, _p(r["mask"]), _p(r["tape"]), _p(r["hits"]),
                                    _p(r["out_ori"]), _p(r["out_dir"]), _p(spn), _p(va), _p(r["per_int"]), _p(r["per_ext"]), _p(r["grad"]), _p(plain),
                                    _p(loss_plain))
    assert r["loss"] == loss_plain[0] and np.array_equal(r["grad"].view(np.int64), plain.view(np.int64))
    pi.hs_destroy(h)
    if not snell:
        h = hp.hs_create(_p(F), len(F), _p(V32), len(V))
        r["grad_lin"] = np.zeros_like(V)
        hp.hp_backward(h, _p(V), _p(on), _p(dn), n, sc["ior_int"], sc["ior_ext"], _p(r["mask"]), _p(r["tape"]), _p(r["hits"]),
                       _p(np.ascontiguousarray(sc["w_ori"].numpy())), _p(np.ascontiguousarray(sc["w_dir"].numpy())), _p(r["grad_lin"]))
        hp.hs_destroy(h)
    _host[(seed, variant)] = r
    return r


def _note(name, value, sc):
    if name not in FIGURES or value > FIGURES[name][0]:
        FIGURES[name] = (float(value), sc["name"])


def _tenth(name, value, tolerance, sc):
    _note(name, value, sc)
    assert value <= 0.1 * tolerance, f"{sc['name']}: {name} {value:.3e} is no longer below a tenth of {tolerance:g}: see FUZZ_TOLERANCES"


def _all(variants=True):
    out = [(s, 0) for s in fz.CASES]
    if variants:
        out += [(s, v) for s, a, b in fz.PAIRS for v in (a, b) if (s, v) not in out]
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. the list
def test_the_generator_is_deterministic_and_a_variant_shares_the_mesh():
    s = fz.CASES[0]
    fz.case.cache_clear()
    a = fz.case(s)
    fz.case.cache_clear()
    b = fz.case(s)
    assert a is not b and a["law"] == b["law"] and torch.equal(a["o"], b["o"]) and torch.equal(a["sp"], b["sp"]) and torch.equal(a["valid"], b["valid"])
    assert np.array_equal(a["mesh"].vertices, b["mesh"].vertices)
    for seed, va, vb in fz.PAIRS:
        x, y = fz.case(seed, va), fz.case(seed, vb)
        assert np.array_equal(x["mesh"].vertices, y["mesh"].vertices) and np.array_equal(x["mesh"].faces, y["mesh"].faces)
        assert x["law"] != y["law"] and (x["n"] != y["n"] or not torch.equal(x["d"], y["d"]))
    assert len(fz.PAIRS) == 3 and len({p[0] for p in fz.PAIRS}) == 3


def test_coverage_of_the_admitted_list():
    rows = [fz.coverage(fz.case(s), fz.trace(s), fz.reference(s)) for s in fz.CASES]
    print()
    print("seed faces two  ior_int ior_ext K tir     refraction size    dist in   rays valid count maxhit fullK mirr tirend exhausted")
    for r in rows:
        print(f"{r['seed']:4d} {r['faces']:5d} {int(r['two']):3d} {r['ior_int']:8.5f} {r['ior_ext']:7.5f} {r['k']} {r['tir']:7s} {r['refraction']:10s} "
              f"{r['size'][0]:2d}x{r['size'][1]:<3d} {r['distance']:4.1f} {int(r['inside']):2d} {r['rays']:6d} {r['valid']:5d} {r['count']:5d} {r['max_hits']:6d} "
              f"{r['full_k']:5d} {r['max_mirrored']:4d} {r['tir_ended']:6d} {r['exhausted']:9d}")
    print("rays in all:", sum(r["rays"] for r in rows))
    assert 14 <= len(fz.CASES) <= 18 and len(set(fz.CASES)) == len(fz.CASES)
    assert {r["k"] for r in rows} == set(range(2, 9))
    assert {(r["tir"], r["refraction"]) for r in rows} == {(t, f) for t in fz.TIRS for f in fz.REFRACTIONS}
    assert {r["ior_int"] for r in rows} == set(fz.IORS_INT) and {r["ior_ext"] for r in rows} == set(fz.IORS_EXT)
    assert sum(r["inside"] for r in rows) >= 2
    assert sum(r["two"] for r in rows) >= 3
    assert sum(r["tir"] == "reflect" and r["k"] >= 6 and r["full_k"] >= 1 for r in rows) >= 3
    assert sum(r["tir"] == "reflect" and r["max_mirrored"] >= 3 for r in rows) >= 1
    assert sum(r["tir"] == "drop" and r["k"] > 2 and r["tir_ended"] >= 1 for r in rows) >= 2
    assert sum(r["exhausted"] >= 1 for r in rows) >= 1
    assert sum(r["count"] == 0 for r in rows) >= 2
    assert sum(r["size"] == (1, 1) for r in rows) == 1
    assert all(r["rays"] <= 2500 for r in rows)
    # an "entering" hit while already inside: a two-body case with a valid path of four or more interactions
    assert sum(r["two"] and r["max_hits"] >= 4 for r in rows) >= 1
    # the pairs of the one-scene test: different laws on one mesh
    for seed, va, vb in fz.PAIRS:
        assert fz.case(seed, va)["k"] != fz.case(seed, vb)["k"] or fz.case(seed, va)["refraction"] != fz.case(seed, vb)["refraction"]


def test_the_wrapper_returns_zeros_where_nothing_contributes():
    zero = [s for s in fz.CASES if fz.reference(s)["count"] == 0]
    assert len(zero) >= 2
    for s in zero:
        ref = fz.reference(s)
        assert ref["loss"] == 0.0 and ref["g_int"] == 0.0 and ref["g_ext"] == 0.0 and not ref["grad_V"].any()
        assert ref["grad_V"].shape == fz.case(s)["mesh"].vertices.shape
    # and with no target at all, on a case that has completed paths
    s = next(s for s in fz.CASES if fz.reference(s)["count"] > 0)
    sc = fz.case(s)
    ref = fz.loss_and_grads(sc, valid=torch.zeros(sc["n"], dtype=torch.bool), aux=fz.trace(s))
    assert ref["loss"] == 0.0 and ref["count"] == 0 and not ref["grad_V"].any() and int(ref["aux"]["valid"].sum()) > 0


# ------------------------------------------------------------------------------------------ 2. the host build against the restatements
def _ids(p):
    return f"{p[0]}" + (f"v{p[1]}" if p[1] else "")


@pytest.mark.parametrize("seed,variant", _all(), ids=[_ids(p) for p in _all()])
def test_trace_is_equal_on_every_ray_and_exit_rays_agree(libs, seed, variant):
    sc, got, aux, ref = fz.case(seed, variant), host(libs, seed, variant), fz.trace(seed, variant), fz.exit_reference(seed, variant)
    differ = (got["tape"].astype(np.int64) != aux["tape"].numpy()).any(0) | (got["mask"].astype(bool) != aux["valid"].numpy()) | \
        (got["hits"].astype(np.int64) != aux["hits"].numpy())
    assert not differ.any(), f"{sc['name']}: rays {np.nonzero(differ)[0][:10]} of {sc['n']} differ in tape, hits or mask"
    dead = got["mask"] == 0
    assert not got["out_ori"][dead].any() and not got["out_dir"][dead].any()
    _tenth("out_ori", np.abs(got["out_ori"] - ref["out_ori"]).max(), RAY_ABS, sc)
    _tenth("out_dir", np.abs(got["out_dir"] - ref["out_dir"]).max(), RAY_ABS, sc)


@pytest.mark.parametrize("seed,variant", _all(), ids=[_ids(p) for p in _all()])
def test_loss_vertex_gradient_and_ior_partials(libs, seed, variant):
    sc, got, ref = fz.case(seed, variant), host(libs, seed, variant), fz.reference(seed, variant)
    assert int(((got["mask"] != 0) & sc["valid"].numpy()).sum()) == ref["count"]
    if ref["count"] == 0:
        assert got["loss"] == 0.0 and not got["grad"].any() and not got["per_int"].any() and not got["per_ext"].any()
        return
    _tenth("loss", abs(got["loss"] - ref["loss"]) / abs(ref["loss"]), LOSS_REL, sc)
    diff, top = np.abs(got["grad"] - ref["grad_V"]).max(), np.abs(ref["grad_V"]).max()
    assert top > 0
    _tenth("grad_V relative", diff / top, GRAD_REL, sc)
    _tenth("grad_V absolute", diff, GRAD_ABS, sc)
    for key in ("int", "ext"):
        per = got["per_" + key]
        assert np.isfinite(per).all() and ref["abs_" + key] > 0
        _tenth("g_" + key, abs(per.sum() - ref["g_" + key]) / ref["abs_" + key], IOR_REL, sc)
        assert (per[np.setdiff1d(np.arange(sc["n"]), ref["rows"])] == 0).all()


@pytest.mark.parametrize("seed,variant", _all(), ids=[_ids(p) for p in _all()])
def test_linear_functional_gradient_under_the_reference_formula(libs, seed, variant):
    sc, got, ref = fz.case(seed, variant), host(libs, seed, variant), fz.exit_reference(seed, variant)
    if sc["refraction"] == "snell":
        assert got["grad_lin"] is None          # hp_backward knows the reference formula only: checked on the device
        return
    if not got["mask"].any():
        assert not got["grad_lin"].any() and not ref["grad_lin"].any()
        return
    diff, top = np.abs(got["grad_lin"] - ref["grad_lin"]).max(), np.abs(ref["grad_lin"]).max()
    assert top > 0
    _tenth("grad_lin relative", diff / top, GRAD_REL, sc)
    _tenth("grad_lin absolute", diff, GRAD_ABS, sc)


# ---------------------------------------------------------------------------------------------------------------- 3. negative controls
def _told_apart(sc, a, b):
    """Whether two results of the restatement on one case are outside the tolerance of each other: tape, hits or mask differ on a
    ray, or an exit ray of a path both complete differs by more than RAY_ABS."""
    if not (torch.equal(a["aux"]["tape"], b["aux"]["tape"]) and torch.equal(a["aux"]["hits"], b["aux"]["hits"])
            and torch.equal(a["aux"]["valid"], b["aux"]["valid"])):
        return True
    return bool(max(np.abs(a["out_ori"] - b["out_ori"]).max(), np.abs(a["out_dir"] - b["out_dir"]).max()) > RAY_ABS)


def _losses_apart(sc, a_law=None, a_iors=None):
    """|loss of the variant - loss of the case| relative to the case's loss (inf when only one of them is 0)."""
    ref, other = fz.reference(sc["seed"]), fz.loss_and_grads(sc, law=a_law, iors=a_iors)
    if ref["loss"] == 0.0:
        return 0.0 if other["loss"] == 0.0 else float("inf")
    return abs(other["loss"] - ref["loss"]) / abs(ref["loss"])


def test_control_the_other_refraction_formula_is_told_apart():
    n = 0
    for s in fz.CASES:
        sc = fz.case(s)
        if int(fz.trace(s)["valid"].sum()) == 0:
            continue          # no completed path: no refraction reaches an output
        other = "snell" if sc["refraction"] == "reference" else "reference"
        assert _told_apart(sc, fz.exit_reference(s), fz.exit_rays(sc, law=(sc["k"], sc["tir"], other))), sc["name"]
        if fz.reference(s)["count"] > 0:
            assert _losses_apart(sc, a_law=(sc["k"], sc["tir"], other)) > LOSS_REL, sc["name"]
        n += 1
    assert n >= len(fz.CASES) - 4


def test_control_the_other_tir_rule_is_told_apart():
    n = 0
    for s in fz.CASES:
        sc = fz.case(s)
        cov = fz.coverage(sc, fz.trace(s), fz.reference(s))
        if not (cov["tir_ended"] > 0 and cov["k"] > 2 or cov["max_mirrored"] > 0):
            continue          # no ray of this case meets TIR where the rule decides something
        other = "reflect" if sc["tir"] == "drop" else "drop"
        assert _told_apart(sc, fz.exit_reference(s), fz.exit_rays(sc, law=(sc["k"], other, sc["refraction"]))), sc["name"]
        if cov["max_mirrored"] > 0:          # a completed path with a mirrored interaction is no path under drop
            assert int(fz.trace_of(sc, law=(sc["k"], other, sc["refraction"]))["valid"].sum()) < cov["valid"]
        n += 1
    assert n >= 4


def test_control_exchanged_iors_are_told_apart():
    n = 0
    for s in fz.CASES:
        sc = fz.case(s)
        if int(fz.trace(s)["valid"].sum()) == 0:
            continue
        assert _told_apart(sc, fz.exit_reference(s), fz.exit_rays(sc, iors=(sc["ior_ext"], sc["ior_int"]))), sc["name"]
        n += 1
    assert n >= len(fz.CASES) - 4


# ------------------------------------------------------------------------------------------------------------------------ 4. figures
def test_zz_figures():
    """Prints the largest disagreement of every quantity over all cases: what MEASURED in the module docstring quotes."""
    print()
    for name, (value, where) in sorted(FIGURES.items()):
        print(f"largest CPU disagreement  {name:20s} {value:.3e}  ({where})")
    assert {"out_ori", "out_dir", "loss", "grad_V relative", "g_int", "g_ext", "grad_lin relative"} <= set(FIGURES)
