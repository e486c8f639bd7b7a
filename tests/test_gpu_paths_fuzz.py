"""GPU: the K-interaction path kernels (drt_amd/csrc/drt_paths.hip: k_paths_start, k_paths_start_fused, k_paths_shade<SNELL>,
k_paths_finish, k_paths_collect, k_paths_count, k_paths_bwd, k_paths_loss_bwd, k_paths_loss_bwd_ior) through their three Scene
methods -- render_paths, paths_ray_loss_fused, paths_ray_loss_ior_fused -- on the random cases of tests/paths_fuzz_cases.py: random closed
shapes (one body, two shells, two lobes), cameras far from, close to and inside the body, interior IORs 1.1 to 2.4 over exteriors 1.0 to
1.2, K = 2..8 under both TIR rules and both refraction formulas, non-square images and a 1 x 1 one, cases in which nothing completes.

References: the float64 restatements tests/snell_ref.py (tape, hit count and mask: EXACT ON EVERY RAY; exit rays) and tests/ior_ref.py
(loss, vertex gradient and both IOR partials by autograd), computed once per case in paths_fuzz_cases and shared.  Tolerances are the
family's own (tests/test_gpu_paths.py, test_gpu_paths_ior.py): RAY_ABS 1e-10, GRAD_REL 1e-9 of the reference's largest entry and GRAD_ABS
1e-5, LOSS_REL 1e-10, IOR_REL 1e-9 of the sum of the absolute per-path contributions, ROUTE_REL 1e-12 across routes in float mode; none
is derived from a device result -- tests/test_paths_fuzz_host.py measures the host build of the same headers at 5.4e-13 (out_ori) and
below 4e-14 (everything else) on these cases.  The linear functional's VALUE is held to RAY_ABS times the sum of the absolute weights
of the completed rows: what an error of RAY_ABS in every exit coordinate can move it by.

Beyond the restatements: two deterministic runs give the same bits; the IOR form's vertex gradient has the one-pass form's bits;
(2, drop, reference) of every case is render_transparent bit for bit; calls that contribute nothing leave marked accumulators alone;
slices of 1, 63, 64, 65, 255 and 257 rays equal the rows of the full call; and ONE scene that serves a dozen calls of different sizes
and forms in turn -- dense, one-pass, IOR form, smaller after bigger, a regrowth of both workspaces -- gives the bits a fresh scene gives
(stale state bytes, stale one-pass ``hits`` / ``tape``, list counters, the parked rows' stride).

The two ``forward`` members run render_paths under no_grad and nothing else on their scenes: they are what a library built without one
statement of the forward kernels is held against, where a backward pass over a wrong mask would not be safe to run.

MEASURED on the device (printed by test_zz_device_figures with -s; 135 tests in 4 s): tape, hits and mask equal on every
ray of every case; out_ori 5.1e-13, out_dir 4.8e-15; loss 4.3e-16 relative; grad_V 1.2e-14 of its largest entry on all three routes, of
the linear functional 5.9e-14 (1.8e-11 absolute); IOR partials 2.9e-15 of sum |per path|; float against deterministic mode 4.5e-16."""
import functools

import numpy as np
import pytest
import torch

import paths_fuzz_cases as fz
from drt_amd import _lib, det, diffrender as Render

pytestmark = pytest.mark.gpu
RAY_ABS, GRAD_REL, GRAD_ABS, LOSS_REL, IOR_REL, ROUTE_REL = 1e-10, 1e-9, 1e-5, 1e-10, 1e-9, 1e-12
SLICES = (1, 63, 64, 65, 255, 257)
FIGURES = {}          # name -> (largest figure, case): printed by test_zz_device_figures
CASE_IDS = [f"fuzz{s}" for s in fz.CASES]


@pytest.fixture(autouse=True)
def _globals_restored():
    saved = (Render.intIOR, Render.extIOR, Render.resx, Render.resy, det.enable(False))
    yield
    Render.intIOR, Render.extIOR, Render.resx, Render.resy = saved[:4]
    det.enable(saved[4])


def _note(name, value, sc):
    if name not in FIGURES or value > FIGURES[name][0]:
        FIGURES[name] = (float(value), sc["name"])


# ------------------------------------------------------------------------------------------------------------------------ the calls
@functools.lru_cache(maxsize=None)
def _dev(seed, variant=0):
    """The case's rays, targets and weights on the device: made once, never written."""
    sc = fz.case(seed, variant)
    return {key: sc[key].cuda() for key in ("o", "d", "sp", "valid", "w_ori", "w_dir")}


def _scene(sc):
    scene = Render.Scene(sc["mesh"], 0)
    V = torch.tensor(sc["mesh"].vertices, dtype=torch.float64, device="cuda", requires_grad=True)
    scene.update_verticex(V)
    return scene, V


def _grad(out, V):
    g, = torch.autograd.grad(out, V, retain_graph=True, allow_unused=True)
    return torch.zeros_like(V) if g is None else g


def _dense(scene, V, o, d, sp, valid, law, iors, weights=None):
    """render_paths + ray_loss + backward (and, with ``weights``, the linear functional and its gradient): every output, cloned."""
    Render.intIOR, Render.extIOR = iors
    out_ori, out_dir, mask = scene.render_paths(o, d, *law)
    tape, hits = scene.last_path_faces, scene.last_path_hits
    loss = Render.ray_loss(out_ori, out_dir, mask, sp, valid)
    r = dict(out_ori=out_ori.detach().clone(), out_dir=out_dir.detach().clone(), mask=mask.clone(), tape=tape.clone(), hits=hits.clone(),
             loss=loss.detach().clone(), grad=_grad(loss, V).clone())
    if weights is not None:
        lin = (out_ori * weights[0]).sum() + (out_dir * weights[1]).sum()
        r["lin"], r["grad_lin"] = lin.detach().clone(), (_grad(lin, V).clone() if lin.requires_grad else torch.zeros_like(V))
    return r


def _fused(scene, V, o, d, sp, valid, law, iors):
    Render.intIOR, Render.extIOR = iors
    loss = scene.paths_ray_loss_fused(o, d, sp, valid, *law)
    assert loss.shape == () and loss.dtype == torch.float64
    return dict(loss=loss.detach().clone(), grad=_grad(loss, V).clone(), count=int(scene.last_path_count))


def _ior(scene, V, o, d, sp, valid, law, iors, vertices=True):
    """paths_ray_loss_ior_fused with tensor IORs, through backward(): loss, both partials, the count, the vertex gradient (None without
    ``vertices``) and whether the mesh was left without a gradient."""
    Render.intIOR, Render.extIOR = 1.9, 1.7          # the globals are not consulted
    ti = torch.tensor(iors[0], dtype=torch.float64, device="cuda", requires_grad=True)
    te = torch.tensor(iors[1], dtype=torch.float64, device="cuda", requires_grad=True)
    V.grad = None
    loss = scene.paths_ray_loss_ior_fused(o, d, sp, valid, ti, te, *law, vertices=vertices)
    assert loss.shape == () and loss.dtype == torch.float64
    loss.backward()
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    r = dict(loss=loss.detach().clone(), g_int=zero if ti.grad is None else ti.grad.clone(), g_ext=zero if te.grad is None else te.grad.clone(),
             count=int(scene.last_path_count), grad=None, mesh_untouched=V.grad is None and scene.vertices.grad is None)
    if vertices:
        r["grad"] = torch.zeros_like(V) if V.grad is None else V.grad.clone()
    V.grad = None
    return r


@functools.lru_cache(maxsize=None)
def _run(seed, deterministic, repeat=0):
    """(a), (b), (c) and (c) without vertices of a case on ONE fresh scene, in float or deterministic mode: computed once per
    (case, mode, repeat) and shared read-only."""
    sc, t = fz.case(seed), _dev(seed)
    was = det.enable(deterministic)
    try:
        scene, V = _scene(sc)
        args = (scene, V, t["o"], t["d"], t["sp"], t["valid"], sc["law"], (sc["ior_int"], sc["ior_ext"]))
        return dict(a=_dense(*args, weights=(t["w_ori"], t["w_dir"])), b=_fused(*args), c=_ior(*args), c0=_ior(*args, vertices=False))
    finally:
        det.enable(was)


def _grad_close(name, got, ref, sc):
    got, ref = got.detach().cpu().numpy(), np.asarray(ref)
    assert np.isfinite(got).all()
    top, diff = np.abs(ref).max(), np.abs(got - ref).max()
    if top == 0.0:
        assert not got.any(), f"{sc['name']}: {name} must be zero"
        return
    _note(name + " relative", diff / top, sc)
    _note(name + " absolute", diff, sc)
    assert diff <= GRAD_ABS and diff <= GRAD_REL * top, (sc["name"], name, diff, top)


def _loss_close(name, got, ref, sc):
    if ref == 0.0:
        assert got == 0.0, f"{sc['name']}: {name} must be exactly 0, is {got}"
        return
    _note(name, abs(got - ref) / abs(ref), sc)
    assert abs(got - ref) <= LOSS_REL * abs(ref), (sc["name"], name, got, ref)


def _same_bits(a, b):
    """Two results of one call (dicts of tensors, ints, bools, None): equal bit for bit."""
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape, key
            same = torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 else torch.equal(x, y)
            assert same, f"{key} differs in {int((x != y).sum())} of {x.numel()} entries"
        else:
            assert x == y, (key, x, y)


def _forward(scene, o, d, law, iors):
    """render_paths alone, no graph: the forward kernels' outputs, cloned."""
    Render.intIOR, Render.extIOR = iors
    with torch.no_grad():
        out_ori, out_dir, mask = scene.render_paths(o, d, *law)
    return dict(out_ori=out_ori.clone(), out_dir=out_dir.clone(), mask=mask.clone(), tape=scene.last_path_faces.clone(), hits=scene.last_path_hits.clone())


# ------------------------------------------------------------------------------------------------------------ (a) render_paths
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_render_paths_forward_alone_is_exact_on_every_ray(seed):
    """The forward kernels by themselves (k_paths_start, k_paths_shade, k_paths_finish) on a fresh scene, nothing else run on it."""
    sc, aux, ex, t = fz.case(seed), fz.trace(seed), fz.exit_reference(seed), _dev(seed)
    scene, _ = _scene(sc)
    got = _forward(scene, t["o"], t["d"], sc["law"], (sc["ior_int"], sc["ior_ext"]))
    tape, hits, mask = got["tape"].cpu().long(), got["hits"].cpu().long(), got["mask"].cpu()
    differ = (tape != aux["tape"]).any(0) | (hits != aux["hits"]) | (mask[:, 0] != aux["valid"])
    assert not differ.any(), f"{sc['name']}: rays {torch.nonzero(differ).squeeze(1)[:10].tolist()} of {sc['n']} differ in tape, hits or mask"
    oo, od = got["out_ori"].cpu().numpy(), got["out_dir"].cpu().numpy()
    dead = ~mask[:, 0].numpy()
    assert not oo[dead].any() and not od[dead].any()
    assert np.abs(oo - ex["out_ori"]).max() <= RAY_ABS and np.abs(od - ex["out_dir"]).max() <= RAY_ABS


@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_render_paths_against_the_restatement(seed):
    sc, aux, ref, ex, got = fz.case(seed), fz.trace(seed), fz.reference(seed), fz.exit_reference(seed), _run(seed, False)["a"]
    P = sc["n"]
    assert got["mask"].dtype == torch.bool and got["mask"].shape == (P, 3) and got["tape"].shape == (sc["k"], P) and got["hits"].shape == (P,)
    assert got["tape"].dtype == torch.int32 and got["hits"].dtype == torch.uint8
    # ids, counts and masks: exact, on every ray
    tape, hits, mask = got["tape"].cpu().long(), got["hits"].cpu().long(), got["mask"].cpu()
    differ = (tape != aux["tape"]).any(0) | (hits != aux["hits"]) | (mask[:, 0] != aux["valid"])
    assert not differ.any(), f"{sc['name']}: rays {torch.nonzero(differ).squeeze(1)[:10].tolist()} of {P} differ in tape, hits or mask"
    assert torch.equal(mask[:, 0], mask[:, 1]) and torch.equal(mask[:, 0], mask[:, 2])
    oo, od = got["out_ori"].cpu().numpy(), got["out_dir"].cpu().numpy()
    dead = ~mask[:, 0].numpy()
    assert not oo[dead].any() and not od[dead].any()
    _note("out_ori", np.abs(oo - ex["out_ori"]).max(), sc)
    _note("out_dir", np.abs(od - ex["out_dir"]).max(), sc)
    assert np.abs(oo - ex["out_ori"]).max() <= RAY_ABS and np.abs(od - ex["out_dir"]).max() <= RAY_ABS
    _loss_close("ray_loss (dense)", got["loss"].item(), ref["loss"], sc)
    _grad_close("grad_V of ray_loss (dense)", got["grad"], ref["grad_V"], sc)
    live = mask[:, 0]
    bound = RAY_ABS * float(sc["w_ori"][live].abs().sum() + sc["w_dir"][live].abs().sum())
    assert abs(got["lin"].item() - ex["lin"]) <= bound, (sc["name"], got["lin"].item(), ex["lin"], bound)
    _grad_close("grad_V of the linear functional", got["grad_lin"], ex["grad_lin"], sc)


# ------------------------------------------------------------------------------------------------------ (b) paths_ray_loss_fused
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_one_pass_loss_against_the_restatement_and_the_dense_route(seed):
    sc, ref, run = fz.case(seed), fz.reference(seed), _run(seed, False)
    got = run["b"]
    assert got["count"] == ref["count"]
    _loss_close("ray_loss (one pass)", got["loss"].item(), ref["loss"], sc)
    _grad_close("grad_V (one pass)", got["grad"], ref["grad_V"], sc)
    assert abs(got["loss"].item() - run["a"]["loss"].item()) <= ROUTE_REL * abs(run["a"]["loss"].item())


# -------------------------------------------------------------------------------------------------- (c) paths_ray_loss_ior_fused
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_ior_form_against_the_restatement(seed):
    sc, ref, run = fz.case(seed), fz.reference(seed), _run(seed, False)
    for key in ("c", "c0"):
        got = run[key]
        assert got["count"] == ref["count"]
        _loss_close("ray_loss (IOR form)", got["loss"].item(), ref["loss"], sc)
        for part in ("int", "ext"):
            g, want, scale = got["g_" + part].item(), ref["g_" + part], ref["abs_" + part]
            assert np.isfinite(g)
            if ref["count"] == 0:
                assert g == 0.0
                continue
            _note("g_" + part, abs(g - want) / scale, sc)
            assert abs(g - want) <= IOR_REL * scale, (sc["name"], key, part, g, want, scale)
    _grad_close("grad_V (IOR form)", run["c"]["grad"], ref["grad_V"], sc)
    assert run["c0"]["mesh_untouched"] and run["c0"]["grad"] is None


# ----------------------------------------------------------------------------------------------------- (d) deterministic mode
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_deterministic_runs_give_the_same_bits_and_the_forms_share_them(seed):
    sc, one, two, flt = fz.case(seed), _run(seed, True, 0), _run(seed, True, 1), _run(seed, False)
    for key in ("a", "b", "c", "c0"):
        _same_bits(one[key], two[key])
    # the IOR form's vertex gradient and loss are the one-pass form's; without vertices the loss and the partials stay
    assert torch.equal(one["c"]["grad"], one["b"]["grad"]) and torch.equal(one["c"]["loss"], one["b"]["loss"]) and one["c"]["count"] == one["b"]["count"]
    for key in ("loss", "g_int", "g_ext", "count"):
        assert (torch.equal(one["c0"][key], one["c"][key]) if isinstance(one["c"][key], torch.Tensor) else one["c0"][key] == one["c"][key]), key
    assert one["c0"]["mesh_untouched"]
    # and the dense route's (tests/test_gpu_paths_fused.py asserts it on the hand)
    assert torch.equal(one["b"]["loss"], one["a"]["loss"]) and torch.equal(one["b"]["grad"], one["a"]["grad"])
    # the forward does not depend on the mode; the float-mode gradients agree with the exact sums
    for key in ("out_ori", "out_dir", "mask", "tape", "hits"):
        assert torch.equal(one["a"][key], flt["a"][key]), key
    for form, key in (("a", "grad"), ("a", "grad_lin"), ("b", "grad"), ("c", "grad")):
        top = one[form][key].abs().max().item()
        diff = (flt[form][key] - one[form][key]).abs().max().item()
        if top > 0:
            _note("float mode against deterministic", diff / top, sc)
        assert diff <= ROUTE_REL * top, (sc["name"], form, key, diff, top)


# --------------------------------------------------------------------------------- (e) (2, drop, reference) IS render_transparent
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_two_bounces_drop_reference_equals_render_transparent(seed):
    sc, t = fz.case(seed), _dev(seed)
    Render.intIOR, Render.extIOR = sc["ior_int"], sc["ior_ext"]
    Render.resx, Render.resy = sc["width"], sc["height"]
    sa, Va = _scene(sc)
    ra = sa.render_transparent(t["o"].clone(), t["d"].clone())
    sb, Vb = _scene(sc)
    rb = sb.render_paths(t["o"].clone(), t["d"].clone(), 2, "drop", "reference")
    for x, y in zip(ra, rb):
        assert x.dtype == y.dtype and torch.equal(x, y)
    keep = rb[2][:, 0]
    assert torch.equal(sb.last_path_faces[0][keep], sa.last_face1[keep]) and torch.equal(sb.last_path_faces[1][keep], sa.last_face2[keep])
    assert torch.equal(sb.last_path_hits, 2 * keep.to(torch.uint8))
    # and the restatement's trace of that law, on every ray
    aux = fz.trace_of(sc, law=(2, "drop", "reference"))
    assert torch.equal(keep.cpu(), aux["valid"]) and torch.equal(sb.last_path_faces.cpu().long(), aux["tape"])
    la, lb = Render.ray_loss(*ra, t["sp"], t["valid"]), Render.ray_loss(*rb, t["sp"], t["valid"])
    assert abs(la.item() - lb.item()) <= 1e-14 * abs(la.item())
    ga, gb = _grad(la, Va), _grad(lb, Vb)
    assert (ga - gb).abs().max().item() <= ROUTE_REL * ga.abs().max().item()


# -------------------------------------------------------------------------------------------------------------- (f) zero cases
def _marked(V, seed):
    rng = np.random.default_rng(seed)
    return (torch.tensor(rng.standard_normal(()), device="cuda"), torch.tensor(rng.standard_normal(tuple(V.shape)), device="cuda"),
            torch.tensor(rng.standard_normal(2), device="cuda"), torch.full((1,), 12345, dtype=torch.int64, device="cuda"))


def _abi_calls(scene, V, o, d, sp, va, sc, acc):
    """Both one-pass entry points, and the IOR form without its gradient table, adding into the cells of ``acc`` (loss, grad_v, grad_ior, count)."""
    lib, h, s = _lib.lib(), scene.optix_mesh._h, torch.cuda.current_stream().cuda_stream
    flags = Render._law_flags(sc["tir"], sc["refraction"])
    head = (h, V.data_ptr(), o.data_ptr(), d.data_ptr(), sp.data_ptr(), va.data_ptr(), o.shape[0], sc["ior_int"], sc["ior_ext"], sc["k"], flags)
    _lib.check(lib.drt_render_paths_law_ray_loss_fused(*head, acc[0].data_ptr(), acc[1].data_ptr(), acc[3].data_ptr(), s))
    _lib.check(lib.drt_render_paths_law_ray_loss_ior_fused(*head, acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), acc[3].data_ptr(), s))
    _lib.check(lib.drt_render_paths_law_ray_loss_ior_fused(*head, acc[0].data_ptr(), None, acc[2].data_ptr(), acc[3].data_ptr(), s))


@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_calls_that_contribute_nothing_return_zero_and_leave_marked_cells_alone(seed):
    sc, t, ref = fz.case(seed), _dev(seed), fz.reference(seed)
    scene, V = _scene(sc)
    Vd = V.detach()
    iors = (sc["ior_int"], sc["ior_ext"])
    valids = [torch.zeros_like(t["valid"])] + ([t["valid"]] if ref["count"] == 0 else [])          # no ray has a target / nothing completes
    for valid in valids:
        acc = _marked(Vd, 11 + seed)
        keep = [x.clone() for x in acc]
        _abi_calls(scene, Vd, t["o"], t["d"], t["sp"], valid.view(torch.uint8), sc, acc)
        torch.cuda.synchronize()
        for a, b in zip(keep, acc):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        got = _fused(scene, V, t["o"], t["d"], t["sp"], valid, sc["law"], iors)
        assert got["loss"].item() == 0.0 and got["count"] == 0 and not got["grad"].any()
        for vertices in (True, False):
            got = _ior(scene, V, t["o"], t["d"], t["sp"], valid, sc["law"], iors, vertices=vertices)
            assert got["loss"].item() == 0.0 and got["count"] == 0 and got["g_int"].item() == 0.0 and got["g_ext"].item() == 0.0
            assert got["grad"] is None or not got["grad"].any()
    # (the cells ARE added to where something contributes: the control of the marks)
    if ref["count"] > 0:
        acc = _marked(Vd, 11 + seed)
        keep = [x.clone() for x in acc]
        _abi_calls(scene, Vd, t["o"], t["d"], t["sp"], t["valid"].view(torch.uint8), sc, acc)
        assert int(acc[3]) == 12345 + 3 * ref["count"] and not torch.equal(acc[0], keep[0]) and not torch.equal(acc[1], keep[1])


# ------------------------------------------------------------------------------------------------------------------ (g) slices
@pytest.mark.parametrize("seed", fz.CASES, ids=CASE_IDS)
def test_slices_equal_the_rows_of_the_full_call(seed):
    sc, t, full = fz.case(seed), _dev(seed), _run(seed, False)
    P, iors = sc["n"], (sc["ior_int"], sc["ior_ext"])
    rng = np.random.default_rng(fz.BASE + 700000 + seed)
    scene, V = _scene(sc)
    Render.intIOR, Render.extIOR = iors
    for size in SLICES:
        if size > P:
            continue
        lo = int(rng.integers(0, P - size + 1))
        hi = lo + size
        part = scene.render_paths(t["o"][lo:hi], t["d"][lo:hi], *sc["law"])
        for key, x in zip(("out_ori", "out_dir", "mask"), part):
            assert torch.equal(x.detach(), full["a"][key][lo:hi]), (sc["name"], size, lo, key)
        assert torch.equal(scene.last_path_faces, full["a"]["tape"][:, lo:hi]) and torch.equal(scene.last_path_hits, full["a"]["hits"][lo:hi]), (size, lo)
    # a partition of the rays into such slices: the one-pass losses and counts add up to the full call's
    total, count, lo, k = 0.0, 0, 0, int(rng.integers(len(SLICES)))
    while lo < P:
        hi = min(P, lo + SLICES[k % len(SLICES)])
        got = _fused(scene, V, t["o"][lo:hi], t["d"][lo:hi], t["sp"][lo:hi], t["valid"][lo:hi], sc["law"], iors)
        total, count, lo, k = total + got["loss"].item(), count + got["count"], hi, k + 1
    assert count == full["b"]["count"]
    assert abs(total - full["b"]["loss"].item()) <= ROUTE_REL * abs(full["b"]["loss"].item())


# ------------------------------------------------------------------------------------------------------ (h) one scene, many calls
def _calls_of(seed, va, vb):
    """The calls of one pair, as (label, variant whose mesh state it needs, function of (scene, V)): 1-ray dense, full one-pass, 63-ray
    IOR form without vertices, full dense at another K under the other formula, 257-ray one-pass, ... in a seeded order; then two calls
    larger than any before (both workspaces regrow), then the first three again."""
    A, B, ta, tb = fz.case(seed, va), fz.case(seed, vb), _dev(seed, va), _dev(seed, vb)
    rng = np.random.default_rng(fz.BASE + 800000 + seed)

    def rows(sc, t, size):
        size = min(size, sc["n"])
        lo = int(rng.integers(0, sc["n"] - size + 1))
        return tuple(t[key][lo:lo + size] for key in ("o", "d", "sp", "valid"))

    def every(sc, t):
        return tuple(t[key] for key in ("o", "d", "sp", "valid"))

    def other(sc):
        return (sc["k"] - 1 if sc["k"] > 2 else 3, sc["tir"], "snell" if sc["refraction"] == "reference" else "reference")

    ia, ib = (A["ior_int"], A["ior_ext"]), (B["ior_int"], B["ior_ext"])
    one, r63, r257, r65, r255 = rows(A, ta, 1), rows(B, tb, 63), rows(B, tb, 257), rows(A, ta, 65), rows(A, ta, 255)
    calls = [("1-ray dense", lambda s, V: _dense(s, V, *one, A["law"], ia)),
             ("full one-pass", lambda s, V: _fused(s, V, *every(A, ta), A["law"], ia)),
             ("63-ray IOR form, no vertices", lambda s, V: _ior(s, V, *r63, B["law"], ib, vertices=False)),
             ("full dense, another K, the other formula", lambda s, V: _dense(s, V, *every(A, ta), other(A), ia)),
             ("257-ray one-pass", lambda s, V: _fused(s, V, *r257, B["law"], ib)),
             ("full dense of the second case", lambda s, V: _dense(s, V, *every(B, tb), B["law"], ib)),
             ("full IOR form", lambda s, V: _ior(s, V, *every(A, ta), A["law"], ia)),
             ("65-ray dense", lambda s, V: _dense(s, V, *r65, A["law"], ia)),
             ("full one-pass of the second case", lambda s, V: _fused(s, V, *every(B, tb), B["law"], ib)),
             ("255-ray one-pass, the other TIR rule", lambda s, V: _fused(s, V, *r255, (A["k"], "drop" if A["tir"] == "reflect" else "reflect", A["refraction"]), ia))]
    order = [calls[0]] + [calls[1 + i] for i in rng.permutation(len(calls) - 1)]
    both = tuple(torch.cat([ta[key], tb[key]]).contiguous() for key in ("o", "d", "sp", "valid"))
    order += [("dense, larger than any before", lambda s, V: _dense(s, V, *both, A["law"], ia)),
              ("one-pass, larger than any before", lambda s, V: _fused(s, V, *both, B["law"], ib))]
    return order + order[:3]


@pytest.mark.parametrize("seed,va,vb", fz.PAIRS, ids=[f"fuzz{p[0]}" for p in fz.PAIRS])
def test_one_scene_serving_many_forward_calls_gives_the_bits_of_fresh_scenes(seed, va, vb):
    """The dense forward alone (state bytes, list counters, ``hits``): calls of 1, 63, 65, 257 and all rays of both cases under their own
    laws and another K with the other formula, a call larger than any before, then the first three again -- on one scene."""
    A, B, ta, tb = fz.case(seed, va), fz.case(seed, vb), _dev(seed, va), _dev(seed, vb)
    rng = np.random.default_rng(fz.BASE + 900000 + seed)
    ia, ib = (A["ior_int"], A["ior_ext"]), (B["ior_int"], B["ior_ext"])

    def rows(sc, t, size):
        size = min(size, sc["n"])
        lo = int(rng.integers(0, sc["n"] - size + 1))
        return t["o"][lo:lo + size], t["d"][lo:lo + size]

    other_a = (A["k"] - 1 if A["k"] > 2 else 3, A["tir"], "snell" if A["refraction"] == "reference" else "reference")
    calls = [(rows(A, ta, 1), A["law"], ia), ((ta["o"], ta["d"]), A["law"], ia), (rows(B, tb, 63), B["law"], ib), ((ta["o"], ta["d"]), other_a, ia),
             (rows(B, tb, 257), B["law"], ib), ((tb["o"], tb["d"]), B["law"], ib), (rows(A, ta, 65), A["law"], ia), (rows(A, ta, 255), other_a, ia)]
    order = [calls[0]] + [calls[1 + i] for i in rng.permutation(len(calls) - 1)]
    order += [((torch.cat([ta["o"], tb["o"]]), torch.cat([ta["d"], tb["d"]])), A["law"], ia)]
    order += order[:3]
    kept, _ = _scene(A)
    for n, ((o, d), law, iors) in enumerate(order):
        got = _forward(kept, o, d, law, iors)
        fresh, _ = _scene(A)
        try:
            _same_bits(got, _forward(fresh, o, d, law, iors))
        except AssertionError as e:
            raise AssertionError(f"{A['name']}: forward call {n} ({o.shape[0]} rays, {law}) on the kept scene differs from a fresh scene's: {e}") from None


@pytest.mark.parametrize("seed,va,vb", fz.PAIRS, ids=[f"fuzz{p[0]}" for p in fz.PAIRS])
def test_one_scene_serving_many_calls_gives_the_bits_of_fresh_scenes(seed, va, vb):
    A = fz.case(seed, va)
    det.enable(True)
    kept, V = _scene(A)
    order = _calls_of(seed, va, vb)
    assert len(order) >= 12
    for n, (label, call) in enumerate(order):
        got = call(kept, V)
        fresh, Vf = _scene(A)
        want = call(fresh, Vf)
        try:
            _same_bits(got, want)
        except AssertionError as e:
            raise AssertionError(f"{A['name']}: call {n} ({label}) on the kept scene differs from a fresh scene's: {e}") from None


# --------------------------------------------------------------------------------------------------------------------- figures
def test_zz_device_figures():
    """Prints the largest disagreement of every quantity over all cases (what DESIGN.md 7.5 quotes)."""
    print()
    for name, (value, where) in sorted(FIGURES.items()):
        print(f"largest device disagreement  {name:45s} {value:.3e}  ({where})")
    assert FIGURES
