"""CPU: admission, coverage, host twins and negative controls of the image family's fuzz cases (tests/image_fuzz_cases.py), the CPU side of
tests/test_gpu_image_fuzz.py.

Admission is computed from the float64 restatements alone -- conditions on the inputs, not measurements of anything under test:
  * the sensitive pixels (grazing, border, pole) are at most image_cases.SENSITIVE_CAP of the image;
  * every gradient-carrying sample keeps TEXEL_MARGIN from the texel lines and borders of the screen (the through samples for the plain
    loss; the direct ones too for the screen and camera members), every read of the environment from its texel lines (and POLE from its
    poles for the texel / rotation member);
  * the loss is more than the rounding of a float32 target (H W C 2^-46, the bound tests/test_gpu_image_loss.py states for a target that
    is the call's own image): a relative tolerance on a loss of rounding alone measures the rounding, not the law;
  * conditioning: with every vertex coordinate moved by one float64 unit in the last place (seeded signs) the restatement's classes and
    count are unchanged and its loss and gradients move by less than a tenth of their tolerance.
Coverage of the literal lists is asserted, the host builds of the headers (tests/hostsim/image_*.cpp) run on the same cases against the
restatements with the GPU test's tolerances (the loss 1e-10 relative, gradients ``image_loss_cases.close``, counts exact), and the negative
controls show that a restatement with a term detached, or with a texture's or environment's extents swapped, is outside them.

Measured here (printed by the tests; -s shows them), the largest over the cases of each list:
  * sensitive share 2.86 % (one pixel of 35); smallest margin 1.3e-6 texel; conditioning, as a share of the tolerance: loss 1.2e-3, vertex
    gradient 3.9e-3, IOR partials 2.6e-3, the other members' gradients at most 1.9e-3;
  * the host twins' difference from the restatement -- loss 4.5e-15 relative; grad_V 2.0e-13 of its largest entry; screen pose 1.2e-15,
    texture 8.7e-16; the three camera groups 2.0e-14; g_sigma 1.5e-15; environment texels 1.1e-14, rotation 1.7e-14; three views listed
    [2, 0, 2], clear and in the room: loss 4.2e-15, grad_V 1.3e-14; counts equal;
  * swapped extents move an image by at least 0.125, against tolerances below 5e-7."""
import functools

import numpy as np
import pytest
import torch

import image_cases
import image_env_cases
import image_fuzz_cases as fz
import image_loss_cases
import image_loss_ref
import image_ref

close = image_loss_cases.close
LOSS_REL = 1e-10             # the ceiling image_loss_cases states, and what the ray-loss fuzz uses
TEXEL_MARGIN = image_loss_cases.TEXEL_MARGIN
CONDITION_SHARE = 0.1        # of a tolerance: how far one unit in the last place of every vertex coordinate may move a result
ENV_IDS = [f"{seed}-{'screen' if ws else 'no-screen'}-{'reflection' if rf else 'no-reflection'}" for seed, ws, rf in fz.ENV_CASES]


def loss_close(got, want):
    """The loss tolerance of the fuzz tests: LOSS_REL relative; a zero reference asks for exactly zero."""
    return got == 0.0 if want == 0.0 else abs(got - want) <= LOSS_REL * abs(want)


def _of_tolerance(got, want):
    """|got - want| as a share of ``close``'s tolerance for ``want`` (0 when both are all zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max()
    if top == 0:
        return 0.0 if not got.any() else np.inf
    return float(np.abs(got - want).max() / min(image_loss_cases.GRAD_ABS, image_loss_cases.GRAD_REL * top))


def _rel_top(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max()
    return float(np.abs(got - want).max() / top) if top > 0 else float(np.abs(got).max())


def nudged(sc, seed):
    """The scene with every vertex coordinate moved to a neighbouring float64, the side drawn from the seed."""
    rng = np.random.default_rng(fz.BASE + 900000 + seed)
    V = np.asarray(sc["mesh"].vertices, np.float64)
    mesh = type(sc["mesh"])(np.nextafter(V, np.where(rng.random(V.shape) < 0.5, -np.inf, np.inf)), sc["mesh"].faces)
    return dict(sc, mesh=mesh)


def _margin(us, vs, tex_h, tex_w):
    """The smallest distance of (u, v) from a texel line or a border of a tex_h x tex_w screen, in texels."""
    best = np.inf
    for w, top in ((us, tex_w - 1), (vs, tex_h - 1)):
        if len(w):
            best = min(best, np.abs(w - np.rint(w)).min(), w.min(), (top - w).min())
    return float(best)


@functools.lru_cache(maxsize=None)
def figures(seed):
    """What admission and coverage read of a case, from the restatements alone."""
    import snell_ref
    sc, st, ref = fz.case(seed), fz.stage(seed), fz.loss_reference(seed)
    fwd = ref["fwd"]
    cls = st["cls"].numpy()
    looks, on = cls != image_ref.INVALID, st["on"].numpy()
    through = cls == image_ref.THROUGH
    tex_h, tex_w = sc["texture3"].shape[:2]
    assert np.array_equal(fwd["cls"].numpy(), cls) and np.array_equal(fwd["on"].numpy(), on)
    assert np.abs(ref["image"].astype(np.float64) - st["image"].numpy().astype(np.float64)).max() <= 2.0 ** -23
    sel = on & through
    o, d = image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
    aux = snell_ref.trace(sc["mesh"].faces, torch.tensor(sc["mesh"].vertices), o, d, sc["ior_int"], sc["ior_ext"], *sc["law"])
    again = fz.loss_of_scene(nudged(sc, seed))
    same = bool(np.array_equal(again["fwd"]["cls"].numpy(), cls) and np.array_equal(again["fwd"]["on"].numpy(), on) and again["count"] == ref["count"])
    cond = dict(loss=abs(again["loss"] - ref["loss"]) / (LOSS_REL * ref["loss"]) if ref["loss"] > 0 else float(again["loss"] != 0),
                grad_V=_of_tolerance(again["grad_V"], ref["grad_V"]), g_int=_of_tolerance(again["g_int"], ref["g_int"]),
                g_ext=_of_tolerance(again["g_ext"], ref["g_ext"]))
    return dict(samples=len(cls), direct=int((cls == image_ref.DIRECT).sum()), through=int(through.sum()), invalid=int((~looks).sum()),
                off_screen=int((looks & ~on).sum()), away=int((looks & ~(st["t"] > 0).numpy()).sum()), through_off=int((through & ~on).sum()),
                count=ref["count"], loss=ref["loss"], sensitive=float(image_cases.sensitive(sc, st).mean()),
                margin=_margin(fwd["u"].detach().numpy()[sel], fwd["v"].detach().numpy()[sel], tex_h, tex_w), same=same, cond=cond,
                max_hits=int(aux["hits"][aux["valid"]].max()) if aux["valid"].any() else 0, two=fz.two_components(sc))


def _admit(seed, fig, margin, cond):
    sc = fz.case(seed)
    print(f"seed {seed}: {sc['height']} x {sc['width']} s {sc['s']} C {sc['texture3'].shape[2]} law {sc['law']} fresnel {sc['fresnel']} ior {sc['ior_int']} / "
          f"{sc['ior_ext']} distance {sc['distance']} texture {sc['texture3'].shape[:2]} span {sc['span']} moved {sc['moved']} environment "
          f"{sc['environment'].shape[:2]} faces {len(sc['mesh'].faces)}; direct {fig['direct']} through {fig['through']} invalid {fig['invalid']} off-screen "
          f"{fig['off_screen']} away {fig['away']} count {fig['count']} loss {fig['loss']:.6e}; sensitive share {fig['sensitive']:.4f}; margin {margin:.2e}; "
          f"conditioning " + ", ".join(f"{k} {v:.1e}" for k, v in cond.items()))
    assert fig["sensitive"] <= image_cases.SENSITIVE_CAP
    assert margin >= TEXEL_MARGIN
    assert fig["loss"] > sc["height"] * sc["width"] * sc["texture3"].shape[2] * 2.0 ** -46
    assert fig["same"] and max(cond.values()) < CONDITION_SHARE


# ---- admission -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", fz.CASES)
def test_admission_of_the_forward_and_plain_loss_cases(seed):
    sc, fig = fz.case(seed), figures(seed)
    assert len(sc["mesh"].faces) <= 1600 and fig["samples"] < fz.MAX_SAMPLES
    assert np.array_equal(sc["mesh"].vertices, sc["mesh"].vertices.astype(np.float32).astype(np.float64))
    _admit(seed, fig, fig["margin"], fig["cond"])


def test_the_lists_are_literal_subsets():
    assert len(fz.CASES) == len(set(fz.CASES)) == 16
    for sub in (fz.SCREEN_CASES, fz.CAMERA_CASES, fz.ABSORB_CASES, [c[0] for c in fz.ENV_CASES]):
        assert len(sub) == len(set(sub)) == 6 and set(sub) <= set(fz.CASES)
    assert len(fz.VIEWS_CASES) == 4 and set(fz.VIEWS_CASES) <= set(fz.CASES)
    assert sum(ws for _, ws, _ in fz.ENV_CASES) == 3 and sum(rf for _, _, rf in fz.ENV_CASES) == 4
    assert {fz.case(seed)["texture3"].shape[:2] for seed in fz.SCREEN_CASES} >= {(2, 2), (2, 37)}
    assert fz.case(fz.CASES[0]) is fz.case(fz.CASES[0]) and np.array_equal(fz.base.__wrapped__(3)["texture3"], fz.base.__wrapped__(3)["texture3"])


def test_coverage_of_the_list():
    scs, figs = [fz.case(seed) for seed in fz.CASES], [figures(seed) for seed in fz.CASES]
    assert {sc["law"] for sc in scs} == set(image_cases.LAWS)
    assert {sc["s"] for sc in scs} == {1, 2, 3, 4} and {sc["texture3"].shape[2] for sc in scs} == {1, 3} and {sc["fresnel"] for sc in scs} == {True, False}
    assert {sc["texture"].ndim for sc in scs if sc["texture3"].shape[2] == 1} == {2, 3}          # C = 1 as [Th, Tw] and as [Th, Tw, 1]
    assert {sc["ior_int"] for sc in scs} == set(fz.IORS_INT) and {sc["ior_ext"] for sc in scs} == set(fz.IORS_EXT)
    assert {sc["distance"] for sc in scs} == set(fz.DISTANCES) and {sc["span"] for sc in scs} == set(fz.SPANS)
    assert {(sc["height"], sc["width"]) for sc in scs} >= {(1, 1), (1, 67), (5, 7), (17, 23), (32, 20), (9, 41)}
    assert sum(f["count"] == 0 and f["loss"] > 1e-3 for f in figs) >= 2
    assert any(f["samples"] < 64 for f in figs) and any(f["samples"] % 64 for f in figs) and any(f["samples"] > 4096 for f in figs)
    assert any(f["two"] and f["max_hits"] >= 4 for f in figs)
    assert any(f["through"] > 0 and 2 * f["through_off"] > f["through"] for f in figs)
    for k in ("direct", "through", "invalid", "off_screen", "away"):
        assert sum(f[k] for f in figs) > 100, k
    assert 2 * sum(sc["texture3"].shape[0] != sc["texture3"].shape[1] for sc in scs) >= len(scs)
    assert 2 * sum(sc["environment"].shape[0] != sc["environment"].shape[1] for sc in scs) >= len(scs)
    assert any(sc["moved"] for sc in scs) and any(sc["weight"] is None for sc in scs) and any(sc["weight"] is not None and (sc["weight"] == 0).any() for sc in scs)
    assert any(np.ndim(sc["void"]) == 0 for sc in scs) and any(np.ndim(sc["void"]) == 1 for sc in scs)


# ---- host twins ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def libs():
    import test_image_absorb_host
    import test_image_camera_host
    import test_image_env_host
    import test_image_env_param_host
    import test_image_loss_host
    import test_image_screen_host
    import test_image_views_env_host
    import test_image_views_host
    return dict(views_env=test_image_views_env_host.load_hv(), loss=test_image_loss_host.load_hs(), screen=test_image_screen_host.load_hs(), camera=test_image_camera_host.load_hs(),
                absorb=test_image_absorb_host.load_hs(), env=test_image_env_host.load_hs(), env_param=test_image_env_param_host.load_hs(),
                views=test_image_views_host.load_hv())


def _check_loss_and_grads(got, ref, what):
    rel = abs(got["loss"] - ref["loss"]) / ref["loss"] if ref["loss"] else abs(got["loss"])
    print(f"{what}: loss {got['loss']:.12e} restatement {ref['loss']:.12e} relative difference {rel:.2e}; grad_V differs by {_rel_top(got['grad_V'], ref['grad_V']):.2e} "
          f"of its largest entry {np.abs(ref['grad_V']).max():.3e}; g_int {got['g_int']:.9e} / {ref['g_int']:.9e}, g_ext {got['g_ext']:.9e} / {ref['g_ext']:.9e}; "
          f"count {got['count']} / {ref['count']}")
    assert got["count"] == ref["count"]
    assert loss_close(got["loss"], ref["loss"])
    assert close(got["grad_V"], ref["grad_V"]) and close(got["g_int"], ref["g_int"]) and close(got["g_ext"], ref["g_ext"])
    if ref["count"] == 0:
        assert not got["grad_V"].any() and got["g_int"] == 0 and got["g_ext"] == 0


@pytest.mark.parametrize("seed", fz.CASES)
def test_host_loss_against_the_restatement(libs, seed):
    import test_image_loss_host as host
    sc, ref = fz.case(seed), fz.loss_reference(seed)
    got = host.HostView(libs["loss"], sc, sc["law"], sc["fresnel"]).run(want_image=True)
    _check_loss_and_grads(got, ref, f"seed {seed}")
    assert np.abs(got["image"].astype(np.float64) - ref["image"].astype(np.float64)).max() <= 2.0 ** -23


@pytest.mark.parametrize("seed", fz.SCREEN_CASES)
def test_host_screen_pose_and_texture_gradients(libs, seed):
    import image_screen_ref
    import test_image_screen_host as host
    sc, ref, fig = fz.case(seed), fz.screen_reference(seed), figures(seed)
    nsc = nudged(sc, seed)
    const = image_screen_ref.trace(nsc["mesh"].faces, nsc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["s"], sc["law"], sc["fresnel"], sc["ior_int"],
                                   sc["ior_ext"])
    moved = image_screen_ref.loss_and_grads(const, image_screen_ref.rows_of(sc["screen"]), sc["texture3"], sc["target"], sc["s"], sc["void"], sc["invalid"],
                                            weight=sc["weight"])
    cond = dict(g_screen=_of_tolerance(moved["g_screen"], ref["g_screen"]), g_texture=_of_tolerance(moved["g_texture"], ref["g_texture"]))
    _admit(seed, fig, ref["margin"], cond)                        # the margin of every sample on the screen, direct ones included
    assert ref["on"] > 0 and np.abs(ref["g_screen"]).max() > 0 and np.abs(ref["g_texture"]).max() > 0
    got = host.HostView(libs["screen"], sc, sc["law"], sc["fresnel"]).run()
    print(f"seed {seed}: g_screen differs by {_rel_top(got['g_screen'], ref['g_screen']):.2e} of its largest entry, g_texture by "
          f"{_rel_top(got['g_texture'], ref['g_texture']):.2e}; loss {got['loss']:.12e} / {ref['loss']:.12e}")
    assert loss_close(got["loss"], ref["loss"]) and got["count"] == ref["on"]
    assert close(got["g_screen"], ref["g_screen"]) and close(got["g_texture"], ref["g_texture"])
    assert ((got["g_texture"] == 0) == (ref["g_texture"] == 0)).all()


@pytest.mark.parametrize("seed", fz.CAMERA_CASES)
def test_host_camera_gradient(libs, seed):
    import image_camera_ref
    import test_image_camera_host as host
    sc, ref, fig = fz.case(seed), fz.camera_reference(seed), figures(seed)
    nsc = nudged(sc, seed)
    moved = image_camera_ref.loss_and_grads(*fz.render_args(nsc), sc["target"], *fz._law_args(sc), weight=sc["weight"])
    want, other = image_camera_ref.groups(ref["g_rinv"], ref["g_kinv"]), image_camera_ref.groups(moved["g_rinv"], moved["g_kinv"])
    _admit(seed, fig, ref["margin"], {k: _of_tolerance(other[k], want[k]) for k in want})
    got = host.HostView(libs["camera"], sc, sc["law"], sc["fresnel"]).run()
    have = image_camera_ref.groups(got["g_rinv"], got["g_kinv"])
    print(f"seed {seed}: " + "; ".join(f"{k} differs by {_rel_top(have[k], want[k]):.2e} of its largest entry {np.abs(want[k]).max():.3e}" for k in want))
    assert loss_close(got["loss"], ref["loss"]) and got["through"] == ref["through_on"] == fig["count"]
    for k in want:
        assert np.abs(want[k]).max() > 0 and close(have[k], want[k]), k


@pytest.mark.parametrize("seed", fz.ABSORB_CASES)
def test_host_absorption(libs, seed):
    import image_absorb_ref
    import test_image_absorb_host as host
    sc, ref, fig = fz.case(seed), fz.absorb_reference(seed), figures(seed)
    nsc = nudged(sc, seed)
    moved = image_absorb_ref.loss_and_grads(*fz.render_args(nsc), sc["target"], *fz._law_args(sc), sc["sigma"], weight=sc["weight"])
    cond = {k: _of_tolerance(moved[k], ref[k]) for k in ("grad_V", "g_int", "g_ext", "g_sigma")}
    cond["loss"] = abs(moved["loss"] - ref["loss"]) / (LOSS_REL * ref["loss"])
    _admit(seed, fig, fig["margin"], cond)
    assert ref["count"] == fig["count"] > 0 and np.abs(ref["g_sigma"]).max() > 0
    got = host.HostView(libs["absorb"], sc, sc["law"], sc["fresnel"]).run(want_image=True)
    _check_loss_and_grads(got, ref, f"seed {seed}")
    print(f"seed {seed}: g_sigma {got['g_sigma']} / {ref['g_sigma']} differs by {_rel_top(got['g_sigma'], ref['g_sigma']):.2e} of its largest entry")
    assert close(got["g_sigma"], ref["g_sigma"])
    want = ref["fwd"]["mean"].detach().to(torch.float32).view(sc["height"], sc["width"], -1).numpy()
    assert np.abs(got["image"].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23


def env_figures(seed, with_screen, reflection):
    """(margin of every read of the environment from its texel lines, smallest 1 - |e_y| of a read, sensitive share) of a case."""
    import image_env_param_cases
    sc = fz.case(seed)
    par = fz.env_param_reference(seed, with_screen, reflection)
    exit_margin, refl_margin, pole, _, _, reads = image_env_param_cases.margins(par["fwd"])
    img = fz.env_image_reference(seed, with_screen, reflection)
    bad = image_env_cases.sensitive(sc, sc["law"], with_screen, reflection, ref=img, stage=fz.stage(seed, True))
    return min(exit_margin, refl_margin), pole, float(bad.mean()), reads


@pytest.mark.parametrize("seed,with_screen,reflection", fz.ENV_CASES, ids=ENV_IDS)
def test_host_environment(libs, seed, with_screen, reflection):
    import image_env_param_ref
    import image_env_ref
    import test_image_env_host as host
    import test_image_env_param_host as host_param
    sc, ref, par = fz.case(seed), fz.env_loss_reference(seed, with_screen, reflection), fz.env_param_reference(seed, with_screen, reflection)
    target = fz.env_target(seed, with_screen, reflection)
    margin, pole, share, reads = env_figures(seed, with_screen, reflection)
    nsc = nudged(sc, seed)
    moved = image_env_ref.loss_and_grads(*fz.env_args(nsc, with_screen), target, sc["s"], sc["law"], sc["invalid"], sc["ior_int"], sc["ior_ext"], weight=sc["weight"],
                                         reflect=reflection)
    moved_par = image_env_param_ref.loss_and_grads(*fz.env_args(nsc, with_screen), target, sc["s"], sc["law"], sc["invalid"], sc["ior_int"], sc["ior_ext"],
                                                   weight=sc["weight"], reflect=reflection)
    cond = {k: _of_tolerance(moved[k], ref[k]) for k in ("grad_V", "g_int", "g_ext")}
    cond.update(loss=abs(moved["loss"] - ref["loss"]) / (LOSS_REL * ref["loss"]), g_env=_of_tolerance(moved_par["g_env"], par["g_env"]),
                g_R=_of_tolerance(moved_par["g_R"], par["g_R"]))
    print(f"seed {seed} screen {with_screen} reflection {reflection}: reads {reads} margin {margin:.2e} pole {pole:.2e} sensitive share {share:.4f} count {ref['count']} "
          f"loss {ref['loss']:.6e}; conditioning " + ", ".join(f"{k} {v:.1e}" for k, v in cond.items()))
    assert share <= image_cases.SENSITIVE_CAP and margin >= image_env_cases.TEXEL_MARGIN and pole >= image_env_cases.POLE
    assert moved["count"] == ref["count"] > 0 and np.array_equal(moved["fwd"]["cls"].numpy(), ref["fwd"]["cls"].numpy()) and max(cond.values()) < CONDITION_SHARE
    assert abs(par["loss"] - ref["loss"]) <= 1e-13 * ref["loss"] and ref["loss"] > sc["height"] * sc["width"] * sc["texture3"].shape[2] * 2.0 ** -46
    assert np.abs(ref["image"].astype(np.float64) - fz.env_image_reference(seed, with_screen, reflection)["image"].numpy().astype(np.float64)).max() <= 2.0 ** -22
    got = host.host_loss_of(libs["env"], sc, sc["law"], with_screen, reflection, ref["fwd"], sc["environment"], sc["rotation"], target, sc["weight"], sc["ior_int"],
                            sc["ior_ext"])
    _check_loss_and_grads(got, ref, f"seed {seed}")
    assert np.abs(got["image"].astype(np.float64) - ref["image"].astype(np.float64)).max() <= 2.0 ** -23
    gp = host_param.host_view_of(libs["env_param"], sc, sc["law"], with_screen, reflection, par["sm"], sc["environment"], sc["rotation"], target, sc["weight"],
                                 sc["ior_int"], sc["ior_ext"])
    print(f"seed {seed}: texel gradient differs by {_rel_top(gp['g_env'], par['g_env']):.2e} of its largest entry {np.abs(par['g_env']).max():.3e}, rotation partials by "
          f"{_rel_top(gp['g_R'], par['g_R']):.2e} of {np.abs(par['g_R']).max():.3e}")
    assert loss_close(gp["loss"], par["loss"]) and np.abs(par["g_env"]).max() > 0 and np.abs(par["g_R"]).max() > 0
    assert close(gp["g_env"], par["g_env"]) and close(gp["g_R"], par["g_R"]) and not gp["g_env"][par["g_env"] == 0].any()


@pytest.mark.parametrize("seed", fz.VIEWS_CASES)
def test_host_views_listed_out_of_order_with_a_repeat(libs, seed):
    """Three cameras at three distances with three screens in one table, listed [2, 0, 2]: the sum of the restatement's per-view results."""
    import test_image_loss_host as host
    sc, cap, refs = fz.case(seed), fz.capture(seed), fz.capture_references(seed)
    assert len({one["distance"] for one in cap["scenes"]}) == 3 and len({tuple(one["screen"].packed()) for one in cap["scenes"]}) == 3
    for one, ref in zip(cap["scenes"], refs):
        again = fz.loss_of_scene(nudged(one, seed))
        cond = dict(loss=abs(again["loss"] - ref["loss"]) / (LOSS_REL * ref["loss"]), grad_V=_of_tolerance(again["grad_V"], ref["grad_V"]),
                    g_int=_of_tolerance(again["g_int"], ref["g_int"]), g_ext=_of_tolerance(again["g_ext"], ref["g_ext"]))
        fwd = ref["fwd"]
        sel = (fwd["on"] & (fwd["cls"] == image_ref.THROUGH)).numpy()
        margin = _margin(fwd["u"].detach().numpy()[sel], fwd["v"].detach().numpy()[sel], *sc["texture3"].shape[:2])
        print(f"{one['name']}: distance {one['distance']} span {one['span']} moved {one['moved']} count {ref['count']} loss {ref['loss']:.6e} margin {margin:.2e}; "
              "conditioning " + ", ".join(f"{k} {v:.1e}" for k, v in cond.items()))
        assert again["count"] == ref["count"] and np.array_equal(again["fwd"]["cls"].numpy(), fwd["cls"].numpy()) and max(cond.values()) < CONDITION_SHARE
        assert margin >= TEXEL_MARGIN and ref["loss"] > one["height"] * one["width"] * one["texture3"].shape[2] * 2.0 ** -46
    want = fz.summed(refs)
    assert want["count"] > 0
    hv = [host.HostView(None, view, view["law"], view["fresnel"]) for view in cap["scenes"]]
    ids = fz.VIEW_IDS
    cams = np.ascontiguousarray(np.stack([host._cam21(one["camera_M"]) for one in cap["scenes"]]))
    screens = np.ascontiguousarray(np.stack([one["screen"].packed() for one in cap["scenes"]]))
    cls = np.ascontiguousarray(np.concatenate([hv[i].cls for i in ids]))
    hits = np.ascontiguousarray(np.concatenate([hv[i].hits for i in ids]))
    tape = np.ascontiguousarray(np.concatenate([hv[i].tape for i in ids], axis=1))
    first = hv[0]
    grad, g_ior, count = np.zeros_like(first.V), np.zeros(2), np.zeros(1, np.int64)
    loss = libs["views"].iv_views_loss(host._p(cams), host._p(screens), 3, host._p(np.ascontiguousarray(ids, np.int32)), len(ids), sc["height"], sc["width"], sc["s"],
                                       host._p(first.tex), first.tex.shape[0], first.tex.shape[1], first.tex.shape[2], host._p(first.F), host._p(first.V), sc["ior_int"], sc["ior_ext"],
                                       int(sc["law"][2] == "snell"), int(sc["fresnel"]), host._p(cls), host._p(tape), host._p(hits), host._p(first.void), host._p(first.invalid),
                                       host._p(np.ascontiguousarray(cap["targets"])), host._p(np.ascontiguousarray(cap["weights"])), host._p(grad), host._p(g_ior),
                                       host._p(count))
    got = dict(loss=loss, grad_V=grad, g_int=g_ior[0], g_ext=g_ior[1], count=int(count[0]))
    _check_loss_and_grads(got, want, f"seed {seed} views {ids}")
    assert not close(grad, refs[2]["grad_V"])                     # (one view alone is outside the tolerance)
    # the same capture in front of the case's environment, reflection on
    import image_env_ref
    room = fz.capture_env(seed)
    for one, ref, target in zip(cap["scenes"], room["refs"], room["targets"]):
        fwd = ref["fwd"]
        worst = np.inf
        for bg, pick in ((fwd["bg"], (fwd["cls"] == image_ref.THROUGH) & ~fwd["bg"]["on"]), (fwd["rb"], ~fwd["rb"]["on"])):
            u, v = bg["u"].detach().numpy()[pick.numpy()], bg["v"].detach().numpy()[pick.numpy()]
            if len(u):
                worst = min(worst, np.abs(u - np.rint(u)).min(), np.abs(v - np.rint(v)).min())
        again = image_env_ref.loss_and_grads(*fz.env_args(nudged(one, seed), True), target, one["s"], one["law"], one["invalid"], one["ior_int"], one["ior_ext"],
                                             weight=one["weight"], reflect=True)
        cond = dict(loss=abs(again["loss"] - ref["loss"]) / (LOSS_REL * ref["loss"]), grad_V=_of_tolerance(again["grad_V"], ref["grad_V"]),
                    g_int=_of_tolerance(again["g_int"], ref["g_int"]), g_ext=_of_tolerance(again["g_ext"], ref["g_ext"]))
        print(f"{one['name']} in the room: count {ref['count']} loss {ref['loss']:.6e} margin {worst:.2e}; conditioning " + ", ".join(f"{k} {v:.1e}" for k, v in cond.items()))
        assert worst >= image_env_cases.TEXEL_MARGIN and again["count"] == ref["count"] and max(cond.values()) < CONDITION_SHARE
        assert ref["loss"] > one["height"] * one["width"] * one["texture3"].shape[2] * 2.0 ** -46
    fwd = [room["refs"][i]["fwd"] for i in ids]
    cls = np.ascontiguousarray(np.concatenate([f["cls"].numpy() for f in fwd]), dtype=np.int32)
    hits = np.ascontiguousarray(np.concatenate([f["hits"].numpy() for f in fwd]), dtype=np.uint8)
    seen = np.ascontiguousarray(np.concatenate([f["seen"].numpy() for f in fwd]), dtype=np.uint8)
    tape = np.ascontiguousarray(np.concatenate([f["tape"].numpy() for f in fwd], axis=1), dtype=np.int32)
    env = np.ascontiguousarray(sc["environment"], np.float32)
    grad, g_ior, count = np.zeros_like(first.V), np.zeros(2), np.zeros(1, np.int64)
    loss = libs["views_env"].ive_views_loss(host._p(cams), host._p(screens), 3, host._p(np.ascontiguousarray(ids, np.int32)), len(ids), sc["height"], sc["width"], sc["s"],
                                            host._p(first.tex), first.tex.shape[0], first.tex.shape[1], first.tex.shape[2], host._p(env), env.shape[0], env.shape[1],
                                            host._p(np.ascontiguousarray(sc["rotation"])), host._p(first.F), host._p(first.V), len(first.F), sc["ior_int"], sc["ior_ext"],
                                            int(sc["law"][2] == "snell"), 1, host._p(cls), host._p(tape), host._p(hits), host._p(seen), host._p(first.invalid),
                                            host._p(np.ascontiguousarray(room["targets"])), host._p(np.ascontiguousarray(cap["weights"])), host._p(grad), host._p(g_ior),
                                            host._p(count))
    _check_loss_and_grads(dict(loss=loss, grad_V=grad, g_int=g_ior[0], g_ext=g_ior[1], count=int(count[0])), fz.summed(room["refs"]), f"seed {seed} views {ids} in the room")


# ---- negative controls -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 64])
def test_a_restatement_without_the_throughput_gradient_is_outside_the_tolerance(seed):
    assert fz.case(seed)["fresnel"] and seed in fz.CASES
    ref, bad = fz.loss_reference(seed), fz.loss_reference(seed, throughput_gradient=False)
    assert bad["loss"] == ref["loss"]
    assert not close(bad["grad_V"], ref["grad_V"]) and not close(bad["g_int"], ref["g_int"]) and not close(bad["g_ext"], ref["g_ext"])


@pytest.mark.parametrize("seed", [0, 1])
def test_a_restatement_with_the_direct_samples_detached_is_outside_the_tolerance(seed):
    assert seed in fz.SCREEN_CASES and figures(seed)["direct"] > 0
    ref, bad = fz.screen_reference(seed), fz.screen_reference(seed, detach_direct=True)
    assert bad["loss"] == ref["loss"]
    assert not close(bad["g_screen"], ref["g_screen"]) and not close(bad["g_texture"], ref["g_texture"])


@pytest.mark.parametrize("seed", [28, 64])
def test_a_restatement_without_the_length_gradient_is_outside_the_tolerance(seed):
    assert seed in fz.ABSORB_CASES
    ref, bad = fz.absorb_reference(seed), fz.absorb_reference(seed, length_gradient=False)
    assert bad["loss"] == ref["loss"]
    assert not close(bad["grad_V"], ref["grad_V"])


def _swapped(a):
    """The same texels read with height and width exchanged (the memory is kept, as a kernel with the two extents swapped would read it)."""
    a = np.ascontiguousarray(a)
    return a.reshape((a.shape[1], a.shape[0]) + a.shape[2:])


@pytest.mark.parametrize("seed", [seed for seed in fz.CASES if fz.base(seed)["texture3"].shape[0] != fz.base(seed)["texture3"].shape[1]])
def test_a_texture_with_height_and_width_swapped_is_outside_the_image_tolerance(seed):
    sc, st = fz.case(seed), fz.stage(seed)
    bad = image_ref.render(sc["mesh"].faces, sc["mesh"].vertices, sc["camera_M"], sc["height"], sc["width"], sc["screen"], _swapped(sc["texture3"]), sc["s"], *sc["law"],
                           sc["fresnel"], sc["void"], sc["invalid"], sc["ior_int"], sc["ior_ext"])
    keep = ~image_cases.sensitive(sc, st)
    diff = (bad["image"].double() - st["image"].double()).abs().amax(2).numpy()
    print(f"seed {seed}: swapped extents move the image by {diff[keep].max():.3e}; tolerance {image_cases.tolerance(sc, st):.3e}")
    assert diff[keep].max() > image_cases.tolerance(sc, st)


@pytest.mark.parametrize("seed,with_screen,reflection", fz.ENV_CASES, ids=ENV_IDS)
def test_an_environment_with_height_and_width_swapped_is_outside_the_image_tolerance(seed, with_screen, reflection):
    import image_env_ref
    sc, img = fz.case(seed), fz.env_image_reference(seed, with_screen, reflection)
    assert sc["environment"].shape[0] != sc["environment"].shape[1]
    refl = None
    if reflection:
        o, d = image_ref.sample_rays(sc["camera_M"][3], sc["camera_M"][2], sc["height"], sc["width"], sc["s"])
        refl = image_env_ref.reflection(sc["mesh"].faces, sc["mesh"].vertices, o, d, sc["ior_int"], sc["ior_ext"])
    bad = image_env_ref.render_from(fz.stage(seed, True), sc["height"], sc["width"], sc["s"], sc["screen"] if with_screen else None,
                                    sc["texture3"] if with_screen else None, _swapped(sc["environment"]), sc["rotation"], sc["invalid"], refl)
    keep = ~image_env_cases.sensitive(sc, sc["law"], with_screen, reflection, ref=img, stage=fz.stage(seed, True))
    tol = image_env_cases.tolerance(sc, sc["law"], with_screen, stage=fz.stage(seed, True))
    diff = (bad["image"].double() - img["image"].double()).abs().amax(2).numpy()
    print(f"seed {seed}: swapped extents move the image by {diff[keep].max():.3e}; tolerance {tol:.3e}")
    assert diff[keep].max() > tol
