"""CPU: ``drt_amd.calibrate.fit_ior`` -- the bisection on the sign of d loss / d IOR against a stub scene whose loss is a torch
function of the IOR it is handed (so the whole of fit_ior runs: the per-view calls, the summed loss, autograd's derivative), its
argument rules, the C-ABI symbol of the call behind it, and the refusals that stay: every call that refused a learnable IOR under a
K-interaction law before ``Scene.paths_ray_loss_ior_fused`` existed still does."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from drt_amd import _lib, calibrate, diffrender as Render, optim as O

ROOT_IOR = 1.4723


class _StubScene:
    """loss(ior) with d loss / d ior = slope(ior): the call returns slope(value) * ior, the derivative of which is slope(value)."""

    def __init__(self, slope):
        self.slope, self.calls, self.last_path_count = slope, [], 0

    def paths_ray_loss_ior_fused(self, origin, ray_dir, screen_pixel, valid, ior_int, ior_ext=None, max_bounces=4, tir="reflect",
                                 refraction="reference", vertices=True):
        assert isinstance(ior_int, torch.Tensor) and ior_int.requires_grad and ior_int.dim() == 0 and ior_int.dtype == torch.float64
        assert vertices is False
        self.calls.append((origin, float(ior_int.detach()), ior_ext, max_bounces, tir, refraction))
        self.last_path_count = 100 + origin
        return self.slope(float(ior_int.detach()), origin) * ior_int


class _StubData:
    def __init__(self, ids):
        self.ids = ids

    def ray_view_ids(self):
        return self.ids

    def get_view(self, v):
        return ("sp", "valid", None, v, "dir", None)          # (the stub scene gets the view id as its `origin`)


def _noisy_slope(x, view):
    """Negative below the root, positive above it -- except inside +-2e-4 of it, where the sign flips with x as it does on a mesh when
    paths switch face; its size varies by view and by orders of magnitude."""
    s = (x - ROOT_IOR) * (1.0 + view) * (1.0 + 50.0 * abs(np.sin(997.0 * x)))
    if abs(x - ROOT_IOR) < 2e-4 and int(x * 1e6) % 2:
        s = -s
    return s


def test_bisection_finds_the_root_of_a_noisy_signed_derivative():
    scene, data = _StubScene(_noisy_slope), _StubData([5, 23, 41, 59])
    fit = calibrate.fit_ior(scene, data, (6, "reflect", "snell"), bracket=(1.3, 1.7), halvings=14)
    lo, hi = fit["bracket"]
    assert fit["evaluations"] == 16 == len(fit["history"]) and len(scene.calls) == 16 * 4
    assert hi - lo == pytest.approx(0.4 / 2 ** 14, rel=1e-12) and fit["ior"] == pytest.approx(0.5 * (lo + hi), rel=1e-15)
    assert abs(fit["ior"] - ROOT_IOR) <= 2e-4 + 0.2 / 2 ** 14          # the noisy zone, plus the final half-width
    # every evaluation: its IOR, the loss and derivative summed over the four views, the contributing rays summed
    xs = [1.3, 1.7]
    for x, loss, g, rays in fit["history"]:
        want = sum(_noisy_slope(x, v) for v in data.ids)
        assert g == pytest.approx(want, rel=1e-12) and loss == pytest.approx(want * x, rel=1e-12) and rays == 400 + sum(data.ids)
    assert [h[0] for h in fit["history"][:2]] == xs
    # each step halves towards the side the sign points to
    lo, hi = 1.3, 1.7
    for x, _, g, _ in fit["history"][2:]:
        assert x == 0.5 * (lo + hi)
        lo, hi = (x, hi) if g < 0 else (lo, x)
    assert (lo, hi) == fit["bracket"]
    # the law and the exterior IOR reach the scene as given; vertices=False (asserted by the stub)
    assert all(c[2:] == (None, 6, "reflect", "snell") for c in scene.calls)
    # a clean derivative is resolved to the final half-width
    fit = calibrate.fit_ior(_StubScene(lambda x, v: x - ROOT_IOR), data, (2, "drop", "snell"), (1.2, 1.6), 14, view_ids=[5], ior_ext=1.0)
    assert abs(fit["ior"] - ROOT_IOR) <= 0.2 / 2 ** 14 and fit["evaluations"] == 16


def test_a_bracket_without_a_sign_change_is_an_error_that_names_it():
    data = _StubData([0])
    with pytest.raises(RuntimeError, match=r"\(1\.5, 1\.7\).*0\.0277.*0\.2277"):
        calibrate.fit_ior(_StubScene(lambda x, v: x - ROOT_IOR), data, bracket=(1.5, 1.7))
    with pytest.raises(RuntimeError, match=r"\(1\.2, 1\.4\)"):
        calibrate.fit_ior(_StubScene(lambda x, v: x - ROOT_IOR), data, bracket=(1.2, 1.4))
    with pytest.raises(RuntimeError, match="minimum"):                      # a maximum inside the bracket is no fit either
        calibrate.fit_ior(_StubScene(lambda x, v: ROOT_IOR - x), data, bracket=(1.3, 1.7))


def test_keyword_rules_and_bad_values():
    data = _StubData([0])

    def law_seen(path_law):
        scene = _StubScene(lambda x, v: x - ROOT_IOR)
        calibrate.fit_ior(scene, data, path_law, (1.3, 1.7), 0)
        return scene.calls[0][3:]

    assert law_seen((2, "drop", "snell")) == (2, "drop", "snell")
    assert law_seen((2, "drop")) == (2, "drop", "reference") == law_seen((2, "drop", "reference")) == law_seen(None)      # today's formula is a law here
    assert law_seen((6.0, "reflect")) == (6, "reflect", "reference") and law_seen([8, "reflect", "snell"]) == (8, "reflect", "snell")
    scene = _StubScene(lambda x, v: x - ROOT_IOR)
    assert calibrate.fit_ior(scene, data)["evaluations"] == 16 and scene.calls[0][3:] == (2, "drop", "snell")                  # the defaults
    for bad in ((1, "drop"), (9, "reflect"), (4, "mirror"), (4, "reflect", "bent"), (4,), 4, (4, "reflect", "snell", "again"), (True, "drop")):
        with pytest.raises(ValueError):
            calibrate.fit_ior(scene, data, bad)
    for bad in ((1.5, 1.5), (1.7, 1.3), (0.0, 1.5), (1.3,)):
        with pytest.raises(ValueError):
            calibrate.fit_ior(scene, data, bracket=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="halvings"):
            calibrate.fit_ior(scene, data, halvings=bad)
    with pytest.raises(ValueError, match="no views"):
        calibrate.fit_ior(scene, _StubData([]))


def test_scene_call_checks_its_law_before_it_touches_anything():
    """The law checks and messages of paths_ray_loss_ior_fused are those of the other K-interaction calls (no scene needed to get there)."""
    call = Render.Scene.paths_ray_loss_ior_fused
    for k in (1, 9, 2.5, True):
        with pytest.raises(ValueError, match="max_bounces must be an integer in 2..8"):
            call(None, None, None, None, None, 1.5, None, k, "drop")
    with pytest.raises(ValueError, match="tir must be 'drop' or 'reflect'"):
        call(None, None, None, None, None, 1.5, None, 4, "mirror")
    with pytest.raises(ValueError, match="refraction must be 'reference' or 'snell'"):
        call(None, None, None, None, None, 1.5, None, 4, "reflect", "bent")
    o = torch.zeros((4, 3), dtype=torch.float64, requires_grad=True)
    d = torch.zeros((4, 3), dtype=torch.float64)
    for rays in ((o, d), (d, o)):
        with pytest.raises(NotImplementedError, match="origin and ray_dir must not require grad"):
            call(None, *rays, None, None, 1.5, None, 4, "reflect")
    with pytest.raises(ValueError, match="ior_int must be a float or a 0-dim tensor"):
        call(None, d, d, None, None, torch.ones(2, dtype=torch.float64), None, 4, "reflect")


# ------------------------------------------------------------------------------------------------------------- the refusals that stay
@pytest.fixture
def _globals():
    saved = (Render.intIOR, Render.extIOR, Render.resx, Render.resy)
    yield
    Render.intIOR, Render.extIOR, Render.resx, Render.resy = saved


def test_every_existing_refusal_of_a_learnable_ior_still_raises(_globals):
    hp = dict(O.HyperParams, ior_lr=1e-4)
    for law in ((4, "reflect"), (4, "reflect", "snell"), (2, "drop", "snell")):
        with pytest.raises(NotImplementedError, match="path_law cannot be combined with HyperParams\\['ior_lr'\\] > 0 in x: the K-interaction law "
                                                      "differentiates the vertices only"):
            O.path_law_keyword(law, hp, "x")
        for call in (lambda: O.FusedIteration(None, None, hp, 0.1, path_law=law), lambda: O.ShardedIteration(None, None, hp, 0.1, path_law=law),
                     lambda: O.optimize(None, None, hp, remesh=None, fused=True, path_law=law),
                     lambda: O.optimize_sharded(None, None, hp, remesh=None, path_law=law)):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(NotImplementedError, match="ior_lr"):
        O.optimize(None, None, dict(hp, refraction="snell"), remesh=None, fused=False)
    # Scene.render_paths / paths_ray_loss_fused: rays or module IORs that require grad
    o = torch.zeros((4, 3), dtype=torch.float64)
    og = o.clone().requires_grad_(True)
    for who in ("render_paths", "paths_ray_loss_fused"):
        msg = f"{who} differentiates the vertices only: origin, ray_dir and the IORs must not require grad"
        for rays in ((og, o), (o, og)):
            with pytest.raises(NotImplementedError, match=msg):
                Render.Scene._check_paths_call(who, *rays, 4, "reflect", "snell")
        for name in ("intIOR", "extIOR"):
            old = getattr(Render, name)
            setattr(Render, name, torch.tensor(1.5, dtype=torch.float64, requires_grad=True))
            try:
                with pytest.raises(NotImplementedError, match=msg):
                    Render.Scene._check_paths_call(who, o, o, 4, "reflect", "snell")
            finally:
                setattr(Render, name, old)


def test_the_c_abi_symbol_is_declared_bound_and_exported():
    name = "drt_render_paths_law_ray_loss_ior_fused"
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert re.search(r"\bint " + name + r"\s*\(", header)
    ret, args = _lib.SIGNATURES[name]
    assert len(args) == len(_lib.SIGNATURES["drt_render_paths_law_ray_loss_fused"][1]) + 1          # ... plus d_grad_ior
    exports = open(os.path.join(ROOT, "drt_amd", "csrc", "exports.map")).read()
    assert "drt_*" in exports
    assert hasattr(_lib.lib(), name) and _lib.lib().drt_version() >= 6
