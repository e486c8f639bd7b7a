"""CPU: the ``path_law=(K, tir)`` keyword of the loops (drt_amd.optim.path_law_keyword) is checked before anything touches the scene or the
capture -- every call here passes ``scene = data = None``."""
import pytest

from drt_amd import diffrender as Render, optim as O


@pytest.fixture(autouse=True)
def _globals():
    saved = (Render.intIOR, Render.resx, Render.resy)
    yield
    Render.intIOR, Render.resx, Render.resy = saved


def _loops(hp, law):
    return [lambda: O.FusedIteration(None, None, hp, 0.1, path_law=law),
            lambda: O.ShardedIteration(None, None, hp, 0.1, path_law=law),
            lambda: O.optimize(None, None, hp, remesh=None, fused=True, path_law=law),
            lambda: O.optimize_sharded(None, None, hp, remesh=None, path_law=law),
            lambda: O.Loss_calculator(None, None, hp, fused=True, path_law=law),
            lambda: O.optimize(None, None, hp, remesh=None, fused=False, path_law=law)]


@pytest.mark.parametrize("law", [(9, "reflect"), (1, "drop"), (4, "mirror"), (2.5, "drop"), (True, "drop"), 6, (6,)])
def test_bad_laws_raise_value_error(law):
    for call in _loops(dict(O.HyperParams), law):
        with pytest.raises(ValueError):
            call()


def test_a_law_together_with_a_learnable_ior_is_refused():
    hp = dict(O.HyperParams, ior_lr=1e-4)
    for call in _loops(hp, (4, "reflect")):
        with pytest.raises(NotImplementedError):
            call()
    # a bad law is still a bad law
    with pytest.raises(ValueError):
        O.FusedIteration(None, None, hp, 0.1, path_law=(9, "reflect"))


def test_two_drop_is_no_law():
    hp = dict(O.HyperParams)
    assert O.path_law_keyword(None, hp, "x") is None and O.path_law_keyword((2, "drop"), hp, "x") is None
    assert O.path_law_keyword((2, "drop"), dict(hp, ior_lr=1e-4), "x") is None          # today's kernels: nothing to refuse
    assert O.path_law_keyword((6.0, "reflect"), hp, "x") == (6, "reflect") and O.path_law_keyword([2, "reflect"], hp, "x") == (2, "reflect")
    # accepted: the constructors get past the checks and only then trip over the missing scene / capture
    for law in (None, (2, "drop")):
        for call in _loops(hp, law):
            with pytest.raises(AttributeError):
                call()


def test_the_hyperparams_refusals_fire_first_and_are_unchanged():
    hp = dict(O.HyperParams, max_bounces=6, tir="reflect")
    for call in _loops(hp, (9, "reflect"))[:4]:
        with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
            call()
    with pytest.raises(ValueError, match="twice"):            # the drop-in loop takes either spelling of the law, not both
        O.optimize(None, None, hp, remesh=None, fused=False, path_law=(4, "reflect"))
