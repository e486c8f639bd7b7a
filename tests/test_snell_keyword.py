"""CPU: the refraction formula as the third element of the path law -- ``optim.path_law`` (``HyperParams["refraction"]``) and the
``path_law=(K, tir, refraction)`` keyword of the loops (``optim.path_law_keyword``) -- is normalised and checked before anything touches
the scene or the capture: every call here passes ``scene = data = None``."""
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


def test_the_reference_refraction_changes_no_result():
    hp = dict(O.HyperParams)
    assert O.path_law_keyword((6, "reflect", "reference"), hp, "x") == (6, "reflect")
    assert O.path_law_keyword((2, "drop", "reference"), hp, "x") is None
    assert O.path_law_keyword((6, "reflect"), hp, "x") == (6, "reflect") and O.path_law_keyword((2, "drop"), hp, "x") is None
    assert O.path_law_keyword(None, hp, "x") is None
    for refraction in ("reference", None):
        assert O.path_law(dict(hp, refraction=refraction)) is None
        assert O.path_law(dict(hp, max_bounces=6, tir="reflect", refraction=refraction)) == (6, "reflect")
    assert O.path_law(dict(hp, max_bounces=6, tir="reflect")) == (6, "reflect") and O.path_law(hp) is None


def test_snell_makes_a_three_tuple_and_two_drop_a_law():
    hp = dict(O.HyperParams)
    assert O.path_law_keyword((6.0, "reflect", "snell"), hp, "x") == (6, "reflect", "snell")
    assert O.path_law_keyword([2, "drop", "snell"], hp, "x") == (2, "drop", "snell")
    assert O.path_law(dict(hp, refraction="snell")) == (2, "drop", "snell")
    assert O.path_law(dict(hp, max_bounces=8, tir="reflect", refraction="snell")) == (8, "reflect", "snell")
    assert O.law_flags((8, "reflect", "snell")) == 3 and O.law_flags((2, "drop", "snell")) == 2 and O.law_flags((8, "reflect")) == 1
    # accepted: the constructors get past the checks and only then trip over the missing scene / capture
    for law in ((2, "drop", "snell"), (6, "reflect", "snell"), (6, "reflect", "reference")):
        for call in _loops(hp, law):
            with pytest.raises(AttributeError):
                call()


@pytest.mark.parametrize("law", [(4, "reflect", "bent"), (4, "reflect", "snell", "again"), (4, "reflect", 1)])
def test_bad_refractions_raise_value_error_from_every_loop(law):
    for call in _loops(dict(O.HyperParams), law):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        O.path_law_keyword(law, dict(O.HyperParams), "x")


@pytest.mark.parametrize("refraction", ["bent", 1, ("snell",)])
def test_bad_hyperparams_refraction_raises_value_error(refraction):
    with pytest.raises(ValueError, match="refraction"):
        O.path_law(dict(O.HyperParams, refraction=refraction))
    with pytest.raises(ValueError, match="refraction"):
        O.optimize(None, None, dict(O.HyperParams, refraction=refraction), remesh=None, fused=False)


def test_snell_together_with_a_learnable_ior_is_refused():
    hp = dict(O.HyperParams, ior_lr=1e-4)
    for law in ((4, "reflect", "snell"), (2, "drop", "snell")):
        for call in _loops(hp, law):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(NotImplementedError, match="ior_lr"):
        O.optimize(None, None, dict(hp, refraction="snell"), remesh=None, fused=False)


def test_the_hyperparams_spelling_of_snell_is_refused_by_the_one_pass_loops_with_the_existing_message():
    hp = dict(O.HyperParams, refraction="snell")
    for call in _loops(hp, None)[:4]:
        with pytest.raises(NotImplementedError, match="optimize\\(\\.\\.\\., fused=False\\)"):
            call()
    with pytest.raises(ValueError, match="twice"):
        O.optimize(None, None, hp, remesh=None, fused=False, path_law=(4, "reflect", "snell"))


def test_scene_calls_name_a_bad_refraction():
    for bad in ("bent", 1, None):
        with pytest.raises(ValueError, match="refraction"):
            Render.Scene._check_paths_call("render_paths", None, None, 4, "reflect", bad)
