"""The host side of the multi-rank loop (drt_amd.optim.optimize_sharded), without a GPU: which rank owns which view, that every rank draws
the same schedule whatever views it holds, and the weights of a step over several refraction views."""
import numpy as np
import pytest

from drt_amd import captured_data, dist as ddist, optim as O


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n_total,num_view,name", [(72, 72, "hand"), (144, 72, "monkey"), (72, 8, "hand"), (72, 72, "mouse"), (8, 8, "hand")])
def test_ownership_partitions_every_view_exactly_once(world, n_total, num_view, name):
    for ids in (captured_data.ray_view_ids(n_total, num_view, name), captured_data.silh_view_ids(n_total)):
        owned = [ddist.owned_views(ids, r, world) for r in range(world)]
        flat = sorted(v for o in owned for v in o)
        assert flat == sorted(ids) and len(set(flat)) == len(flat)
        for r, o in enumerate(owned):
            assert all(ddist.owner(v, ids, world) == r for v in o)
        sizes = [len(o) for o in owned]
        assert max(sizes) - min(sizes) <= 1                   # position modulo world: as even as the list allows
    with pytest.raises(KeyError):
        ddist.owner(n_total + 1, captured_data.ray_view_ids(n_total, num_view, name), world)


def test_a_full_turntable_is_shard_views_and_every_other_view_still_spreads_over_eight_ranks():
    ids = captured_data.ray_view_ids(72, 72)
    for r in range(8):
        assert ddist.owned_views(ids, r, 8) == ddist.shard_views(72, r, 8)
    # config 5: --views 144 with num_view 72 -- only even ids are ray views; raw v % 8 would leave ranks 1, 3, 5, 7 without one
    ids = captured_data.ray_view_ids(144, 72)
    assert ids == list(range(0, 144, 2))
    assert [len(ddist.owned_views(ids, r, 8)) for r in range(8)] == [9] * 8
    assert [len(ddist.owned_views(captured_data.silh_view_ids(144), r, 8)) for r in range(8)] == [18] * 8


def test_mouse_subset_is_sorted_view_ids():
    ids = captured_data.ray_view_ids(72, 72, "mouse")
    assert ids == sorted(list(range(0, 10)) + list(range(67, 72)) + list(range(22, 40)))


class _Views(captured_data.Data):
    """A capture that holds only the views it is given (the schedule does not look at them)."""

    def __init__(self, view_ids, seed, n_total=144, num_view=72):
        self.n_total, self.num_view, self.name = n_total, num_view, "monkey"
        self.rng = np.random.RandomState(seed)
        self.Views = {v: None for v in view_ids}


def _schedule(data, iters, k):
    ray, silh = data.ray_view_generator(), data.silh_view_generator()
    out = []
    for _ in range(iters):                     # the draw order of ShardedIteration.draw: k refraction views, then the 8 silhouette views
        out.append(([next(ray) for _ in range(k)], [next(silh) for _ in range(8)]))
    return out


@pytest.mark.parametrize("k", [1, 4, 72])
def test_same_seed_same_schedule_whatever_views_a_rank_holds(k):
    world = 3
    ray_ids = captured_data.ray_view_ids(144, 72, "monkey")
    held = [sorted(set(ddist.owned_views(ray_ids, r, world)) | set(ddist.owned_views(list(range(144)), r, world))) for r in range(world)]
    datas = [_Views(h, seed=5) for h in held]
    assert datas[0].ray_view_ids() == datas[1].ray_view_ids() == ray_ids
    assert datas[0].silh_view_ids() == list(range(144))
    scheds = [_schedule(d, 40, k) for d in datas]
    assert scheds[0] == scheds[1] == scheds[2]
    # every drawn view is evaluated by exactly one rank, and that rank holds it
    for ray, silh in scheds[0]:
        for v in ray:
            r = ddist.owner(v, ray_ids, world)
            assert v in datas[r].Views
        for v in silh:
            assert v in datas[ddist.owner(v, list(range(144)), world)].Views
    # a different seed is a different schedule
    assert _schedule(_Views(held[0], seed=6), 40, k) != scheds[0]


def test_one_view_per_step_gives_exactly_the_reference_weights():
    hp = O.HyperParams
    for resy, mean_len in ((64, 3.3), (1024, 0.71), (960, 1.0)):
        w = O.loss_weights(hp, resy, mean_len)
        assert O.sharded_loss_weights(hp, resy, mean_len, 1) == w
        for k in (2, 4, 72):
            wk = O.sharded_loss_weights(hp, resy, mean_len, k)
            assert wk[0] == w[0] / k and wk[1:] == w[1:]
