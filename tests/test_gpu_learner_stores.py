"""The stores of the batched learners as the host sees them, whichever module holds them: a read of envs env0 .. env0+n-1 is that
slice of the read of all envs, for every getter; and a grid of another size drops every store sized by the grid -- and nothing else --
while a grid of the same size keeps them all."""
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms.exploration import ucb_tables
from griduniverse_amd.algorithms.function_approximation import tile_coding
from griduniverse_amd.algorithms.search import uct_tables
from griduniverse_amd.engine import Engine

from ._tabular_cases import GRIDS, _spec

pytestmark = pytest.mark.gpu


def _parts(x):
    """A getter's result as a list of (key, array)."""
    if isinstance(x, dict):
        return sorted(x.items())
    return list(enumerate(x)) if isinstance(x, tuple) else [(None, x)]


def _slices_of_the_full_read(getter, N):
    full = _parts(getter(0, N))
    for env0, n in ((0, N), (5, 9), (60, 9), (N - 1, 1), (N, 0), (3, 0)):
        got = _parts(getter(env0, n))
        assert [k for k, _ in got] == [k for k, _ in full]
        for (k, f), (_, g) in zip(full, got):
            want = f[env0:env0 + n]
            assert g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes(), (getter.__name__, k, env0, n)
    return dict((k, f) for k, f in full)


def test_a_read_of_some_envs_is_that_slice_of_the_read_of_all():
    N = 70
    with Engine(N, _spec(GRIDS['default4x4']()), seed=11) as eng:
        eng.td_init(0.0)
        eng.td_run(40)
        assert _slices_of_the_full_read(eng.td_get_q, N)[None].any()
        eng.explore_init()
        eng.set_exploration(*ucb_tables(1.0, 16))
        eng.explore_run(20)
        assert _slices_of_the_full_read(eng.explore_get_counts, N)[None].any()
        eng.dyna_init()
        eng.dyna_run(20, 3)
        assert _slices_of_the_full_read(eng.dyna_get_model, N)['count'].all()
        eng.search_run(10, 2, 3)
        assert _slices_of_the_full_read(eng.search_get, N)['sim_steps'].any()
        eng.mcts_init(8)
        eng.set_tree_tables(*uct_tables(3.0, 16))
        eng.mcts_run(10, 4, 3, 2)
        assert _slices_of_the_full_read(eng.mcts_get, N)['nodes'].any()
        assert _slices_of_the_full_read(eng.mcts_tree, N)['count'].any()
        # the windows and buffers are read right behind their own launch: any other launch drops them
        eng.nstep_run(13, n=4)
        assert _slices_of_the_full_read(eng.nstep_get_window, N)['count'].any()
        eng.lambda_run(13, K=8)
        assert (_slices_of_the_full_read(eng.lambda_get_window, N)[None] >= 0).any()
        eng.is_init()
        eng.is_run(20, L=7)
        assert _slices_of_the_full_read(eng.is_get_episode, N)['count'].any()
        _slices_of_the_full_read(eng.is_get, N)
        eng.ac_init()
        eng.ac_run(20)
        assert _slices_of_the_full_read(eng.ac_get, N)[0].any()
        eng.reinforce_run(20, L=16)
        assert _slices_of_the_full_read(eng.reinforce_get_episode, N)['count'].any()
        eng.fa_init(*tile_coding(4, 4, 2, 2))
        eng.fa_run(20)
        assert _slices_of_the_full_read(eng.fa_get_w, N)[None].any()
        assert _slices_of_the_full_read(eng.fa_get_q, N)[None].any()


def _everything_once(eng):
    eng.td_init(0.0)
    eng.td_run(10)
    eng.explore_init()
    eng.set_exploration(*ucb_tables(1.0, 16))
    eng.explore_run(10)
    eng.dyna_init()
    eng.dyna_run(10, 2)
    eng.search_run(5, 2, 3)
    eng.mcts_init(8)
    eng.set_tree_tables(*uct_tables(3.0, 16))
    eng.mcts_run(5, 4, 3, 2)
    eng.nstep_run(9, n=4)
    eng.lambda_run(9, K=8)
    eng.is_init()
    eng.is_run(10, L=7)
    eng.ac_init()
    eng.ac_run(10)
    eng.reinforce_run(10, L=16)
    eng.fa_init(*tile_coding(4, 4, 2, 2))
    eng.fa_run(10)


def _fails_for_want_of_a_store(call):
    with pytest.raises(gua.GuError) as err:
        call()
    assert err.value.code == -4


def _drop_and_keep(N, seed):
    with Engine(N, _spec(GRIDS['default4x4']()), seed=seed) as eng:
        _everything_once(eng)
        eng.set_grid(_spec(GRIDS['open8x8']()))
        for run in (lambda: eng.td_run(5), lambda: eng.dyna_run(5, 2), lambda: eng.search_run(5, 2, 3), lambda: eng.explore_run(5),
                    lambda: eng.mcts_run(5, 4, 3, 2), lambda: eng.nstep_run(5, n=4), lambda: eng.lambda_run(5, K=8), lambda: eng.ac_run(5),
                    lambda: eng.reinforce_run(5, L=16), lambda: eng.is_run(5, L=7), lambda: eng.fa_run(5)):
            _fails_for_want_of_a_store(run)
        for get in (eng.td_get_q, eng.explore_get_counts, eng.is_get, eng.ac_get, eng.search_get, eng.mcts_get, eng.mcts_tree, eng.dyna_get_model,
                    eng.fa_get_q):
            _fails_for_want_of_a_store(get)
        with pytest.raises(RuntimeError) as err:  # (the engine sizes the weights' array by what the library holds, and it holds none)
            eng.fa_get_w()
        assert str(err.value) == 'no features: call fa_init first'
        for get in (eng.nstep_get_window, eng.reinforce_get_episode, eng.is_get_episode):
            got = get()
            assert not got['count'].any() and (got['sa'] == -1).all() and got['sa'].shape[0] == N
        assert (eng.lambda_get_window() == -1).all()
        # the schedule tables are no store of a grid: counts and pools come back without them being set again
        eng.td_init(0.0)
        eng.explore_init()
        eng.mcts_init(8)
        eng.explore_run(10)
        eng.mcts_run(5, 4, 3, 2)
        assert eng.mcts_get()['sim_steps'].any()
        assert eng.td_get_q().shape == (N, 64, 4)
        # another grid of as many states keeps every store
        q, counts = eng.td_get_q(), eng.explore_get_counts()
        assert q.any() and counts.any()
        other = dict(GRIDS['open8x8'](), walls=[27, 28, 35])
        eng.set_grid(_spec(other))
        assert eng.td_get_q().tobytes() == q.tobytes() and eng.explore_get_counts().tobytes() == counts.tobytes()
        eng.explore_run(10)
        eng.mcts_run(5, 4, 3, 2)
        assert eng.explore_get_counts().sum() > counts.sum()


def test_a_grid_of_another_size_drops_every_store_and_only_those():
    for life in range(3):  # (one engine after another: the destroy path frees every store each time)
        _drop_and_keep(8, 5 + life)
