"""Batched simulation-based search on the device (gu_search_run, csrc/gu_search.hip) against the CPU restatement
tests/_search_oracle.py: Q tables, trajectory rows, statistics, env state, score rows and simulated-move counts compared byte for
byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.search import rollout_search
from griduniverse_amd.engine import Engine

from . import _search_oracle as SO
from . import _td_oracle as TD
from ._behaviour import SEARCH_BEHAVIOUR, search_behaviour_totals
from ._tabular_cases import GRIDS, _eps, _pair, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, same_env_state

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, SO.SearchOracle)


def _same_search(vec, oracles):
    got = vec.search_scores()
    assert got['score'].tobytes() == np.concatenate([o.score for o in oracles]).tobytes()
    assert got['sim_steps'].dtype == np.int64 and np.array_equal(got['sim_steps'], np.concatenate([o.sim_steps for o in oracles]))


def _run(vec, o, T, M, D, eps_sim, alpha=0.25, gamma=0.9, eps=0.2):
    got = vec.search_run(T, M, D, alpha=alpha, discount_factor=gamma, epsilon=eps, rollout_epsilon=eps_sim / 65536.0, trajectory=True,
                         stats=True)
    _same(got, o.search(T, M, D, alpha, gamma, _eps(eps), eps_sim))
    assert vec.q_table().tobytes() == o.q.tobytes()
    _same_search(vec, [o])


# (M, D, eps_sim_q16, T): 4 M D T near 2e4 simulated moves per learner at the most
CASES = [(1, 0, 0, 200), (2, 5, 65536, 500), (4, 16, 6554, 80), (3, 7, 0, 240)]


@pytest.mark.parametrize('M,D,eps_sim,T', CASES)
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_tables_rows_stats_state_and_scores_equal_the_oracle(grid, M, D, eps_sim, T):
    g = GRIDS[grid]()
    vec, o = _pair(g, 63, 3, q0=0.5 if M in (1, 4) else 0.0)
    try:
        for part in (T - T // 3, T // 3):  # two launches: the second starts from the first one's tables
            _run(vec, o, part, M, D, eps_sim)
        same_env_state(vec, o)
        if D > 0:
            assert o.sim_steps.sum() > 0
    finally:
        vec.close()


def test_4096_learners_equal_the_oracle():
    g = GRIDS['lava32']()
    vec, o = _pair(g, 4096, 5)
    try:
        _run(vec, o, 30, 2, 8, 13107, alpha=0.3, gamma=0.95, eps=0.3)
        _run(vec, o, 10, 2, 8, 65536, alpha=0.3, gamma=0.95, eps=0.3)
        same_env_state(vec, o)
    finally:
        vec.close()


def test_without_simulations_equals_td_q_learning():
    g = GRIDS['maze11']()
    a, _ = _pair(g, 300, 7, q0=0.1)
    b, _ = _pair(g, 300, 7, q0=0.1)
    try:
        for T, D, eps_sim in ((250, 16, 1.0), (77, 0, 0.0)):  # any depth, any rollout epsilon
            got = a.search_run(T, 0, D, alpha=0.3, discount_factor=0.95, epsilon=0.15, rollout_epsilon=eps_sim, trajectory=True, stats=True)
            want = b.td_run(T, 'q_learning', alpha=0.3, discount_factor=0.95, epsilon=0.15, trajectory=True, stats=True)
            _same(got, want)
            assert a.q_table().tobytes() == b.q_table().tobytes()
        sa, sb = a.get_state(), b.get_state()
        assert all(np.array_equal(sa[k], sb[k]) for k in ('pos', 'done', 'episode', 'tcount'))
        s = a.search_scores()
        assert not s['score'].any() and not s['sim_steps'].any()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('M,D,eps_sim', [(2, 6, 1.0), (3, 4, 0.25)])
def test_split_launch_equals_one_launch(M, D, eps_sim):
    g = GRIDS['test_env']()
    a, o = _pair(g, 130, 8)
    b, _ = _pair(g, 130, 8)
    try:
        T, kw = 120, dict(alpha=0.4, discount_factor=0.9, epsilon=0.3, rollout_epsilon=eps_sim, trajectory=True, stats=True)
        whole = a.search_run(T, M, D, **kw)
        first = b.search_run(1, M, D, **kw)
        n1 = b.search_scores()['sim_steps']
        rest = b.search_run(T - 1, M, D, **kw)
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(whole[k], np.concatenate([first[k], rest[k]])), k
        assert np.array_equal(whole['ret'], first['ret'] + rest['ret'])
        assert a.q_table().tobytes() == b.q_table().tobytes()
        sa, sb = a.search_scores(), b.search_scores()
        assert sa['score'].tobytes() == sb['score'].tobytes()
        assert np.array_equal(sa['sim_steps'], n1 + sb['sim_steps'])
        _same(whole, o.search(T, M, D, 0.4, 0.9, _eps(0.3), _eps(eps_sim)))
        assert a.q_table().tobytes() == o.q.tobytes()
        _same_search(a, [o])
    finally:
        a.close()
        b.close()


def _group_run(vec, side, launches):
    assert np.array_equal(vec.reset(), side.reset())
    for T, M, D, eps_sim in launches:
        got = vec.search_run(T, M, D, alpha=0.2, discount_factor=0.9, epsilon=0.25, rollout_epsilon=eps_sim, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.search(T, M, D, 0.2, 0.9, _eps(0.25), _eps(eps_sim))))
    assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
    _same_search(vec, side.oracles)
    same_env_state(vec, side)


@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(n_grids, N):
    vec, side = multigrid_batch(SO.SearchOracle, n_grids, N)
    try:
        _group_run(vec, side, ((16, 2, 4, 1.0), (8, 2, 4, 0.2)))
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(SO.SearchOracle, n_grids)
    try:
        _group_run(vec, side, ((20, 2, 5, 0.1),))
    finally:
        vec.close()


@pytest.mark.parametrize('M,D,t0', [(2, 4, 2 ** 32 - 30), (4, 16, (2 ** 32) // (4 * 4 * 16) - 20), (3, 5, 2 * (2 ** 32) // (4 * 3 * 5) - 10)])
def test_step_counts_across_the_epoch_boundaries(M, D, t0):
    """The stream-4 count t crosses 2^32, or the simulated-move count c = ((t * 4 + b) * M + j) * D + i does, mid-launch."""
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N, t0)
        _run(vec, o, 60, M, D, 32768, alpha=0.2, gamma=0.9, eps=0.3)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(60))
        same_env_state(vec, o)
    finally:
        vec.close()


def test_always_exploring_simulates_nothing():
    g = GRIDS['open8x8']()
    vec, o = _pair(g, 100, 4, q0=0.3)
    try:
        _run(vec, o, 50, 3, 6, 65536, eps=0.5)
        before = vec.search_scores()['score'].copy()
        assert before.any()
        _run(vec, o, 80, 3, 6, 65536, eps=1.0)
        s = vec.search_scores()
        assert not s['sim_steps'].any() and s['score'].tobytes() == before.tobytes()  # (the rows of the last SEARCHED iteration stay)
    finally:
        vec.close()


def test_search_run_ends_the_sarsa_carry():
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 9)
    try:
        kw = dict(alpha=0.3, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        _same(vec.td_run(40, 'sarsa', **kw), o.run(40, TD.SARSA, 0.3, 0.9, _eps(0.3)))
        _run(vec, o, 10, 2, 4, 65536, alpha=0.3, gamma=0.9, eps=0.3)
        assert not o.carry_valid
        _same(vec.td_run(40, 'sarsa', **kw), o.run(40, TD.SARSA, 0.3, 0.9, _eps(0.3)))  # a' drawn afresh at the first step
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


def test_edges_and_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1, q0=1.25)
    try:
        eng = vec.engine
        s = eng.search_get()  # before the first launch: zeros
        assert s['score'].shape == (64, 4) and not s['score'].any() and not s['sim_steps'].any()
        _run(vec, o, 30, 2, 3, 6554)
        before, q, sc = vec.get_state(), vec.q_table(), eng.search_get()
        eng.search_run(0, 4, 8)  # T = 0 changes nothing
        assert all(np.array_equal(before[k], vec.get_state()[k]) for k in before) and vec.q_table().tobytes() == q.tobytes()
        after = eng.search_get()
        assert all(after[k].tobytes() == sc[k].tobytes() for k in sc)
        # either output pointer may be NULL
        steps = np.empty(3, np.int64)
        _lib.check(eng.lib.gu_search_get(eng._h, 5, 3, None, _lib.ptr(steps)))
        assert np.array_equal(steps, o.sim_steps[5:8])
        row = np.empty((2, 4), np.float64)
        _lib.check(eng.lib.gu_search_get(eng._h, 62, 2, _lib.ptr(row), None))
        assert row.tobytes() == o.score[62:].tobytes()
        _run(vec, o, 1, 64, 256, 65536, eps=0.0)  # the largest M and D
        _run(vec, o, 2, 64, 256, 0, eps=1.0)
        for kw in (dict(M=-1), dict(M=65), dict(D=-1), dict(D=257), dict(eps_q16=65537), dict(eps_sim=65537), dict(T=-1),
                   dict(T=100000001, M=0), dict(T=400000, M=4, D=16), dict(alpha=float('nan')), dict(gamma=float('inf'))):
            args = dict(T=10, M=1, D=1, alpha=0.1, gamma=0.9, eps_q16=0, eps_sim=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_search_run(eng._h, args['T'], args['M'], args['D'], args['alpha'], args['gamma'], args['eps_q16'],
                                                 args['eps_sim'], 0))
            assert err.value.code == -1, kw
        eng.search_run(389000, 4, 16, eps_q16=65536)  # T * (1 + 4 M D) just below the bound; always exploring: nothing simulated
        assert not eng.search_get()['sim_steps'].any()
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_search_run(eng._h, 10, 1, 1, 0.1, 0.9, 0, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.search_get(60, 5)
        assert err.value.code == -1
        for bad in (dict(epsilon=1.5), dict(rollout_epsilon=-0.5)):
            with pytest.raises(ValueError):
                vec.search_run(10, **bad)
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        for call in (lambda: eng.search_run(10), lambda: eng.search_get()):
            with pytest.raises(gua.GuError) as err:  # no Q tables
                call()
            assert err.value.code == -4
        eng.td_init()
        eng.search_run(10, 2, 2)
        assert eng.search_get()['sim_steps'].sum() > 0
        eng.set_grid(_spec(GRIDS['default4x4']()))  # a grid of another size drops the storage with the tables
        with pytest.raises(gua.GuError) as err:
            eng.search_get()
        assert err.value.code == -4
        eng.td_init()
        assert not eng.search_get()['score'].any() and not eng.search_get()['sim_steps'].any()


def test_search_finishes_more_episodes_than_plain_q_learning_on_the_device():
    """The totals of tests/test_search_host.py, which the device equals by construction: asserted here once on open8x8."""
    b = SEARCH_BEHAVIOUR
    g = GRIDS['open8x8']()
    kw = dict(alpha=b['alpha'], discount_factor=b['gamma'], epsilon=b['eps_q16'] / 65536.0, stats=True)
    vec = gua.VecGridUniverse(b['N'], template=_spec(g), seed=b['seed'])
    try:
        vec.reset()
        plain = vec.td_run(b['T'], 'q_learning', **kw)['episodes']
    finally:
        vec.close()
    vec = gua.VecGridUniverse(b['N'], template=_spec(g), seed=b['seed'])
    try:
        vec.reset()
        got = vec.search_run(b['T'], b['M'], b['D'], rollout_epsilon=b['eps_sim_q16'] / 65536.0, **kw)['episodes']
    finally:
        vec.close()
    print('open8x8 on the device: search {} finished episodes (least per learner {}), plain Q-learning {}'.format(
        int(got.sum()), int(got.min()), int(plain.sum())))
    assert (int(got.sum()), int(plain.sum()), int(got.min())) == search_behaviour_totals('open8x8')
    assert got.sum() >= 3 * plain.sum() and got.min() >= 2


def test_rollout_search_returns_tables_of_q_learnings_shape():
    env = gua.GridUniverseEnv(grid_shape=(4, 4))
    q = rollout_search(env, 200, simulations=2, depth=4, num_learners=8, seed=1)
    assert q.shape == (8, env.world.size, 4) and q.dtype == np.float64 and np.isfinite(q).all() and q.any()
    q1 = rollout_search(env, 50, simulations=1, depth=2, seed=1)
    assert q1.shape == (env.world.size, 4)
