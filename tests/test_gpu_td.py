"""Batched tabular Q-learning / SARSA on the device (gu_td_run, csrc/gu_td.hip) against the CPU restatement tests/_td_oracle.py:
Q tables, trajectory rows and statistics compared byte for byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import greedy_policy, q_learning
from griduniverse_amd.engine import Engine
from griduniverse_amd.grid import GridSpec
from oracle import c_oracle as C

from . import _td_oracle as O
from . import _golden as G
from ._tabular_cases import GRIDS, _eps, _grid, _pair, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, same_env_state

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, O.TdOracle)

METHODS = {'q_learning': O.Q_LEARNING, 'sarsa': O.SARSA}


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('N', [1, 63, 4096])
def test_tables_rows_and_stats_equal_the_oracle(grid, method, N):
    g = GRIDS[grid]()
    T = 300 if N < 4096 else 60
    q0 = 0.0 if N != 63 else 0.5
    vec, o = _pair(g, N, 3, q0)
    try:
        for _ in range(2):  # two launches: the second starts from the first one's state (and, for SARSA, its carried action)
            got = vec.td_run(T, method, alpha=0.25, discount_factor=0.9, epsilon=0.2, trajectory=True, stats=True)
            want = o.run(T, METHODS[method], 0.25, 0.9, _eps(0.2))
            _same(got, want)
            assert vec.q_table().tobytes() == o.q.tobytes()
        same_env_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
def test_split_launches_with_changed_hyper_parameters(method):
    g = GRIDS['test_env']()
    vec, o = _pair(g, 130, 8)
    try:
        for alpha, eps in ((0.5, 0.3), (0.1, 0.05), (0.3, 1.0)):
            got = vec.td_run(257, method, alpha=alpha, discount_factor=0.95, epsilon=eps, trajectory=True, stats=True)
            _same(got, o.run(257, METHODS[method], alpha, 0.95, _eps(eps)))
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


def test_sarsa_interrupted_by_reset_starts_with_a_fresh_action():
    g = GRIDS['open8x8']()
    vec, o = _pair(g, 200, 4)
    try:
        vec.td_run(50, 'sarsa', epsilon=0.3)
        o.run(50, O.SARSA, 0.1, 0.99, _eps(0.3))
        assert np.array_equal(vec.reset(), o.reset())  # drops the carried action
        got = vec.td_run(70, 'sarsa', epsilon=0.3, trajectory=True)
        _same(got, o.run(70, O.SARSA, 0.1, 0.99, _eps(0.3)), ('obs', 'reward', 'done'))
        vec.set_q_table(o.q[:5] * 0.5, env0=3)  # ... and so does installing tables
        o.set_q(o.q[:5] * 0.5, env0=3)
        got = vec.td_run(70, 'sarsa', epsilon=0.3, trajectory=True)
        _same(got, o.run(70, O.SARSA, 0.1, 0.99, _eps(0.3)), ('obs', 'reward', 'done'))
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(method, n_grids, N):
    vec, side = multigrid_batch(O.TdOracle, n_grids, N)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        for T in (150, 90):
            got = vec.td_run(T, method, alpha=0.2, discount_factor=0.9, epsilon=0.25, trajectory=True, stats=True)
            _same(got, side.run(lambda o: o.run(T, METHODS[method], 0.2, 0.9, _eps(0.25))))
        assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(O.TdOracle, n_grids)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        got = vec.td_run(200, 'q_learning', alpha=0.3, discount_factor=0.9, epsilon=0.1, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.run(200, O.Q_LEARNING, 0.3, 0.9, _eps(0.1))))
        assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
def test_step_counts_across_the_epoch_boundary(method):
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N)
        got = vec.td_run(300, method, alpha=0.2, discount_factor=0.9, epsilon=0.5, trajectory=True, stats=True)
        _same(got, o.run(300, METHODS[method], 0.2, 0.9, _eps(0.5)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


def test_edges_epsilon_alpha_and_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1, q0=1.25)
    try:
        for eps in (0.0, 1.0):
            got = vec.td_run(120, 'q_learning', alpha=0.3, discount_factor=0.9, epsilon=eps, trajectory=True, stats=True)
            _same(got, o.run(120, O.Q_LEARNING, 0.3, 0.9, _eps(eps)))
            assert vec.q_table().tobytes() == o.q.tobytes()
        vec.engine.td_init(1.25)
        vec.td_run(200, 'sarsa', alpha=0.0, epsilon=0.4)
        assert vec.q_table().tobytes() == np.full((64, _grid(g).S, 4), 1.25).tobytes()  # alpha = 0: q0 bit for bit
        eng = vec.engine
        for kw, code in ((dict(method=2), -1), (dict(eps_q16=65537), -1), (dict(alpha=float('nan')), -1), (dict(gamma=float('inf')), -1),
                         (dict(T=-1), -1)):
            args = dict(T=10, method=0, alpha=0.1, gamma=0.9, eps_q16=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_td_run(eng._h, args['T'], args['method'], args['alpha'], args['gamma'], args['eps_q16'], 0))
            assert err.value.code == code, kw
        with pytest.raises(gua.GuError) as err:  # a flag other than GU_F_TRAJECTORY / GU_F_STATS
            _lib.check(eng.lib.gu_td_run(eng._h, 10, 0, 0.1, 0.9, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.td_get_q(60, 5)
        assert err.value.code == -1
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        with pytest.raises(gua.GuError) as err:
            eng.td_run(10)
        assert err.value.code == -4
        with pytest.raises(gua.GuError) as err:
            eng.td_get_q()
        assert err.value.code == -4


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
def test_step_counts_advance_and_a_rollout_continues_from_the_learners_state(method):
    g = GRIDS['maze11']()
    vec, o = _pair(g, 500, 21)
    try:
        t_before = vec.get_state()['tcount'].copy()
        vec.td_run(333, method, epsilon=0.2)
        o.run(333, METHODS[method], 0.1, 0.99, _eps(0.2))
        st = vec.get_state()
        assert np.array_equal(st['tcount'], t_before + np.uint64(333)) and np.array_equal(st['pos'], o.state.pos)
        got = vec.rollout(100, 'uniform', auto_reset=True, stats=True)
        _same(got, o.rollout(100, auto_reset=True, stats=True))
    finally:
        vec.close()


def test_learning_end_to_end_finds_the_shortest_path():
    env = gua.GridUniverseEnv(custom_world_fp=G.level_path('maze_11x11.txt'))
    q = q_learning(env, 20000, alpha=0.2, discount_factor=0.99, epsilon=0.1, num_learners=4096, seed=1)
    assert q.shape == (4096, env.world.size, 4)
    pi = greedy_policy(q[0], env)
    with Engine(1, GridSpec.from_env(env)) as eng:
        paths, _ = eng.shortest_paths()
    grid = C.Grid.from_env(env)
    s, n = int(env.starting_states[0]), 0
    while not (grid.goal[s] or grid.lava[s]) and n <= grid.S:
        nxt, _, _ = C.look_step_ahead(grid, np.array([s], np.int32), np.array([int(np.argmax(pi[s]))], np.int32), True)
        s, n = int(nxt[0]), n + 1
    assert grid.goal[s] and n == len(paths[0])
