"""Batched tabular SARSA(lambda) / Watkins's Q(lambda) on the device (gu_lambda_run, csrc/gu_lambda.hip) against the CPU
restatement tests/_lambda_oracle.py: Q tables, trajectory rows, statistics and trace windows compared byte for byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import sarsa_lambda, watkins_q_lambda
from griduniverse_amd.engine import Engine
from oracle import c_oracle as C

from . import _lambda_oracle as LO
from . import _td_oracle as O
from ._lambda_oracle import signed_zero_table
from ._tabular_cases import (GRIDS, _eps, _pair, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, open_grid,
                             same_env_state)

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, LO.LambdaOracle)

METHODS = {'q_learning': LO.WATKINS, 'sarsa': LO.SARSA}


def _launch(vec, o, T, method, K, lam=0.9, alpha=0.25, gamma=0.9, eps=0.2):
    got = vec.lambda_run(T, lam, K, method, alpha=alpha, discount_factor=gamma, epsilon=eps, trajectory=True, stats=True)
    _same(got, o.lam(T, METHODS[method], K, lam, alpha, gamma, _eps(eps)))
    assert vec.q_table().tobytes() == o.q.tobytes()
    assert vec.lambda_window().tobytes() == o.window().tobytes()


@pytest.mark.parametrize('K', [1, 2, 8, 9, 32, 33, 64])  # every capacity the launch picks (1, 8, 32, 64), both sides of each boundary
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('N', [63, 4096])
def test_tables_rows_stats_and_windows_equal_the_oracle(grid, method, K, N):
    g = GRIDS[grid]()
    T = 151 if N < 4096 else 37  # not multiples of K: the window crosses the launch boundary mid-episode
    vec, o = _pair(g, N, 3, 0.5 if N == 63 else 0.0)
    try:
        for _ in range(2):
            _launch(vec, o, T, method, K)
        if K > 1:
            assert (o.win >= 0).any()  # (the boundary did cut windows)
        same_env_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('K,lam,signed_zeros', [(1, 0.7, False), (64, 0.0, False), (64, 0.0, True)])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('grid', ['test_env', 'maze11'])
def test_K_1_or_lambda_0_equals_td_run_on_the_device(grid, method, K, lam, signed_zeros):
    """signed_zeros: a table of -0.0 and 2.0 learned with alpha = -0.0, where only the P_j != 0 rule keeps lambda = 0 exact (a
    kernel that added g * 0.0 for the older ages would turn -0.0 entries of its window into +0.0)."""
    g = GRIDS[grid]()
    a = gua.VecGridUniverse(300, template=_spec(g), seed=5)
    b = gua.VecGridUniverse(300, template=_spec(g), seed=5)
    try:
        a._ensure_q(0.125)
        b._ensure_q(0.125)
        alpha = 0.3
        if signed_zeros:
            alpha = -0.0
            a.set_q_table(signed_zero_table(300, a.spec.S))
            b.set_q_table(signed_zero_table(300, b.spec.S))
        assert np.array_equal(a.reset(), b.reset())
        for T in (211, 97):  # the second launch starts from the first one's carried SARSA action
            got = a.lambda_run(T, lam, K, method, alpha=alpha, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
            want = b.td_run(T, method, alpha=alpha, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
            _same(got, want)
            assert a.q_table().tobytes() == b.q_table().tobytes()
        if signed_zeros:
            q = a.q_table()
            assert ((q == 0.0) & np.signbit(q)).any()
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('fn,method', [(sarsa_lambda, LO.SARSA), (watkins_q_lambda, LO.WATKINS)])
def test_the_algorithms_equal_the_restatement_across_chunks(fn, method):
    """sarsa_lambda / watkins_q_lambda end to end: 7000 steps at trace_len 64 are two launches (chunks of 6250), which carry the
    window, so the result is the restatement's one run."""
    env = gua.GridUniverseEnv((4, 4))
    q = fn(env, 7000, lam=0.8, trace_len=64, alpha=0.2, discount_factor=0.9, epsilon=0.2, num_learners=4, seed=3, q0=0.5)
    o = LO.LambdaOracle(C.Grid.from_env(env), 3, 4, q0=0.5)
    o.reset()
    o.lam(7000, method, 64, 0.8, 0.2, 0.9, _eps(0.2))
    assert q.tobytes() == o.q.tobytes()
    env.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('K', [5, 64])
def test_one_launch_equals_split_launches(method, K):
    g = GRIDS['open8x8']()
    a = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    b = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    try:
        a.reset()
        b.reset()
        whole = a.lambda_run(500, 0.9, K, method, epsilon=0.3, trajectory=True, stats=True)
        p1 = b.lambda_run(213, 0.9, K, method, epsilon=0.3, trajectory=True, stats=True)
        p2 = b.lambda_run(287, 0.9, K, method, epsilon=0.3, trajectory=True, stats=True)
        for k in ('obs', 'reward', 'done'):
            assert np.concatenate([p1[k], p2[k]]).tobytes() == whole[k].tobytes(), k
        assert a.q_table().tobytes() == b.q_table().tobytes()
        assert a.lambda_window().tobytes() == b.lambda_window().tobytes()
    finally:
        a.close()
        b.close()


def _follow(vec, o):
    """After a learner call the restatement does not model: take the device's tables and env state, and drop what the call drops."""
    o.q[:] = vec.q_table()
    st = vec.get_state()
    o.state.pos[:], o.state.done[:], o.state.episode[:], o.state.tcount[:] = st['pos'], st['done'], st['episode'], st['tcount']
    o.other_call()


def _drop_by(kind, vec, o):
    if kind == 'reset':
        assert np.array_equal(vec.reset(), o.reset())
    elif kind == 'rollout':
        _same(vec.rollout(20, 'uniform', auto_reset=True, stats=True), o.rollout(20, auto_reset=True, stats=True))
    elif kind == 'set_state':
        tc = vec.get_state()['tcount'] + np.uint64(5)
        vec.set_state(tcount=tc)
        o.set_state(tcount=tc)
    elif kind == 'td_run':
        _same(vec.td_run(15, 'sarsa', epsilon=0.3, trajectory=True), o.run(15, O.SARSA, 0.1, 0.99, _eps(0.3)), ('obs', 'reward', 'done'))
    elif kind == 'set_q':
        vec.set_q_table(o.q[:3] * 0.5, env0=2)
        o.set_q(o.q[:3] * 0.5, env0=2)
    elif kind == 'nstep_run':
        vec.nstep_run(15, 4, 'sarsa', epsilon=0.3)
        _follow(vec, o)
    elif kind == 'dyna_run':
        vec.dyna_run(15, 2, epsilon=0.3)
        _follow(vec, o)
    elif kind == 'ac_run':
        vec.actor_critic_run(15)
        _follow(vec, o)


@pytest.mark.parametrize('kind', ['reset', 'rollout', 'set_state', 'td_run', 'set_q', 'nstep_run', 'dyna_run', 'ac_run', 'other_K',
                                  'other_method'])
def test_the_window_is_dropped_by_any_other_call(kind):
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 4)
    try:
        _launch(vec, o, 45, 'sarsa', 16, eps=0.3)
        assert (o.win >= 0).any()
        method, K = 'sarsa', 16
        if kind == 'other_K':
            K = 12
        elif kind == 'other_method':
            method = 'q_learning'
        else:
            _drop_by(kind, vec, o)
            assert (vec.lambda_window() == -1).all()
        _launch(vec, o, 45, method, K, eps=0.3)
    finally:
        vec.close()


def test_lambda_run_drops_the_nstep_window_and_the_sarsa_carry():
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 8)
    try:
        vec.nstep_run(45, 8, 'sarsa', epsilon=0.3)
        assert vec.nstep_window()['count'].any()
        _follow(vec, o)
        _launch(vec, o, 30, 'sarsa', 8, eps=0.3)
        assert (vec.nstep_window()['count'] == 0).all()
        # a SARSA td_run, then a lambda run, then a SARSA td_run: the last one draws a fresh action
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        assert o.carry_valid
        _launch(vec, o, 30, 'sarsa', 8, eps=0.3)
        assert not o.carry_valid
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('eps', [0.0, 0.5])
@pytest.mark.parametrize('K', [8, 64])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('W,H', [(2, 2), (4, 4)])
def test_forwarding_on_small_open_grids(W, H, method, K, eps):
    """On tiny grids window pairs often lie in the row of s' that the lane holds in registers (the wall bump included)."""
    vec, o = _pair(open_grid(W, H), 256, 7, 0.5)
    try:
        for T in (123, 77):
            _launch(vec, o, T, method, K, lam=1.0, alpha=0.4, gamma=0.8, eps=eps)
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
@pytest.mark.parametrize('K', [8, 64])
def test_multigrid_learners_equal_the_oracle(method, n_grids, N, K):
    vec, side = multigrid_batch(LO.LambdaOracle, n_grids, N)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        for T in (150, 91):
            got = vec.lambda_run(T, 0.9, K, method, alpha=0.2, discount_factor=0.9, epsilon=0.25, trajectory=True, stats=True)
            _same(got, side.run(lambda o: o.lam(T, METHODS[method], K, 0.9, 0.2, 0.9, _eps(0.25))))
        assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
        assert vec.lambda_window().tobytes() == side.cat(lambda o: o.window()).tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(LO.LambdaOracle, n_grids)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        got = vec.lambda_run(200, 0.9, 32, 'sarsa', alpha=0.3, discount_factor=0.9, epsilon=0.1, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.lam(200, LO.SARSA, 32, 0.9, 0.3, 0.9, _eps(0.1))))
        assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
        assert vec.lambda_window().tobytes() == side.cat(lambda o: o.window()).tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
def test_step_counts_across_the_epoch_boundary(method):
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N)
        for T in (130, 170):
            _launch(vec, o, T, method, 12, alpha=0.2, eps=0.5)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


def test_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1)
    try:
        eng = vec.engine
        for kw, text in ((dict(K=0), 'K 0'), (dict(K=65), 'K 65'), (dict(method=2), 'method 2'), (dict(method=-1), 'method -1'),
                         (dict(lam=-0.1), 'lambda'), (dict(lam=1.5), 'lambda'), (dict(lam=float('nan')), 'lambda'),
                         (dict(eps_q16=65537), 'eps_q16'), (dict(alpha=float('nan')), 'alpha'), (dict(gamma=float('inf')), 'gamma'),
                         (dict(T=-1), 'T -1')):
            args = dict(T=10, method=0, K=4, alpha=0.1, gamma=0.9, lam=0.9, eps_q16=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_lambda_run(eng._h, args['T'], args['method'], args['K'], args['alpha'], args['gamma'], args['lam'],
                                                 args['eps_q16'], 0))
            assert err.value.code == -1, kw
            assert text in str(err.value), (kw, str(err.value))
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_lambda_run(eng._h, 10, 0, 4, 0.1, 0.9, 0.9, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1 and 'gu_lambda_run accepts GU_F_TRAJECTORY and GU_F_STATS only' in str(err.value)
        with pytest.raises(gua.GuError) as err:
            eng.lambda_get_window(60, 5)
        assert err.value.code == -1
        vec.lambda_run(0, 0.9, 4)  # T = 0 changes nothing
        assert vec.q_table().tobytes() == o.q.tobytes() and (vec.lambda_window() == -1).all()
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        with pytest.raises(gua.GuError) as err:
            eng.lambda_run(10)
        assert err.value.code == -4 and 'gu_td_init' in str(err.value)
        assert (eng.lambda_get_window() == -1).all()
