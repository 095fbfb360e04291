"""Batched tabular n-step Q-learning / SARSA on the device (gu_nstep_run, csrc/gu_nstep.hip) against the CPU restatement
tests/_nstep_oracle.py: Q tables, trajectory rows, statistics and windows compared byte for byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.engine import Engine

from . import _nstep_oracle as NO
from . import _td_oracle as O
from ._tabular_cases import (GRIDS, _eps, _pair, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, open_grid,
                             same_env_state)

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, NO.NstepOracle)

METHODS = {'q_learning': O.Q_LEARNING, 'sarsa': O.SARSA}


def _same_window(vec, o):
    w, want = vec.nstep_window(), o.window()
    for k in ('count', 'sa', 'reward'):
        assert w[k].tobytes() == want[k].tobytes(), k


def _launch(vec, o, T, method, n, alpha=0.25, gamma=0.9, eps=0.2):
    got = vec.nstep_run(T, n, method, alpha=alpha, discount_factor=gamma, epsilon=eps, trajectory=True, stats=True)
    _same(got, o.nstep(T, METHODS[method], n, alpha, gamma, _eps(eps)))
    assert vec.q_table().tobytes() == o.q.tobytes()
    _same_window(vec, o)


@pytest.mark.parametrize('n', [1, 2, 4, 16])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('N', [63, 4096])
def test_tables_rows_stats_and_windows_equal_the_oracle(grid, method, n, N):
    g = GRIDS[grid]()
    T = 151 if N < 4096 else 37  # not multiples of n: the window crosses the launch boundary mid-episode
    vec, o = _pair(g, N, 3, 0.5 if N == 63 else 0.0)
    try:
        for _ in range(2):
            _launch(vec, o, T, method, n)
        if n > 1:
            assert o.count.any()  # (the boundary did cut windows)
        same_env_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('grid', ['test_env', 'maze11'])
def test_n_1_equals_td_run_on_the_device(grid, method):
    g = GRIDS[grid]()
    a = gua.VecGridUniverse(300, template=_spec(g), seed=5)
    b = gua.VecGridUniverse(300, template=_spec(g), seed=5)
    try:
        a._ensure_q(0.125)
        b._ensure_q(0.125)
        assert np.array_equal(a.reset(), b.reset())
        for T in (211, 97):  # the second launch starts from the first one's carried SARSA action
            got = a.nstep_run(T, 1, method, alpha=0.3, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
            want = b.td_run(T, method, alpha=0.3, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
            _same(got, want)
            assert a.q_table().tobytes() == b.q_table().tobytes()
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('n', [3, 16])
def test_one_launch_equals_split_launches(method, n):
    g = GRIDS['open8x8']()
    a = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    b = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    try:
        a.reset()
        b.reset()
        whole = a.nstep_run(500, n, method, epsilon=0.3, trajectory=True, stats=True)
        p1 = b.nstep_run(213, n, method, epsilon=0.3, trajectory=True, stats=True)
        p2 = b.nstep_run(287, n, method, epsilon=0.3, trajectory=True, stats=True)
        for k in ('obs', 'reward', 'done'):
            assert np.concatenate([p1[k], p2[k]]).tobytes() == whole[k].tobytes(), k
        assert a.q_table().tobytes() == b.q_table().tobytes()
        wa, wb = a.nstep_window(), b.nstep_window()
        for k in wa:
            assert wa[k].tobytes() == wb[k].tobytes(), k
    finally:
        a.close()
        b.close()


def _drop_by(kind, vec, o, g):
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


@pytest.mark.parametrize('kind', ['reset', 'rollout', 'set_state', 'td_run', 'set_q', 'other_n', 'other_method'])
def test_the_window_is_dropped_by_any_other_call(kind):
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 4)
    try:
        _launch(vec, o, 45, 'sarsa', 8, eps=0.3)
        assert o.count.any()
        method, n = 'sarsa', 8
        if kind == 'other_n':
            n = 5
        elif kind == 'other_method':
            method = 'q_learning'
        else:
            _drop_by(kind, vec, o, g)
            assert (vec.nstep_window()['count'] == 0).all()
        _launch(vec, o, 45, method, n, eps=0.3)
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('eps', [0.0, 0.5])
@pytest.mark.parametrize('n', [4, 16])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('W,H', [(2, 2), (4, 4)])
def test_forwarding_on_small_open_grids(W, H, method, n, eps):
    """On tiny grids the updated pair often lies in the row of s' that the lane holds in registers."""
    g = open_grid(W, H)
    vec, o = _pair(g, 256, 7, 0.5)
    try:
        for T in (123, 77):
            _launch(vec, o, T, method, n, alpha=0.4, gamma=0.8, eps=eps)
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(method, n_grids, N):
    vec, side = multigrid_batch(NO.NstepOracle, n_grids, N)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        for T in (150, 91):
            got = vec.nstep_run(T, 6, method, alpha=0.2, discount_factor=0.9, epsilon=0.25, trajectory=True, stats=True)
            _same(got, side.run(lambda o: o.nstep(T, METHODS[method], 6, 0.2, 0.9, _eps(0.25))))
        assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
        w = vec.nstep_window()
        for k in ('count', 'sa', 'reward'):
            assert w[k].tobytes() == side.cat(lambda o: o.window()[k]).tobytes(), k
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(NO.NstepOracle, n_grids)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        got = vec.nstep_run(200, 8, 'sarsa', alpha=0.3, discount_factor=0.9, epsilon=0.1, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.nstep(200, O.SARSA, 8, 0.3, 0.9, _eps(0.1))))
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
        for T in (130, 170):
            _launch(vec, o, T, method, 5, alpha=0.2, eps=0.5)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


def test_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1)
    try:
        eng = vec.engine
        for kw in (dict(n=0), dict(n=17), dict(method=2), dict(method=-1), dict(eps_q16=65537), dict(alpha=float('nan')), dict(T=-1)):
            args = dict(T=10, method=0, n=4, alpha=0.1, gamma=0.9, eps_q16=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_nstep_run(eng._h, args['T'], args['method'], args['n'], args['alpha'], args['gamma'],
                                                args['eps_q16'], 0))
            assert err.value.code == -1, kw
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_nstep_run(eng._h, 10, 0, 4, 0.1, 0.9, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.nstep_get_window(60, 5)
        assert err.value.code == -1
        vec.nstep_run(0, 4)  # T = 0 changes nothing
        assert vec.q_table().tobytes() == o.q.tobytes() and (vec.nstep_window()['count'] == 0).all()
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        with pytest.raises(gua.GuError) as err:
            eng.nstep_run(10)
        assert err.value.code == -4
        assert (eng.nstep_get_window()['count'] == 0).all()
