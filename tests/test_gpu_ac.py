"""Batched tabular softmax actor-critic on the device (gu_ac_run, csrc/gu_ac.hip) against the CPU restatement tests/_ac_oracle.py:
preferences, values, trajectory rows and statistics compared byte for byte; plus one check of the critic that does not depend on
the restatement."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms import utils
from griduniverse_amd.algorithms.policy_gradient import actor_critic
from griduniverse_amd.engine import Engine

from . import _ac_oracle as AO
from . import _td_oracle as O
from ._tabular_cases import (GRIDS, _eps, _grid, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, open_grid,
                             same_env_state)

pytestmark = pytest.mark.gpu


def _pair(g, N, seed, h0=0.0, v0=0.0):
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    vec._ensure_ac(h0, v0)
    o = AO.AcOracle(_grid(g), seed, N, h0=h0, v0=v0)
    assert np.array_equal(vec.reset(), o.reset())
    return vec, o


def _same_tables(vec, o):
    assert vec.preferences().tobytes() == o.h.tobytes()
    assert vec.state_values().tobytes() == o.v.tobytes()


def _launch(vec, o, T, aa=0.2, ac=0.3, gamma=0.9):
    got = vec.actor_critic_run(T, actor_lr=aa, critic_lr=ac, discount_factor=gamma, trajectory=True, stats=True)
    _same(got, o.ac(T, aa, ac, gamma))
    _same_tables(vec, o)


@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('N', [63, 4096])
def test_tables_rows_and_stats_equal_the_oracle(grid, N):
    g = GRIDS[grid]()
    T = 151 if N < 4096 else 37
    vec, o = _pair(g, N, 3, 0.5 if N == 63 else 0.0, -0.25 if N == 63 else 0.0)
    try:
        for _ in range(2):
            _launch(vec, o, T)
        same_env_state(vec, o)
        assert o.h.any() and o.v.any()
    finally:
        vec.close()


def test_one_launch_equals_two():
    g = GRIDS['open8x8']()
    a = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    b = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    try:
        a.reset()
        b.reset()
        whole = a.actor_critic_run(500, 0.3, 0.2, 0.95, trajectory=True, stats=True)
        p1 = b.actor_critic_run(250, 0.3, 0.2, 0.95, trajectory=True, stats=True)
        p2 = b.actor_critic_run(250, 0.3, 0.2, 0.95, trajectory=True, stats=True)
        for k in ('obs', 'reward', 'done'):
            assert np.concatenate([p1[k], p2[k]]).tobytes() == whole[k].tobytes(), k
        assert a.preferences().tobytes() == b.preferences().tobytes()
        assert a.state_values().tobytes() == b.state_values().tobytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('W,H', [(2, 2), (4, 4)])
def test_wall_bump_forwarding_on_small_open_grids(W, H):
    """On tiny grids many moves bump into the edge (s' == s): the next step must see the updated row and value."""
    vec, o = _pair(open_grid(W, H), 256, 7, 0.5, 1.0)
    try:
        for T in (123, 77):
            _launch(vec, o, T, aa=0.4, ac=0.5, gamma=0.8)
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(n_grids, N):
    vec, side = multigrid_batch(AO.AcOracle, n_grids, N)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        for T in (150, 91):
            got = vec.actor_critic_run(T, 0.2, 0.25, 0.9, trajectory=True, stats=True)
            _same(got, side.run(lambda o: o.ac(T, 0.2, 0.25, 0.9)))
        assert vec.preferences().tobytes() == side.cat(lambda o: o.h).tobytes()
        assert vec.state_values().tobytes() == side.cat(lambda o: o.v).tobytes()
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(AO.AcOracle, n_grids)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        got = vec.actor_critic_run(200, 0.3, 0.3, 0.9, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.ac(200, 0.3, 0.3, 0.9)))
        assert vec.preferences().tobytes() == side.cat(lambda o: o.h).tobytes()
        assert vec.state_values().tobytes() == side.cat(lambda o: o.v).tobytes()
    finally:
        vec.close()


def test_step_counts_across_the_epoch_boundary():
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N)
        for T in (130, 170):
            _launch(vec, o, T)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


def test_installed_tables_then_run():
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 4)
    try:
        _launch(vec, o, 40)
        rng = np.random.default_rng(2)
        h, v = rng.normal(0, 2, (5, g['W'] * g['H'], 4)), rng.normal(0, 3, (5, g['W'] * g['H']))
        vec.set_actor_critic(h, v, env0=7)
        o.set_ac(h, v, env0=7)
        vec.set_actor_critic(v=v[:2] * 0.5, env0=100)
        o.set_ac(v=v[:2] * 0.5, env0=100)
        _same_tables(vec, o)
        for T in (60, 45):
            _launch(vec, o, T)
        assert np.array_equal(vec.softmax_policy(7, 5), AO.softmax(o.h[7:12].reshape(-1, 4))[2].reshape(5, -1, 4))
    finally:
        vec.close()


def test_actor_critic_run_between_two_sarsa_runs_drops_the_carry():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(200, template=_spec(g), seed=9)
    o = AO.AcOracle(_grid(g), 9, 200)
    try:
        vec._ensure_q(0.0)
        vec._ensure_ac()
        assert np.array_equal(vec.reset(), o.reset())
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        assert o.carry_valid
        _launch(vec, o, 30)
        assert not o.carry_valid
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        _same_tables(vec, o)
    finally:
        vec.close()


def test_errors():
    g = GRIDS['test_env']()
    with Engine(8, _spec(g)) as eng:
        for call in (lambda: eng.ac_run(10), lambda: eng.ac_get(), lambda: eng.ac_set(v=np.zeros(eng.spec.S))):
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -4  # GU_ERR_STATE before gu_ac_init
    vec, o = _pair(g, 64, 1)
    try:
        eng = vec.engine
        S = eng.spec.S
        for kw in (dict(T=-1), dict(T=100000001), dict(aa=float('nan')), dict(ac=float('inf')), dict(gamma=float('nan')),
                   dict(flags=_lib.F_AUTO_RESET), dict(flags=_lib.F_PACKED)):
            args = dict(T=10, aa=0.1, ac=0.1, gamma=0.9, flags=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_ac_run(eng._h, args['T'], args['aa'], args['ac'], args['gamma'], args['flags']))
            assert err.value.code == -1, kw
        for h0, v0 in ((float('nan'), 0.0), (0.0, float('inf'))):
            with pytest.raises(gua.GuError) as err:
                eng.ac_init(h0, v0)
            assert err.value.code == -1
        bad_h = np.zeros((2, S, 4))
        bad_h[1, 3, 2] = np.nan
        bad_v = np.zeros((2, S))
        bad_v[0, 1] = -np.inf
        for kw in (dict(h=bad_h), dict(v=bad_v)):
            with pytest.raises(gua.GuError) as err:
                eng.ac_set(env0=0, **kw)
            assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.ac_get(60, 5)
        assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.ac_set(v=np.zeros((5, S)), env0=62)
        assert err.value.code == -1
        vec.actor_critic_run(0)  # T = 0 changes nothing
        _same_tables(vec, o)
        _launch(vec, o, 20)  # (the rejected calls changed nothing either)
    finally:
        vec.close()


def test_softmax_policy_drives_a_sampled_rollout():
    env = gua.GridUniverseEnv(grid_shape=(5, 5), lava_states=[12])
    pi, v = actor_critic(env, 3000, num_learners=1, seed=1)
    S = env.world.size
    assert pi.shape == (S, 4) and v.shape == (S,)
    terminal = np.array([bool(env.is_terminal(s)) for s in range(S)])
    assert (pi[terminal] == 0).all() and np.allclose(pi[~terminal].sum(axis=1), 1.0)
    utils.get_policy_map(pi, (5, 5), mode='ansi')
    vec = gua.VecGridUniverse(128, template=env, seed=3, auto_reset=True)
    try:
        vec.engine.vi_set(v, pi)
        vec.reset()
        out = vec.rollout(200, policy='sample', stats=True)
        assert out['obs'].shape == (200, 128) and out['episodes'].sum() > 0
    finally:
        vec.close()
    many, vs = actor_critic(env, 500, num_learners=3, seed=1)
    assert many.shape == (3, S, 4) and vs.shape == (3, S)


def test_critic_of_a_frozen_uniform_actor_approaches_the_policy_value():
    """actor_lr = 0 and zero preferences: every learner acts uniformly at random, so V approaches the value of the uniform policy.
    That value comes from utils.single_step_policy_evaluation iterated to convergence, with the terminal row of the policy zero.
    The reference's sweep counts the reward of the state itself, v(s) = R(s) + gamma * sum_a pi(a) v(s'), where the learners'
    target is the reward of the state entered, so on non-terminal states the learners' value is (v(s) - R(s)) / gamma.
    The mean of V over 4096 learners (critic_lr 0.1, gamma 0.9, 10 000 steps, seed 5) is compared with it.  Tolerance 0.5 on
    the non-terminal states: the restatement gives a largest gap of 0.445 (states 11 and 14, next to the goal: constant-step
    TD(0) correlates V(s) with the recent visits to s), against 8.58 for the tables of zeros."""
    gamma = 0.9
    env = gua.GridUniverseEnv((4, 4))
    S = env.world.size
    terminal = np.array([bool(env.is_terminal(s)) for s in range(S)])
    pi = np.full((S, 4), 0.25)
    pi[terminal] = 0.0  # (the episode ends there)
    v = np.zeros(S)
    for _ in range(3000):
        v = utils.single_step_policy_evaluation(pi, env, gamma, v)
    want = (v - np.asarray(env.reward_matrix, np.float64)) / gamma
    vec = gua.VecGridUniverse(4096, template=env, seed=5)
    try:
        vec.reset()
        vec.actor_critic_run(10000, actor_lr=0.0, critic_lr=0.1, discount_factor=gamma)
        mean = vec.state_values().mean(axis=0)
        assert not vec.preferences().any()
    finally:
        vec.close()
    gap = np.abs(mean - want)[~terminal].max()
    assert gap < 0.5, (gap, mean, want)
    assert np.abs(want[~terminal]).max() > 8.0
