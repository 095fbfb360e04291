"""Batched off-policy Monte-Carlo control with weighted importance sampling on the device (gu_is_run, csrc/gu_is.hip) against the
CPU restatement tests/_is_oracle.py: Q tables, cumulative weights, trajectory rows, statistics, env state and the episode buffers
compared byte for byte; plus checks that do not depend on the restatement."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms import utils
from griduniverse_amd.algorithms.off_policy import off_policy_mc_control
from griduniverse_amd.algorithms.temporal_difference import greedy_policy
from griduniverse_amd.engine import Engine

from . import _is_oracle as IO
from . import _lambda_oracle as LO
from . import _nstep_oracle as NO
from . import _reinforce_oracle as RO
from . import _td_oracle as O
from ._behaviour import is_behaviour_totals
from ._tabular_cases import (GRIDS, _eps, _grid, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, open_grid,
                             same_env_state)

pytestmark = pytest.mark.gpu


def _pair(g, N, seed, q0=0.0):
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    vec._ensure_q(q0)
    vec._ensure_is()
    o = IO.IsOracle(_grid(g), seed, N, q0=q0)
    assert np.array_equal(vec.reset(), o.reset())
    return vec, o


def _same_tables(vec, o):
    assert vec.q_table().tobytes() == o.q.tobytes()
    assert vec.importance_weights().tobytes() == o.c.tobytes()


def _same_buffer(vec, oracles):
    buf = vec.off_policy_episode_buffer()
    assert buf['sa'].shape == (vec.engine.N, _lib.IS_MAX)
    assert buf['count'].tobytes() == np.concatenate([o.buf_cnt for o in oracles]).tobytes()
    assert buf['sa'].tobytes() == np.concatenate([o.buf_sa for o in oracles]).tobytes()
    assert buf['reward'].tobytes() == np.concatenate([o.buf_r for o in oracles]).tobytes()
    assert buf['cls'].tobytes() == np.concatenate([o.buf_c for o in oracles]).tobytes()


def _launch(vec, o, T, L, gamma=0.9, epsilon=0.2, w_cap=2.0 ** 64):
    got = vec.off_policy_mc_run(T, L, discount_factor=gamma, epsilon=epsilon, w_cap=w_cap, trajectory=True, stats=True)
    _same(got, o.is_run(T, L, gamma, _eps(epsilon), w_cap))
    _same_tables(vec, o)
    _same_buffer(vec, [o])


# The seed of each case: the first from 1 on with which, in the restatement, the first launch (150 steps) ends with some lane on a
# terminal step and, for L > 1, some lane in the middle of a segment.  (grid, N) -> seeds for L = 1, 7, 64.
_SEEDS = {
    ('default4x4', 63): (1, 1, 1),
    ('lava32', 63): (103, 103, 103),
    ('maze11', 63): (10, 31, 423), ('maze11', 4096): (8, 8, 8),
    ('open8x8', 63): (5, 5, 5), ('open8x8', 4096): (1, 1, 1),
    ('test_env', 63): (1, 1, 1),
}


@pytest.mark.parametrize('L', [1, 7, 64])
@pytest.mark.parametrize('grid,N', sorted(_SEEDS))
def test_tables_rows_stats_state_and_buffer_equal_the_oracle(grid, N, L):
    """Two launches, of 150 and 100 steps.  The first ends with some lanes on a terminal step (_SEEDS) and, for L > 1, some in
    the middle of a segment; both are asserted on the restatement."""
    g = GRIDS[grid]()
    vec, o = _pair(g, N, _SEEDS[grid, N][(1, 7, 64).index(L)], 0.25 if N == 63 else 0.0)
    try:
        for launch, T in enumerate((150, 100)):
            _launch(vec, o, T, L)
            same_env_state(vec, o)
            if launch == 0:
                assert (o.state.done != 0).any() and ((o.buf_cnt > 0).any() or L == 1)
        assert o.c.any() and o.passes > 0 and (L == 1 or grid == 'lava32' or o.walked > o.passes)  # (lava32: every pass ends at once)
    finally:
        vec.close()


@pytest.mark.parametrize('epsilon', [0.1, 1.0])
def test_other_epsilons(epsilon):
    vec, o = _pair(GRIDS['open8x8'](), 200, 4)
    try:
        for T in (150, 100):
            _launch(vec, o, T, 24, epsilon=epsilon)
        same_env_state(vec, o)
    finally:
        vec.close()


def test_without_exploration_class_zero_never_occurs():
    vec, o = _pair(GRIDS['default4x4'](), 200, 4)
    try:
        for T in (150, 100):
            _launch(vec, o, T, 24, epsilon=0.0)
            assert o.buf_cnt.any()
            live = np.arange(IO.IS_MAX)[None, :] < o.buf_cnt[:, None]
            assert (o.buf_c[live] > 0).all()
        same_env_state(vec, o)
    finally:
        vec.close()


def test_one_launch_equals_two():
    g = GRIDS['open8x8']()
    a = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    b = gua.VecGridUniverse(1000, template=_spec(g), seed=11)
    try:
        a.reset()
        b.reset()
        whole = a.off_policy_mc_run(300, 64, 0.95, 0.2, trajectory=True, stats=True)
        p1 = b.off_policy_mc_run(150, 64, 0.95, 0.2, trajectory=True, stats=True)
        assert b.off_policy_episode_buffer()['count'].any()  # (something is carried)
        p2 = b.off_policy_mc_run(150, 64, 0.95, 0.2, trajectory=True, stats=True)
        for k in ('obs', 'reward', 'done'):
            assert np.concatenate([p1[k], p2[k]]).tobytes() == whole[k].tobytes(), k
        assert a.q_table().tobytes() == b.q_table().tobytes()
        assert a.importance_weights().tobytes() == b.importance_weights().tobytes()
        assert a.importance_weights().any()
        x, y = a.off_policy_episode_buffer(), b.off_policy_episode_buffer()
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
    finally:
        a.close()
        b.close()


def _shared(cls, o):
    """A restatement of another learner on o's env state and Q tables."""
    other = cls(o.grid, o.seed, o.n)
    other.state, other.q = o.state, o.q
    return other


def _between_td(vec, o):
    _same(vec.td_run(20, 'q_learning', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(20, O.Q_LEARNING, 0.2, 0.9, _eps(0.3)))


def _between_nstep(vec, o):
    _same(vec.nstep_run(20, 3, 'q_learning', 0.2, 0.9, 0.3, trajectory=True, stats=True),
          _shared(NO.NstepOracle, o).nstep(20, O.Q_LEARNING, 3, 0.2, 0.9, _eps(0.3)))
    o.drop_buffer()


def _between_lambda(vec, o):
    _same(vec.lambda_run(20, 0.8, 8, 'q_learning', 0.2, 0.9, 0.3, trajectory=True, stats=True),
          _shared(LO.LambdaOracle, o).lam(20, O.Q_LEARNING, 8, 0.8, 0.2, 0.9, _eps(0.3)))
    o.drop_buffer()


def _between_ac(vec, o):
    _same(vec.actor_critic_run(20, 0.1, 0.2, 0.9, trajectory=True, stats=True), _shared(RO.ReinforceOracle, o).ac(20, 0.1, 0.2, 0.9))
    o.drop_buffer()


def _between_reinforce(vec, o):
    _same(vec.reinforce_run(20, 16, 0.05, 0.3, 0.9, trajectory=True, stats=True), _shared(RO.ReinforceOracle, o).reinforce(20, 16, 0.05, 0.3, 0.9))
    assert vec.episode_buffer()['count'].any()
    o.drop_buffer()


def _between_reset(vec, o):
    mask = np.zeros(o.n, np.uint8)
    mask[::7] = 1
    assert np.array_equal(vec.reset(mask), o.reset(mask))


def _between_ensure_q(vec, o):
    vec._ensure_q(0.5)  # (gu_td_init: new tables; the cumulative weights stay)
    o.set_q(np.full_like(o.q, 0.5))


def _between_set_q(vec, o):
    q = np.full((1, o.grid.S, 4), 0.5)
    vec.set_q_table(q, env0=5)
    o.set_q(q, env0=5)


def _between_other_len(vec, o):
    _same(vec.off_policy_mc_run(20, 16, 0.9, 0.2, trajectory=True, stats=True), o.is_run(20, 16, 0.9, _eps(0.2), 2.0 ** 64))


@pytest.mark.parametrize('between', [_between_td, _between_nstep, _between_lambda, _between_ac, _between_reinforce, _between_reset,
                                     _between_ensure_q, _between_set_q, _between_other_len], ids=lambda f: f.__name__[9:])
def test_another_call_in_between_drops_the_buffer(between):
    """150 + another call + 150 against the restatement, which drops the buffer there: the pending transitions are not learned
    from."""
    g = GRIDS['open8x8']()
    vec, o = _pair(g, 300, 13)
    try:
        _launch(vec, o, 150, 64)
        assert o.buf_cnt.any()
        c_before = o.c.copy()
        between(vec, o)
        if between is not _between_other_len:
            assert not o.buf_cnt.any() and o.buf_L == 0
            buf = vec.off_policy_episode_buffer()
            assert not buf['count'].any() and (buf['sa'] == -1).all() and not buf['cls'].any()
            assert vec.importance_weights().tobytes() == c_before.tobytes()  # (none of these calls touches the weights)
        else:
            _same_buffer(vec, [o])
        _launch(vec, o, 150, 64)
        same_env_state(vec, o)
    finally:
        vec.close()


def test_off_policy_mc_run_drops_the_reinforce_buffer_the_sarsa_carry_and_both_windows():
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 9)
    try:
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        assert o.carry_valid
        _launch(vec, o, 30, 7)
        assert not o.carry_valid
        _same(vec.td_run(40, 'sarsa', 0.2, 0.9, 0.3, trajectory=True, stats=True), o.run(40, O.SARSA, 0.2, 0.9, _eps(0.3)))
        _same_tables(vec, o)
        vec.nstep_run(25, 4, 'sarsa', 0.2, 0.9, 0.3)
        assert vec.nstep_window()['count'].any()
        vec.off_policy_mc_run(5, 7)
        assert not vec.nstep_window()['count'].any()
        vec.lambda_run(25, 0.9, 8, 'sarsa', 0.2, 0.9, 0.3)
        assert (vec.lambda_window() >= 0).any()
        vec.off_policy_mc_run(5, 7)
        assert (vec.lambda_window() == -1).all()
        vec.reinforce_run(25, 64)
        assert vec.episode_buffer()['count'].any()
        vec.off_policy_mc_run(5, 7)
        assert not vec.episode_buffer()['count'].any()
    finally:
        vec.close()


@pytest.mark.parametrize('L', [3, 64])
@pytest.mark.parametrize('W,H', [(2, 2), (4, 4)])
def test_repeated_states_and_rewritten_rows_on_small_open_grids(W, H, L):
    """Tiny grids: many wall bumps, states repeated inside a segment, and with L = 3 truncations whose pass rewrites the row of
    the state the lane stands in (the next step must act on the rewritten row)."""
    vec, o = _pair(open_grid(W, H), 256, 7, 0.5)
    try:
        for T in (123, 77):
            _launch(vec, o, T, L, gamma=0.8, epsilon=0.3)
        same_env_state(vec, o)
    finally:
        vec.close()


def test_a_small_weight_cap():
    vec, o = _pair(open_grid(4, 4), 256, 7)
    ref = IO.IsOracle(o.grid, 7, 256)
    ref.reset()
    try:
        for T in (150, 100):
            _launch(vec, o, T, 64, epsilon=0.1, w_cap=2.0)
            ref.is_run(T, 64, 0.9, _eps(0.1), 2.0 ** 64)
        same_env_state(vec, o)
        assert o.q.tobytes() != ref.q.tobytes()  # (the cap ended passes: another cap, other tables)
    finally:
        vec.close()


def _group_launches(vec, side, runs):
    vec._ensure_is()
    assert np.array_equal(vec.reset(), side.reset())
    for T, L in runs:
        got = vec.off_policy_mc_run(T, L, 0.9, 0.2, trajectory=True, stats=True)
        _same(got, side.run(lambda o: o.is_run(T, L, 0.9, _eps(0.2), 2.0 ** 64)))
        _same_buffer(vec, side.oracles)
    assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
    assert vec.importance_weights().tobytes() == side.cat(lambda o: o.c).tobytes()


@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(n_grids, N):
    vec, side = multigrid_batch(IO.IsOracle, n_grids, N)
    try:
        _group_launches(vec, side, [(150, 24), (91, 24)])
    finally:
        vec.close()


def test_device_maze_learners_equal_the_oracle():
    vec, side = device_maze_batch(IO.IsOracle, 4)
    try:
        _group_launches(vec, side, [(120, 32), (80, 32)])
    finally:
        vec.close()


def test_step_counts_across_the_epoch_boundary():
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N)
        for T in (130, 170):
            _launch(vec, o, T, 24)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


# ---- without the restatement, on the device alone

@pytest.mark.parametrize('q0', [0.0, 0.25])
def test_without_discount_and_with_segments_of_one_q_holds_rewards_only(q0):
    vec = gua.VecGridUniverse(500, template=_spec(GRIDS['default4x4']()), seed=5)
    try:
        vec._ensure_q(q0)
        vec.reset()
        vec.off_policy_mc_run(300, 1, 0.0, 0.3)
        q, c = vec.q_table(), vec.importance_weights()
        assert np.isin(q, [q0, -1.0, 10.0, -10.0]).all() and (q == -1.0).any() and (q == 10.0).any()
        assert (q[c == 0] == q0).all() and (q[c > 0] != q0).all()
        assert not vec.off_policy_episode_buffer()['count'].any()
    finally:
        vec.close()


@pytest.mark.parametrize('grid', ['open8x8', 'maze11'])
def test_with_segments_of_one_the_weights_of_a_learner_sum_to_the_steps(grid):
    vec = gua.VecGridUniverse(500, template=_spec(GRIDS[grid]()), seed=5)
    try:
        vec.reset()
        for T in (211, 89):
            vec.off_policy_mc_run(T, 1, 0.9, 0.2)
        c = vec.importance_weights()
        assert (c == np.rint(c)).all() and (c.sum(axis=(1, 2)) == 300).all()
    finally:
        vec.close()


def test_a_second_run_from_zeroed_weights_reproduces_the_first():
    vec = gua.VecGridUniverse(500, template=_spec(GRIDS['default4x4']()), seed=8)
    try:
        def run():
            vec.seed(8)
            vec._ensure_q(0.25)
            vec.reset()
            vec.off_policy_mc_run(300, 64, 0.9, 0.1)
            return vec.q_table(), vec.importance_weights()
        q1, c1 = run()
        assert c1.any() and np.isfinite(c1).all() and np.isfinite(q1).all()
        vec.set_importance_weights(np.zeros_like(c1))
        assert not vec.importance_weights().any()
        q2, c2 = run()
        assert q1.tobytes() == q2.tobytes() and c1.tobytes() == c2.tobytes()
        q3, c3 = run()  # (and without zeroing them it does not: the weights are state)
        assert c3.tobytes() != c1.tobytes()
    finally:
        vec.close()


def test_the_device_finishes_the_restatements_episodes():
    """The behaviour bound of test_is_host.py, on the device: the same totals."""
    total, _ = is_behaviour_totals(7)
    vec = gua.VecGridUniverse(64, template=_spec(GRIDS['default4x4']()), seed=7)
    try:
        vec.reset()
        got = vec.off_policy_mc_run(500, 64, 0.9, 0.1, stats=True)
        assert int(got['episodes'].sum()) == total >= 3000
    finally:
        vec.close()


def test_errors():
    g = GRIDS['test_env']()
    with Engine(8, _spec(g)) as eng:
        for call in (eng.is_init, lambda: eng.is_run(10), eng.is_get, lambda: eng.is_set(np.zeros((1, eng.spec.S, 4)))):
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -4  # GU_ERR_STATE before gu_td_init
        assert not eng.is_get_episode()['count'].any()
        eng.td_init(0.0)
        for call in (lambda: eng.is_run(10), eng.is_get, lambda: eng.is_set(np.zeros((1, eng.spec.S, 4)))):
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -4  # GU_ERR_STATE before gu_is_init
    vec, o = _pair(g, 64, 1)
    try:
        eng = vec.engine
        _launch(vec, o, 30, 16)
        assert o.buf_cnt.any()
        for kw in (dict(T=-1), dict(T=100000001), dict(L=0), dict(L=-3), dict(L=_lib.IS_MAX + 1), dict(gamma=float('nan')),
                   dict(gamma=float('inf')), dict(eps=65537), dict(w_cap=0.5), dict(w_cap=2.0 ** 257), dict(w_cap=float('inf')),
                   dict(w_cap=float('nan')), dict(w_cap=-1.0), dict(flags=_lib.F_AUTO_RESET), dict(flags=_lib.F_PACKED)):
            args = dict(T=10, L=16, gamma=0.9, eps=6554, w_cap=2.0 ** 64, flags=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_is_run(eng._h, args['T'], args['L'], args['gamma'], args['eps'], args['w_cap'], args['flags']))
            assert err.value.code == -1, kw
        with pytest.raises(gua.GuError) as err:  # rows without a reservation that holds them
            eng.is_run(100000, 16, trajectory=True)
        assert err.value.code == -4
        for call in (lambda: eng.is_get_episode(60, 5), lambda: eng.is_get(60, 5), lambda: eng.is_set(np.zeros((5, o.grid.S, 4)), 60)):
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_is_get(eng._h, 0, 1, None))
        assert err.value.code == -1
        _lib.check(eng.lib.gu_is_get_episode(eng._h, 0, 64, None, None, None, None))  # any pointer may be NULL
        for bad in (-1.0, float('nan'), float('inf')):
            c = np.zeros((2, o.grid.S, 4))
            c[1, 3, 2] = bad
            with pytest.raises(gua.GuError) as err:
                vec.set_importance_weights(c, env0=3)
            assert err.value.code == -1
        vec.off_policy_mc_run(0, 16)  # T = 0 changes nothing ...
        vec.off_policy_mc_run(0, 5)   # ... whatever its L
        _same_tables(vec, o)  # (the rejected weights wrote nothing)
        _same_buffer(vec, [o])
        _launch(vec, o, 20, 16)  # (the rejected calls changed nothing either: the buffer is still carried)
        same_env_state(vec, o)
        part = vec.off_policy_episode_buffer(10, 3)
        assert part['count'].tobytes() == o.buf_cnt[10:13].tobytes() and part['cls'].tobytes() == o.buf_c[10:13].tobytes()
        c = np.full((1, o.grid.S, 4), 2.5)
        vec.set_importance_weights(c, env0=7)  # installs weights and drops the buffer
        o.set_c(c, env0=7)
        _same_buffer(vec, [o])
        _launch(vec, o, 20, 16)
        for kw in (dict(max_episode_len=0), dict(max_episode_len=1025), dict(epsilon=1.5), dict(w_cap=0.5), dict(w_cap=float('nan'))):
            with pytest.raises(ValueError):
                vec.off_policy_mc_run(10, **kw)
    finally:
        vec.close()


def test_off_policy_mc_control_returns_a_table_in_q_learning_format():
    env = gua.GridUniverseEnv(grid_shape=(5, 5), lava_states=[12])
    q = off_policy_mc_control(env, 3000, max_episode_len=64, discount_factor=0.9, num_learners=1, seed=1)
    S = env.world.size
    assert q.shape == (S, 4) and q.any() and np.isfinite(q).all()
    pi = greedy_policy(q, env)
    assert pi.shape == (S, 4)
    utils.get_policy_map(pi, (5, 5), mode='ansi')
    many = off_policy_mc_control(env, 500, num_learners=3, seed=1, q0=0.5)
    assert many.shape == (3, S, 4)
