"""Batched Expected SARSA (gu_esarsa_run, csrc/gu_td.hip) and Double Q-learning (gu_double_run, csrc/gu_double.hip) on the device
against the CPU restatements of tests/_double_oracle.py: tables (both of a pair), trajectory rows, statistics and env state compared
byte for byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.engine import Engine
from griduniverse_amd.grid import door_plane, fruit_plane, wind_plane

from . import _double_oracle as O
from . import _nstep_oracle as NO
from . import _td_oracle as TD
from ._learners import DoubleQ, ExpectedSarsa, _crossing, _shared_grid_beyond_lds, _stores_past_a_boundary, big182
from ._tabular_cases import (GRIDS, _eps, _grid, _same, _spec, code, counts_near_2_32, device_maze_batch, multigrid_batch, same_env_state,
                             spread_grid)

pytestmark = pytest.mark.gpu

KINDS = ('expected_sarsa', 'double_q')


def _oracle(kind, grid, seed, n, env_id0=0, q0=0.0):
    return (O.DoubleOracle if kind == 'double_q' else O.EsarsaOracle)(grid, seed, n, env_id0, q0)


def _fill(vec, kind, q0):
    if kind == 'double_q':
        vec._ensure_pairs(q0)
    else:
        vec._ensure_q(q0)


def _pair(kind, g, N, seed, q0=0.0):
    """A batch of N learners on grid g with tables of q0 and the restatement of it, both reset."""
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    _fill(vec, kind, q0)
    o = _oracle(kind, _grid(g), seed, N, q0=q0)
    assert np.array_equal(vec.reset(), o.reset())
    return vec, o


def _device(vec, kind, T, alpha, gamma, eps, **kw):
    run = vec.double_q_run if kind == 'double_q' else vec.expected_sarsa_run
    return run(T, alpha=alpha, discount_factor=gamma, epsilon=eps, **kw)


def _restate(o, kind, T, alpha, gamma, eps):
    return o.run(T, alpha, gamma, _eps(eps)) if kind == 'double_q' else o.esarsa(T, alpha, gamma, _eps(eps))


def _launch(vec, o, kind, T, alpha=0.1, gamma=0.99, eps=0.1):
    _same(_device(vec, kind, T, alpha, gamma, eps, trajectory=True, stats=True), _restate(o, kind, T, alpha, gamma, eps))


def _tables(vec, kind):
    return vec.double_q_tables() if kind == 'double_q' else vec.q_table()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('N', [1, 63, 4096])
def test_tables_rows_and_stats_equal_the_oracle(grid, kind, N):
    g = GRIDS[grid]()
    T = 300 if N < 4096 else 60
    q0 = 0.0 if N != 63 else 0.5  # (0.5: four-way ties in every row a learner has not touched)
    vec, o = _pair(kind, g, N, 3, q0)
    try:
        for _ in range(2):  # two launches: the second starts from the first one's state
            _launch(vec, o, kind, T, 0.25, 0.9, 0.2)
            got = _tables(vec, kind)
            assert got.shape == o.q.shape and got.tobytes() == o.q.tobytes()
        assert (o.q != q0).any()
        same_env_state(vec, o)
    finally:
        vec.close()


def test_expected_sarsa_without_exploration_is_q_learning_byte_for_byte():
    g = GRIDS['maze11']()
    a = gua.VecGridUniverse(130, template=_spec(g), seed=5)
    b = gua.VecGridUniverse(130, template=_spec(g), seed=5)
    try:
        a._ensure_q(0.125)
        b._ensure_q(0.125)
        assert np.array_equal(a.reset(), b.reset())
        for T in (211, 97):
            got = a.expected_sarsa_run(T, alpha=0.3, discount_factor=0.9, epsilon=0.0, trajectory=True, stats=True)
            want = b.td_run(T, 'q_learning', alpha=0.3, discount_factor=0.9, epsilon=0.0, trajectory=True, stats=True)
            _same(got, want)
            assert a.q_table().tobytes() == b.q_table().tobytes()
        assert (a.q_table() != 0.125).any()
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('kind', KINDS)
def test_split_launches_with_changed_hyper_parameters(kind):
    vec, o = _pair(kind, GRIDS['test_env'](), 130, 8)
    try:
        for alpha, eps in ((0.5, 0.3), (0.1, 0.0), (0.3, 1.0), (0.2, 0.05)):
            _launch(vec, o, kind, 257, alpha, 0.95, eps)
        assert _tables(vec, kind).tobytes() == o.q.tobytes()
        same_env_state(vec, o)
    finally:
        vec.close()


def _grouped(kind, vec, side, launches):
    assert np.array_equal(vec.reset(), side.reset())
    for T in launches:
        got = _device(vec, kind, T, 0.2, 0.9, 0.25, trajectory=True, stats=True)
        _same(got, side.run(lambda o: _restate(o, kind, T, 0.2, 0.9, 0.25)))
    assert _tables(vec, kind).tobytes() == side.cat(lambda o: o.q).tobytes()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(kind, n_grids, N):
    vec, side = multigrid_batch(functools.partial(_oracle, kind), n_grids, N)
    try:
        _fill(vec, kind, 0.0)
        _grouped(kind, vec, side, (150, 90) if n_grids == 4 else (60, 40))  # (one restatement per grid: shorter launches where there are 256)
    finally:
        vec.close()


@pytest.mark.parametrize('kind', KINDS)
def test_device_maze_learners_equal_the_oracle(kind):
    vec, side = device_maze_batch(functools.partial(_oracle, kind), 256)
    try:
        _fill(vec, kind, 0.0)
        _grouped(kind, vec, side, (50, 30))
    finally:
        vec.close()


@pytest.mark.parametrize('kind', KINDS)
def test_step_counts_across_the_epoch_boundary(kind):
    """Both streams are re-keyed where an env's count passes 2^32: stream 4 (the action) and stream 10 (the coin)."""
    N = 96
    vec, o = _pair(kind, GRIDS['open8x8'](), N, 12)
    try:
        tc = counts_near_2_32(vec, o, N)
        _launch(vec, o, kind, 300, 0.2, 0.9, 0.5)
        assert _tables(vec, kind).tobytes() == o.q.tobytes()
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(300))
    finally:
        vec.close()


def test_expected_sarsa_between_two_sarsa_launches_ends_the_carried_action():
    vec, o = _pair('expected_sarsa', GRIDS['open8x8'](), 200, 4)
    try:
        rows = ('obs', 'reward', 'done')
        _same(vec.td_run(50, 'sarsa', epsilon=0.3, trajectory=True), o.run(50, TD.SARSA, 0.1, 0.99, _eps(0.3)), rows)
        assert o.carry_valid and (o.carry >= 0).any()
        _same(vec.expected_sarsa_run(40, epsilon=0.3, trajectory=True), o.esarsa(40, 0.1, 0.99, _eps(0.3)), rows)
        assert not o.carry_valid
        _same(vec.td_run(70, 'sarsa', epsilon=0.3, trajectory=True), o.run(70, TD.SARSA, 0.1, 0.99, _eps(0.3)), rows)
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


def test_double_q_between_two_n_step_launches_drops_the_window():
    g, N, seed = GRIDS['maze11'](), 200, 4
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    try:
        vec._ensure_q(0.0)
        vec._ensure_pairs(0.0)
        o = NO.NstepOracle(_grid(g), seed, N)
        d = O.DoubleOracle(_grid(g), seed, N, share=o)
        assert np.array_equal(vec.reset(), o.reset())
        _same(vec.nstep_run(45, 8, 'sarsa', epsilon=0.3, trajectory=True, stats=True), o.nstep(45, TD.SARSA, 8, 0.1, 0.99, _eps(0.3)))
        assert o.count.any()
        _same(vec.double_q_run(20, epsilon=0.3, trajectory=True, stats=True), d.run(20, 0.1, 0.99, _eps(0.3)))
        assert not o.count.any() and o.key is None
        _same(vec.nstep_run(45, 8, 'sarsa', epsilon=0.3, trajectory=True, stats=True), o.nstep(45, TD.SARSA, 8, 0.1, 0.99, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes() and vec.double_q_tables().tobytes() == d.q.tobytes()
        win = vec.engine.nstep_get_window()
        for k in ('sa', 'reward', 'count'):
            assert np.array_equal(win[k], o.window()[k]), k
    finally:
        vec.close()


def test_pairs_installed_for_some_envs_are_read_back_and_learned_on():
    vec, o = _pair('double_q', GRIDS['test_env'](), 70, 9)
    try:
        _launch(vec, o, 'double_q', 60, 0.3, 0.9, 0.2)
        new = o.q[:5] * 0.5 + np.arange(5).reshape(5, 1, 1, 1) * 0.125
        new[:, :, 1] -= 1.0  # (B unlike A)
        vec.set_double_q_tables(new, env0=61)
        o.set_q(new, env0=61)
        assert vec.double_q_tables(61, 5).tobytes() == new.tobytes() and vec.double_q_tables().tobytes() == o.q.tobytes()
        _launch(vec, o, 'double_q', 60, 0.3, 0.9, 0.2)
        assert vec.double_q_tables().tobytes() == o.q.tobytes()
        vec.set_double_q_tables(new[0], env0=69)  # [S, 2, 4]: the pair of one env
        assert vec.double_q_tables(69, 1)[0].tobytes() == new[0].tobytes()
    finally:
        vec.close()


def test_argument_and_state_errors():
    g = GRIDS['test_env']()
    with Engine(64, _spec(g)) as eng:
        lib, h = eng.lib, eng._h
        assert code(lambda: eng.double_run(10)) == -4  # before gu_double_init
        assert code(eng.double_get_q) == -4
        assert code(lambda: eng.double_set_q(np.zeros((1, eng.spec.S, 2, 4)))) == -4
        assert code(lambda: eng.esarsa_run(10)) == -4  # before gu_td_init
        eng.td_init(0.25)
        eng.double_init(0.25)
        assert code(lambda: eng.double_get_q(60, 5)) == -1
        assert code(lambda: eng.double_get_q(-1, 2)) == -1
        assert code(lambda: eng.double_set_q(np.zeros((5, eng.spec.S, 2, 4)), env0=60)) == -1
        assert code(lambda: eng.double_init(float('inf'))) == -1
        for fn in (lib.gu_esarsa_run, lib.gu_double_run):
            for kw in (dict(eps_q16=65537), dict(alpha=float('nan')), dict(gamma=float('inf')), dict(T=-1), dict(flags=_lib.F_AUTO_RESET)):
                args = dict(T=10, alpha=0.1, gamma=0.9, eps_q16=0, flags=0)
                args.update(kw)
                assert code(lambda: _lib.check(fn(h, args['T'], args['alpha'], args['gamma'], args['eps_q16'], args['flags']))) == -1, kw
        # the agent trail is on and the launch writes no rows to feed it
        eng.trail_enable(16)
        assert code(lambda: eng.esarsa_run(10)) == -6
        assert code(lambda: eng.double_run(10)) == -6
        assert eng.td_get_q().tobytes() == np.full((64, eng.spec.S, 4), 0.25).tobytes()
        assert eng.double_get_q().tobytes() == np.full((64, eng.spec.S, 2, 4), 0.25).tobytes()


@pytest.mark.parametrize('kind', KINDS)
def test_alpha_zero_leaves_the_tables_at_their_fill(kind):
    vec, o = _pair(kind, GRIDS['test_env'](), 64, 1, q0=1.25)
    try:
        got = _device(vec, kind, 200, 0.0, 0.9, 0.4, stats=True)
        assert np.asarray(got['episodes']).any()
        assert _tables(vec, kind).tobytes() == o.q.tobytes()  # q0 bit for bit, in both tables of a pair
    finally:
        vec.close()


@pytest.mark.parametrize('overlay', ['wind', 'fruit', 'doors'])
def test_both_calls_are_refused_under_an_overlay_and_change_nothing(overlay):
    W = H = 8
    g = dict(W=W, H=H, starts=[0], goals=[63], lava=[36], walls=[21, 45])
    with Engine(70, _spec(g), seed=3) as eng:
        eng.td_init(0.0)
        eng.double_init(0.0)
        eng.reset()
        eng.esarsa_run(30)
        eng.double_run(30)
        if overlay == 'wind':
            eng.set_wind(wind_plane(W, H, np.array([0, 1, 2, 1, 0, 3, 1, 0]), 'down'), 43691)
        elif overlay == 'fruit':
            eng.set_fruit(fruit_plane(W, H, [2, W + 1], ['apple', 'lemon']), (1, 5, -5))
        else:
            eng.set_doors(door_plane(W, H, {0: [2 * W + 1, 2 * W + 2]}, keys={0: 1}))
        eng.td_init(0.5)  # (fruit and doors change the tables' row count: tables of the overlay's size)

        def snapshot():
            return [v.tobytes() for _, v in sorted(eng.get_state().items())] + [eng.td_get_q().tobytes(), eng.double_get_q().tobytes()]

        before = snapshot()
        assert eng.double_get_q().any()
        for run in (eng.esarsa_run, eng.double_run):
            with pytest.raises(gua.GuError) as err:
                run(10, stats=True)
            assert err.value.code == -6 and overlay in str(err.value)
        assert snapshot() == before


def test_a_grid_of_another_state_count_drops_the_pairs():
    with Engine(8, _spec(GRIDS['default4x4']()), seed=5) as eng:
        eng.double_init(0.0)
        eng.double_run(40)
        assert eng.double_get_q().shape == (8, 16, 2, 4) and eng.double_get_q().any()
        eng.set_grid(_spec(GRIDS['open8x8']()))
        assert code(lambda: eng.double_run(5)) == -4
        assert code(eng.double_get_q) == -4
        eng.double_init(0.5)
        assert eng.double_get_q().tobytes() == np.full((8, 64, 2, 4), 0.5).tobytes()
        eng.double_run(40)
        q = eng.double_get_q()
        assert (q != 0.5).any()
        eng.set_grid(_spec(dict(GRIDS['open8x8'](), walls=[27, 28, 35])))  # as many states: the pairs stay
        assert eng.double_get_q().tobytes() == q.tobytes()
        eng.double_run(10)


# ---- big grids and a store past 4 GiB, with the adapters and the harness of tests/_learners.py ----
@pytest.mark.parametrize('learner', [ExpectedSarsa, DoubleQ])
def test_a_shared_grid_beyond_lds(learner):
    """182 x 182: the planes do not fit LDS, so the L2 instantiations run, on cells past 32 767."""
    _shared_grid_beyond_lds(learner(), big182(), 32768)


def test_pairs_of_more_than_4_gib():
    """128 x 128 states: 1 MiB of pairs per env, so byte 2^32 of the store is the first of env 4 096; 4 200 envs hold 4.4 GB.  The
    first and the last 64 envs and the 64 around the crossing, each group whole against its restatement, through two launches, an
    install across the crossing and a third launch.  Short launches: the restatements' time goes into N * S, not T."""
    N, per_env = 4200, 64 * 128 * 128
    e = _crossing(per_env, N)
    assert e == 4096
    _stores_past_a_boundary(DoubleQ(), spread_grid(128, 128), N, [e], (12, 8), width=64)
