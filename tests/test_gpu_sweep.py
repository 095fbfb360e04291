"""Batched prioritized sweeping on the device (gu_sweep_run, csrc/gu_sweep.hip) against the CPU restatement tests/_sweep_oracle.py:
Q tables, every model plane, the queues' keys and sizes, trajectory rows, statistics and env state compared byte for byte after every
launch, and the device's raw heap checked for its shape.  The restatement keeps dense keys and pops by argmax; the device keeps a
heap: equal results come from the semantics, not from a shared structure."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.dyna import prioritized_sweeping
from griduniverse_amd.algorithms.temporal_difference import greedy_policy
from griduniverse_amd.engine import Engine
from griduniverse_amd.grid import GridSpec
from oracle import c_oracle as C

from . import _golden as G
from . import _sweep_oracle as SW
from ._tabular_cases import (GRIDS, SideBySide, _eps, _grid, _pair, _random_grids, _same, _spec, counts_near_2_32, device_maze_batch,
                             multigrid_batch, open_grid, same_env_state)

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, SW.SweepOracle)


def _same_heap(vec, oracles):
    """The raw form: a 1-based max-heap of exactly the queued keys, pos its inverse."""
    raw = vec.engine.diag_sweep_heap()
    key = np.concatenate([o.key for o in oracles]).reshape(vec.num_envs, -1)
    size = (key != 0).sum(axis=1)
    heap, pos = raw['heap'], raw['pos']
    assert heap.shape == (vec.num_envs, key.shape[1] + 2) and pos.shape == key.shape
    for e in range(vec.num_envs):
        n = int(size[e])
        h = heap[e, 1:n + 1]
        i = np.arange(2, n + 1)
        assert (heap[e, i >> 1] >= heap[e, i]).all(), e  # every parent >= its children
        assert sorted(h.tolist()) == sorted(key[e][key[e] != 0].tolist()), e
        queued = np.flatnonzero(key[e])
        assert ((heap[e, pos[e, queued]] & np.uint64(0xFFFF)) == queued.astype(np.uint64)).all(), e
        assert (pos[e, queued] >= 1).all() and (pos[e, queued] <= n).all(), e
        assert (pos[e, key[e] == 0] == -1).all(), e


def _same_all(vec, oracles, heap=True):
    assert vec.q_table().tobytes() == np.concatenate([o.q for o in oracles]).tobytes()
    got = vec.model()
    for k in ('next', 'reward', 'done', 'list', 'count'):
        assert got[k].tobytes() == np.concatenate([o.model()[k] for o in oracles]).astype(np.int32).tobytes(), k
    q = vec.priority_queue()
    key = np.concatenate([o.key for o in oracles])
    assert q['key'].dtype == np.uint64 and q['key'].tobytes() == key.tobytes()
    assert q['size'].dtype == np.int32 and q['size'].tobytes() == np.concatenate([o.size for o in oracles]).tobytes()
    assert q['priority'].tobytes() == SW.priorities(key).tobytes()
    same_env_state(vec, oracles)
    if heap:
        _same_heap(vec, oracles)


def _run(vec, oracles, T, P, theta, alpha, gamma, eps, heap=True):
    got = vec.sweep_run(T, P, theta=theta, alpha=alpha, discount_factor=gamma, epsilon=eps, trajectory=True, stats=True)
    _same(got, SideBySide(oracles).run(lambda o: o.sweep(T, P, theta, alpha, gamma, _eps(eps))))
    _same_all(vec, oracles, heap)


@pytest.mark.parametrize('theta', [0.0, 1e-4])
@pytest.mark.parametrize('P', [0, 1, 5, 50])
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_everything_equals_the_oracle_and_the_heap_is_a_heap(grid, P, theta):
    g = GRIDS[grid]()
    N, T = 63, (200 if P < 50 else 60)
    vec, o = _pair(g, N, 3, q0=0.5 if P == 1 else 0.0)
    try:
        for _ in range(2):  # the second launch continues from the first: tables, model and queue carry over
            _run(vec, [o], T, P, theta, 0.25, 0.9, 0.2)
    finally:
        vec.close()


@pytest.mark.parametrize('W,H', [(2, 2), (4, 4)])
def test_planning_that_rewrites_the_current_row_and_drains_the_queue(W, H):
    vec, o = _pair(open_grid(W, H), 128, 13, q0=0.75)
    try:
        for eps in (0.0, 0.2):
            _run(vec, [o], 150, 50, 1e-4, 0.5, 0.9, eps)
        assert o.pops < 2 * 150 * 50 * 128  # (the queue ran empty before the budget did)
    finally:
        vec.close()


def test_the_largest_grid_uses_every_bit_of_the_pair_index():
    W = 128
    g = dict(W=W, H=W, starts=[W * W - 1], goals=[0], lava=[], walls=[])  # 4S = 65 536; the learners start in the cell of pair 65 535
    vec, o = _pair(g, 64, 21)
    try:
        _run(vec, [o], 300, 5, 1e-4, 0.3, 0.9, 0.3)
        assert (o.next[:, -1, 3] >= 0).any() and o.pops > 64 * 300  # pair 65 535 was observed; the queues were at work
    finally:
        vec.close()


def test_an_oversized_grid_is_refused():
    with Engine(4, GridSpec(127, 130, [0], [127 * 130 - 1], [], [])) as eng:
        eng.td_init()
        with pytest.raises(gua.GuError) as err:
            eng.sweep_init()
        assert err.value.code == -1
        eng.dyna_init()  # (Dyna-Q itself has no such limit)


@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(n_grids, N):
    vec, side = multigrid_batch(SW.SweepOracle, n_grids, N)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        for T, P in (((100, 5), (60, 1)) if n_grids == 4 else ((40, 5), (20, 1))):  # (256 one-env oracles: the CPU side is the slow one)
            _run(vec, side.oracles, T, P, 1e-4, 0.2, 0.9, 0.25)
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(SW.SweepOracle, n_grids)
    try:
        assert np.array_equal(vec.reset(), side.reset())
        _run(vec, side.oracles, 120 if n_grids == 4 else 50, 5, 1e-4, 0.3, 0.9, 0.1)  # (256 one-env oracles: the CPU side is the slow one)
    finally:
        vec.close()


@pytest.mark.parametrize('grid', ['open8x8', 'lava32'])
def test_4096_learners_equal_the_oracle(grid):
    vec, o = _pair(GRIDS[grid](), 4096, 5)
    try:
        _run(vec, [o], 40, 5, 1e-4, 0.3, 0.95, 0.3, heap=False)
    finally:
        vec.close()


@pytest.mark.parametrize('P', [1, 5])
def test_split_launch_equals_one_launch(P):
    g = GRIDS['test_env']()
    a, o = _pair(g, 130, 8)
    b, _ = _pair(g, 130, 8)
    try:
        T, kw = 240, dict(theta=1e-4, alpha=0.4, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        whole = a.sweep_run(T, P, **kw)
        first = b.sweep_run(1, P, **kw)
        rest = b.sweep_run(T - 1, P, **kw)
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(whole[k], np.concatenate([first[k], rest[k]])), k
        assert np.array_equal(whole['ret'], first['ret'] + rest['ret'])
        assert a.q_table().tobytes() == b.q_table().tobytes()
        ma, mb = a.model(), b.model()
        assert all(ma[k].tobytes() == mb[k].tobytes() for k in ma)
        qa, qb = a.priority_queue(), b.priority_queue()
        assert all(qa[k].tobytes() == qb[k].tobytes() for k in qa)
        _same(whole, o.sweep(T, P, 1e-4, 0.4, 0.9, _eps(0.3)))
        _same_all(a, [o])
    finally:
        a.close()
        b.close()


def test_step_counts_across_the_epoch_boundary():
    """The stream-4 count t crosses 2^32 at different steps in different envs."""
    N, t0 = 96, 2 ** 32 - 60
    vec, o = _pair(GRIDS['open8x8'](), N, 12)
    try:
        tc = counts_near_2_32(vec, o, N, t0)
        _run(vec, [o], 100, 3, 1e-4, 0.2, 0.9, 0.5)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(100))
    finally:
        vec.close()


def _install(vec, o, g):
    vec.engine.set_grid(_spec(g))
    o.grid = _grid(g)
    assert np.array_equal(vec.reset(), o.reset())


def test_a_grid_of_the_same_shape_keeps_model_and_queue():
    """A 9x9 install onto a 9x9 grid: model and queue stay, every observation is compared with the stored word from now on."""
    first, second = _random_grids(2, 9, 9, 23)
    second['lava'] = [c for c in range(81) if c not in second['walls'] and c not in second['starts'] + second['goals']][:5]
    vec, o = _pair(first, 64, 4)
    try:
        _run(vec, [o], 150, 5, 1e-4, 0.3, 0.9, 0.5)
        assert (o.size > 0).any()
        _install(vec, o, second)
        _same_all(vec, [o])  # the install touched neither
        for T in (150, 80):
            _run(vec, [o], T, 5, 1e-4, 0.3, 0.9, 0.5)
        vec.engine.dyna_init()  # clears the model AND the queue
        o.clear_model()
        _same_all(vec, [o])
        assert not vec.priority_queue()['key'].any()
        _run(vec, [o], 100, 5, 1e-4, 0.3, 0.9, 0.5)
    finally:
        vec.close()


def test_a_grid_of_the_same_size_and_another_width_leaves_a_stale_model():
    """8x8 -> 16x4: S stays, W changes.  The kept model's entries lead where the old cells led; the geometric predecessor rule
    stays defined on them (with the new W) and the device follows it exactly."""
    a = GRIDS['open8x8']()
    b = dict(W=16, H=4, starts=[0], goals=[63], lava=[21], walls=[5, 37])
    vec, o = _pair(a, 64, 9)
    try:
        _run(vec, [o], 150, 5, 1e-4, 0.3, 0.9, 0.5)
        _install(vec, o, b)
        for T in (120, 80):
            _run(vec, [o], T, 5, 0.0, 0.3, 0.9, 0.5)
        vec.engine.dyna_init()
        o.clear_model()
        _same_all(vec, [o])
        _run(vec, [o], 100, 5, 1e-4, 0.3, 0.9, 0.5)
    finally:
        vec.close()


def test_a_dyna_run_in_between_shares_the_model_and_leaves_the_queue():
    vec, o = _pair(GRIDS['maze11'](), 100, 15)
    try:
        _run(vec, [o], 120, 5, 1e-4, 0.3, 0.9, 0.3)
        before = vec.priority_queue()
        got = vec.dyna_run(80, 3, alpha=0.3, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        _same(got, o.dyna(80, 3, 0.3, 0.9, _eps(0.3)))
        after = vec.priority_queue()
        assert all(before[k].tobytes() == after[k].tobytes() for k in before)
        _same_all(vec, [o])
        _run(vec, [o], 120, 5, 1e-4, 0.3, 0.9, 0.3)
    finally:
        vec.close()


def test_edges_and_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1, q0=1.25)
    try:
        vec._ensure_queue()
        eng = vec.engine
        S = _grid(g).S
        before = vec.get_state()
        eng.sweep_run(0, 5)  # T = 0 changes nothing
        assert all(np.array_equal(before[k], vec.get_state()[k]) for k in before)
        assert vec.model()['count'].tolist() == [0] * 64 and not vec.priority_queue()['key'].any()
        for eps in (0.0, 1.0):
            _run(vec, [o], 80, 4, 1e-4, 0.3, 0.9, eps)
        # either output pointer may be NULL
        size = np.empty(3, np.int32)
        _lib.check(eng.lib.gu_sweep_get_queue(eng._h, 5, 3, None, _lib.ptr(size)))
        assert np.array_equal(size, o.size[5:8])
        key = np.empty((4, S, 4), np.uint64)
        _lib.check(eng.lib.gu_sweep_get_queue(eng._h, 10, 4, _lib.ptr(key), None))
        assert key.tobytes() == o.key[10:14].tobytes()
        _lib.check(eng.lib.gu_sweep_get_queue(eng._h, 0, 0, None, None))
        pos = np.empty((2, 4 * S), np.int32)
        _lib.check(eng.lib.gu_diag_sweep_heap(eng._h, 3, 2, None, _lib.ptr(pos)))
        assert ((pos >= 1) == (o.key[3:5].reshape(2, -1) != 0)).all()
        part = eng.sweep_get_queue(60)
        assert part['key'].shape == (4, S, 4) and part['size'].tobytes() == o.size[60:].tobytes()
        # gu_td_init and gu_td_set_q leave model and queue alone
        eng.td_init(0.0)
        vec.set_q_table(np.ones((2, S, 4)), env0=1)
        assert vec.priority_queue()['key'].tobytes() == o.key.tobytes()
        nan, inf = float('nan'), float('inf')
        for kw in (dict(P=-1), dict(P=257), dict(theta=nan), dict(theta=-1e-9), dict(theta=inf), dict(T=1000000, P=100), dict(T=-1),
                   dict(T=100000001, P=0), dict(eps_q16=65537), dict(alpha=nan), dict(gamma=inf)):
            args = dict(T=10, P=1, theta=1e-4, alpha=0.1, gamma=0.9, eps_q16=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_sweep_run(eng._h, args['T'], args['P'], args['theta'], args['alpha'], args['gamma'], args['eps_q16'], 0))
            assert err.value.code == -1, kw
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_sweep_run(eng._h, 10, 1, 1e-4, 0.1, 0.9, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1
        with pytest.raises(gua.GuError) as err:
            eng.sweep_get_queue(60, 5)
        assert err.value.code == -1
        assert vec.priority_queue()['key'].tobytes() == o.key.tobytes()  # the refused calls changed nothing
        vec.set_wind(np.ones(g['W'], np.int64))  # wind is refused, as by gu_dyna_run
        with pytest.raises(gua.GuError) as err:
            eng.sweep_run(10, 1)
        assert err.value.code == -6 and 'wind' in str(err.value)
        vec.set_wind(None)
        eng.sweep_run(10, 1)
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        for call in (lambda: eng.sweep_run(10), lambda: eng.sweep_get_queue(), lambda: eng.diag_sweep_heap()):
            with pytest.raises(gua.GuError) as err:  # no queue
                call()
            assert err.value.code == -4
        eng.td_init()
        eng.dyna_init()
        with pytest.raises(gua.GuError) as err:  # tables and a model, but no queue
            eng.sweep_run(10)
        assert err.value.code == -4
    with Engine(8, _spec(g)) as eng:
        eng.sweep_init()
        with pytest.raises(gua.GuError) as err:  # a queue, but no Q tables
            eng.sweep_run(10)
        assert err.value.code == -4
        eng.td_init()
        eng.sweep_run(10, 256)
        eng.set_grid(_spec(GRIDS['default4x4']()))  # a grid of another size drops the queue with the model and the tables
        with pytest.raises(gua.GuError) as err:
            eng.sweep_get_queue()
        assert err.value.code == -4
        eng.td_init()
        eng.sweep_init()
        eng.sweep_run(10, 3)
        assert eng.sweep_get_queue()['key'].shape == (8, 16, 4)


def _shortest(env):
    with Engine(1, GridSpec.from_env(env)) as eng:
        paths, _ = eng.shortest_paths()
    return len(paths[0])


def test_prioritized_sweeping_learners_find_the_shortest_path():
    """1500 real steps with 20 planning updates each (the CPU restatement walks a shortest path from there with the same streams)."""
    env = gua.GridUniverseEnv(custom_world_fp=G.level_path('maze_11x11.txt'))
    q = prioritized_sweeping(env, 1500, planning_steps=20, theta=1e-4, alpha=0.5, discount_factor=0.95, epsilon=0.1, num_learners=4096, seed=1)
    assert q.shape == (4096, env.world.size, 4)
    grid = C.Grid.from_env(env)
    best = _shortest(env)
    for e in (0, 1, 4095):
        pi = greedy_policy(q[e], env)
        s, n = int(env.starting_states[0]), 0
        while not (grid.goal[s] or grid.lava[s]) and n <= grid.S:
            nxt, _, _ = C.look_step_ahead(grid, np.array([s], np.int32), np.array([int(np.argmax(pi[s]))], np.int32), True)
            s, n = int(nxt[0]), n + 1
        assert grid.goal[s] and n == best, e
