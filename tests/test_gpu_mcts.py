"""Batched Monte-Carlo tree search on the device (gu_mcts_run, csrc/gu_mcts.hip) against the CPU restatement tests/_mcts_oracle.py:
Q tables, trajectory rows, statistics, env state, root rows, node counts, simulated-move counts and the whole tree dump compared
byte for byte."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.search import tree_search, uct_tables
from griduniverse_amd.engine import Engine

from . import _mcts_oracle as MO
from . import _td_oracle as TD
from ._behaviour import SEARCH_BEHAVIOUR, TREE_BEHAVIOUR, plain_total, tree_behaviour_totals
from ._tabular_cases import GRIDS, _eps, _pair, _same, _spec, counts_near_2_32, device_maze_batch, multigrid_batch, same_env_state

pytestmark = pytest.mark.gpu

_pair = functools.partial(_pair, MO.MctsOracle)


def _same_trees(vec, oracles):
    cat = lambda name: np.concatenate([getattr(o, name) for o in oracles])
    got = vec.tree_search_roots()
    assert got['w'].tobytes() == cat('root_w').tobytes()
    assert got['visits'].dtype == np.uint32 and got['visits'].tobytes() == cat('root_visits').tobytes()
    assert got['nodes'].dtype == np.int32 and np.array_equal(got['nodes'], cat('count'))
    assert got['sim_steps'].dtype == np.int64 and np.array_equal(got['sim_steps'], cat('sim_steps'))
    tree = vec.tree_search_tree()
    for k, name in (('state', 't_state'), ('parent', 't_parent'), ('child', 't_child'), ('visits', 't_visits'), ('w', 't_w'), ('count', 'count')):
        want = cat(name)
        assert tree[k].dtype == want.dtype and tree[k].shape == want.shape and tree[k].tobytes() == want.tobytes(), k


def _run(vec, o, T, M, H, D, eps_sim, alpha=0.25, gamma=0.9, eps=0.2):
    got = vec.tree_search_run(T, M, H, D, alpha=alpha, discount_factor=gamma, epsilon=eps, rollout_epsilon=eps_sim / 65536.0,
                              trajectory=True, stats=True)
    _same(got, o.tree_search(T, M, H, D, alpha, gamma, _eps(eps), eps_sim))
    assert vec.q_table().tobytes() == o.q.tobytes()
    _same_trees(vec, [o])


# (M, H, D, eps_sim_q16, T): one simulation of one level that bootstraps at once; M < 4 leaves untried root actions and H = 2 hits
# the depth cap; a mid-sized tree under an epsilon-greedy rollout policy; a deep tree without rollouts (TD tree search)
CASES = [(1, 1, 0, 0, 200), (3, 2, 5, 65536, 200), (16, 8, 4, 6554, 60), (40, 64, 0, 0, 30)]


@pytest.mark.parametrize('M,H,D,eps_sim,T', CASES)
@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_tables_rows_stats_state_and_trees_equal_the_oracle(grid, M, H, D, eps_sim, T):
    g = GRIDS[grid]()
    vec, o = _pair(g, 63, 3, q0=0.5 if M in (1, 16) else 0.0)
    try:
        for part in (T - T // 3, T // 3):  # two launches: the second starts from the first one's tables
            _run(vec, o, part, M, H, D, eps_sim)
        same_env_state(vec, o)
        assert o.sim_steps.sum() > 0
    finally:
        vec.close()


def test_4096_learners_equal_the_oracle():
    g = GRIDS['lava32']()
    vec, o = _pair(g, 4096, 5)
    try:
        _run(vec, o, 12, 8, 4, 8, 13107, alpha=0.3, gamma=0.95, eps=0.3)
        same_env_state(vec, o)
    finally:
        vec.close()


def test_the_largest_shapes():
    g = GRIDS['open8x8']()
    vec, o = _pair(g, 64, 2, q0=0.25)
    try:
        _run(vec, o, 1, 255, 64, 256, 65536, eps=0.0)
        assert (o.root_visits.sum(axis=1) == 255).all() and o.count.max() > 64
        same_env_state(vec, o)
    finally:
        vec.close()


def test_without_simulations_equals_td_q_learning():
    g = GRIDS['maze11']()
    a, _ = _pair(g, 300, 7, q0=0.1)
    b, _ = _pair(g, 300, 7, q0=0.1)
    try:
        for T, H, D, eps_sim in ((250, 8, 16, 1.0), (77, 64, 0, 0.0)):  # any tree depth, rollout depth and rollout epsilon
            got = a.tree_search_run(T, 0, H, D, alpha=0.3, discount_factor=0.95, epsilon=0.15, rollout_epsilon=eps_sim, trajectory=True,
                                    stats=True)
            want = b.td_run(T, 'q_learning', alpha=0.3, discount_factor=0.95, epsilon=0.15, trajectory=True, stats=True)
            _same(got, want)
            assert a.q_table().tobytes() == b.q_table().tobytes()
        sa, sb = a.get_state(), b.get_state()
        assert all(np.array_equal(sa[k], sb[k]) for k in ('pos', 'done', 'episode', 'tcount'))
        s = a.tree_search_roots()
        assert not s['w'].any() and not s['visits'].any() and not s['nodes'].any() and not s['sim_steps'].any()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('M,H,D,eps_sim', [(6, 3, 6, 1.0), (9, 8, 2, 0.25)])
def test_split_launch_equals_one_launch(M, H, D, eps_sim):
    g = GRIDS['test_env']()
    a, o = _pair(g, 130, 8)
    b, _ = _pair(g, 130, 8)
    try:
        T, kw = 60, dict(alpha=0.4, discount_factor=0.9, epsilon=0.3, rollout_epsilon=eps_sim, trajectory=True, stats=True)
        whole = a.tree_search_run(T, M, H, D, **kw)
        first = b.tree_search_run(1, M, H, D, **kw)
        n1 = b.tree_search_roots()['sim_steps']
        rest = b.tree_search_run(T - 1, M, H, D, **kw)
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(whole[k], np.concatenate([first[k], rest[k]])), k
        assert np.array_equal(whole['ret'], first['ret'] + rest['ret'])
        assert a.q_table().tobytes() == b.q_table().tobytes()
        sa, sb = a.tree_search_roots(), b.tree_search_roots()
        assert all(sa[k].tobytes() == sb[k].tobytes() for k in ('w', 'visits', 'nodes'))
        assert np.array_equal(sa['sim_steps'], n1 + sb['sim_steps'])
        ta, tb = a.tree_search_tree(), b.tree_search_tree()
        assert all(ta[k].tobytes() == tb[k].tobytes() for k in ta)
        _same(whole, o.tree_search(T, M, H, D, 0.4, 0.9, _eps(0.3), _eps(eps_sim)))
        assert a.q_table().tobytes() == o.q.tobytes()
        _same_trees(a, [o])
    finally:
        a.close()
        b.close()


def _group_run(vec, side, launches):
    assert np.array_equal(vec.reset(), side.reset())
    for T, M, H, D, eps_sim in launches:
        got = vec.tree_search_run(T, M, H, D, alpha=0.2, discount_factor=0.9, epsilon=0.25, rollout_epsilon=eps_sim, trajectory=True,
                                  stats=True)
        _same(got, side.run(lambda o: o.tree_search(T, M, H, D, 0.2, 0.9, _eps(0.25), _eps(eps_sim))))
    assert vec.q_table().tobytes() == side.cat(lambda o: o.q).tobytes()
    _same_trees(vec, side.oracles)
    same_env_state(vec, side)


@pytest.mark.parametrize('n_grids,N', [(4, 256), (256, 256)])  # groups of 64 (LDS-staged map), one grid per env (global map)
def test_multigrid_learners_equal_the_oracle(n_grids, N):
    vec, side = multigrid_batch(MO.MctsOracle, n_grids, N)
    try:
        _group_run(vec, side, ((3, 3, 2, 2, 1.0), (2, 3, 2, 2, 0.2)) if n_grids == 256 else ((12, 8, 4, 4, 1.0), (6, 8, 4, 4, 0.2)))
    finally:
        vec.close()


@pytest.mark.parametrize('n_grids', [4, 256])
def test_device_maze_learners_equal_the_oracle(n_grids):
    vec, side = device_maze_batch(MO.MctsOracle, n_grids)
    try:
        _group_run(vec, side, ((4, 3, 2, 2, 0.1),) if n_grids == 256 else ((12, 8, 5, 3, 0.1),))
    finally:
        vec.close()


@pytest.mark.parametrize('M,H,D,t0', [(2, 3, 4, 2 ** 32 - 30), (4, 4, 12, (2 ** 32) // (4 * 16) - 20), (3, 3, 4, 2 * (2 ** 32) // (3 * 7) - 10)])
def test_step_counts_across_the_epoch_boundaries(M, H, D, t0):
    """The stream-4 count t crosses 2^32, or the stream-8 count c = (t * M + j) * (H + D) + i does, mid-launch."""
    g = GRIDS['open8x8']()
    N = 96
    vec, o = _pair(g, N, 12)
    try:
        tc = counts_near_2_32(vec, o, N, t0)
        _run(vec, o, 60, M, H, D, 32768, alpha=0.2, gamma=0.9, eps=0.3)
        assert np.array_equal(vec.get_state()['tcount'], tc + np.uint64(60))
        same_env_state(vec, o)
    finally:
        vec.close()


def test_always_exploring_simulates_nothing_and_keeps_the_last_trees():
    g = GRIDS['open8x8']()
    vec, o = _pair(g, 100, 4, q0=0.3)
    try:
        _run(vec, o, 50, 3, 2, 6, 65536, eps=0.5)
        before, tree = vec.tree_search_roots(), vec.tree_search_tree()
        assert before['visits'].any()
        _run(vec, o, 80, 3, 2, 6, 65536, eps=1.0)
        s, t = vec.tree_search_roots(), vec.tree_search_tree()
        assert not s['sim_steps'].any()
        assert all(s[k].tobytes() == before[k].tobytes() for k in ('w', 'visits', 'nodes'))  # (of the last SEARCHED iteration)
        assert all(t[k].tobytes() == tree[k].tobytes() for k in tree)
    finally:
        vec.close()


def test_tree_search_run_ends_the_sarsa_carry():
    g = GRIDS['maze11']()
    vec, o = _pair(g, 200, 9)
    try:
        kw = dict(alpha=0.3, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        _same(vec.td_run(40, 'sarsa', **kw), o.run(40, TD.SARSA, 0.3, 0.9, _eps(0.3)))
        _run(vec, o, 10, 4, 4, 4, 65536, alpha=0.3, gamma=0.9, eps=0.3)
        assert not o.carry_valid
        _same(vec.td_run(40, 'sarsa', **kw), o.run(40, TD.SARSA, 0.3, 0.9, _eps(0.3)))  # a' drawn afresh at the first step
        assert vec.q_table().tobytes() == o.q.tobytes()
    finally:
        vec.close()


# counts beyond the tables (clamped); an odd size (24 C bytes are no whole 16-byte pieces); tables too large for LDS (read through L2)
@pytest.mark.parametrize('c,size', [(1.0, 4), (1.5, 37), (2.0, 4096)])
def test_other_tables(c, size):
    g = GRIDS['lava32']()
    vec, o = _pair(g, 70, 11)
    try:
        vec.set_tree_search(*uct_tables(c, size))
        o.tables = MO.uct_tables(c, size)
        _run(vec, o, 25, 20, 6, 3, 65536)
        _run(vec, o, 15, 20, 6, 3, 3277)
    finally:
        vec.close()


def test_edges_and_errors():
    g = GRIDS['test_env']()
    vec, o = _pair(g, 64, 1, q0=1.25)
    try:
        eng = vec.engine
        s = vec.tree_search_roots()  # before the first launch: zeros
        assert s['w'].shape == (64, 4) and not s['w'].any() and not s['visits'].any() and not s['nodes'].any() and not s['sim_steps'].any()
        t = vec.tree_search_tree()
        assert (t['state'] == -1).all() and (t['parent'] == -1).all() and (t['child'] == -1).all() and not t['visits'].any() and not t['w'].any()
        _run(vec, o, 30, 5, 3, 3, 6554)
        before, q, sc, tr = vec.get_state(), vec.q_table(), eng.mcts_get(), eng.mcts_tree()
        eng.mcts_run(0, 4, 8, 8)  # T = 0 changes nothing
        assert all(np.array_equal(before[k], vec.get_state()[k]) for k in before) and vec.q_table().tobytes() == q.tobytes()
        after, tr2 = eng.mcts_get(), eng.mcts_tree()
        assert all(after[k].tobytes() == sc[k].tobytes() for k in sc) and all(tr2[k].tobytes() == tr[k].tobytes() for k in tr)
        # any output pointer may be NULL
        steps = np.empty(3, np.int64)
        _lib.check(eng.lib.gu_mcts_get(eng._h, 5, 3, None, None, None, _lib.ptr(steps)))
        assert np.array_equal(steps, o.sim_steps[5:8])
        row, vis = np.empty((2, 4), np.float64), np.empty((2, 4), np.uint32)
        _lib.check(eng.lib.gu_mcts_get(eng._h, 62, 2, _lib.ptr(row), _lib.ptr(vis), None, None))
        assert row.tobytes() == o.root_w[62:].tobytes() and vis.tobytes() == o.root_visits[62:].tobytes()
        nodes = np.empty(4, np.int32)
        _lib.check(eng.lib.gu_mcts_get(eng._h, 10, 4, None, None, _lib.ptr(nodes), None))
        assert np.array_equal(nodes, o.count[10:14])
        child, count = np.empty((3, 6, 4), np.int32), np.empty(3, np.int32)
        _lib.check(eng.lib.gu_mcts_get_tree(eng._h, 7, 3, None, None, _lib.ptr(child), None, None, _lib.ptr(count)))
        assert child.tobytes() == o.t_child[7:10].tobytes() and np.array_equal(count, o.count[7:10])
        _lib.check(eng.lib.gu_mcts_get_tree(eng._h, 0, 64, None, None, None, None, None, None))
        for kw in (dict(M=-1), dict(M=6), dict(H=0), dict(H=65), dict(D=-1), dict(D=257), dict(eps_q16=65537), dict(eps_sim=65537), dict(T=-1),
                   dict(T=100000001, M=0), dict(T=63000, M=5, H=64, D=256), dict(alpha=float('nan')), dict(gamma=float('inf'))):
            args = dict(T=10, M=1, H=1, D=1, alpha=0.1, gamma=0.9, eps_q16=0, eps_sim=0)
            args.update(kw)
            with pytest.raises(gua.GuError) as err:
                _lib.check(eng.lib.gu_mcts_run(eng._h, args['T'], args['M'], args['H'], args['D'], args['alpha'], args['gamma'], args['eps_q16'],
                                               args['eps_sim'], 0))
            assert err.value.code == -1, kw
        eng.mcts_run(62000, 5, 64, 256, eps_q16=65536)  # T * (1 + M (H + D)) just below the bound; always exploring: nothing simulated
        assert not eng.mcts_get()['sim_steps'].any()
        with pytest.raises(gua.GuError) as err:
            _lib.check(eng.lib.gu_mcts_run(eng._h, 10, 1, 1, 1, 0.1, 0.9, 0, 0, _lib.F_AUTO_RESET))
        assert err.value.code == -1
        for call in (lambda: eng.mcts_get(60, 5), lambda: eng.mcts_init(0), lambda: eng.mcts_init(256),
                     lambda: eng.set_tree_tables(*uct_tables(1.0, 8)[:2], -np.ones(8)), lambda: eng.set_tree_tables(np.full(8, np.inf), np.ones(8), np.ones(8))):
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -1
        for bad in (np.ones(1), np.ones(4097)):
            with pytest.raises(gua.GuError) as err:
                eng.set_tree_tables(bad, bad, bad)
            assert err.value.code == -1
        with pytest.raises(ValueError):
            eng.set_tree_tables(np.ones(8), np.ones(8), np.ones(9))
        for bad in (dict(epsilon=1.5), dict(rollout_epsilon=-0.5), dict(simulations=256)):
            with pytest.raises(ValueError):
                vec.tree_search_run(10, **bad)
    finally:
        vec.close()
    with Engine(8, _spec(g)) as eng:
        for call in (lambda: eng.mcts_init(4), lambda: eng.mcts_run(10), lambda: eng.mcts_get(), lambda: eng.mcts_tree()):
            with pytest.raises(gua.GuError) as err:  # no Q tables
                call()
            assert err.value.code == -4
        eng.td_init()
        for call in (lambda: eng.mcts_run(10, 2), lambda: eng.mcts_get(), lambda: eng.mcts_tree()):
            with pytest.raises(gua.GuError) as err:  # no pool
                call()
            assert err.value.code == -4
        eng.mcts_init(4)
        eng.mcts_run(10, 0, 2, 2)  # without simulations no tables are needed
        with pytest.raises(gua.GuError) as err:  # no tables
            eng.mcts_run(10, 2, 2, 2)
        assert err.value.code == -4
        eng.set_tree_tables(*uct_tables())
        eng.mcts_run(10, 4, 2, 2)
        assert eng.mcts_get()['sim_steps'].sum() > 0
        with pytest.raises(gua.GuError) as err:  # more simulations than the pool holds
            eng.mcts_run(10, 5, 2, 2)
        assert err.value.code == -1
        eng.set_grid(_spec(GRIDS['default4x4']()))  # a grid of another size drops the pool with the Q tables; the U, B, I tables stay
        eng.td_init()
        with pytest.raises(gua.GuError) as err:
            eng.mcts_get()
        assert err.value.code == -4
        eng.mcts_init(3)
        got = eng.mcts_get()
        assert not got['w'].any() and not got['nodes'].any() and not got['sim_steps'].any()
        eng.mcts_run(10, 3, 2, 2)
        assert eng.mcts_get()['sim_steps'].sum() > 0 and eng.mcts_tree()['state'].shape == (8, 4)


def test_tree_search_finishes_more_episodes_than_plain_q_learning_on_the_device():
    """The totals of tests/test_mcts_host.py, which the device equals by construction: asserted here once, on open8x8."""
    b = SEARCH_BEHAVIOUR
    M, H, D = TREE_BEHAVIOUR['open8x8']
    vec = gua.VecGridUniverse(b['N'], template=_spec(GRIDS['open8x8']()), seed=b['seed'])
    try:
        vec.reset()
        vec.set_tree_search(*uct_tables(3.0))
        got = vec.tree_search_run(b['T'], M, H, D, alpha=b['alpha'], discount_factor=b['gamma'], epsilon=b['eps_q16'] / 65536.0,
                                  rollout_epsilon=1.0, stats=True)['episodes']
    finally:
        vec.close()
    plain = plain_total('open8x8')
    print('open8x8 on the device: tree search {} finished episodes (least per learner {}), plain Q-learning {}'.format(
        int(got.sum()), int(got.min()), plain))
    assert (int(got.sum()), int(got.min())) == tree_behaviour_totals('open8x8')
    assert got.sum() >= 3 * plain and got.min() >= 2


def test_tree_search_returns_tables_of_q_learnings_shape():
    env = gua.GridUniverseEnv(grid_shape=(4, 4))
    q = tree_search(env, 200, simulations=8, tree_depth=4, depth=2, num_learners=8, seed=1)
    assert q.shape == (8, env.world.size, 4) and q.dtype == np.float64 and np.isfinite(q).all() and q.any()
    q1 = tree_search(env, 50, simulations=2, tree_depth=2, depth=0, seed=1)
    assert q1.shape == (env.world.size, 4)
