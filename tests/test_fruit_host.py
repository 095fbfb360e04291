"""Fruit, the parts that need no GPU: the fruit plane, the CPU restatement against the calm C oracle, what fruit changes in a rollout's
rows (and what it does not), the argument checks, the library's symbols and the learning claim on the 5 x 3 grid."""
import re
import subprocess

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.grid import FRUIT_KINDS, fruit_plane
from oracle import c_oracle as C

from . import _fruit_oracle as O
from ._tabular_cases import GRIDS, _grid, _spec

CLAIM_STEPS = O.CLAIM_STEPS  # the learning claim's measured budget


def _free(g):
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    return [s for s in range(g['W'] * g['H']) if s not in taken]


def _some_fruit(g, n, seed=0):
    """n fruit cells of grid g (none on a wall or terminal cell), the first start cell among them, with kinds 1, 2, 3, 1, .."""
    free = [s for s in _free(g) if s != g['starts'][0]]
    cells = [g['starts'][0]] + [int(c) for c in np.random.RandomState(seed).choice(free, n - 1, replace=False)]
    return fruit_plane(g['W'], g['H'], cells, [1 + k % 3 for k in range(n)])


def test_fruit_plane_shapes_slot_order_and_errors():
    assert FRUIT_KINDS == {'apple': 1, 'lemon': 2, 'melon': 3}
    W, H = 5, 3
    p = fruit_plane(W, H, [7, 2, 11], ['lemon', 'melon', 1])
    assert p.dtype == np.uint8 and p.shape == (15,)
    want = np.zeros(15, np.uint8)
    want[2], want[7], want[11] = 0 | (3 << 5), 1 | (2 << 5), 2 | (1 << 5)  # slots by ascending cell index, kinds follow their cells
    assert np.array_equal(p, want)
    assert np.array_equal(fruit_plane(W, H, [4], 'apple'), np.eye(15, dtype=np.uint8)[4] * 32)
    assert np.array_equal(fruit_plane(W, H, np.array([0, 14]), 3), np.array([96] + [0] * 13 + [97], np.uint8))
    full = fruit_plane(8, 8, list(range(63, 31, -1)), 'melon')  # 32 fruits: slot 31 is in range
    assert np.array_equal(full[32:], np.arange(32, dtype=np.uint8) | 96) and not full[:32].any()
    for bad in (dict(cells=[]), dict(cells=list(range(33))), dict(cells=[64]), dict(cells=[-1]), dict(cells=[3, 3]), dict(cells=[[1, 2]]),
                dict(cells=[1.5]), dict(cells=3), dict(cells=[1], kinds='pear'), dict(cells=[1], kinds=0), dict(cells=[1], kinds=4),
                dict(cells=[1, 2], kinds=['apple']), dict(cells=[1], kinds=[True]), dict(cells=[1], kinds=1.0)):
        with pytest.raises(ValueError):
            fruit_plane(8, 8, **bad)


@pytest.mark.parametrize('name', ['default4x4', 'maze11', 'open8x8'])
def test_the_oracle_with_values_zero_equals_the_calm_c_oracle(name):
    g = GRIDS[name]()
    grid, T = _grid(g), 150
    plane = _some_fruit(g, 5)
    for N, seed in ((1, 2), (64, 9), (37, 5)):
        for auto in (True, False):
            o = O.FruitOracle(grid, seed, N, plane, (0, 0, 0), q0=None)
            st = C.State(N)
            assert np.array_equal(o.reset(), C.reset(grid, seed, st))
            got = o.rollout(T, 'uniform', auto_reset=auto)
            want = C.rollout(grid, seed, st, T, auto, stats=True)
            for k in ('obs', 'reward', 'done', 'ret', 'episodes'):
                assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), (k, auto, N)
            assert np.array_equal(o.state.pos, st.pos) and np.array_equal(o.state.done, st.done)
            assert np.array_equal(o.state.episode, st.episode) and np.array_equal(o.state.tcount, st.tcount)


@pytest.mark.parametrize('name', ['default4x4', 'maze11', 'open8x8'])
def test_fruit_pays_at_its_first_visit_of_an_episode_and_changes_nothing_else(name):
    g = GRIDS[name]()
    grid, N, T, seed, values = _grid(g), 48, 300, 4, (3, -7, 16)
    plane = _some_fruit(g, 6, seed=1)
    o = O.FruitOracle(grid, seed, N, plane, values, q0=None)
    st = C.State(N)
    assert np.array_equal(o.reset(), C.reset(grid, seed, st))
    got = o.rollout(T, 'uniform', auto_reset=True)
    calm = C.rollout(grid, seed, st, T, True)
    assert np.array_equal(got['obs'], calm['obs']) and np.array_equal(got['done'] != 0, calm['done'] != 0)
    extra = got['reward'].astype(np.int64) - calm['reward']
    kind, slot = O.kinds_of(plane), plane & 31
    paid = 0
    for e in range(N):
        seen = set()  # slots eaten in the running episode (a reset does not eat the start cell's fruit)
        for i in range(T):
            s = int(got['obs'][i, e])
            first = kind[s] != 0 and int(slot[s]) not in seen
            assert extra[i, e] == (values[kind[s] - 1] if first else 0), (e, i)  # .. so no fruit pays twice before a done
            if first:
                seen.add(int(slot[s]))
                paid += 1
            if got['done'][i, e]:
                seen = set()
    assert paid > N  # the case does eat
    assert np.array_equal(got['ret'], got['reward'].astype(np.int64).sum(axis=0))


class _NoEngine(object):
    """Stands in for Engine: any call on it is a library call that must not have been made."""

    def __init__(self, *a, **kw):
        self.calls, self.args, self.held = [], [], {}

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            self.args.append(a)
        return call

    def stores(self):
        """What the library would report (Engine.stores): the test sets `held`.  A query, so it is not recorded."""
        return self.held


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    free = _free(g)
    for kw in (dict(cells=[g['walls'][0]]), dict(cells=[g['goals'][0]]), dict(cells=[free[0], free[0]]), dict(cells=[]), dict(cells=free[:33]),
               dict(cells=[121]), dict(cells=[free[0]], kinds='pear'), dict(cells=[free[0]], values=(1, 2)), dict(cells=[free[0]], values=(17, 0, 0)),
               dict(cells=[free[0]], values=(0, -17, 0)), dict(cells=[free[0]], values=(1.5, 0, 0)), dict(cells=[free[0]], values=(True, False, True))):
        with pytest.raises(ValueError):
            vec.set_fruit(**kw)
    assert vec.engine.calls == []
    vec.set_fruit(free[:3], ['apple', 'lemon', 'melon'])
    vec.engine.held = dict(overlay=2, overlay_bits=3)
    for bad in ([8], [-1], [0.5], [[1]]):  # three fruits: bits 0 .. 2
        with pytest.raises(ValueError):
            vec.set_fruit_eaten(bad)
    assert vec.engine.calls == ['set_fruit']
    vec.set_fruit_eaten([7, 0], env0=1)
    vec.set_fruit(None)
    assert vec.engine.calls == ['set_fruit', 'set_fruit_state', 'set_fruit']
    from griduniverse_amd.algorithms.temporal_difference import q_learning, sarsa
    for learn in (q_learning, sarsa):
        with pytest.raises(ValueError):  # fruit and wind exclude each other
            learn(None, 10, wind=np.zeros(11, int), fruit=(free[:1], 'apple', (1, 5, -5)))
        with pytest.raises(ValueError):
            learn(None, 10, fruit=(free[:1], 'apple'))


def test_the_facade_asks_the_library_for_the_tables_after_set_fruit():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    free = _free(g)
    # The facade keeps no flag of its own: after set_fruit it asks the library, which drops tables of another row count
    # (tests/test_gpu_stores.py checks that half) and says so in stores().
    def inits():
        return [(c, a) for c, a in zip(vec.engine.calls, vec.engine.args) if c != 'set_fruit']

    vec.set_fruit(free[:2])
    vec.engine.held = dict(td_rows=0)  # another row count: the tables went
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))]
    vec.set_fruit(free[5:7], 'melon')  # two fruits again: the rows stay, and so do the tables
    vec.engine.held = dict(td_rows=121 << 2)
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))]
    vec.set_fruit(None)
    vec.engine.held = dict(td_rows=0)
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))] * 2
    assert vec.engine.calls == ['set_fruit', 'td_init', 'set_fruit', 'set_fruit', 'td_init']


def test_library_exports_the_fruit_entry_points_and_kernels():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_set_fruit', 'gu_get_fruit', 'gu_get_fruit_state', 'gu_set_fruit_state'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    blob = open(_lib.LIB_PATH, 'rb').read()
    for frame in (b'gu_overlay_step_kernel', b'gu_overlay_rollout_kernel'):  # the frame's name and the kind's rule type in ONE mangled symbol
        assert re.search(frame + rb'I\d+FruitRule', blob), frame
    assert b'gu_overlay_reset_kernel' in blob
    assert gua.Engine.ROLLOUT_FAMILIES[5] == 'fruit'


def _claim_value_iteration():
    """Exact undiscounted value iteration over the 15 x 4 states (cell, eaten) of the claim's grid, written out: the optimal return
    from the start and the moves of the greedy walk."""
    W, H, S = O.CLAIM_W, O.CLAIM_H, O.CLAIM_W * O.CLAIM_H
    goal, start = O.CLAIM['goals'][0], O.CLAIM['starts'][0]
    fruit = {2: (0, 8), 7: (1, -8)}  # cell: (slot, value)
    delta = [(0, -1), (1, 0), (0, 1), (-1, 0)]  # UP, RIGHT, DOWN, LEFT

    def step(s, m, a):
        x, y = s % W + delta[a][0], s // W + delta[a][1]
        s2 = y * W + x if 0 <= x < W and 0 <= y < H else s
        r = 10 if s2 == goal else -1
        if s2 in fruit and not (m >> fruit[s2][0]) & 1:
            r += fruit[s2][1]
            m |= 1 << fruit[s2][0]
        return s2, m, r, s2 == goal

    v = np.zeros((4, S))
    for _ in range(100):
        new = np.zeros_like(v)
        for m in range(4):
            for s in range(S):
                if s != goal:
                    new[m, s] = max(r + (0 if d else v[m2, s2]) for s2, m2, r, d in (step(s, m, a) for a in range(4)))
        if np.array_equal(new, v):
            break
        v = new
    s, m, moves, total = start, 0, 0, 0
    while s != goal:
        s, m, r, d = max((step(s, m, a) for a in range(4)), key=lambda o: o[2] + (0 if o[3] else v[o[1], o[0]]))
        moves, total = moves + 1, total + r
    s2, m2, straight = start, 0, 0
    for _ in range(4):  # RIGHT along the middle row, over the lemon
        s2, m2, r, d = step(s2, m2, 1)
        straight += r
    assert s2 == goal
    return v[0, start], moves, total, m, straight


def test_the_claims_optimal_walk_eats_the_melon_and_avoids_the_lemon():
    best, moves, total, eaten, straight = _claim_value_iteration()
    assert best == total == O.CLAIM_RETURN == 13 and moves == 6
    assert eaten == 1  # slot 0, the melon at (2, 0), and not slot 1, the lemon at (2, 1)
    assert straight == -1  # four moves along the middle row: -1 - 1 - 8 - 1 + 10


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_restated_q_learners_all_find_the_melon_walk(seed):
    grid = _grid(O.CLAIM)
    plane = fruit_plane(O.CLAIM_W, O.CLAIM_H, O.CLAIM_CELLS, O.CLAIM_KINDS)
    o = O.FruitOracle(grid, seed, O.CLAIM_LEARNERS, plane, O.CLAIM_VALUES, q0=0.0)
    o.reset()
    o.td_run(CLAIM_STEPS, O.Q_LEARNING, O.CLAIM_ALPHA, O.CLAIM_GAMMA, O.CLAIM_EPS_Q16)
    assert o.q.shape == (O.CLAIM_LEARNERS, 15 << 2, 4)
    returns = [O.greedy_walk(grid, plane, O.CLAIM_VALUES, o.q[e]) for e in range(O.CLAIM_LEARNERS)]
    assert returns == [O.CLAIM_RETURN] * O.CLAIM_LEARNERS, returns
