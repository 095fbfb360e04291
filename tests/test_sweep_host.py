"""Batched prioritized sweeping, the parts that need no GPU: the key packing, the invariants of the CPU restatement
(tests/_sweep_oracle.py), the geometric predecessor rule against a full scan of the model, prioritized sweeping learning in fewer real
steps than Dyna-Q at the same planning budget, prioritized_sweeping's argument checks and the library's new symbols."""
import os
import subprocess

import numpy as np
import pytest

from griduniverse_amd import _lib
from griduniverse_amd.algorithms import prioritized_sweeping as exported
from griduniverse_amd.algorithms.dyna import prioritized_sweeping
from griduniverse_amd.envs.griduniverse_env import GridUniverseEnv
from oracle import c_oracle as C

from . import _dyna_oracle as D
from . import _golden as G
from . import _sweep_oracle as SW
from . import _walks
from ._tabular_cases import GRIDS, _grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = int(0.1 * 65536)


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def test_keys_hold_the_pair_and_order_by_priority_then_pair():
    p = np.array([0, 1, 7, 65535, 4 * 121 - 1])
    x = np.array([1.0, 0.3, 10.95, 1e-3, 2.5])
    key = SW.pack_keys(p, x, 0.0)
    assert key.dtype == np.uint64
    assert ((key & np.uint64(0xFFFF)) == p.astype(np.uint64)).all()  # the low 16 bits hold the pair
    assert [int(k) >> 16 for k in key] == [_bits(v) >> 16 for v in x]  # ... the rest the priority's pattern
    # the order follows the priority, whatever the pairs
    xs = np.sort(np.random.RandomState(0).uniform(1e-6, 20.0, 200))
    ps = np.random.RandomState(1).randint(0, 65536, 200)
    assert (np.diff(SW.pack_keys(ps, xs, 0.0).astype(np.float64)) >= 0).all()
    ks = SW.pack_keys(ps, xs, 0.0)
    distinct = (ks[1:] >> np.uint64(16)) != (ks[:-1] >> np.uint64(16))
    assert (ks[1:][distinct] > ks[:-1][distinct]).all() and distinct.sum() > 150
    # priorities that differ below the 36 kept mantissa bits are equal: the larger pair wins
    a, b = 1.0, float(np.nextafter(1.0, 2.0))
    assert _bits(a) != _bits(b) and _bits(a) >> 16 == _bits(b) >> 16
    ka, kb = SW.pack_keys([9], [b], 0.0)[0], SW.pack_keys([10], [a], 0.0)[0]
    assert kb > ka and SW.priorities(ka) == SW.priorities(kb) == 1.0
    # what is never queued: x <= theta, NaN, and a pattern whose kept bits are all zero (denormals below 2^-1058)
    tiny = np.uint64(0xFFFF).view(np.float64)
    assert tiny > 0.0 and _bits(tiny) >> 16 == 0
    assert SW.pack_keys([3, 3, 3], [tiny, 0.0, float('nan')], 0.0).tolist() == [0, 0, 0]
    assert SW.pack_keys([3, 3], [0.5, 0.25], 0.5).tolist() == [0, 0] and SW.pack_keys([3], [0.5000001], 0.5)[0] != 0
    assert SW.pack_keys([3], [float('inf')], 1e300)[0] == np.uint64((0x7FF0 << 48) | 3)


def _invariants(o, grid):
    key = o.key.reshape(o.n, -1)
    assert (o.size == (key != 0).sum(axis=1)).all()
    assert (o.next.reshape(o.n, -1)[key != 0] >= 0).all()  # every queued pair is observed
    e, p = np.nonzero(key)
    assert ((key[e, p] & np.uint64(0xFFFF)) == p.astype(np.uint64)).all()
    assert (SW.priorities(o.key)[o.key != 0] > 0).all() and (SW.priorities(o.key)[o.key == 0] == 0).all()


@pytest.mark.parametrize('W,H', [(4, 4), (8, 8)])
def test_restatement_keeps_its_invariants(W, H):
    grid = C.Grid.from_lists(W, H, lava=[W + 1])
    o = SW.SweepOracle(grid, 9, 24, q0=0.25)
    o.reset()
    for T, P, theta, eps in ((120, 3, 0.0, 0.3), (80, 1, 1e-4, 1.0), (60, 20, 1e-4, 0.1)):
        o.sweep(T, P, theta, 0.3, 0.9, int(eps * 65536))
        _invariants(o, grid)
    assert o.pops > 0 and o.inserts >= o.pops
    # a threshold above any reachable |delta|: nothing is ever queued and, all learning going through the queue, Q never changes
    o = SW.SweepOracle(grid, 9, 24, q0=0.25)
    o.reset()
    o.sweep(150, 5, 1e9, 0.3, 0.9, EPS)
    assert not o.key.any() and (o.size == 0).all() and (o.q == 0.25).all() and o.pops == 0
    assert (o.count > 0).all()  # (the model was recorded all the same)
    # P = 0: Q never changes and the queue only grows
    o = SW.SweepOracle(grid, 9, 24)
    o.reset()
    before = o.key.copy()
    for _ in range(6):
        o.sweep(25, 0, 0.0, 0.3, 0.9, 2 * EPS)
        assert (o.q == 0.0).all() and (o.key >= before).all()
        before = o.key.copy()
    assert (o.size > 0).all() and o.pops == 0
    _invariants(o, grid)


def test_real_steps_are_those_of_q_learning_without_its_update():
    """With nothing ever queued the tables stay flat, so the walk is the one of a Dyna-Q learner with alpha = 0."""
    grid = C.Grid.from_lists(4, 4, lava=[6])
    o, d = SW.SweepOracle(grid, 5, 16, q0=0.5), D.DynaOracle(grid, 5, 16, q0=0.5)
    assert np.array_equal(o.reset(), d.reset())
    got, want = o.sweep(200, 4, 1e9, 0.3, 0.9, EPS), d.dyna(200, 0, 0.0, 0.9, EPS)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for k, v in d.model().items():
        assert np.array_equal(o.model()[k], v), k


@pytest.mark.parametrize('name', ['maze11', 'test_env'])
def test_geometric_predecessors_are_all_predecessors(name):
    """On a model recorded under the current grid the 20 candidates hold every pair whose model entry leads to S."""
    grid = _grid(GRIDS[name]())
    o = SW.SweepOracle(grid, 2, 6)
    o.reset()
    o.sweep(1500, 0, 1e9, 0.1, 0.9, 65536)  # a random walk records the model
    assert (o.count > 20).all()
    for e in range(o.n):
        nxt = o.next[e]
        for S in range(grid.S):
            scan = set(np.flatnonzero(nxt.reshape(-1) == S).tolist())
            geo = set(c * 4 + b for c in SW.candidate_cells(S, grid.W, grid.S) for b in range(4) if nxt[c, b] == S)
            assert geo == scan, (e, S)


def steps_to_shortest(o, run, grid, best, chunk=50, limit=20000):
    """Real steps until every learner's greedy walk from the start is a shortest path."""
    o.reset()
    done = 0
    while done < limit:
        run(chunk)
        done += chunk
        if all(_walks._greedy_walk(grid, o.q[e]) == best for e in range(o.n)):
            return done
    return None


def test_prioritized_sweeping_needs_fewer_real_steps_than_dyna_q():
    """4 learners on maze_11x11, alpha 0.5, gamma 0.95, epsilon 0.1, P = 5: real steps until every learner's greedy walk is a
    shortest path.  The direction only is asserted; README.md quotes the two counts (printed here)."""
    grid = C.Grid.from_env(GridUniverseEnv(custom_world_fp=G.level_path('maze_11x11.txt')))
    best = _walks._shortest_from_start(grid)
    sw = SW.SweepOracle(grid, 3, 4)
    sweeping = steps_to_shortest(sw, lambda T: sw.sweep(T, 5, 1e-4, 0.5, 0.95, EPS), grid, best)
    assert sweeping is not None
    dy = D.DynaOracle(grid, 3, 4)
    dyna = steps_to_shortest(dy, lambda T: dy.dyna(T, 5, 0.5, 0.95, EPS), grid, best, limit=sweeping)
    print('real steps to a shortest greedy path at P = 5: prioritized sweeping', sweeping, 'Dyna-Q', dyna, '(None: not within the former)')
    assert dyna is None or dyna > sweeping, (sweeping, dyna)


def test_prioritized_sweeping_checks_its_arguments():
    env = GridUniverseEnv((4, 4))
    for kw in (dict(planning_steps=-1), dict(planning_steps=257), dict(num_learners=0), dict(epsilon=1.5), dict(epsilon=-0.1),
               dict(theta=-1e-9), dict(theta=float('nan')), dict(theta=float('inf'))):
        with pytest.raises(ValueError):
            prioritized_sweeping(env, 10, **kw)
    with pytest.raises(ValueError):
        prioritized_sweeping(env, -1)
    with pytest.raises(ValueError):  # S = 16 510: the pair index does not fit the key
        prioritized_sweeping(GridUniverseEnv((127, 130)), 10)
    assert exported is prioritized_sweeping


def test_library_exports_the_sweep_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    headers = ''.join(open(os.path.join(ROOT, 'include', h)).read() for h in ('gu.h', 'gu_diag.h'))
    for name in ('gu_sweep_init', 'gu_sweep_run', 'gu_sweep_get_queue', 'gu_diag_sweep_heap'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
        assert 'int ' + name + '(' in headers
    assert _lib.load().gu_version() == 1
