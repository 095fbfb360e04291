"""Simulation-based search (Monte-Carlo rollouts at decision time), the parts that need no GPU: the CPU restatement against the
tabular one, what the search buys over plain Q-learning, the argument checks of the Python layer and the library's new symbols."""
import subprocess

import numpy as np
import pytest

import griduniverse_amd.algorithms as algorithms
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.search import rollout_search
from oracle import c_oracle as C

from . import _search_oracle as SO
from . import _td_oracle as O
from ._behaviour import search_behaviour_totals
from ._tabular_cases import GRIDS, _grid


@pytest.mark.parametrize('grid', ['default4x4', 'open8x8', 'maze11', 'lava32'])
def test_without_simulations_the_restatement_is_the_q_learning_oracle_byte_for_byte(grid):
    g = _grid(GRIDS[grid]())
    a = O.TdOracle(g, 7, 64, q0=0.25)
    b = SO.SearchOracle(g, 7, 64, q0=0.25)
    assert np.array_equal(a.reset(), b.reset())
    for T, D, eps_sim in ((200, 16, 65536), (100, 0, 0)):  # any depth, any rollout epsilon
        want = a.run(T, O.Q_LEARNING, 0.1, 0.99, 6554)
        got = b.search(T, 0, D, 0.1, 0.99, 6554, eps_sim)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert b.q.tobytes() == a.q.tobytes()
    for k in ('pos', 'done', 'episode', 'tcount'):
        assert np.array_equal(getattr(a.state, k), getattr(b.state, k)), k
    assert not b.score.any() and not b.sim_steps.any()


def _look(grid, s, a):
    nxt, r, d = C.look_step_ahead(grid, np.array([s], np.int32), np.array([a], np.int32), True)
    return int(nxt[0]), int(r[0]), bool(d[0])


def test_restated_skips_and_counts():
    """An exploring step simulates nothing; a rollout simulates at most D moves, none behind a terminal first move; with D = 0
    the score of an action is M times one value."""
    g = _grid(GRIDS['default4x4']())
    o = SO.SearchOracle(g, 3, 16, q0=0.5)
    o.reset()
    o.search(20, 3, 5, 0.1, 0.9, 65536, 0)  # always exploring
    assert not o.sim_steps.any() and not o.score.any()
    o.search(10, 3, 5, 0.1, 0.9, 0, 13107)
    assert (o.sim_steps > 0).all() and (o.sim_steps <= 10 * 4 * 3 * 5).all()
    q = o.q.copy()
    s = o.state.pos.copy()
    o.state.done[:] = 0
    o.search(1, 3, 0, 0.0, 0.9, 0, 0)  # alpha = 0: the table stays
    assert not o.sim_steps.any() and o.q.tobytes() == q.tobytes()
    for e in range(16):
        for b in range(4):
            s1, r1, d1 = _look(g, s[e], b)
            g0 = float(r1) if d1 else float(r1) + 0.9 * O.row_max(q[e, s1])
            assert o.score[e, b] == (g0 + g0) + g0


@pytest.mark.parametrize('grid,ratio', [('open8x8', 3.0), ('default4x4', 1.4)])
def test_search_finishes_more_episodes_than_plain_q_learning(grid, ratio):
    """Same seeds, same 300 steps of 64 learners, alpha 0.1, gamma 0.99, epsilon 0.1: 4 uniform rollouts of depth 16 per action
    against none.  Bounds: the issue's -- on open8x8 three times plain Q-learning's total (half of the 5.9x of its prototype, as
    margin for a detail restated differently) and every learner at least 2 episodes; on default4x4 1.4 times.
    Observed with this restatement (finished episodes, search against plain): open8x8 427 (every learner at least 2) against
    72; default4x4 1832 against 1001 -- the prototype's totals exactly."""
    total, plain, least = search_behaviour_totals(grid)
    print('{}: search {} finished episodes (least per learner {}), plain Q-learning {}'.format(grid, total, least, plain))
    assert plain > 0 and total >= ratio * plain
    if grid == 'open8x8':
        assert least >= 2


def test_python_argument_checks():
    env = object()  # (never reached: the checks come first)
    for kw in (dict(simulations=-1), dict(simulations=65), dict(depth=-1), dict(depth=257), dict(epsilon=1.5), dict(epsilon=-0.1),
               dict(rollout_epsilon=1.01), dict(rollout_epsilon=-1.0), dict(num_learners=0)):
        with pytest.raises(ValueError):
            rollout_search(env, 10, **kw)
    with pytest.raises(ValueError):
        rollout_search(env, -1)
    assert algorithms.rollout_search is rollout_search
    with pytest.raises(AttributeError):
        algorithms.no_such_algorithm


def test_library_exports_the_search_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_search_run', 'gu_search_get'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    assert _lib.SEARCH_MAX_M == 64 and _lib.SEARCH_MAX_D == 256
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'gu_search_kernel' in blob
