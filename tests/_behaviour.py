"""What a learner buys over plain Q-learning, measured on the CPU restatements: the settings and totals of the behaviour checks.  The
host tests assert the bounds on these totals and the device tests assert that the device reaches the very same ones."""
import functools

import numpy as np

from . import _is_oracle as IO
from . import _mcts_oracle as MO
from . import _search_oracle as SO
from . import _td_oracle as O
from ._tabular_cases import GRIDS, _eps, _grid


# the settings of the search behaviour check (test_search_host.py; test_gpu_search.py asserts the same totals on the device)
SEARCH_BEHAVIOUR = dict(N=64, seed=7, T=300, alpha=0.1, gamma=0.99, eps_q16=6554, M=4, D=16, eps_sim_q16=65536)


def search_behaviour_totals(name):
    """(finished episodes of the search learners, of plain Q-learning, the least of one search learner) on grid `name`."""
    b = SEARCH_BEHAVIOUR
    grid = _grid(GRIDS[name]())
    plain = O.TdOracle(grid, b['seed'], b['N'])
    plain.reset()
    base = plain.run(b['T'], O.Q_LEARNING, b['alpha'], b['gamma'], b['eps_q16'])['episodes']
    srch = SO.SearchOracle(grid, b['seed'], b['N'])
    srch.reset()
    got = srch.search(b['T'], b['M'], b['D'], b['alpha'], b['gamma'], b['eps_q16'], b['eps_sim_q16'])['episodes']
    return int(got.sum()), int(base.sum()), int(got.min())


# the settings of the exploration behaviour checks (test_explore_host.py, test_gpu_explore.py)
EXPLORE_BEHAVIOUR = dict(N=64, seed=7, alpha=0.1, gamma=0.99, plain_eps_q16=6554)


def coverage(counts):
    """Per learner: the state-action pairs it has tried."""
    return (np.asarray(counts) != 0).sum(axis=(1, 2))


@functools.lru_cache(maxsize=None)
def is_behaviour_totals(seed):
    """(finished episodes of the off-policy Monte-Carlo learners, of plain Q-learning at alpha = 0.1) on the 4x4 grid: 64 learners x
    500 steps, epsilon 0.1, gamma 0.9, L = 64, w_cap 2^64; computed once per process (test_gpu_is.py asserts the same totals on the
    device)."""
    o = IO.IsOracle(_grid(GRIDS['default4x4']()), seed, 64)
    o.reset()
    out = o.is_run(500, 64, 0.9, _eps(0.1), 2.0 ** 64)
    plain = O.TdOracle(_grid(GRIDS['default4x4']()), seed, 64)
    plain.reset()
    return int(out['episodes'].sum()), int(plain.run(500, O.Q_LEARNING, 0.1, 0.9, _eps(0.1))['episodes'].sum())


# (M, H, D) of the behaviour check per grid, at the SEARCH_BEHAVIOUR settings, uniform rollouts, uct_tables(3.0)
TREE_BEHAVIOUR = {'open8x8': (16, 16, 16), 'default4x4': (64, 8, 4)}


@functools.lru_cache(maxsize=None)
def tree_behaviour_totals(name):
    """(finished episodes of the tree-search learners, the least of one learner) on grid `name`; computed once per process
    (test_gpu_mcts.py asserts the same totals on the device)."""
    b = SEARCH_BEHAVIOUR
    M, H, D = TREE_BEHAVIOUR[name]
    o = MO.MctsOracle(_grid(GRIDS[name]()), b['seed'], b['N'])
    o.tables = MO.uct_tables(3.0)
    o.reset()
    got = o.tree_search(b['T'], M, H, D, b['alpha'], b['gamma'], b['eps_q16'], 65536)['episodes']
    return int(got.sum()), int(got.min())


@functools.lru_cache(maxsize=None)
def plain_total(name):
    """Finished episodes of plain Q-learning at the same settings (the second entry of search_behaviour_totals)."""
    b = SEARCH_BEHAVIOUR
    plain = O.TdOracle(_grid(GRIDS[name]()), b['seed'], b['N'])
    plain.reset()
    return int(plain.run(b['T'], O.Q_LEARNING, b['alpha'], b['gamma'], b['eps_q16'])['episodes'].sum())
