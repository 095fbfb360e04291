"""The cases of tests/test_gpu_eval.py's main matrix and of their host twin in tests/test_eval_host.py: the grids and planes of
tests/_overlay_starts.py under no overlay and under each kind, the tables the learners walk on, the start cells that are given, and the
conditions that keep a comparison from being vacuous.  Nothing here needs a device.

Tables.  On the small grids every learner has a table of its own: the restated learner (tests/_td_oracle.py, or the kind's td_run)
trains TRAIN steps from a table of small random integers, so that rows the learners never reached keep their ties, some walks end and
others loop.  On 'open150' (tables of up to 180 000 rows) the learners share a base table of small random integers in which two cells
of three lean towards the nearest terminal cell, and differ by an offset per (learner, action): tests/_eval_oracle.py's Shared.

Starts.  Every case is walked from the drawn starts.  On 'open150' only the first start lies near a terminal cell, so the case is walked
a second time from given cells (`first_states`): around the lava cell, around the goal and beside the cells of the kind's plane."""
import functools

import numpy as np

from . import _eval_oracle as EO
from . import _overlay_starts as OS
from . import _td_oracle as TD

K, L, GAMMA = 3, 33, 0.9
N, SEED, IDS = OS.N, OS.SEED, OS.IDS
TRAIN = {None: 300, 'boxes': 1500}  # steps of the restated learner behind a small grid's tables (other kinds: 300)
ALPHA, TRAIN_GAMMA, EPS_Q16 = 0.5, 0.9, 19661  # eps 0.3

CASES = [(None, 'starts8'), (None, 'open150')] + [(kind, OS.td_grid(kind, grid)) for kind in OS.KINDS for grid in ('starts8', 'open150')
                                                  if (kind, grid) != ('boxes', 'open150')]
assert ('boxes', 'learn4') in CASES and ('errands', 'open150:td') in CASES and len(CASES) == 13


def is_big(name):
    return name.split(':')[0] == 'open150'


def bits(kind, name):
    if kind is None:
        return 0
    return OS.oracle(kind, name, 0, n=1, q0=None)._bits()


@functools.lru_cache(maxsize=None)
def table(kind, name, env_id0):
    """The tables of the N learners of a case: float64 [N, rows, 4], or a Shared on 'open150'."""
    g = OS.grid_dict(name)
    S = g['W'] * g['H']
    rows = S << bits(kind, name)
    rs = np.random.RandomState(7)
    if is_big(name):
        base = rs.randint(0, 3, (rows, 4)).astype(np.float64)
        act = np.argmax(OS.policy_table(name.split(':')[0]), axis=1)
        lean = np.flatnonzero(np.arange(S) % 3 != 0)
        for word in range(rows // S):
            base[word * S + lean, act[lean]] += 3.0
        return EO.Shared(base, rs.randint(0, 2, (N, 4)))
    q0 = rs.randint(0, 3, (N, rows, 4)).astype(np.float64)
    steps = TRAIN.get(kind, TRAIN[None])
    if kind is None:
        o = TD.TdOracle(OS.c_grid(name), SEED, N, env_id0)
        o.q[:] = q0
        o.reset()
        o.run(steps, TD.Q_LEARNING, ALPHA, TRAIN_GAMMA, EPS_Q16)
    else:
        o = OS.oracle(kind, name, env_id0, q0=0.0)
        o.q[:] = q0
        o.reset()
        o.td_run(steps, TD.Q_LEARNING, ALPHA, TRAIN_GAMMA, EPS_Q16)
    return o.q


@functools.lru_cache(maxsize=None)
def first_states(kind, name):
    """int32[K, N] on 'open150', else None (the case is walked from the drawn starts only)."""
    if not is_big(name):
        return None
    g = OS.grid_dict(name)
    W, H = g['W'], g['H']
    p = np.zeros(W * H, np.uint8) if kind in (None, 'wind', 'gusts') else OS.plane(kind, name)
    cells = [y * W + x for y in range(3, 8) for x in range(3, 8)] + [y * W + x for y in range(H - 3, H) for x in range(W - 3, W)]
    for c in np.flatnonzero(p).tolist():
        cells += [c - 1, c + 1, c - W, c + W]
    cells = np.array([c for c in cells if c not in g['lava'] and p[c] == 0] + [g['lava'][0], g['goals'][0]], np.int32)  # (two terminal starts)
    return cells[np.random.RandomState(3).randint(0, len(cells), (K, N))]


def restate(kind, name, env_id0, first=None, log=None):
    q = table(kind, name, env_id0)
    if kind is None:
        return EO.evaluate_calm(OS.c_grid(name), SEED, N, env_id0, q, K, L, GAMMA, first, log)
    return EO.evaluate_overlay(kind, name, env_id0, q, K, L, GAMMA, first, log=log)


def not_vacuous(kind, name, log):
    """What the walks of a case (from the drawn starts and, on 'open150', from the given cells) must have met."""
    g = OS.grid_dict(name)
    want = {0} | ({1} if g['goals'] else set()) | ({2} if g['lava'] else set()) | ({3} if kind in ('boxes', 'errands') else set())
    assert want <= log['outcomes'], (want, log['outcomes'])
    assert log['ties'] > 0
    assert set(g['starts']) <= log['starts'], log['starts']
    if kind == 'gusts':
        assert log['gust_moved'] > 0
    if kind == 'errands':
        assert log['drawn'] == set(range(len(OS.extra(kind, name)[0]))), log['drawn']
