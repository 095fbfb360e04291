"""The cases of tests/test_gpu_overlay_starts.py and of its host twin in tests/test_env_ids_host.py: grids with THREE start cells
under each overlay kind, the planes on them, the restatement of each, where the envs are put, and the policy table.  Nothing here
needs a device.

Grids.  'starts8': 8 x 8, starts 9, 33 and 54, goals 63 and 36, lava 27 and 42, no walls -- three planes fit LDS, and from every
start a terminal cell is a few moves away, so episodes end all through a run of 33 steps.  'open150': the 150 x 150 grid of
tests/test_gpu_boxes.py (goal in the far corner, lava on (5, 5)) with starts (1, 1), (75, 75) and (140, 20) -- three planes do not
fit 64 KiB: the L2 kernels.  Only the first start lies near a terminal cell there, so after the first reset the envs are PUT on the
cells around the lava cell (`place`): episodes then end from the first step on, and every reset behind them draws among all three
starts.  'learn4': 4 x 4 with starts 4, 3 and 13, lava 12, one box on 5 and its target on 10 -- the boxes' learners (four bits).
'one_box8': 'starts8' with one box (six bits), for td_run under boxes where the five boxes of 'starts8' are refused.  A name with
':td' behind it is the same grid under the plane the errands' learners run on (GRIDS[name]['errands_td'], else the three fruit and two
instructions of tests/_errands_oracle.py's TD_* constants: six bits where the CASE_* plane takes ten).  tests/_overlay_scale.py adds
its own grids to GRIDS: such a grid names the cells of its planes ('cells') and the cells its envs are put on ('around') itself.

Planes, away from the start cells.  Wind: a random direction and strength 0 .. 3 per cell, with and without gusts ('gusts', 'wind').
Fruit: three fruit, one of each kind.  Doors: one door and its key.  Boxes on 'starts8': the five boxes of tests/test_gpu_boxes.py.
Errands: the five fruit and three instructions of tests/test_gpu_errands.py (CASE_*, the 'wander' lists)."""
import functools

import numpy as np

from griduniverse_amd.grid import box_plane, door_plane, fruit_plane, wind_plane

from . import _boxes_oracle as BO
from . import _errands_oracle as EO
from . import _wind_oracle as WO
from ._overlays import masks_of, overlay  # noqa: F401  (masks_of: re-exported for the tests)

N, T, SEED = 130, 33, 6
IDS = (0, 2 ** 31 - 40)
KINDS = ('wind', 'gusts', 'fruit', 'doors', 'boxes', 'errands')
POLICIES = ('uniform', 'stream', 'greedy', 'sample')
FRUIT_VALUES = (3, -7, 16)
ON_TARGET = 5
Q0 = 0.5
UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3
TD = ':td'


def _open150():
    W = 150
    assert 2 * ((W * W + 15) & ~15) <= 65536 < 3 * ((W * W + 15) & ~15)
    # (the errands' learners: an apple and a lemon and one instruction, three bits as under fruit -- 5.8 MB a table)
    return dict(W=W, H=W, starts=[W + 1, 75 * W + 75, 20 * W + 140], goals=[W * W - 1], lava=[5 * W + 5], walls=[],
                errands_td=dict(cells=[2 * W + 2, 4 * W + 3], kinds=['apple', 'lemon'], instructions=[['apple']]))


_STARTS8 = dict(W=8, H=8, starts=[9, 33, 54], goals=[63, 36], lava=[27, 42], walls=[])
GRIDS = {'starts8': _STARTS8, 'one_box8': _STARTS8, 'learn4': dict(W=4, H=4, starts=[4, 3, 13], goals=[], lava=[12], walls=[]), 'open150': _open150()}


def grid_dict(name):
    return GRIDS[name[:-len(TD)] if name.endswith(TD) else name]


def td_grid(kind, name='starts8'):
    """The grid on which the learners of `kind` run where the other cases run on `name`: the boxes' word and the errands' CASE_* word
    take more bits there than gu_td_init admits or than a test's tables should."""
    return {'boxes': {'starts8': 'learn4'}.get(name, name), 'errands': name + TD}.get(kind, name)


@functools.lru_cache(maxsize=None)
def c_grid(name):
    return BO.grid_of(grid_dict(name))  # (takes a grid without a goal cell)


def box_cells(name):
    """(boxes, targets)"""
    g = grid_dict(name)
    if 'cells' in g:
        return g['cells']['boxes']
    W = g['W']
    return {'starts8': ([1, 10, 12, 17, 25], [2, 11, 13, 19, 26]), 'one_box8': ([10], [11]), 'learn4': ([5], [10]),
            'open150': ([W + 2, 2 * W + 1], [W + 3, 3 * W + 1])}[name]


def _errands(name):
    """(cells, kinds, instructions) of the errands on `name`."""
    g = grid_dict(name)
    W = g['W']
    if name.endswith(TD):
        own = g.get('errands_td')
        return (own['cells'], own['kinds'], own['instructions']) if own else (EO.case_cells(W, EO.TD_XY), EO.TD_KINDS, EO.TD_INSTRUCTIONS)
    cells = g['cells']['errands'] if 'cells' in g else EO.case_cells(W, EO.CASE_XY_150 if name == 'open150' else EO.CASE_XY)
    return cells, EO.CASE_KINDS, EO.CASE_INSTRUCTIONS['wander']


@functools.lru_cache(maxsize=None)
def plane(kind, name):
    g = grid_dict(name)
    W, H, own = g['W'], g['H'], g.get('cells', {})
    if kind in ('wind', 'gusts'):
        rs = np.random.RandomState(5)
        return wind_plane(W, H, rs.randint(0, 4, (H, W)), rs.randint(0, 4, (H, W)))
    if kind == 'fruit':
        cells = own.get('fruit') or ([18, 35, 45] if name != 'open150' else [2 * W + 2, 4 * W + 4, 5 * W + 3])
        return fruit_plane(W, H, cells, ['apple', 'lemon', 'melon'])
    if kind == 'doors':
        cells = own.get('doors') or ((28, 10) if name != 'open150' else (4 * W + 5, 2 * W + 3))
        if isinstance(cells, dict):  # (several slots: doors, keys and levers as door_plane takes them)
            return door_plane(W, H, cells['doors'], keys=cells.get('keys'), levers=cells.get('levers'))
        door, key = cells
        return door_plane(W, H, {0: door}, keys={0: key})
    if kind == 'errands':
        cells, kinds, _ = _errands(name)
        return EO.plane_of(W * H, cells, kinds)
    assert kind == 'boxes'
    return box_plane(W, H, *box_cells(name))


def extra(kind, name='starts8'):
    """The setter's arguments behind the plane of `kind` (as the restatement takes them: tests/_overlays.py): the gust probability,
    the fruit values, the boxes' pay, the errands' instructions on `name` and their pay."""
    if kind == 'errands':
        return (_errands(name)[2], EO.CASE_PAY)
    return {'wind': (0,), 'gusts': (WO.GUST_THIRDS,), 'fruit': (FRUIT_VALUES,), 'doors': (), 'boxes': (ON_TARGET,)}[kind]


def oracle(kind, name, env_id0, n=N, seed=SEED, q0=None):
    """The restatement of n envs under `kind` on grid `name`, its first env the global id env_id0.  q0 None: no learners."""
    return overlay(kind).oracle(c_grid(name), seed, n, plane(kind, name), *extra(kind, name), env_id0=env_id0, q0=q0)


@functools.lru_cache(maxsize=None)
def placement(kind, name, n=N):
    """int32[n] or None: where the envs of 'open150' are put after a reset -- free cells within two of the lava cell (5, 5), none of
    them on the kind's plane; on a grid that names them, the cells of its 'around'."""
    g = grid_dict(name)
    if name.split(':')[0] != 'open150' and 'around' not in g:
        return None
    W, p = g['W'], plane(kind, name)
    around = g.get('around') or [y * W + x for y in range(3, 8) for x in range(3, 8) if (x, y) != (5, 5)]
    free = np.array([s for s in around if kind in ('wind', 'gusts') or p[s] == 0], np.int32)
    return free[np.random.RandomState(n).randint(0, len(free), n)]


def place(kind, name, o, vec=None):
    """Puts the restatement's envs (and the batch's) where `placement` says."""
    pos = placement(kind, name, o.n)
    if pos is not None:
        o.state.pos[:] = pos
        if vec is not None:
            vec.set_state(pos=pos)


@functools.lru_cache(maxsize=None)
def policy_table(name):
    """float64[S, 4]: every row leans towards the nearest terminal cell (along x first), so that greedy and sampling envs keep ending
    episodes; every seventh row is one-hot (thresholds that no word reaches)."""
    g = grid_dict(name)
    W, S = g['W'], g['W'] * g['H']
    x, y = np.arange(S) % W, np.arange(S) // W
    best, act = np.full(S, 1 << 30), np.zeros(S, np.int64)
    for t in g['goals'] + g['lava']:
        tx, ty = t % W, t // W
        dist = np.abs(x - tx) + np.abs(y - ty)
        a = np.where(x < tx, RIGHT, np.where(x > tx, LEFT, np.where(y < ty, DOWN, UP)))
        act, best = np.where(dist < best, a, act), np.minimum(dist, best)
    pi = 0.5 * np.random.RandomState(1).dirichlet(np.ones(4), S) + 0.5 * np.eye(4)[act]
    pi[::7] = np.eye(4)[act[::7]]
    return pi


def stream_actions(n=N):
    return np.random.RandomState(2).randint(0, 4, (T, n)).astype(np.int32)


def step_actions(n=N):
    return np.random.RandomState(11).randint(-4, 4, (T, n)).astype(np.int32)


def rollout_of(o, name, policy, steps=T, auto=True, t0=0):
    acts = stream_actions(o.n)[t0:t0 + steps] if policy == 'stream' else None
    pi = policy_table(name) if policy in ('greedy', 'sample') else None
    return o.rollout(steps, policy, auto, actions=acts, pi=pi)


def drew_every_start(o):
    """Every one of the three start cells was drawn by a lazy reset, and some step reset two envs to different cells."""
    assert len(o.starts.cells) == 3
    assert o.starts.every_start_was_drawn_and_some_step_mixed_them(), (o.starts.drawn, o.starts.mixed)
