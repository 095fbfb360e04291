"""CPU restatement of doors, keys and levers (include/gu.h: gu_set_doors; csrc/gu_doors.hip, csrc/gu_td.hip) in numpy: every candidate
cell comes from the C oracle's look_step_ahead (care_about_terminal on) and every reset from its reset, the action words come from
oracle/gu_rng.py, and the learner on (cell, open) reuses the epsilon-greedy rule of tests/_td_oracle.py.  The oracle keeps a log of
what its runs met (bumps on closed doors, passages, key pick-ups, lever pulls), so that a comparison can show it compared something.
Only the rule is here: the resets, gu_step's rejected actions, the rollout policies and td_run around it are
tests/_overlay_oracle.py's.  Test infrastructure; it imports oracle/ read-only."""
import collections

import numpy as np

from oracle import c_oracle as C

from ._overlay_oracle import OverlayOracle
from ._td_oracle import Q_LEARNING, SARSA, choose, row_max, words  # noqa: F401  (re-exported for the tests)

DOOR, KEY, LEVER = 1, 2, 3
EVENTS = ('bump', 'passage', 'key', 'lever_open', 'lever_shut')


def kinds_of(door):
    return (np.asarray(door, np.int64) >> 4) & 3


def slots_of(door):
    return np.asarray(door, np.int64) & 7


class DoorsOracle(OverlayOracle):
    """N envs (and learners) on `grid` (a C.Grid) under the door plane `door` uint8[S] (None: no doors).  The learner's row is
    open * S + cell."""

    def __init__(self, grid, seed, n, door=None, env_id0=0, q0=0.0):
        super().__init__(grid, seed, n, env_id0, q0)
        self.log = dict.fromkeys(EVENTS, 0)
        self.terminal = (np.asarray(grid.goal) | np.asarray(grid.lava)).astype(np.int32)
        self.set_doors(door)

    def set_doors(self, door):
        """gu_set_doors: clears every mask; the tables go (back to q0: the caller's gu_td_init) when their row count changes."""
        self.door = np.zeros(self.grid.S, np.uint8) if door is None else np.asarray(door, np.uint8).copy()
        self.D = int(np.unique(self.door[self.door != 0] & 7).size)
        self.open = np.zeros(self.n, np.uint32)
        self._installed()

    def set_open(self, mask, env0=0):
        m = np.atleast_1d(np.asarray(mask, np.uint32))
        self.open[env0:env0 + m.size] = m
        self.carry_valid = False

    def _bits(self):
        return self.D

    def _row(self, pos):
        return self.open.astype(np.int64) * self.grid.S + pos

    def _restore(self, took, lazy=False):
        self.open[took] = 0

    def saw_everything(self):
        return all(self.log[k] > 0 for k in EVENTS)

    # one move of the envs in `who` (bool[n]) with actions act[n]: rules 2 .. 6 of gu_set_doors
    def _move(self, act, who=None):
        st = self.state
        who = np.ones(self.n, bool) if who is None else who
        s = st.pos.copy()
        c, rc, dc = C.look_step_ahead(self.grid, s, (np.asarray(act) & 3).astype(np.int32), True)  # the candidate, as without doors
        byte = self.door[c].astype(np.int64)
        kind, bit = (byte >> 4) & 3, (np.int64(1) << (byte & 7)).astype(np.uint32)
        is_open = (self.open & bit) != 0
        shut = (kind == DOOR) & ~is_open
        s2 = np.where(shut, s, c).astype(np.int32)
        r = np.where(shut, self.grid.reward[s], rc).astype(np.int32)  # a bump on a closed door pays what a wall bump from s pays
        d = np.where(shut, self.terminal[s], dc).astype(np.int32)
        entered = s2 != s
        key, lever = entered & (kind == KEY), entered & (kind == LEVER)
        new = np.where(key, self.open | bit, np.where(lever, self.open ^ bit, self.open)).astype(np.uint32)
        # (a bump on a closed door is a refused ENTRY: a wall bump of an agent that stands on a closed door cell is none)
        for name, m in (('bump', shut & (c != s)), ('passage', entered & (kind == DOOR)), ('key', key & ~is_open), ('lever_open', lever & ~is_open),
                        ('lever_shut', lever & is_open)):
            self.log[name] += int((m & who).sum())
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        self.open[who] = new[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()


def shortest_walk(grid, door, start):
    """(moves, return) of a shortest walk from `start` with all doors shut to a terminal cell: a breadth-first search over (cell, mask),
    every move one step of a one-env DoorsOracle.  None where no terminal cell can be reached.  The yardstick of the learning claim."""
    o = DoorsOracle(grid, 0, 1, door, q0=None)
    seen = {(int(start), 0): (0, 0)}
    queue = collections.deque([(int(start), 0)])
    while queue:
        s, mask = queue.popleft()
        moves, ret = seen[(s, mask)]
        for a in range(4):
            o.state.pos[0], o.open[0] = s, mask
            obs, r, d = o._move(np.array([a], np.int32))
            nxt = (int(obs[0]), int(o.open[0]))
            if d[0]:
                return moves + 1, ret + int(r[0])
            if nxt not in seen:
                seen[nxt] = (moves + 1, ret + int(r[0]))
                queue.append(nxt)
    return None


def greedy_walk(grid, door, q, cap=100):
    """(moves, return) of the greedy walk (first maximum) of one table q [S << D, 4] from the grid's first start cell, or None where it
    has not ended after `cap` moves."""
    o = DoorsOracle(grid, 0, 1, door, q0=None)
    o.reset()
    total = 0
    for i in range(cap):
        row = int(o.open[0]) * grid.S + int(o.state.pos[0])
        _, r, d = o._move(np.array([int(np.argmax(q[row]))], np.int32))
        total += int(r[0])
        if d[0]:
            return i + 1, total
    return None


# ---- the learning claim (tests/test_doors_host.py, tests/test_gpu_doors.py): a 7 x 3 grid cut in two by the column x = 4 -- walls above
# and below, a door of slot 0 in the middle --, the key at (2, 0) off the straight line, start (0, 1), goal (6, 1) ----
CLAIM_W, CLAIM_H = 7, 3
CLAIM = dict(W=CLAIM_W, H=CLAIM_H, starts=[7], goals=[13], lava=[], walls=[4, 18])
CLAIM_DOORS = dict(doors={0: 11}, keys={0: 2})
CLAIM_LEARNERS, CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16 = 64, 0.5, 0.95, 6554  # eps 0.1
CLAIM_WALK = (8, 3)  # three moves to the key, three to the door, two to the goal: -1 * 7 + 10
# the budget B: with DoorsOracle.td_run all 64 restated Q-learners walk greedily along a shortest walk from 700 steps on for each of the
# seeds 0, 1 and 2 (700 / 700 / 700; 51, 51 and 55 of 64 at 600), and stay there at every multiple of 100 up to 6000.  Doubled: the
# margin is for seeds not tried
CLAIM_STEPS = 1400


# ---- the two identities that rest on the calm engine alone (tests/test_doors_host.py against the C oracle, tests/test_gpu_doors.py
# against an engine without doors) ----
def _neighbours(g, s):
    W, H = g['W'], g['H']
    x, y = s % W, s // W
    return [yy * W + xx for xx, yy in ((x, y - 1), (x + 1, y), (x, y + 1), (x - 1, y)) if 0 <= xx < W and 0 <= yy < H]


def free_cells(g):
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    return [s for s in range(g['W'] * g['H']) if s not in taken]


def walled_in_case(g, n_slots=2):
    """(grid, plane, twin): `grid` is g with walls added around `n_slots` free cells, each of which holds the key of one slot and
    cannot be reached; `plane` puts the slots' doors on free cells near the start; `twin` is `grid` with walls at the door cells.
    Under masks 0 the doors never open, so the engine with doors walks as the twin does."""
    special = set(g['starts']) | set(g['goals']) | set(g['lava'])
    walls, keys = set(g['walls']), []
    open_sides = lambda s: [c for c in _neighbours(g, s) if c not in g['walls']]  # noqa: E731
    for s in sorted(free_cells(g), key=lambda s: (len(open_sides(s)), -s)):  # dead ends and corners first: few walls to add
        around = [c for c in _neighbours(g, s) if c not in walls]
        if s in special or s in walls or any(c in special or c in keys for c in around):
            continue
        walls |= set(around)
        keys.append(s)
        if len(keys) == n_slots:
            break
    assert len(keys) == n_slots
    grid = dict(g, walls=sorted(walls))
    free = [s for s in free_cells(grid) if s not in keys and s not in g['starts']]
    doors = free[1:1 + 2 * n_slots:2]
    plane = np.zeros(g['W'] * g['H'], np.uint8)
    for k in range(n_slots):
        plane[keys[k]] = k | (KEY << 4)
        plane[doors[k]] = k | (DOOR << 4)
    return grid, plane, dict(grid, walls=sorted(walls | set(doors)))


def keys_only_case(g, n_slots=2):
    """(grid, plane): keys and doors only (no lever) on free cells of g.  Under masks of all ones (and no reset) every door stays
    open, so the engine with doors walks as the engine without them does."""
    free = [s for s in free_cells(g) if s not in g['starts']]
    plane = np.zeros(g['W'] * g['H'], np.uint8)
    for k in range(n_slots):
        plane[free[1 + 2 * k]] = k | (DOOR << 4)
        plane[free[-2 - 2 * k]] = k | (KEY << 4)
    return g, plane
