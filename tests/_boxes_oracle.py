"""CPU restatement of pushable boxes (include/gu.h: gu_set_boxes; csrc/gu_boxes.hip, csrc/gu_td.hip) in numpy: every candidate cell --
the agent's and the pushed box's -- comes from the C oracle's look_step_ahead (care_about_terminal on) and every reset from its
reset, the action words come from oracle/gu_rng.py, and the learner on (cell, word) reuses the epsilon-greedy rule of
tests/_td_oracle.py.  The oracle keeps a log of what its runs met (the nine EVENTS), so that a comparison can show it compared
something.  Only the rule is here: the resets, gu_step's rejected actions, the rollout policies and td_run around it are
tests/_overlay_oracle.py's.  Test infrastructure; it imports oracle/ read-only."""
import collections

import numpy as np

from oracle import c_oracle as C

from ._overlay_oracle import OverlayOracle
from ._td_oracle import Q_LEARNING, SARSA, choose, row_max, words  # noqa: F401  (re-exported for the tests)

TARGET, INITIAL = 1, 2
SOLVED_REWARD = 10
EVENTS = ('push', 'refused_wall', 'refused_box', 'refused_terminal', 'onto_target', 'off_target', 'solved', 'absorbing', 'reset_restored')


def grid_of(g):
    """The C oracle's grid of a grid dict; unlike C.Grid.from_lists it takes a grid without a goal cell."""
    S = g['W'] * g['H']
    flags = lambda idx: np.isin(np.arange(S), list(idx)).astype(np.uint8)  # noqa: E731
    reward = np.full(S, -1, np.int64)
    reward[list(g['goals'])] = 10
    reward[list(g['lava'])] = -10
    return C.Grid(g['W'], g['H'], flags(g['walls']), flags(g['lava']), flags(g['goals']), reward, list(g['starts']))


def bits_of(S):
    return max(1, int(S - 1).bit_length())


def plane_of(S, boxes, targets):
    p = np.zeros(S, np.uint8)
    p[list(targets)] |= TARGET
    p[list(boxes)] |= INITIAL
    return p


def pack(S, cells):
    """uint32[n] from box cells [n, B]."""
    c = np.asarray(cells, np.uint64).reshape(-1, np.shape(cells)[-1])
    return (c << (np.arange(c.shape[1], dtype=np.uint64) * np.uint64(bits_of(S)))).sum(axis=1).astype(np.uint32)


class BoxesOracle(OverlayOracle):
    """N envs (and learners) on `grid` (a C.Grid) under the box plane `box` uint8[S] (None: no boxes) with on_target = v.  The
    learner's row is word * S + cell."""

    def __init__(self, grid, seed, n, box=None, v=5, env_id0=0, q0=0.0):
        super().__init__(grid, seed, n, env_id0, q0)
        self.log = dict.fromkeys(EVENTS, 0)
        self.terminal = (np.asarray(grid.goal) | np.asarray(grid.lava)).astype(np.int32)
        self.set_boxes(box, v)

    def set_boxes(self, box, v=5):
        """gu_set_boxes: every env's boxes go to their initial cells; the tables go (back to q0) when their row count changes."""
        S = self.grid.S
        self.box = np.zeros(S, np.uint8) if box is None else np.asarray(box, np.uint8).copy()
        self.v = int(v)
        self.target = (self.box & TARGET).astype(np.int32)
        self.init = np.flatnonzero(self.box & INITIAL).astype(np.int32)  # box k by ascending cell
        self.B, self.b = len(self.init), bits_of(S)
        self.cells = np.tile(self.init, (self.n, 1))  # [n, B]
        self._installed()

    @property
    def words(self):
        return pack(self.grid.S, self.cells) if self.B else np.zeros(self.n, np.uint32)

    def set_cells(self, cells, env0=0):
        c = np.asarray(cells, np.int32).reshape(-1, self.B)
        self.cells[env0:env0 + len(c)] = c
        self.carry_valid = False

    def _bits(self):
        return self.b * self.B

    def _row(self, pos):
        return self.words.astype(np.int64) * self.grid.S + pos

    def _restore(self, took, lazy=False):
        if lazy:
            self.log['reset_restored'] += int((self.cells[took] != self.init).any(axis=1).sum()) if self.B else 0
        self.cells[took] = self.init

    def saw_everything(self, resets=True):
        """Has the log met every event?  resets=False: all but the lazy reset, which a run without auto-reset cannot meet."""
        return all(self.log[k] > 0 for k in EVENTS if resets or k != 'reset_restored')

    def solved(self):
        return self.target[self.cells].all(axis=1) if self.B else np.zeros(self.n, bool)

    # one move of the envs in `who` (bool[n]) with actions act[n]: rules 2 .. 7 of gu_set_boxes
    def _move(self, act, who=None):
        st, n, idx = self.state, self.n, np.arange(self.n)
        who = np.ones(n, bool) if who is None else who
        act = (np.asarray(act) & 3).astype(np.int32)
        s = st.pos.copy()
        solved0 = self.solved()
        c, _, _ = C.look_step_ahead(self.grid, s, act, True)  # the candidate, as without boxes
        hit = (self.cells == c[:, None]) & (c != s)[:, None] & ~solved0[:, None]  # [n, B]: box k stands on c, and c is entered
        pushing = hit.any(axis=1)
        k = hit.argmax(axis=1)
        c2, _, _ = C.look_step_ahead(self.grid, c, act, True)  # the engine's move from c with the same action
        by_wall = pushing & (c2 == c)
        by_terminal = pushing & ~by_wall & (self.terminal[c2] != 0)
        by_box = pushing & ~by_wall & ~by_terminal & (self.cells == c2[:, None]).any(axis=1)
        refused = by_wall | by_terminal | by_box
        pushed = pushing & ~refused
        stay = solved0 | refused
        s2 = np.where(stay, s, c).astype(np.int32)
        cells2 = self.cells.copy()
        cells2[idx[pushed], k[pushed]] = c2[pushed]
        gain = np.where(pushed, self.target[c2] - self.target[c], 0).astype(np.int32)
        won = self.target[cells2].all(axis=1) if self.B else np.zeros(n, bool)
        r = np.where(won, SOLVED_REWARD, self.grid.reward[s2] + self.v * gain).astype(np.int32)
        d = np.where(won, 1, self.terminal[s2]).astype(np.int32)
        for name, m in (('push', pushed), ('refused_wall', by_wall), ('refused_box', by_box), ('refused_terminal', by_terminal),
                        ('onto_target', gain > 0), ('off_target', gain < 0), ('solved', won & ~solved0), ('absorbing', solved0)):
            self.log[name] += int((m & who).sum())
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        self.cells[who] = cells2[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()


def shortest_solution(grid, box, v, start):
    """(moves, return) of a shortest walk from `start` with the boxes on their initial cells to a SOLVED word: a breadth-first search
    over (cell, word), every move one step of a one-env BoxesOracle; walks that end on a goal or lava cell are not continued.  None
    where the level cannot be solved.  The yardstick of the learning claim."""
    o = BoxesOracle(grid, 0, 1, box, v, q0=None)
    first = (int(start), tuple(int(x) for x in o.init))
    seen = {first: (0, 0)}
    queue = collections.deque([first])
    while queue:
        s, cells = queue.popleft()
        moves, ret = seen[(s, cells)]
        for a in range(4):
            o.state.pos[0], o.cells[0] = s, cells
            obs, r, d = o._move(np.array([a], np.int32))
            nxt = (int(obs[0]), tuple(int(x) for x in o.cells[0]))
            if o.solved()[0]:
                return moves + 1, ret + int(r[0])
            if not d[0] and nxt not in seen:
                seen[nxt] = (moves + 1, ret + int(r[0]))
                queue.append(nxt)
    return None


def greedy_walk(grid, box, v, q, cap=100):
    """(moves, return, solved) of the greedy walk (first maximum) of one table q [S << (b * B), 4] from the grid's first start cell, or
    None where it has not ended after `cap` moves."""
    o = BoxesOracle(grid, 0, 1, box, v, q0=None)
    o.reset()
    total = 0
    for i in range(cap):
        row = int(o.words[0]) * grid.S + int(o.state.pos[0])
        _, r, d = o._move(np.array([int(np.argmax(q[row]))], np.int32))
        total += int(r[0])
        if d[0]:
            return i + 1, total, bool(o.solved()[0])
    return None


# ---- the learning claim (tests/test_boxes_host.py, tests/test_gpu_boxes.py): a 4 x 4 grid, start 4, one box on 5, its target on 10, a
# lava cell on 12 (below the start) as the way out of a deadlock ----
CLAIM = dict(W=4, H=4, starts=[4], goals=[], lava=[12], walls=[])  # (no goal cell: a GridSpec, not a GridUniverseEnv, carries it)
CLAIM_BOXES = dict(boxes=[5], targets=[10], on_target=5)
CLAIM_LEARNERS, CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16 = 64, 0.5, 0.95, 6554  # eps 0.1
CLAIM_WALK = (4, 7, True)  # push right (5 -> 6), up, right, push down (6 -> 10): -1 * 3 + 10
# the budget: with BoxesOracle.td_run all 64 restated Q-learners walk greedily along a shortest solution from 3100 / 2400 / 2800 steps on
# for the seeds 0 / 1 / 2 (61, 61 and 62 of 64 two hundred steps earlier), and stay there at every multiple of 100 up to ten times
# that (31000 / 24000 / 28000).  The largest, doubled: the margin is for seeds not tried
CLAIM_STEPS = 6200


def free_cells(g):
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    return [s for s in range(g['W'] * g['H']) if s not in taken]
