"""CPU restatement of fruit (include/gu.h: gu_set_fruit; csrc/gu_fruit.hip, csrc/gu_td.hip) in numpy: every move goes through the C
oracle's look_step_ahead (care_about_terminal on) and every reset through its reset, the action words come from oracle/gu_rng.py,
and the learner on (cell, eaten) reuses the epsilon-greedy rule of tests/_td_oracle.py.  Only the rule is here: the resets,
gu_step's rejected actions, the rollout policies and td_run around it are tests/_overlay_oracle.py's.  Test infrastructure; it
imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C

from ._overlay_oracle import OverlayOracle
from ._td_oracle import Q_LEARNING, SARSA, choose, row_max, words  # noqa: F401  (re-exported for the tests)


def kinds_of(fruit):
    return (np.asarray(fruit, np.int64) >> 5) & 3


class FruitOracle(OverlayOracle):
    """N envs (and learners) on `grid` (a C.Grid) under the fruit plane `fruit` uint8[S] (None: no fruit) with the kinds' `values`.
    The learner's row is eaten * S + cell."""

    def __init__(self, grid, seed, n, fruit=None, values=(0, 0, 0), env_id0=0, q0=0.0):
        super().__init__(grid, seed, n, env_id0, q0)
        self.log = dict(eaten=0)  # fruit eaten
        self.set_fruit(fruit, values)

    def set_fruit(self, fruit, values=(0, 0, 0)):
        """gu_set_fruit: clears every mask; the tables go (back to q0: the caller's gu_td_init) when their row count changes."""
        self.fruit = np.zeros(self.grid.S, np.uint8) if fruit is None else np.asarray(fruit, np.uint8).copy()
        self.F = int(np.count_nonzero(self.fruit))
        self.value = np.concatenate([[0], np.asarray(values, np.int64)])  # by kind; kind 0 pays nothing
        self.eaten = np.zeros(self.n, np.uint32)
        self._installed()

    def set_eaten(self, eaten, env0=0):
        e = np.atleast_1d(np.asarray(eaten, np.uint32))
        self.eaten[env0:env0 + e.size] = e
        self.carry_valid = False

    def _bits(self):
        return self.F

    def _row(self, pos):
        return self.eaten.astype(np.int64) * self.grid.S + pos

    def _restore(self, took, lazy=False):
        self.eaten[took] = 0

    # one move of the envs in `who` (bool[n]) with actions act[n]: rules 2 .. 4 of gu_set_fruit
    def _move(self, act, who=None):
        st = self.state
        who = np.ones(self.n, bool) if who is None else who
        s2, r, d = C.look_step_ahead(self.grid, st.pos.copy(), (np.asarray(act) & 3).astype(np.int32), True)
        c = self.fruit[s2].astype(np.int64)
        kind = (c >> 5) & 3
        bit = np.where(kind != 0, np.int64(1) << (c & 31), 0).astype(np.uint32)
        fresh = (bit & ~self.eaten) != 0
        r = (r + np.where(fresh, self.value[kind], 0)).astype(np.int32)
        self.log['eaten'] += int((fresh & who).sum())
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        self.eaten[who] |= bit[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()


# ---- the learning claim (tests/test_fruit_host.py, tests/test_gpu_fruit.py): a 5 x 3 open grid, start (0, 1), goal (4, 1), a melon
# worth +8 at (2, 0) off the straight path and a lemon worth -8 at (2, 1) on it ----
CLAIM_W, CLAIM_H = 5, 3
CLAIM = dict(W=CLAIM_W, H=CLAIM_H, starts=[1 * CLAIM_W + 0], goals=[1 * CLAIM_W + 4], lava=[], walls=[])
CLAIM_CELLS, CLAIM_KINDS, CLAIM_VALUES = [2, 7], ['melon', 'lemon'], (0, -8, 8)  # cell 2 = (2, 0), cell 7 = (2, 1)
CLAIM_LEARNERS, CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16 = 64, 0.5, 0.95, 6554  # eps 0.1
CLAIM_RETURN = 13  # six moves: -1 * 5 + 8 + 10
# the budget: the smallest multiple of 500 steps at which all 64 restated Q-learners walk greedily to the optimal return for each of
# the seeds 0, 1, 2 (measured with FruitOracle.td_run: 64 / 64 / 64 at 500 steps already)
CLAIM_STEPS = 500


def greedy_walk(grid, fruit, values, q, cap=100):
    """The undiscounted return of the greedy walk (first maximum) of one table q [S << F, 4] from the grid's first start cell."""
    o = FruitOracle(grid, 0, 1, fruit, values, q0=None)
    o.reset()
    total = 0
    for _ in range(cap):
        row = int(o.eaten[0]) * grid.S + int(o.state.pos[0])
        _, r, d = o._move(np.array([int(np.argmax(q[row]))], np.int32))
        total += int(r[0])
        if d[0]:
            return total
    return None
