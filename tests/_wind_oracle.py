"""CPU restatement of wind (include/gu.h: gu_set_wind; csrc/gu_wind.hip, csrc/gu_td.hip) in numpy: every sub-move of a windy step goes
through the C oracle's look_step_ahead (care_about_terminal on), the gust words come from oracle/gu_rng.py (stream 9), and the windy
TD learner reuses the epsilon-greedy rule of tests/_td_oracle.py.  Only the rule is here: the resets, gu_step's rejected actions,
the rollout policies and td_run around it are tests/_overlay_oracle.py's.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from ._overlay_oracle import OverlayOracle
from ._td_oracle import Q_LEARNING, SARSA, choose, row_max, words  # noqa: F401  (re-exported for the tests)

M32 = 0xFFFFFFFF
GUST_THIRDS = 43691  # round(2 / 3 * 65536): one third each for k - 1, k and k + 1 (Sutton & Barto, Exercise 6.10)

# Sutton & Barto's windy gridworld (Example 6.5): 10 x 7, the columns' upward strengths, start (0, 3), goal (7, 3)
BOOK_W, BOOK_H = 10, 7
BOOK_STRENGTH = np.array([0, 0, 0, 1, 1, 1, 2, 2, 1, 0])
BOOK = dict(W=BOOK_W, H=BOOK_H, starts=[3 * BOOK_W + 0], goals=[3 * BOOK_W + 7], lava=[], walls=[])


def gust_words(seed, env_ids, t):
    """The stream-9 words of global env ids `env_ids` at 64-bit step counts `t`."""
    t = np.asarray(t, np.uint64)
    return R.word_v(seed, env_ids, 9, t & np.uint64(M32), epoch=t >> np.uint64(32))


def gusted(k, w, gust_q16):
    """The strengths k after the gust test on the words w: k > 0 becomes k + 1 or k - 1 where (w >> 16) < gust_q16."""
    k = np.asarray(k, np.int64)
    w = np.asarray(w).astype(np.int64)
    hit = (k > 0) & ((w >> 16) < int(gust_q16))
    return np.where(hit, np.where((w & 1) == 1, k + 1, k - 1), k)


def push(grid, s, act, k, direction):
    """move(s, act), then k[i] times move(., direction[i]): (cell, reward, done) of where every agent ends."""
    s1, r, d = C.look_step_ahead(grid, s, act, True)
    k = np.asarray(k, np.int64)
    for j in range(4):
        todo = k > j
        if not todo.any():
            break
        n1, nr, nd = C.look_step_ahead(grid, s1, direction, True)
        s1, r, d = np.where(todo, n1, s1).astype(np.int32), np.where(todo, nr, r).astype(np.int32), np.where(todo, nd, d).astype(np.int32)
    return s1, r, d


def outcomes(grid, wind, s, a, gusts):
    """The cells one step with action a can lead to from cell s: one without gusts, up to three with."""
    c = int(wind[s])
    k = (c >> 2) & 3
    ks = {k} if (not gusts or k == 0) else {k - 1, k, k + 1}
    one = lambda x: np.array([x], np.int32)  # noqa: E731
    return {int(push(grid, one(s), one(a), one(kk), one(c & 3))[0][0]) for kk in ks}


def bfs(grid, wind, start, gusts=False):
    """Breadth-first search over `outcomes` from `start`: {cell: fewest moves}."""
    dist, frontier = {int(start): 0}, [int(start)]
    while frontier:
        nxt = []
        for s in frontier:
            for a in range(4):
                for s2 in outcomes(grid, wind, s, a, gusts):
                    if s2 not in dist:
                        dist[s2] = dist[s] + 1
                        nxt.append(s2)
        frontier = nxt
    return dist


class WindOracle(OverlayOracle):
    """N envs (and learners) on `grid` (a C.Grid) under the wind plane `wind` uint8[S] (None: calm) with gust probability gust_q16.
    Wind keeps no state per env: the learner's row is the cell, and the tables keep their grid.S rows through every set_wind."""

    def __init__(self, grid, seed, n, wind=None, gust_q16=0, env_id0=0, q0=0.0):
        super().__init__(grid, seed, n, env_id0, q0)
        self.log = dict(gust_moved=0)  # moves that a gust ended on another cell than the cell's own strength would
        self.set_wind(wind, gust_q16)

    def set_wind(self, wind, gust_q16=0):
        self.wind = np.zeros(self.grid.S, np.uint8) if wind is None else np.asarray(wind, np.uint8).copy()
        self.gust_q16 = int(gust_q16) if wind is not None else 0
        self._installed()

    def _bits(self):
        return 0

    def _row(self, pos):
        return pos.copy()

    # one windy move of the envs in `who` (bool[n]) with actions act[n]: rules 1 .. 5 of gu_set_wind
    def _move(self, act, who=None):
        st = self.state
        who = np.ones(self.n, bool) if who is None else who
        s = st.pos.copy()
        c = self.wind[s].astype(np.int64)
        k = k0 = (c >> 2) & 3
        if self.gust_q16:
            k = gusted(k, gust_words(self.seed, self.env_ids, st.tcount), self.gust_q16)
        a, direction = (np.asarray(act) & 3).astype(np.int32), (c & 3).astype(np.int32)
        s2, r, d = push(self.grid, s, a, k, direction)
        if self.gust_q16:
            self.log['gust_moved'] += int(((s2 != push(self.grid, s, a, k0, direction)[0]) & who).sum())
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()
