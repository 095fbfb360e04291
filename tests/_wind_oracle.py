"""CPU restatement of wind (include/gu.h: gu_set_wind; csrc/gu_wind.hip, csrc/gu_td.hip) in numpy: every sub-move of a windy step goes
through the C oracle's look_step_ahead (care_about_terminal on), the gust words come from oracle/gu_rng.py (stream 9), and the windy
TD learner reuses the epsilon-greedy rule of tests/_td_oracle.py.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from ._start_log import StartLog
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


class WindOracle(object):
    """N envs (and learners) on `grid` (a C.Grid) under the wind plane `wind` uint8[S] (None: calm) with gust probability gust_q16."""

    def __init__(self, grid, seed, n, wind=None, gust_q16=0, env_id0=0, q0=0.0):
        self.grid, self.seed, self.n = grid, int(seed), int(n)
        self.state = C.State(n, env_id0)
        self.state.pos[:] = grid.starts[0]  # where gu_set_grid puts every env
        self.reward = np.zeros(n, np.int32)
        self.env_ids = np.arange(env_id0, env_id0 + n, dtype=np.uint64)
        self.starts = StartLog(grid.starts)  # what the lazy resets drew
        self.q = None if q0 is None else np.full((n, grid.S, 4), float(q0), np.float64)  # (None: no learners, no tables)
        self.carry = np.full(n, -1, np.int32)
        self.carry_valid = False
        self.set_wind(wind, gust_q16)

    def set_wind(self, wind, gust_q16=0):
        self.wind = np.zeros(self.grid.S, np.uint8) if wind is None else np.asarray(wind, np.uint8).copy()
        self.gust_q16 = int(gust_q16) if wind is not None else 0
        self.carry_valid = False

    def reset(self, mask=None):
        self.carry_valid = False
        return C.reset(self.grid, self.seed, self.state, mask)

    def reset_done(self):
        d = self._lazy_reset()
        self.carry_valid = False
        return d

    def set_state(self, tcount=None):
        self.carry_valid = False
        if tcount is not None:
            self.state.tcount[:] = tcount

    # one windy move of the envs in `who` (bool[n]) with actions act[n]: rules 1 .. 5 of gu_set_wind
    def _move(self, act, who=None):
        st = self.state
        who = np.ones(self.n, bool) if who is None else who
        s = st.pos.copy()
        c = self.wind[s].astype(np.int64)
        k = (c >> 2) & 3
        if self.gust_q16:
            k = gusted(k, gust_words(self.seed, self.env_ids, st.tcount), self.gust_q16)
        s2, r, d = push(self.grid, s, (np.asarray(act) & 3).astype(np.int32), k, (c & 3).astype(np.int32))
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()

    def _lazy_reset(self, who=None):
        d = self.state.done != 0
        if who is not None:
            d &= who
        if d.any():
            C.reset(self.grid, self.seed, self.state, d.astype(np.uint8))
            self.starts.note(self.state.pos[d])
        return d

    def step(self, actions, auto_reset=False):
        """gu_step: envs whose action lies outside -4 .. 3 do not step (nor reset, nor draw); returns (obs, reward, done, rejected)."""
        self.carry_valid = False
        a = np.asarray(actions, np.int64)
        ok = (a >= -4) & (a <= 3)
        if auto_reset:
            self._lazy_reset(ok)
        obs, rew, don = self._move(np.where(ok, a, 0), ok)
        return obs, rew, don, ~ok

    def rollout(self, T, policy='uniform', auto_reset=True, actions=None, pi=None):
        """gu_rollout: rows [T, n], statistics and the state left behind."""
        self.carry_valid = False
        st = self.state
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            if auto_reset:
                self._lazy_reset()
            s = st.pos
            if policy == 'uniform':
                act = R.actions_v(self.seed, self.env_ids, st.tcount)
            elif policy == 'stream':
                act = np.asarray(actions[i], np.int32)
            elif policy == 'greedy':
                act = np.argmax(pi[s], axis=1).astype(np.int32)
            else:
                act = np.array([R.sampled_action(self.seed, int(e), int(t), pi[int(c)]) for e, t, c in zip(self.env_ids, st.tcount, s)], np.int32)
            obs[i], rew[i], don[i] = self._move(act)
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=(don != 0).sum(axis=0).astype(np.int32))

    def td_run(self, T, method, alpha, gamma, eps_q16):
        """gu_td_run under wind: tests/_td_oracle.py's TdOracle.run with the windy move."""
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        act = self.carry.copy() if (method == SARSA and self.carry_valid) else np.full(self.n, -1, np.int32)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = self._lazy_reset()
            act[d] = -1
            s = st.pos.copy()
            need = act < 0
            if need.any():
                w = words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, choose(self.q[idx, s], w, eps_q16), act).astype(np.int32)
            s2, r, dn = self._move(act)
            dn = dn != 0
            nxt = self.q[idx, s2].copy()  # pre-update row of s'
            if method == SARSA:
                a2 = choose(nxt, words(self.seed, self.env_ids, st.tcount), eps_q16)
                m = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                m = row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * m)
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry = act
            self.carry_valid = method == SARSA
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
