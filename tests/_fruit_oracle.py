"""CPU restatement of fruit (include/gu.h: gu_set_fruit; csrc/gu_fruit.hip, csrc/gu_td.hip) in numpy: every move goes through the C
oracle's look_step_ahead (care_about_terminal on) and every reset through its reset, the action words come from oracle/gu_rng.py,
and the learner on (cell, eaten) reuses the epsilon-greedy rule of tests/_td_oracle.py.  Test infrastructure; it imports oracle/
read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from ._start_log import StartLog
from ._td_oracle import Q_LEARNING, SARSA, choose, row_max, words  # noqa: F401  (re-exported for the tests)


def kinds_of(fruit):
    return (np.asarray(fruit, np.int64) >> 5) & 3


class FruitOracle(object):
    """N envs (and learners) on `grid` (a C.Grid) under the fruit plane `fruit` uint8[S] (None: no fruit) with the kinds' `values`."""

    def __init__(self, grid, seed, n, fruit=None, values=(0, 0, 0), env_id0=0, q0=0.0):
        self.grid, self.seed, self.n = grid, int(seed), int(n)
        self.state = C.State(n, env_id0)
        self.state.pos[:] = grid.starts[0]  # where gu_set_grid puts every env
        self.reward = np.zeros(n, np.int32)
        self.env_ids = np.arange(env_id0, env_id0 + n, dtype=np.uint64)
        self.starts = StartLog(grid.starts)  # what the lazy resets drew
        self.q0 = q0
        self.carry = np.full(n, -1, np.int32)
        self.carry_valid = False
        self.q = None
        self.set_fruit(fruit, values)

    def set_fruit(self, fruit, values=(0, 0, 0)):
        """gu_set_fruit: clears every mask; the tables go (back to q0: the caller's gu_td_init) when their row count changes."""
        S = self.grid.S
        self.fruit = np.zeros(S, np.uint8) if fruit is None else np.asarray(fruit, np.uint8).copy()
        self.F = int(np.count_nonzero(self.fruit))
        self.value = np.concatenate([[0], np.asarray(values, np.int64)])  # by kind; kind 0 pays nothing
        self.eaten = np.zeros(self.n, np.uint32)
        self.carry_valid = False
        if self.q0 is not None and (self.q is None or self.q.shape[1] != S << self.F):
            self.q = np.full((self.n, S << self.F, 4), float(self.q0), np.float64)

    def set_eaten(self, eaten, env0=0):
        e = np.atleast_1d(np.asarray(eaten, np.uint32))
        self.eaten[env0:env0 + e.size] = e
        self.carry_valid = False

    def reset(self, mask=None):
        self.carry_valid = False
        took = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.eaten[took] = 0
        return C.reset(self.grid, self.seed, self.state, mask)

    def reset_done(self):
        d = self._lazy_reset()
        self.carry_valid = False
        return d

    def set_state(self, tcount=None):
        self.carry_valid = False
        if tcount is not None:
            self.state.tcount[:] = tcount

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
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        self.eaten[who] |= bit[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()

    def _lazy_reset(self, who=None):
        d = self.state.done != 0
        if who is not None:
            d &= who
        if d.any():
            C.reset(self.grid, self.seed, self.state, d.astype(np.uint8))
            self.starts.note(self.state.pos[d])
            self.eaten[d] = 0
        return d

    def step(self, actions, auto_reset=False):
        """gu_step: envs whose action lies outside -4 .. 3 do not step (nor reset, nor eat); returns (obs, reward, done, rejected)."""
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
        """gu_td_run under fruit: tests/_td_oracle.py's TdOracle.run on the rows eaten * S + s."""
        st, idx, S = self.state, np.arange(self.n), self.grid.S
        alpha, gamma = float(alpha), float(gamma)
        act = self.carry.copy() if (method == SARSA and self.carry_valid) else np.full(self.n, -1, np.int32)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = self._lazy_reset()
            act[d] = -1
            row = self.eaten.astype(np.int64) * S + st.pos
            need = act < 0
            if need.any():
                w = words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, choose(self.q[idx, row], w, eps_q16), act).astype(np.int32)
            s2, r, dn = self._move(act)
            dn = dn != 0
            row2 = self.eaten.astype(np.int64) * S + s2
            nxt = self.q[idx, row2].copy()  # pre-update row of (s', eaten')
            if method == SARSA:
                a2 = choose(nxt, words(self.seed, self.env_ids, st.tcount), eps_q16)
                m = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                m = row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * m)
            qa = self.q[idx, row, act]
            self.q[idx, row, act] = qa + alpha * (target - qa)
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry = act
            self.carry_valid = method == SARSA
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))


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
