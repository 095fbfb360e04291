"""What the CPU restatements of the overlays (tests/_wind_oracle.py, _fruit_oracle.py, _doors_oracle.py, _boxes_oracle.py) share: the
envs and their start log, every reset path, gu_step's rejected actions, the rollout policies and the TD learner with its SARSA
carry.  None of this belongs to a kind's rule.  A kind supplies `_move` (its rule), `_row` (the learner's row of every env), `_bits`
(the state bits in a row index) and `_restore` (the per-env state of the envs a reset takes), and calls `_installed` from its set_*.
Resets go through the C oracle's reset, the action words come from oracle/gu_rng.py, and the learner reuses the epsilon-greedy rule
of tests/_td_oracle.py.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from ._start_log import StartLog
from ._td_oracle import SARSA, choose, row_max, words


class OverlayOracle(object):
    """N envs (and learners) on `grid` (a C.Grid), the first the global env id env_id0.  q0 None: no learners, no tables."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
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

    # ---- what a kind supplies ----
    def _move(self, act, who=None):
        """One move of the envs in `who` (bool[n]) with actions act[n]: (pos, reward, done) of every env afterwards."""
        raise NotImplementedError

    def _row(self, pos):
        """The learner's row of every env when it stands on pos[n]."""
        raise NotImplementedError

    def _bits(self):
        """The bits of per-env state in a row index: the tables have S << bits rows."""
        raise NotImplementedError

    def _restore(self, took, lazy=False):
        """The per-env state of the envs a reset took (bool[n]); lazy: the reset that a step, rollout or learner makes by itself."""

    def _installed(self):
        """The end of every set_<plane>: the carry goes; the tables go (back to q0: the caller's gu_td_init) when their row count changes."""
        self.carry_valid = False
        rows = self.grid.S << self._bits()
        if self.q0 is not None and (self.q is None or self.q.shape[1] != rows):
            self.q = np.full((self.n, rows, 4), float(self.q0), np.float64)

    # ---- the frame ----
    def reset(self, mask=None):
        self.carry_valid = False
        self._restore(np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0)
        return C.reset(self.grid, self.seed, self.state, mask)

    def reset_done(self):
        d = self._lazy_reset()
        self.carry_valid = False
        return d

    def set_state(self, tcount=None):
        self.carry_valid = False
        if tcount is not None:
            self.state.tcount[:] = tcount

    def _lazy_reset(self, who=None):
        d = self.state.done != 0
        if who is not None:
            d &= who
        if d.any():
            C.reset(self.grid, self.seed, self.state, d.astype(np.uint8))
            self.starts.note(self.state.pos[d])
            self._restore(d, lazy=True)
        return d

    def step(self, actions, auto_reset=False):
        """gu_step: envs whose action lies outside -4 .. 3 do not step (nor reset, nor draw, nor touch their overlay state); returns
        (obs, reward, done, rejected)."""
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
        """gu_td_run under an overlay: tests/_td_oracle.py's TdOracle.run with the kind's move, on the kind's rows."""
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        act = self.carry.copy() if (method == SARSA and self.carry_valid) else np.full(self.n, -1, np.int32)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = self._lazy_reset()
            act[d] = -1
            row = self._row(st.pos)
            need = act < 0
            if need.any():
                w = words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, choose(self.q[idx, row], w, eps_q16), act).astype(np.int32)
            s2, r, dn = self._move(act)
            dn = dn != 0
            nxt = self.q[idx, self._row(s2)].copy()  # pre-update row of s' (and of the overlay state after the move)
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
