"""CPU restatement of gu_fa_run (include/gu.h, csrc/gu_fa.hip): N independent epsilon-greedy semi-gradient SARSA / Q-learning
learners over K active binary features per state, on the pieces of tests/_td_oracle.py (the stream-4 words, the epsilon-greedy
choice, the row maximum, the C oracle stepped one step per call).  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _td_oracle as O

Q_LEARNING, SARSA = O.Q_LEARNING, O.SARSA


class FaOracle(O.TdOracle):
    """N learners on `grid` with the shared feature table phi [S][K] (0 <= phi < F) and weights w [N][F][4] of w0."""

    def __init__(self, grid, seed, n, phi, F, w0=0.0, env_id0=0):
        O.TdOracle.__init__(self, grid, seed, n, env_id0)
        self.q = None  # (the action values are computed: q_tables())
        self.set_features(phi, F, w0)

    def set_features(self, phi, F, w0=0.0):
        """gu_fa_init: another table, fresh weights, no carried action."""
        phi = np.asarray(phi, np.int32)
        self.phi = phi[:, None] if phi.ndim == 1 else phi
        assert self.phi.shape[0] == self.grid.S
        self.K, self.F = self.phi.shape[1], int(F)
        self.w = np.full((self.n, self.F, 4), float(w0), np.float64)
        self.carry_valid = False

    def set_w(self, w, env0=0):
        self.carry_valid = False
        w = np.asarray(w, np.float64)
        self.w[env0:env0 + len(w)] = w

    def other_learner(self):
        """A run of any other learner on the engine ends the carry."""
        self.carry_valid = False

    def rows(self, s):
        """Q_e(s[e]) for every learner e: row phi[s][0], then + row phi[s][k] in column order, one rounded add each."""
        idx = np.arange(self.n)
        acc = self.w[idx, self.phi[s, 0]].copy()
        for k in range(1, self.K):
            acc = acc + self.w[idx, self.phi[s, k]]
        return acc

    def q_tables(self):
        """[N][S][4]: what gu_fa_get_q folds."""
        acc = self.w[:, self.phi[:, 0]].copy()
        for k in range(1, self.K):
            acc = acc + self.w[:, self.phi[:, k]]
        return acc

    def run(self, T, method, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        act = self.carry.copy() if (method == SARSA and self.carry_valid) else np.full(self.n, -1, np.int32)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = st.done != 0
            if d.any():  # lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
                act[d] = -1
            s = st.pos.copy()
            cur = self.rows(s)
            need = act < 0
            if need.any():
                w = O.words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, O.choose(cur, w, eps_q16), act).astype(np.int32)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            nxt = self.rows(s2)  # from the weights before this step's update
            if method == SARSA:
                a2 = O.choose(nxt, O.words(self.seed, self.env_ids, st.tcount), eps_q16)
                m = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                m = O.row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * m)
            g = alpha * (target - cur[idx, act])
            for k in range(self.K):
                f = self.phi[s, k]
                self.w[idx, f, act] = self.w[idx, f, act] + g
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:  # (a launch of zero steps changes nothing)
            self.carry = act
            self.carry_valid = method == SARSA
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
