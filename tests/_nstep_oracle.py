"""CPU restatement of gu_nstep_run (include/gu.h, csrc/gu_nstep.hip): N independent n-step Q-learning / SARSA learners on one
grid, stepped through the C oracle like tests/_td_oracle.py and reusing its `choose`, `words` and `row_max`.  The window of env e
is win_sa[e, :count[e]] / win_r[e, :count[e]], oldest first.  Test infrastructure; it imports oracle/ and tests/_td_oracle.py
read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _td_oracle as TD

NSTEP_MAX = 16


class NstepOracle(TD.TdOracle):
    """TdOracle plus one window per learner and the carry rule of gu_nstep_run."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(NstepOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.win_sa = np.full((self.n, NSTEP_MAX), -1, np.int32)
        self.win_r = np.zeros((self.n, NSTEP_MAX), np.int32)
        self.count = np.zeros(self.n, np.int32)
        self.key = None  # (method, n) of the last call if it was an n-step run, else None: the window is dropped

    def drop(self):
        self.key = None
        self.win_sa[:] = -1
        self.win_r[:] = 0
        self.count[:] = 0

    def window(self):
        return dict(sa=self.win_sa, reward=self.win_r, count=self.count)

    # every other call that touches the envs drops the window (and, through TdOracle, SARSA's a')
    def reset(self, mask=None):
        self.drop()
        return super(NstepOracle, self).reset(mask)

    def rollout(self, T, **kw):
        self.drop()
        return super(NstepOracle, self).rollout(T, **kw)

    def set_state(self, tcount=None):
        self.drop()
        super(NstepOracle, self).set_state(tcount)

    def set_q(self, q, env0=0):
        self.drop()
        super(NstepOracle, self).set_q(q, env0)

    def run(self, T, method, alpha, gamma, eps_q16):
        if T > 0:
            self.drop()
        return super(NstepOracle, self).run(T, method, alpha, gamma, eps_q16)

    def _update(self, envs, sa, G, alpha):
        """Q[e][s][a] += alpha * (G - Q[e][s][a]) for distinct envs e (one pair each)."""
        s, a = sa >> 2, sa & 3
        qa = self.q[envs, s, a]
        self.q[envs, s, a] = qa + alpha * (G - qa)

    def nstep(self, T, method, n, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma, n = float(alpha), float(gamma), int(n)
        assert 1 <= n <= NSTEP_MAX
        if T == 0:
            return dict(obs=np.empty((0, self.n), np.int32), reward=np.empty((0, self.n), np.int32),
                        done=np.empty((0, self.n), np.int32), ret=np.zeros(self.n, np.int64), episodes=np.zeros(self.n, np.int32))
        if self.key != (method, n):
            self.drop()
            act = np.full(self.n, -1, np.int32)
        else:
            act = self.carry.copy() if method == TD.SARSA else np.full(self.n, -1, np.int32)
        ws, wr, cnt = self.win_sa, self.win_r, self.count
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = st.done != 0
            if d.any():  # 1. lazy auto-reset
                assert (cnt[d] == 0).all()
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
                act[d] = -1
            s = st.pos.copy()
            need = act < 0
            if need.any():  # 2. action
                w = TD.words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, TD.choose(self.q[idx, s], w, eps_q16), act).astype(np.int32)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])  # 3. move, t += 1
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            ws[idx, cnt] = s * 4 + act
            wr[idx, cnt] = r
            cnt += 1
            nxt = self.q[idx, s2].copy()  # pre-update row of s'
            if method == TD.SARSA:
                a2 = TD.choose(nxt, TD.words(self.seed, self.env_ids, st.tcount), eps_q16)
                B = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                B = TD.row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            full = idx[~dn & (cnt == n)]
            if len(full):  # 4. the n-step update of the oldest entry, then drop it
                G = B[full]
                for k in range(n - 1, -1, -1):
                    G = wr[full, k].astype(np.float64) + gamma * G
                self._update(full, ws[full, 0], G, alpha)
                ws[full, :-1], wr[full, :-1] = ws[full, 1:], wr[full, 1:]
                cnt[full] -= 1
            if dn.any():  # 5. flush, oldest first, each update reading the table the ones before it left
                for j in range(int(cnt[dn].max())):
                    m = idx[dn & (cnt > j)]
                    G = wr[m, cnt[m] - 1].astype(np.float64)  # the newest: G = r
                    for k in range(NSTEP_MAX - 2, j - 1, -1):
                        G = np.where(k < cnt[m] - 1, wr[m, k].astype(np.float64) + gamma * G, G)
                    self._update(m, ws[m, j], G, alpha)
                cnt[dn] = 0
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        slot = np.arange(NSTEP_MAX)[None, :]
        ws[:] = np.where(slot < cnt[:, None], ws, -1)
        wr[:] = np.where(slot < cnt[:, None], wr, 0)
        self.carry = act
        self.carry_valid = False  # gu_nstep_run ends gu_td_run's SARSA carry
        self.key = (method, n)
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
