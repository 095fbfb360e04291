"""CPU restatement of gu_reinforce_run (include/gu.h, csrc/gu_reinforce.hip): N independent REINFORCE-with-baseline learners on one
grid, written from the header's rules on top of tests/_ac_oracle.py (env state, tables, the build's exp and softmax).  Learners
are independent, so the backward passes of all learners whose segments end on the same step run together, entry by entry: one
vector operation per entry age instead of one Python loop per learner.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _ac_oracle as AC
from . import _td_oracle as TD

REINFORCE_MAX = 1024  # GU_REINFORCE_MAX


class ReinforceOracle(AC.AcOracle):
    """AcOracle plus the episode buffers: buf_sa / buf_r [n][REINFORCE_MAX] (s*4+a and r, oldest first; -1 / 0 beyond the
    count), buf_cnt [n], and buf_L, the L of the last call that touched the envs if it was a `reinforce`, else 0 (dropped)."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0, h0=0.0, v0=0.0):
        super(ReinforceOracle, self).__init__(grid, seed, n, env_id0, q0, h0, v0)
        self.buf_sa = np.full((self.n, REINFORCE_MAX), -1, np.int32)
        self.buf_r = np.zeros((self.n, REINFORCE_MAX), np.int32)
        self.buf_cnt = np.zeros(self.n, np.int32)
        self.buf_L = 0

    def drop_buffer(self):
        """What every other call that touches the envs or the tables does to the buffer."""
        self.buf_sa[:] = -1
        self.buf_r[:] = 0
        self.buf_cnt[:] = 0
        self.buf_L = 0

    # every inherited call that touches the envs or the tables drops the buffer
    def reset(self, mask=None):
        self.drop_buffer()
        return super(ReinforceOracle, self).reset(mask)

    def rollout(self, T, **kw):
        self.drop_buffer()
        return super(ReinforceOracle, self).rollout(T, **kw)

    def set_state(self, tcount=None):
        self.drop_buffer()
        super(ReinforceOracle, self).set_state(tcount)

    def set_q(self, q, env0=0):
        self.drop_buffer()
        super(ReinforceOracle, self).set_q(q, env0)

    def set_ac(self, h=None, v=None, env0=0):
        self.drop_buffer()
        super(ReinforceOracle, self).set_ac(h, v, env0)

    def run(self, T, method, alpha, gamma, eps_q16):
        if T > 0:
            self.drop_buffer()
        return super(ReinforceOracle, self).run(T, method, alpha, gamma, eps_q16)

    def ac(self, T, alpha_actor, alpha_critic, gamma):
        if T > 0:
            self.drop_buffer()
        return super(ReinforceOracle, self).ac(T, alpha_actor, alpha_critic, gamma)

    def _backward(self, who, G, aa, ab, gamma):
        """Rule 5 for the learners `who` (distinct), G [len(who)] the start of their returns: entry by entry, newest first."""
        cnt = self.buf_cnt[who].copy()
        for j in range(int(cnt.max())):
            live = cnt > j
            e, k = who[live], cnt[live] - 1 - j
            sa, r = self.buf_sa[e, k], self.buf_r[e, k]
            s, a = sa >> 2, sa & 3
            g_ret = r.astype(np.float64) + gamma * G[live]
            G[live] = g_ret
            vs = self.v[e, s]
            delta = g_ret - vs
            self.v[e, s] = vs + ab * delta
            h = self.h[e, s]
            pi = AC.softmax(h)[2]  # H as it is now: earlier entries of this pass included
            g = aa * delta
            ind = (np.arange(4)[None, :] == a[:, None]).astype(np.float64)
            self.h[e, s] = h + g[:, None] * (ind - pi)
        self.buf_sa[who] = -1
        self.buf_r[who] = 0
        self.buf_cnt[who] = 0

    def reinforce(self, T, L, alpha_actor, alpha_baseline, gamma):
        st, idx = self.state, np.arange(self.n)
        aa, ab, gamma, L = float(alpha_actor), float(alpha_baseline), float(gamma), int(L)
        assert 1 <= L <= REINFORCE_MAX
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        if T > 0 and self.buf_L != L:  # (a launch of zero steps changes nothing)
            self.drop_buffer()
        for i in range(T):
            d = st.done != 0
            if d.any():  # 1. lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            e, Z, _ = AC.softmax(self.h[idx, s])  # 2. policy and action
            a = AC.action(e, Z, TD.words(self.seed, self.env_ids, st.tcount))
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=a[None, :])  # 3. move, t += 1, append
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            self.buf_sa[idx, self.buf_cnt] = s * 4 + a
            self.buf_r[idx, self.buf_cnt] = r
            self.buf_cnt += 1
            end = dn | (self.buf_cnt == L)  # 4.
            if end.any():  # 5. segment end
                who = np.flatnonzero(end)
                G = np.where(dn[who], 0.0, self.v[who, s2[who]])
                self._backward(who, G, aa, ab, gamma)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False  # gu_reinforce_run ends gu_td_run's SARSA carry
            self.buf_L = L
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
