"""CPU restatement of gu_is_run (include/gu.h, csrc/gu_is.hip): N independent off-policy every-visit Monte-Carlo control learners
with weighted importance sampling on one grid, written from the header's rules on top of tests/_td_oracle.py (env state, Q
tables, the behaviour policy's words and tie rule).  Learners are independent, so the backward passes of all learners whose
segments end on the same step run together, entry by entry, the ones whose pass has ended dropping out.  The reciprocal is
written 1.0 / x.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _td_oracle as TD

IS_MAX = 1024  # GU_IS_MAX
W_MIN = 2.0 ** -256


def ratio_table(eps_q16):
    """R[m][c], m = 0 .. 4 (row 0 unused, zeros), c = 0 .. 4: the header's formulas, one rounding per operation."""
    eps = int(eps_q16) / 65536.0
    R = np.zeros((5, 5), np.float64)
    for c in range(5):
        b = eps * 0.25 if c == 0 else (1.0 - eps) / c + eps * 0.25
        for m in range(1, 5):
            R[m][c] = 0.0 if b == 0 else (1.0 / m) / b
    return R


class IsOracle(TD.TdOracle):
    """TdOracle plus the cumulative weights c [n][S][4] and the episode buffers: buf_sa / buf_r / buf_c [n][IS_MAX] (s*4+a, r and
    the class of the action, oldest first; -1 / 0 / 0 beyond the count), buf_cnt [n], and buf_L, the L of the last call that
    touched the envs if it was an `is_run`, else 0 (dropped).  walked / passes count the entries learned from and the passes,
    cap_eq / cap_gt / low the passes that the weight window ended and on which side."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(IsOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.c = np.zeros((self.n, grid.S, 4), np.float64)
        self.buf_sa = np.full((self.n, IS_MAX), -1, np.int32)
        self.buf_r = np.zeros((self.n, IS_MAX), np.int32)
        self.buf_c = np.zeros((self.n, IS_MAX), np.int32)
        self.buf_cnt = np.zeros(self.n, np.int32)
        self.buf_L = 0
        self.walked = self.passes = 0
        self.cap_eq = self.cap_gt = self.low = 0  # passes ended on a greedy entry by W == w_cap, by W > w_cap, by W < 2^-256

    def drop_buffer(self):
        """What every other call that touches the envs or the tables does to the buffer."""
        self.buf_sa[:] = -1
        self.buf_r[:] = 0
        self.buf_c[:] = 0
        self.buf_cnt[:] = 0
        self.buf_L = 0

    # every inherited call that touches the envs or the tables drops the buffer
    def reset(self, mask=None):
        self.drop_buffer()
        return super(IsOracle, self).reset(mask)

    def rollout(self, T, **kw):
        self.drop_buffer()
        return super(IsOracle, self).rollout(T, **kw)

    def set_state(self, tcount=None):
        self.drop_buffer()
        super(IsOracle, self).set_state(tcount)

    def set_q(self, q, env0=0):
        self.drop_buffer()
        super(IsOracle, self).set_q(q, env0)

    def set_c(self, c, env0=0):
        self.drop_buffer()
        c = np.asarray(c, np.float64)
        self.c[env0:env0 + len(c)] = c

    def run(self, T, method, alpha, gamma, eps_q16):
        if T > 0:
            self.drop_buffer()
        return super(IsOracle, self).run(T, method, alpha, gamma, eps_q16)

    def _backward(self, who, G, gamma, R, w_cap):
        """Rule 5 for the learners `who` (distinct), G [len(who)] the start of their returns: entry by entry, newest first."""
        cnt = self.buf_cnt[who].copy()
        W = np.ones(len(who), np.float64)
        alive = np.ones(len(who), bool)
        self.passes += len(who)
        for j in range(int(cnt.max())):
            live = alive & (cnt > j)
            if not live.any():
                break
            self.walked += int(live.sum())
            e, k = who[live], cnt[live] - 1 - j
            sa, r, cl = self.buf_sa[e, k], self.buf_r[e, k], self.buf_c[e, k]
            s, a = sa >> 2, sa & 3
            g = r.astype(np.float64) + gamma * G[live]
            G[live] = g
            cc = self.c[e, s, a] + W[live]
            self.c[e, s, a] = cc
            qa = self.q[e, s, a]
            qa = qa + (W[live] * (1.0 / cc)) * (g - qa)
            self.q[e, s, a] = qa
            row = self.q[e, s]  # the row as it is now
            mx = TD.row_max(row)
            m_now = (row == mx[:, None]).sum(axis=1)
            Wn = W[live] * R[m_now, cl]
            W[live] = Wn
            greedy = qa == mx
            self.cap_eq += int((greedy & (Wn == w_cap)).sum())
            self.cap_gt += int((greedy & (Wn > w_cap)).sum())
            self.low += int((greedy & (Wn < W_MIN)).sum())
            alive[live] = greedy & (Wn >= W_MIN) & (Wn < w_cap)
        self.buf_sa[who] = -1
        self.buf_r[who] = 0
        self.buf_c[who] = 0
        self.buf_cnt[who] = 0

    def is_run(self, T, L, gamma, eps_q16, w_cap):
        st, idx = self.state, np.arange(self.n)
        gamma, L, w_cap = float(gamma), int(L), float(w_cap)
        assert 1 <= L <= IS_MAX and 1.0 <= w_cap <= 2.0 ** 256
        R = ratio_table(eps_q16)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        if T > 0 and self.buf_L != L:  # (a launch of zero steps changes nothing)
            self.drop_buffer()
        for i in range(T):
            d = st.done != 0
            if d.any():  # 1. lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            row = self.q[idx, s]  # 2. behaviour action and its class
            a = TD.choose(row, TD.words(self.seed, self.env_ids, st.tcount), eps_q16)
            mx = TD.row_max(row)
            cl = np.where(row[idx, a] == mx, (row == mx[:, None]).sum(axis=1), 0).astype(np.int32)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=a[None, :])  # 3. move, t += 1, append
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            self.buf_sa[idx, self.buf_cnt] = s * 4 + a
            self.buf_r[idx, self.buf_cnt] = r
            self.buf_c[idx, self.buf_cnt] = cl
            self.buf_cnt += 1
            end = dn | (self.buf_cnt == L)  # 4.
            if end.any():  # 5. segment end
                who = np.flatnonzero(end)
                G = np.where(dn[who], 0.0, TD.row_max(self.q[who, s2[who]]))
                self._backward(who, G, gamma, R, w_cap)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False  # gu_is_run ends gu_td_run's SARSA carry
            self.buf_L = L
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
