"""CPU restatement of gu_dyna_run (include/gu.h, csrc/gu_dyna.hip): N independent Dyna-Q learners on one grid.  The real step is
tests/_td_oracle.py's Q-learning step (the C oracle moves the envs, its `choose` / `row_max` / `words` pick the actions); the
model and the planning updates are restated here, with the stream-5 words from oracle/gu_rng.py.  Test infrastructure; it imports
oracle/ and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as TD

M32 = 0xFFFFFFFF
STREAM_DYNA = 5


def planning_words(seed, env_ids, c):
    """Stream-5 words of planning draws c (uint64, one per env): counter c & 0xFFFFFFFF, epoch c >> 32."""
    c = np.asarray(c, np.uint64)
    return R.word_v(seed, env_ids, STREAM_DYNA, c & np.uint64(M32), epoch=c >> np.uint64(32))


class DynaOracle(TD.TdOracle):
    """TdOracle plus one model per learner: next / reward / done [n][S][4], list [n][4S] (-1 beyond count) and count [n]."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(DynaOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.clear_model()

    def clear_model(self):
        S = self.grid.S
        self.next = np.full((self.n, S, 4), -1, np.int32)
        self.mreward = np.zeros((self.n, S, 4), np.int32)
        self.mdone = np.zeros((self.n, S, 4), np.int32)
        self.list = np.full((self.n, 4 * S), -1, np.int32)
        self.count = np.zeros(self.n, np.int32)

    def model(self):
        return dict(next=self.next, reward=self.mreward, done=self.mdone, list=self.list, count=self.count)

    def dyna(self, T, P, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma, P = float(alpha), float(gamma), int(P)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            # 1. the real step: gu_td_run's Q-learning step
            d = st.done != 0
            if d.any():
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            t_old = st.tcount.astype(np.uint64)
            act = TD.choose(self.q[idx, s], TD.words(self.seed, self.env_ids, t_old), eps_q16)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * TD.row_max(self.q[idx, s2]))
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            # 2. the model
            new = self.next[idx, s, act] < 0
            self.next[idx, s, act], self.mreward[idx, s, act], self.mdone[idx, s, act] = s2, r, dn
            self.list[idx[new], self.count[new]] = (s * 4 + act)[new]
            self.count += new
            # 3. planning
            for j in range(P):
                c = t_old * np.uint64(P) + np.uint64(j)
                w = planning_words(self.seed, self.env_ids, c).astype(np.uint64)
                k = ((w * self.count.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                p = self.list[idx, k]
                sp, ap = p >> 2, p & 3
                sp2, rp, dp = self.next[idx, sp, ap], self.mreward[idx, sp, ap].astype(np.float64), self.mdone[idx, sp, ap] != 0
                tgt = np.where(dp, rp, rp + gamma * TD.row_max(self.q[idx, sp2]))
                qp = self.q[idx, sp, ap]
                self.q[idx, sp, ap] = qp + alpha * (tgt - qp)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
