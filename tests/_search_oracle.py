"""CPU restatement of gu_search_run (include/gu.h, csrc/gu_search.hip): N independent learners on one grid that choose every
non-exploring real action by M simulated rollouts per action, of depth D, and learn from the real transition by Q-learning.  The
real step is tests/_td_oracle.py's (the C oracle moves the envs, its `choose` / `row_max` / `words` pick the actions); the
rollouts are restated here, simulated with oracle.c_oracle.look_step_ahead and drawing the stream-6 words with oracle/gu_rng.py.
Test infrastructure; it imports oracle/ and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as TD

M32 = 0xFFFFFFFF
STREAM_SEARCH = 6


def sim_words(seed, env_ids, c):
    """Stream-6 words of simulated moves c (uint64, one per env): counter c & 0xFFFFFFFF, epoch c >> 32."""
    c = np.asarray(c, np.uint64)
    return R.word_v(seed, env_ids, STREAM_SEARCH, c & np.uint64(M32), epoch=c >> np.uint64(32))


class SearchOracle(TD.TdOracle):
    """TdOracle plus, per learner, the score row of its most recent searched iteration and the simulated moves of the last launch."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(SearchOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.score = np.zeros((self.n, 4), np.float64)
        self.sim_steps = np.zeros(self.n, np.int64)

    def _scores(self, ids, s, t, M, D, gamma, eps_sim_q16):
        """The score rows [k, 4] of the learners `ids` standing in s at step counts t (uint64); counts their simulated moves."""
        k = len(ids)
        env_ids = self.env_ids[ids]
        score = np.zeros((k, 4), np.float64)
        with np.errstate(over='ignore'):
            for b in range(4):
                s1, r1, d1 = C.look_step_ahead(self.grid, s, np.full(k, b, np.int32), True)
                for j in range(M):
                    G, disc, x, dn = r1.astype(np.float64), np.full(k, gamma, np.float64), s1.copy(), d1 != 0
                    base = ((t * np.uint64(4) + np.uint64(b)) * np.uint64(M) + np.uint64(j)) * np.uint64(D)  # (wraps)
                    for i in range(D):
                        li = np.flatnonzero(~dn)
                        if li.size == 0:
                            break
                        w = sim_words(self.seed, env_ids[li], base[li] + np.uint64(i))
                        u = TD.choose(self.q[ids[li], x[li]], w, eps_sim_q16)
                        x2, r2, d2 = C.look_step_ahead(self.grid, x[li], u, True)
                        G[li] = G[li] + disc[li] * r2.astype(np.float64)
                        disc[li] = disc[li] * gamma
                        x[li], dn[li] = x2, d2 != 0
                        self.sim_steps[ids[li]] += 1
                    li = np.flatnonzero(~dn)
                    G[li] = G[li] + disc[li] * TD.row_max(self.q[ids[li], x[li]])
                    score[:, b] = G if j == 0 else score[:, b] + G
        return score

    def search(self, T, M, D, alpha, gamma, eps_q16, eps_sim_q16=65536):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma, M, D = float(alpha), float(gamma), int(M), int(D)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        if T > 0:
            self.sim_steps[:] = 0
        for i in range(T):
            # 1. lazy auto-reset
            d = st.done != 0
            if d.any():
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            # 2. the real-step word
            t = st.tcount.astype(np.uint64)
            w = TD.words(self.seed, self.env_ids, t)
            # 3. the action: exploring (and every M = 0) learner by rule 2 of gu_td_run, the others by search
            act = TD.choose(self.q[idx, s], w, eps_q16)
            if M > 0:
                ids = np.flatnonzero((w.astype(np.int64) >> 16) >= int(eps_q16))
                if ids.size:
                    sc = self._scores(ids, s[ids], t[ids], M, D, gamma, eps_sim_q16)
                    self.score[ids] = sc
                    act[ids] = TD.choose(sc, w[ids], eps_q16)
            # 4. the move
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            # 5. the Q-learning update
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * TD.row_max(self.q[idx, s2]))
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
