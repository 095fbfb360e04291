"""CPU restatement of gu_explore_run (include/gu.h, csrc/gu_explore.hip): N independent Q-learners on one grid that keep visit
counts and choose every non-exploring action greedily on Q + bonus (UCB) or Q + bonus * noise (Thompson), the bonus from the
counts and the two host tables U and B.  The real step is tests/_td_oracle.py's (the C oracle moves the envs, its `choose` /
`row_max` / `words` pick and learn); the counts, the table look-ups and the stream-7 variates are restated here with
oracle/gu_rng.py.  Test infrastructure; it imports oracle/ and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as TD

M32 = 0xFFFFFFFF
STREAM_EXPLORE = 7
COUNT_MAX = 0x3FFFFFFF
UCB, THOMPSON = 0, 1


def sample_next_v(x):
    """oracle.gu_rng.sample_next on a uint64 array of 32-bit words."""
    m = np.uint64(M32)
    x = x ^ ((x << np.uint64(13)) & m)
    x = x ^ (x >> np.uint64(17))
    x = x ^ ((x << np.uint64(5)) & m)
    return (x + np.uint64(0x9E3779B9)) & m


def variates(seed, env_ids, t):
    """z [n, 4] float64: the four Irwin-Hall variates of step counts t (uint64, one per env) -- x_0 the stream-7 word at t, keyed
    like stream 4; x_{b+1} = sample_next(x_b); z_b = the sum of the four bytes of x_b, minus 510."""
    t = np.asarray(t, np.uint64)
    x = R.word_v(seed, env_ids, STREAM_EXPLORE, t & np.uint64(M32), epoch=t >> np.uint64(32)).astype(np.uint64)
    z = np.empty((len(x), 4), np.float64)
    for b in range(4):
        s = sum(((x >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.int64) for k in range(4))
        z[:, b] = (s - 510).astype(np.float64)
        x = sample_next_v(x)
    return z


class ExploreOracle(TD.TdOracle):
    """TdOracle plus the visit counts uint32 [n, S, 4] and the tables U, B (float64 [C])."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(ExploreOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.counts = np.zeros((self.n, grid.S, 4), np.uint32)
        self.U = self.B = None

    def set_tables(self, U, B):
        self.U, self.B = np.array(U, np.float64), np.array(B, np.float64)
        assert self.U.ndim == 1 and self.U.shape == self.B.shape and len(self.U) >= 2

    def set_counts(self, counts, env0=0):
        counts = np.asarray(counts, np.uint32)
        self.counts[env0:env0 + len(counts)] = counts

    def scores(self, s, t, mode):
        """The score rows [n, 4] of all learners standing in s at step counts t."""
        idx = np.arange(self.n)
        top = len(self.U) - 1
        nb = self.counts[idx, s].astype(np.int64)          # [n, 4]
        u = self.U[np.minimum(nb.sum(axis=1), top)]         # (the sum fits 32 bits: the counts saturate)
        p = u[:, None] * self.B[np.minimum(nb, top)]
        if mode == THOMPSON:
            p = p * variates(self.seed, self.env_ids, t)
        return self.q[idx, s] + p

    def explore(self, T, mode, alpha, gamma, eps_q16):
        assert mode in (UCB, THOMPSON) and self.U is not None
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            # 1. lazy auto-reset
            d = st.done != 0
            if d.any():
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            # 2. the stream-4 word; 3. the action: epsilon, else greedy on the score row with rule 2's tie rule
            t = st.tcount.astype(np.uint64)
            w = TD.words(self.seed, self.env_ids, t)
            act = TD.choose(self.scores(s, t, mode), w, eps_q16)
            # 4. the count, on exploring steps too
            self.counts[idx, s, act] = np.minimum(self.counts[idx, s, act].astype(np.int64) + 1, COUNT_MAX).astype(np.uint32)
            # 5. the move and the Q-learning update
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * TD.row_max(self.q[idx, s2]))
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
