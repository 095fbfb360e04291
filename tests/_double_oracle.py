"""CPU restatements of gu_esarsa_run and gu_double_run (include/gu.h, csrc/gu_td.hip, csrc/gu_double.hip): N independent Expected
SARSA / Double Q-learning learners on one grid, stepped through the C oracle like tests/_td_oracle.py and reusing its `choose`,
`words` and `row_max`.  numpy float64 in the kernels' operation order, one rounding per operation.  Test infrastructure; it imports
oracle/ and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as TD

STREAM_DOUBLE = 10


def expectation(n, eps_q16):
    """[..., 4] -> [...]: the mean of a row under the epsilon-greedy policy, pe * sum + pg * max (gu_esarsa_run rule 3)."""
    pe = float(int(eps_q16)) * 2.0 ** -18
    pg = float(65536 - int(eps_q16)) * 2.0 ** -16
    total = ((n[..., 0] + n[..., 1]) + n[..., 2]) + n[..., 3]
    return pe * total + pg * TD.row_max(n)


def coins(seed, env_ids, t):
    """Bit 0 of the stream-10 words at step counts t."""
    t = np.asarray(t, np.uint64)
    return (R.word_v(seed, env_ids, STREAM_DOUBLE, t & np.uint64(TD.M32), epoch=t >> np.uint64(32)) & np.uint32(1)).astype(np.int64)


def _result(obs, rew, don):
    return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))


def _ends_what_is_carried(o):
    """A launch of another learner: SARSA's a' goes, and so does a window where the oracle has one (tests/_nstep_oracle.py)."""
    o.carry_valid = False
    if hasattr(o, 'drop'):
        o.drop()


class EsarsaOracle(TD.TdOracle):
    """TdOracle plus gu_esarsa_run on the same tables."""

    def esarsa(self, T, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = st.done != 0
            if d.any():  # lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            act = TD.choose(self.q[idx, s], TD.words(self.seed, self.env_ids, st.tcount), eps_q16)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            E = expectation(self.q[idx, s2], eps_q16)  # of the pre-update row of s'
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * E)
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            _ends_what_is_carried(self)
        return _result(obs, rew, don)


class DoubleOracle(TD.TdOracle):
    """N Double Q-learning learners: q[n, S, 2, 4], [:, :, 0] is A and [:, :, 1] is B.  `share`: another oracle whose env state this
    one steps (the engine's envs are one set, whichever learner moves them); a launch here ends what that one carries."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0, share=None):
        super(DoubleOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.q = np.full((self.n, grid.S, 2, 4), float(q0), np.float64)
        self.share = share
        if share is not None:
            self.state = share.state

    def run(self, T, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma = float(alpha), float(gamma)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        self.last_coin = self.last_sa = None
        for i in range(T):
            d = st.done != 0
            if d.any():  # lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            pair = self.q[idx, s]
            act = TD.choose(pair[:, 0] + pair[:, 1], TD.words(self.seed, self.env_ids, st.tcount), eps_q16)
            coin = coins(self.seed, self.env_ids, st.tcount)  # at the count before the move; 0: A learns from B, 1: B from A
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            nxt = self.q[idx, s2].copy()  # the pre-update pair of s'
            X, Y = nxt[idx, coin], nxt[idx, 1 - coin]
            eq = X == TD.row_max(X)[:, None]
            best = np.where(eq.any(axis=1), np.argmax(eq, axis=1), 0)  # the lowest action at the maximum
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * Y[idx, best])
            qa = self.q[idx, s, coin, act]
            self.q[idx, s, coin, act] = qa + alpha * (target - qa)
            obs[i], rew[i], don[i] = s2, r, dn
            self.last_coin, self.last_sa = coin, s * 4 + act
        if T > 0:
            _ends_what_is_carried(self)
            if self.share is not None:
                _ends_what_is_carried(self.share)
        return _result(obs, rew, don)
