"""CPU restatement of gu_td_run (include/gu.h, csrc/gu_td.hip): N independent epsilon-greedy Q-learning / SARSA learners on one
grid, stepped through the C oracle (oracle/c_oracle.py, one step per call with the chosen actions) and drawing the stream-4 words
with oracle/gu_rng.py.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

M32 = 0xFFFFFFFF
Q_LEARNING, SARSA = 0, 1


def row_max(q):
    """[..., 4] -> [...]: the maximum folded left to right with `>` (the kernel's order)."""
    mx = q[..., 0]
    for k in (1, 2, 3):
        mx = np.where(q[..., k] > mx, q[..., k], mx)
    return mx


def choose(q, w, eps_q16):
    """Epsilon-greedy action per row of q [n, 4] with words w [n] (uint32)."""
    w = w.astype(np.int64)
    mx = row_max(q)
    eq = (q == mx[:, None]).astype(np.int64)
    m = eq.sum(axis=1)
    k = (((w >> 2) & 0x3FFF) * m) >> 14
    before = np.cumsum(eq, axis=1) - eq  # ties ahead of each action
    a = w & 3
    for j in range(4):
        a = np.where((eq[:, j] == 1) & (before[:, j] == k), j, a)
    return np.where((w >> 16) < int(eps_q16), w & 3, a).astype(np.int32)


def words(seed, env_ids, t):
    t = np.asarray(t, np.uint64)
    return R.word_v(seed, env_ids, 4, t & np.uint64(M32), epoch=t >> np.uint64(32))


class TdOracle(object):
    """N learners on `grid` (a C.Grid), global env ids env_id0 .. env_id0+N-1, with the engine's env state in `state`."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        self.grid, self.seed, self.n = grid, int(seed), int(n)
        self.state = C.State(n, env_id0)
        self.state.pos[:] = grid.starts[0]  # where gu_set_grid puts every env
        self.env_ids = np.arange(env_id0, env_id0 + n, dtype=np.uint64)
        self.q = np.full((n, grid.S, 4), float(q0), np.float64)
        self.carry = np.full(n, -1, np.int32)  # SARSA's a' of the last launch
        self.carry_valid = False               # ... and whether the next launch "directly follows" it

    def reset(self, mask=None):
        self.carry_valid = False
        return C.reset(self.grid, self.seed, self.state, mask)

    def rollout(self, T, **kw):
        """A gu_rollout from the current state (it ends the SARSA carry)."""
        self.carry_valid = False
        return C.rollout(self.grid, self.seed, self.state, T, **kw)

    def set_state(self, tcount=None):
        self.carry_valid = False
        if tcount is not None:
            self.state.tcount[:] = tcount

    def set_q(self, q, env0=0):
        self.carry_valid = False
        q = np.asarray(q, np.float64)
        self.q[env0:env0 + len(q)] = q

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
            need = act < 0
            if need.any():
                w = words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, choose(self.q[idx, s], w, eps_q16), act).astype(np.int32)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            nxt = self.q[idx, s2].copy()  # pre-update row of s'
            if method == SARSA:
                a2 = choose(nxt, words(self.seed, self.env_ids, st.tcount), eps_q16)
                m = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                m = row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * m)
            qa = self.q[idx, s, act]
            self.q[idx, s, act] = qa + alpha * (target - qa)
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:  # (a launch of zero steps changes nothing)
            self.carry = act
            self.carry_valid = method == SARSA
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
