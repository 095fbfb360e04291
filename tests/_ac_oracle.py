"""CPU restatement of gu_ac_run (include/gu.h, csrc/gu_ac.hip): N independent one-step softmax actor-critic learners on one grid,
stepped through the C oracle like tests/_td_oracle.py and drawing the stream-4 words with its `words`.  It keeps its own copy of
the build's exp (`gu_exp`), written from the header's rule, not imported from the product.  Test infrastructure; it imports
oracle/ and tests/_td_oracle.py read-only."""
import math

import numpy as np

from oracle import c_oracle as C

from . import _td_oracle as TD

_C = [1.0 / math.factorial(n) for n in range(13, -1, -1)]  # 1/13!, ..., 1/2!, 1, 1 (each correctly rounded)


def gu_exp(x):
    """The header's gu_exp, float64, for x <= 0."""
    x = np.asarray(x, np.float64)
    k = np.rint(x * 1.4426950408889634)
    r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    p = np.full_like(x, _C[0])
    for c in _C[1:]:
        p = p * r + c
    lo = x < -700.0
    return np.where(lo, 0.0, np.ldexp(p, np.where(lo, 0.0, k).astype(np.int64)))


def softmax(h):
    """Rule 2 on rows h [n, 4]: (e [n, 4], Z [n], pi [n, 4])."""
    m = TD.row_max(h)
    e = gu_exp(h - m[:, None])
    Z = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
    return e, Z, e * (1.0 / Z)[:, None]


def action(e, Z, w):
    """Rule 3: x = (w 2^-32) Z, the first b with x < c_b, else 3."""
    x = (w.astype(np.float64) * 2.0 ** -32) * Z
    c0 = e[:, 0]
    c1 = c0 + e[:, 1]
    c2 = c1 + e[:, 2]
    return np.where(x < c0, 0, np.where(x < c1, 1, np.where(x < c2, 2, 3))).astype(np.int32)


class AcOracle(TD.TdOracle):
    """TdOracle's env state, its Q tables and SARSA carry (gu_ac_run ends that carry), plus preferences h [n][S][4] and values
    v [n][S]."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0, h0=0.0, v0=0.0):
        super(AcOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.h = np.full((self.n, grid.S, 4), float(h0), np.float64)
        self.v = np.full((self.n, grid.S), float(v0), np.float64)

    def set_ac(self, h=None, v=None, env0=0):
        self.carry_valid = False
        if h is not None:
            h = np.asarray(h, np.float64)
            self.h[env0:env0 + len(h)] = h
        if v is not None:
            v = np.asarray(v, np.float64)
            self.v[env0:env0 + len(v)] = v

    def ac(self, T, alpha_actor, alpha_critic, gamma):
        st, idx = self.state, np.arange(self.n)
        aa, ac, gamma = float(alpha_actor), float(alpha_critic), float(gamma)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = st.done != 0
            if d.any():  # 1. lazy auto-reset
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            e, Z, pi = softmax(self.h[idx, s])  # 2. policy
            a = action(e, Z, TD.words(self.seed, self.env_ids, st.tcount))  # 3. action
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=a[None, :])  # 4. move, t += 1
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            rf = r.astype(np.float64)
            vs = self.v[idx, s]
            v2 = self.v[idx, s2]  # (read before this step's writes; not used behind a terminal s')
            delta = np.where(dn, rf, rf + gamma * v2) - vs  # 5. TD error
            self.v[idx, s] = vs + ac * delta  # 6. critic
            g = aa * delta  # 7. actor
            ind = (np.arange(4)[None, :] == a[:, None]).astype(np.float64)
            self.h[idx, s] = self.h[idx, s] + g[:, None] * (ind - pi)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False  # gu_ac_run ends gu_td_run's SARSA carry
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
