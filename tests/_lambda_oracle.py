"""CPU restatement of gu_lambda_run (include/gu.h, csrc/gu_lambda.hip): N independent SARSA(lambda) / Watkins's Q(lambda) learners
with replacing traces truncated after K steps, on one grid, stepped through the C oracle like tests/_td_oracle.py and reusing its
`choose`, `words` and `row_max`.  The window of env e is win[e], index = age (-1: none).  Test infrastructure; it imports oracle/
and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _td_oracle as TD

LAMBDA_MAX = 64
WATKINS, SARSA = TD.Q_LEARNING, TD.SARSA


def coefficients(K, gamma, lam):
    """P_0 .. P_{K-1}: P_0 = 1, P_j = P_{j-1} * (gamma * lambda), float64 with one rounding per multiply."""
    c = float(gamma) * float(lam)
    P = [1.0]
    for _ in range(1, int(K)):
        P.append(P[-1] * c)
    return P


class LambdaOracle(TD.TdOracle):
    """TdOracle plus one trace window per learner and the carry rule of gu_lambda_run."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(LambdaOracle, self).__init__(grid, seed, n, env_id0, q0)
        self.win = np.full((self.n, LAMBDA_MAX), -1, np.int32)
        self.key = None  # (method, K) of the last call if it was a lambda run, else None: the window is dropped

    def drop(self):
        self.key = None
        self.win[:] = -1

    def window(self):
        return self.win

    def other_call(self):
        """Any other learner call that touches the envs (gu_nstep_run, gu_dyna_run, gu_ac_run): the window and SARSA's a' go."""
        self.drop()
        self.carry_valid = False

    # every other call that touches the envs drops the window (and, through TdOracle, SARSA's a')
    def reset(self, mask=None):
        self.drop()
        return super(LambdaOracle, self).reset(mask)

    def rollout(self, T, **kw):
        self.drop()
        return super(LambdaOracle, self).rollout(T, **kw)

    def set_state(self, tcount=None):
        self.drop()
        super(LambdaOracle, self).set_state(tcount)

    def set_q(self, q, env0=0):
        self.drop()
        super(LambdaOracle, self).set_q(q, env0)

    def run(self, T, method, alpha, gamma, eps_q16):
        if T > 0:
            self.drop()
        return super(LambdaOracle, self).run(T, method, alpha, gamma, eps_q16)

    def lam(self, T, method, K, lam, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma, K = float(alpha), float(gamma), int(K)
        assert 1 <= K <= LAMBDA_MAX and 0.0 <= lam <= 1.0
        if T == 0:
            return dict(obs=np.empty((0, self.n), np.int32), reward=np.empty((0, self.n), np.int32),
                        done=np.empty((0, self.n), np.int32), ret=np.zeros(self.n, np.int64), episodes=np.zeros(self.n, np.int32))
        if self.key != (method, K):
            self.drop()
            act = np.full(self.n, -1, np.int32)
        else:
            act = self.carry.copy() if method == SARSA else np.full(self.n, -1, np.int32)
        P = coefficients(K, gamma, lam)
        W = self.win
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            d = st.done != 0
            if d.any():  # 1. lazy auto-reset
                assert (W[d] < 0).all()
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
                act[d] = -1
            s = st.pos.copy()
            need = act < 0
            if need.any():  # 2. action
                w = TD.words(self.seed, self.env_ids, st.tcount)
                act = np.where(need, TD.choose(self.q[idx, s], w, eps_q16), act).astype(np.int32)
            row = self.q[idx, s]  # the row the action was chosen from
            qsa = row[idx, act]
            if method == WATKINS:  # the cut: a non-greedy action empties the window
                W[~(qsa == TD.row_max(row))] = -1
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])  # 3. move, t += 1
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            nxt = self.q[idx, s2].copy()  # 4. pre-update row of s'
            if method == SARSA:
                a2 = TD.choose(nxt, TD.words(self.seed, self.env_ids, st.tcount), eps_q16)
                m = nxt[idx, a2]
                a2 = np.where(dn, -1, a2).astype(np.int32)
            else:
                m = TD.row_max(nxt)
                a2 = np.full(self.n, -1, np.int32)
            rf = r.astype(np.float64)
            g = alpha * (np.where(dn, rf, rf + gamma * m) - qsa)
            sa = (s * 4 + act).astype(np.int32)
            head = W[:, :K]  # 5. replace, then Q[p] += g * P_j over the live ages with P_j != 0
            head[head == sa[:, None]] = -1
            W[:, 0] = sa
            for j in range(K):
                if not P[j] != 0.0:
                    continue
                e = idx[W[:, j] >= 0]
                p = W[e, j]
                self.q[e, p >> 2, p & 3] = self.q[e, p >> 2, p & 3] + g[e] * P[j]
            W[dn] = -1  # 6. end, or age by one
            live = idx[~dn]
            W[live, 1:K] = W[live, :K - 1]
            W[live, 0] = -1
            act = a2
            obs[i], rew[i], don[i] = s2, r, dn
        self.carry = act
        self.carry_valid = False  # gu_lambda_run ends gu_td_run's SARSA carry
        self.key = (method, K)
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))


def signed_zero_table(n, S, seed=1):
    """A table of -0.0 and 2.0 entries.  Learned with alpha = -0.0 it keeps -0.0 in pairs of the window while later steps have
    g = +0.0, so an update by g * P_j with P_j = 0 would turn them into +0.0: only the P_j != 0 rule keeps lambda = 0 exact there."""
    return np.where(np.random.default_rng(seed).random((n, S, 4)) < 0.5, -0.0, 2.0)
