"""CPU restatement of gu_sweep_run (include/gu.h, csrc/gu_sweep.hip): N independent prioritized-sweeping learners on one grid.  The
real step is tests/_td_oracle.py's choice and move without its update, the model is tests/_dyna_oracle.py's; the queue is restated
here as a DENSE array key[n][S][4] (0 = not queued) and a pop as an argmax over it -- deliberately not a heap: the device's structure
is checked against the semantics, not against a copy of itself.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C

from . import _dyna_oracle as D
from . import _td_oracle as TD

MAX_PAIRS = 65536
PAIR_MASK = np.uint64(0xFFFF)


def pack_keys(p, x, theta):
    """Keys of pairs p (int) under priorities x (float64), 0 where insert(p, x) does nothing: x > theta fails (a NaN too) or the
    truncated pattern is zero."""
    x = np.asarray(x, np.float64)
    bits = x.view(np.uint64) >> np.uint64(16)
    with np.errstate(invalid='ignore'):
        ok = (x > theta) & (bits != 0)
    key = (bits << np.uint64(16)) | np.asarray(p).astype(np.uint64)
    return np.where(ok, key, np.uint64(0))


def priorities(key):
    """float64 priorities of keys: the low 16 bits cleared; 0.0 where nothing is queued."""
    return (np.asarray(key, np.uint64) & ~PAIR_MASK).view(np.float64)


def candidate_cells(S, W, cells):
    """The candidate predecessor cells of state S on a grid of width W with `cells` states."""
    return [c for c in (S, S - W, S + 1, S + W, S - 1) if 0 <= c < cells]


class SweepOracle(D.DynaOracle):
    """DynaOracle plus one queue per learner: key uint64[n][S][4] (0 = not queued), size int32[n]."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(SweepOracle, self).__init__(grid, seed, n, env_id0, q0)
        assert 4 * grid.S <= MAX_PAIRS

    def clear_model(self):
        super(SweepOracle, self).clear_model()
        self.key = np.zeros((self.n, self.grid.S, 4), np.uint64)
        self.pops = 0
        self.inserts = 0

    @property
    def size(self):
        return (self.key != 0).reshape(self.n, -1).sum(axis=1).astype(np.int32)

    def queue(self):
        return dict(key=self.key, priority=priorities(self.key), size=self.size)

    def _insert(self, e, p, x, theta):
        """insert(p[i], x[i]) for learners e[i]."""
        new = pack_keys(p, x, theta)
        flat = self.key.reshape(self.n, -1)
        old = flat[e, p]
        self.inserts += int((new > old).sum())
        flat[e, p] = np.maximum(old, new)

    def sweep(self, T, P, theta, alpha, gamma, eps_q16):
        st, idx = self.state, np.arange(self.n)
        theta, alpha, gamma, P = float(theta), float(alpha), float(gamma), int(P)
        cells, W = self.grid.S, int(self.grid.W)
        flat = self.key.reshape(self.n, -1)
        offs = np.array(sorted(set((0, -W, 1, W, -1))), np.int64)
        obs, rew, don = (np.empty((T, self.n), np.int32) for _ in range(3))
        for i in range(T):
            # 1. the real step, without gu_td_run's update
            d = st.done != 0
            if d.any():
                C.reset(self.grid, self.seed, st, d.astype(np.uint8))
            s = st.pos.copy()
            act = TD.choose(self.q[idx, s], TD.words(self.seed, self.env_ids, st.tcount.astype(np.uint64)), eps_q16)
            out = C.rollout(self.grid, self.seed, st, 1, True, actions=act[None, :])
            s2, r, dn = out['obs'][0], out['reward'][0], out['done'][0] != 0
            # 2. the model
            new = self.next[idx, s, act] < 0
            self.next[idx, s, act], self.mreward[idx, s, act], self.mdone[idx, s, act] = s2, r, dn
            self.list[idx[new], self.count[new]] = (s * 4 + act)[new]
            self.count += new
            # 3. the priority of the real pair
            rf = r.astype(np.float64)
            target = np.where(dn, rf, rf + gamma * TD.row_max(self.q[idx, s2]))
            self._insert(idx, s * 4 + act, np.abs(target - self.q[idx, s, act]), theta)
            # 4. planning
            for _ in range(P):
                # (queued pairs are observed pairs, so the argmax over the dense keys is the argmax over the listed ones: no key
                # array of 4S entries per learner is scanned where a few hundred pairs are observed)
                m = int(self.count.max())
                lst = self.list[:, :m]
                keys = np.where(np.arange(m)[None, :] < self.count[:, None], flat[idx[:, None], np.maximum(lst, 0)], np.uint64(0))
                k = np.argmax(keys, axis=1)
                e = np.flatnonzero(keys[idx, k] != 0)
                if not len(e):
                    break
                p = lst[e, k[e]].astype(np.int64)
                flat[e, p] = 0
                self.pops += len(e)
                S, A = p >> 2, p & 3
                S2, R, Dn = self.next[e, S, A], self.mreward[e, S, A].astype(np.float64), self.mdone[e, S, A] != 0
                tgt = np.where(Dn, R, R + gamma * TD.row_max(self.q[e, S2]))
                qp = self.q[e, S, A]
                self.q[e, S, A] = qp + alpha * (tgt - qp)
                mS = TD.row_max(self.q[e, S])
                # the candidate predecessors, all learners and all 5 x 4 candidates at once (distinct cells: inserts of one call must not collide)
                c = S[:, None] + offs[None, :]
                inside = (c >= 0) & (c < cells)
                cc = np.where(inside, c, 0)
                hit = inside[:, :, None] & (self.next[e[:, None], cc] == S[:, None, None])
                i_, k_, b_ = np.nonzero(hit)
                eh, ch = e[i_], cc[i_, k_]
                Rb = self.mreward[eh, ch, b_].astype(np.float64)
                tb = np.where(self.mdone[eh, ch, b_] != 0, Rb, Rb + gamma * mS[i_])
                self._insert(eh, ch * 4 + b_, np.abs(tb - self.q[eh, ch, b_]), theta)
            obs[i], rew[i], don[i] = s2, r, dn
        if T > 0:
            self.carry_valid = False
        return dict(obs=obs, reward=rew, done=don, ret=rew.astype(np.int64).sum(axis=0), episodes=don.sum(axis=0).astype(np.int32))
