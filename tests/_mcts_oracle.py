"""CPU restatement of gu_mcts_run (include/gu.h, csrc/gu_mcts.hip): N independent learners on one grid that choose every
non-exploring real action by a UCT tree of M simulations -- UCB1 selection down to H levels, one new node, a rollout of D moves, a
backup -- and learn from the real transition by Q-learning.  The real step is tests/_td_oracle.py's (the C oracle moves the envs,
its `choose` / `row_max` / `words` pick the actions); the trees are restated here in numpy, one array slot per node and learner,
simulated on a transition table read once from oracle.c_oracle.look_step_ahead and drawing the stream-8 words with
oracle/gu_rng.py.  Every learner of a batch is in the same simulation j at the same time (a simulation's draws depend on j, not on
what the others do), so the loops run over levels and the arrays over learners.
Test infrastructure; it imports oracle/ and tests/_td_oracle.py read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as TD

M32 = 0xFFFFFFFF
STREAM_MCTS = 8
_BLOCK = 1 << 21  # words drawn in one piece: a whole real step's where they are fewer, else one simulation's


def sim_words(seed, env_ids, c):
    """Stream-8 words of draws c (uint64, one per env id): counter c & 0xFFFFFFFF, epoch c >> 32."""
    c = np.asarray(c, np.uint64)
    return R.word_v(seed, env_ids, STREAM_MCTS, c & np.uint64(M32), epoch=c >> np.uint64(32))


def uct_tables(c=3.0, size=256):
    """UCB1's U, B, I restated: U[n] = c sqrt(ln(n + 1)), B[n] = 1 / sqrt(n), I[n] = 1 / n, B[0] = I[0] = 0."""
    n = np.arange(size, dtype=np.float64)
    B, I = np.zeros(size, np.float64), np.zeros(size, np.float64)
    B[1:] = 1.0 / np.sqrt(n[1:])
    I[1:] = 1.0 / n[1:]
    return float(c) * np.sqrt(np.log(n + 1.0)), B, I


def greedy(score, w):
    """The greedy branch of TD.choose on score [k, 4] with words w [k]: the pick among the exactly-maximal actions."""
    return TD.choose(score, w, 0)


class MctsOracle(TD.TdOracle):
    """TdOracle plus, per learner, the tree of its most recent searched iteration (slots beyond `count` hold -1 / -1 / -1 / 0 /
    0.0, as gu_mcts_get_tree reports them) and the simulated moves of the last launch."""

    def __init__(self, grid, seed, n, env_id0=0, q0=0.0):
        super(MctsOracle, self).__init__(grid, seed, n, env_id0, q0)
        S = grid.S
        cells, acts = np.repeat(np.arange(S, dtype=np.int32), 4), np.tile(np.arange(4, dtype=np.int32), S)
        nxt, rew, don = C.look_step_ahead(grid, cells, acts, True)
        self.nxt, self.rew, self.don = nxt.astype(np.int64), rew.astype(np.int64), don != 0  # flat [S * 4]
        self.tables = uct_tables()
        self.max_sims = 0
        self.sim_steps = np.zeros(self.n, np.int64)
        self.pool(1)
        self.max_sims = 0  # (no pool asked for yet: the first search makes one, as VecGridUniverse.tree_search_run does)

    def pool(self, max_sims):
        """gu_mcts_init: empty trees of max_sims + 1 slots."""
        P = int(max_sims) + 1
        self.max_sims = int(max_sims)
        self.t_state = np.full((self.n, P), -1, np.int32)
        self.t_parent = np.full((self.n, P), -1, np.int32)
        self.t_child = np.full((self.n, P, 4), -1, np.int32)
        self.t_visits = np.zeros((self.n, P, 4), np.uint32)
        self.t_w = np.zeros((self.n, P, 4), np.float64)
        self.count = np.zeros(self.n, np.int32)
        self.sim_steps[:] = 0

    @property
    def root_w(self):
        return self.t_w[:, 0]

    @property
    def root_visits(self):
        return self.t_visits[:, 0]

    def _trees(self, ids, s, t, M, H, D, gamma, eps_sim_q16):
        """Build the trees of the learners `ids` standing in s at step counts t (uint64); returns their final rows [k, 4]."""
        U, B, I = self.tables
        top = len(U) - 1
        k, P, span = len(ids), self.max_sims + 1, H + D
        env_ids = self.env_ids[ids]
        lane = np.arange(k)
        state = np.full((k, P), -1, np.int64)
        parent = np.full((k, P), -1, np.int64)
        edge_r = np.zeros((k, P), np.int64)  # the reward of the edge into each node
        child = np.full((k, P, 4), -1, np.int64)
        visits = np.zeros((k, P, 4), np.int64)
        wsum = np.zeros((k, P, 4), np.float64)
        state[:, 0] = s
        cnt = np.ones(k, np.int64)
        steps = np.zeros(k, np.int64)
        with np.errstate(over='ignore'):
            first = t * np.uint64(M) * np.uint64(span)  # (wraps) the counter of draw 0 of simulation 0
            whole = k * M * span <= _BLOCK
            if whole:
                block = sim_words(self.seed, np.repeat(env_ids, M * span),
                                  (first[:, None] + np.arange(M * span, dtype=np.uint64)[None, :]).ravel()).reshape(k, M, span)
            for j in range(M):
                if whole:
                    words = block[:, j]
                else:
                    c = first[:, None] + np.uint64(j * span) + np.arange(span, dtype=np.uint64)[None, :]
                    words = sim_words(self.seed, np.repeat(env_ids, span), c.ravel()).reshape(k, span)
                drawn = np.zeros(k, np.int64)
                # ---- selection: every lane in its node v, until it leaves the tree
                v = np.zeros(k, np.int64)
                x = np.asarray(s, np.int64).copy()
                sel = np.ones(k, bool)
                roll = np.zeros(k, bool)
                ev, eu, er = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)  # the last edge and its reward
                for depth in range(1, H + 1):
                    if not sel.any():
                        break
                    nv, wv = visits[lane, v], wsum[lane, v]
                    idx = np.minimum(nv, top)
                    score = wv * I[idx] + U[np.minimum(nv.sum(axis=1), top)][:, None] * B[idx]
                    score[nv == 0] = np.inf
                    u = greedy(score, words[lane, drawn]).astype(np.int64)
                    x2, r2, d2 = self.nxt[x * 4 + u], self.rew[x * 4 + u], self.don[x * 4 + u]
                    ch = child[lane, v, u]
                    down = sel & ~d2 & (ch >= 0) & (depth < H)
                    out = sel & ~d2 & ~down  # a rollout starts at x2 ...
                    new = out & (ch < 0)     # ... behind a new node
                    ev[sel], eu[sel], er[sel] = v[sel], u[sel], r2[sel]
                    drawn[sel] += 1
                    steps[sel] += 1
                    ln = lane[new]
                    state[ln, cnt[ln]] = x2[ln]
                    parent[ln, cnt[ln]] = v[ln] * 4 + u[ln]
                    edge_r[ln, cnt[ln]] = r2[ln]
                    child[ln, v[ln], u[ln]] = cnt[ln]
                    cnt[ln] += 1
                    x[sel] = x2[sel]
                    v[down] = ch[down]
                    roll |= out
                    sel = down
                # ---- rollout: gu_search_run's, from x
                G, disc, live = np.zeros(k, np.float64), np.ones(k, np.float64), roll.copy()
                for _ in range(D):
                    if not live.any():
                        break
                    wq = words[lane, np.minimum(drawn, span - 1)]
                    u = ((wq & 3) if eps_sim_q16 == 65536 else TD.choose(self.q[ids, x], wq, eps_sim_q16)).astype(np.int64)
                    x2, r2, d2 = self.nxt[x * 4 + u], self.rew[x * 4 + u], self.don[x * 4 + u]
                    G[live] = (G + disc * r2.astype(np.float64))[live]
                    disc[live] = (disc * gamma)[live]
                    x[live] = x2[live]
                    drawn[live] += 1
                    steps[live] += 1
                    live &= ~d2
                G[live] = (G + disc * TD.row_max(self.q[ids, x]))[live]  # the leaf's bootstrap; a lane that ended in a terminal cell has none
                # ---- backup: along the parent links (G = 0.0 where selection ended in a terminal cell)
                bv, bu, br, back = ev, eu, er, np.ones(k, bool)
                while back.any():
                    G = br.astype(np.float64) + gamma * G
                    lb = lane[back]
                    wsum[lb, bv[lb], bu[lb]] = wsum[lb, bv[lb], bu[lb]] + G[lb]
                    visits[lb, bv[lb], bu[lb]] += 1
                    back &= bv != 0
                    link = parent[lane, bv]
                    br = np.where(back, edge_r[lane, bv], br)
                    bu = np.where(back, link & 3, bu)
                    bv = np.where(back, link >> 2, bv)
        self.sim_steps[ids] += steps
        self.t_state[ids], self.t_parent[ids], self.t_child[ids] = state, parent, child
        self.t_visits[ids], self.t_w[ids], self.count[ids] = visits, wsum, cnt
        n0 = visits[:, 0]
        return np.where(n0 == 0, -np.inf, wsum[:, 0] * I[np.minimum(n0, top)])

    def tree_search(self, T, M, H, D, alpha, gamma, eps_q16, eps_sim_q16=65536):
        st, idx = self.state, np.arange(self.n)
        alpha, gamma, M, H, D = float(alpha), float(gamma), int(M), int(H), int(D)
        if M > self.max_sims or not self.max_sims:
            self.pool(max(M, 1))
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
            # 3. the action: exploring (and every M = 0) learner by rule 2 of gu_td_run, the others by their tree
            act = TD.choose(self.q[idx, s], w, eps_q16)
            if M > 0:
                ids = np.flatnonzero((w.astype(np.int64) >> 16) >= int(eps_q16))
                if ids.size:
                    act[ids] = TD.choose(self._trees(ids, s[ids], t[ids], M, H, D, gamma, eps_sim_q16), w[ids], eps_q16)
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
