"""CPU restatement of errands (include/gu.h: gu_set_errands; csrc/gu_errands.hip, csrc/gu_td.hip) in numpy: every candidate cell comes
from the C oracle's look_step_ahead (care_about_terminal on) and every reset from its reset, the action words and the stream-11 words
that draw the instruction come from oracle/gu_rng.py, and the learner on (cell, word) reuses the epsilon-greedy rule of
tests/_td_oracle.py.  The oracle keeps a log of what its runs met (EVENTS), so that a comparison can show it compared something.
Only the rule is here: the resets, gu_step's rejected actions, the rollout policies and td_run around it are
tests/_overlay_oracle.py's.  Test infrastructure; it imports oracle/ read-only."""
import numpy as np

from oracle import c_oracle as C
from oracle import gu_rng as R

from ._overlay_oracle import OverlayOracle
from ._td_oracle import Q_LEARNING, SARSA  # noqa: F401  (re-exported for the tests)

KINDS = {'apple': 1, 'lemon': 2, 'melon': 3}
STREAM_ERRAND = 11
EVENTS = ('right', 'wrong', 'completed', 'absorbed', 'drawn')  # 'drawn': the set of instruction indices that resets drew


def codes_of(instruction):
    return [KINDS.get(k, k) for k in instruction]


def plane_of(S, cells, kinds):
    """The errand plane: slots by ascending cell, kinds in the order of `cells` (restated here, not imported from the package)."""
    p = np.zeros(S, np.uint8)
    order = np.argsort(cells, kind='stable')
    for slot, i in enumerate(order):
        p[cells[i]] = slot | (KINDS.get(kinds[i], kinds[i]) << 5)
    return p


class ErrandsOracle(OverlayOracle):
    """N envs (and learners) on `grid` (a C.Grid) under the errand plane `errand` uint8[S] (None: no errands), the `instructions`
    (lists of kind names or codes) and pay = (right, wrong, finish).  The learner's row is word * S + cell, the word
    eaten | p << F | j << (F + pb)."""

    def __init__(self, grid, seed, n, errand=None, instructions=(('apple',),), pay=(5, -8, 10), env_id0=0, q0=0.0):
        super().__init__(grid, seed, n, env_id0, q0)
        self.log = dict(right=0, wrong=0, completed=0, absorbed=0, drawn=set())
        self.set_errands(errand, instructions, pay)

    def set_errands(self, errand, instructions=(('apple',),), pay=(5, -8, 10)):
        """gu_set_errands: every word is 0 (instruction 0, nothing eaten); the tables go (back to q0) when their row count changes."""
        self.errand = np.zeros(self.grid.S, np.uint8) if errand is None else np.asarray(errand, np.uint8).copy()
        self.F = int(np.count_nonzero(self.errand))
        self.instr = [codes_of(ins) for ins in instructions] if errand is not None else []
        self.length = np.array([len(i) for i in self.instr] or [0], np.int64)
        # entry p of instruction j; 0 behind the end
        self.table = np.zeros((max(len(self.instr), 1), 5), np.int64)
        for j, ins in enumerate(self.instr):
            self.table[j, :len(ins)] = ins
        self.pb = int(self.length.max()).bit_length() if self.instr else 0
        self.ib = (len(self.instr) - 1).bit_length() if self.instr else 0
        self.right, self.wrong, self.finish = (int(v) for v in pay)
        self.eaten, self.p, self.j = (np.zeros(self.n, np.int64) for _ in range(3))
        self._installed()

    @property
    def words(self):
        return (self.eaten | (self.p << self.F) | (self.j << (self.F + self.pb))).astype(np.uint32)

    def set_words(self, words, env0=0):
        w = np.atleast_1d(np.asarray(words)).astype(np.int64)
        k = slice(env0, env0 + w.size)
        self.eaten[k] = w & ((1 << self.F) - 1)
        self.p[k] = (w >> self.F) & ((1 << self.pb) - 1)
        self.j[k] = w >> (self.F + self.pb)
        self.carry_valid = False

    def _bits(self):
        return self.F + self.pb + self.ib if self.F else 0

    def _row(self, pos):
        return self.words.astype(np.int64) * self.grid.S + pos

    def _restore(self, took, lazy=False):
        """Rule 1.  reset() calls this BEFORE the C oracle's reset increments the episode counts, the lazy reset AFTER it: the draw is
        keyed by the count before the reset either way."""
        if not self.F:
            return
        self.eaten[took] = 0
        self.p[took] = 0
        ep = self.state.episode.astype(np.uint64) - np.uint64(1 if lazy else 0)
        I = len(self.instr)
        w = R.word_v(self.seed, self.env_ids, STREAM_ERRAND, ep).astype(np.uint64)
        j = ((w * np.uint64(I)) >> np.uint64(32)).astype(np.int64)
        self.j[took] = j[took]
        self.log['drawn'] |= set(j[took].tolist())

    # one move of the envs in `who` (bool[n]) with actions act[n]: rules 2 .. 6 of gu_set_errands
    def _move(self, act, who=None):
        st = self.state
        who = np.ones(self.n, bool) if who is None else who
        s2, r, d = C.look_step_ahead(self.grid, st.pos.copy(), (np.asarray(act) & 3).astype(np.int32), True)
        r, d = r.astype(np.int64), d.astype(np.int64)
        if self.F:
            absorbed = self.p == self.length[self.j]  # rule 2
            s2 = np.where(absorbed, st.pos, s2)
            c = self.errand[s2].astype(np.int64)
            kind = (c >> 5) & 3
            bit = np.where(kind != 0, np.int64(1) << (c & 31), 0)
            fresh = ~absorbed & ((bit & ~self.eaten) != 0)
            right = fresh & (kind == self.table[self.j, self.p])
            wrong = fresh & ~right
            p2 = self.p + right
            completed = right & (p2 == self.length[self.j])
            r = np.where(right, r + self.right, np.where(wrong, r + self.wrong, r))
            r = np.where(absorbed | completed, self.finish, r)
            d = np.where(absorbed | completed, 1, d)
            self.eaten[who] |= np.where(fresh, bit, 0)[who]
            self.p[who] = p2[who]
            for name, ev in (('right', right), ('wrong', wrong), ('completed', completed), ('absorbed', absorbed)):
                self.log[name] += int((ev & who).sum())
        st.pos[who] = s2[who]
        st.done[who] = d[who]
        self.reward[who] = r[who]
        st.tcount[who] += np.uint64(1)
        return st.pos.copy(), self.reward.copy(), st.done.copy()


# ---- the learning claim (tests/test_errands_host.py, tests/test_gpu_errands.py): a 5 x 3 open grid, start (0, 1), goal (4, 1), an
# apple on cell 2 = (2, 0) and a lemon on cell 12 = (2, 2), two instructions and pay (5, -8, 16) ----
CLAIM_W, CLAIM_H = 5, 3
CLAIM = dict(W=CLAIM_W, H=CLAIM_H, starts=[1 * CLAIM_W + 0], goals=[1 * CLAIM_W + 4], lava=[], walls=[])
CLAIM_CELLS, CLAIM_KINDS = [2, 12], ['apple', 'lemon']
CLAIM_TEXTS = ['collect the lemon and then the apple', 'collect the apple and then the lemon']
CLAIM_INSTRUCTIONS = [['lemon', 'apple'], ['apple', 'lemon']]
CLAIM_PAY = (5, -8, 16)
CLAIM_LEARNERS, CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16 = 64, 0.5, 0.95, 13107  # eps 0.2
CLAIM_SHORTEST, CLAIM_RETURN = 5, 17  # the shortest walk that completes an instruction: -1 * 3 + (5 - 1) + 16
# K: twice the smallest multiple of 500 steps at which, for each of the seeds 0, 1, 2, the greedy walk of all 64 restated Q-learners
# under EACH instruction ends by completing it (measured with ErrandsOracle.td_run: see CLAIM_MEASURED).
CLAIM_MEASURED = {0: 3000, 1: 3000, 2: 1500}  # seed: the smallest multiple of 500 at which all 64 complete under both instructions
CLAIM_STEPS = 2 * max(CLAIM_MEASURED.values())  # 6000
# Recorded, not asserted: every learner's greedy walk under both instructions is a SHORTEST one (5 moves, return 17) only after
# 15000, 11000 and 3500 steps for the seeds 0, 1, 2.
CLAIM_SHORTEST_MEASURED = {0: 15000, 1: 11000, 2: 3500}


def greedy_walk(grid, plane, q, j, cap=100):
    """(completed, moves, return) of the greedy walk (first maximum) of one table q [S << bits, 4] from the grid's first start cell
    under instruction j, with p = 0 and nothing eaten."""
    o = ErrandsOracle(grid, 0, 1, plane, CLAIM_INSTRUCTIONS, CLAIM_PAY, q0=None)
    o.reset()
    o.set_words([j << (o.F + o.pb)])
    total = 0
    for move in range(1, cap + 1):
        row = int(o._row(o.state.pos)[0])
        _, r, d = o._move(np.array([int(np.argmax(q[row]))], np.int32))
        total += int(r[0])
        if d[0]:
            return bool(o.log['completed']), move, total
    return False, cap, total


# ---- the device cases (tests/test_gpu_errands.py; their conditions are held without a device by tests/test_errands_host.py): the
# grids 'starts8' (LDS kernels) and 'open150' (L2 kernels) of tests/_overlay_starts.py with five fruit, two kinds doubled, and three
# instructions -- ib = 2 with index 3 unused, one list of four, one that names a kind twice ----
CASE_KINDS = ['apple', 'lemon', 'melon', 'apple', 'lemon']
CASE_XY = [(2, 2), (3, 4), (5, 5), (4, 2), (2, 6)]  # on 'starts8' the cells 18, 35, 45, 20, 50
CASE_XY_150 = [(2, 2), (3, 4), (5, 6), (4, 2), (2, 6)]  # on 'open150' (5, 5) is the lava cell: the melon lies one row below
CASE_PAY = (5, -8, 10)
# uniform and stream walks wander: short instructions first.  greedy and sample walks follow the snake of case_policy, which passes
# the two apples of row 2 first: instructions that begin with them.
CASE_INSTRUCTIONS = {'wander': [['lemon', 'apple'], ['apple', 'apple', 'melon', 'lemon'], ['melon']],
                     'snake': [['apple', 'apple'], ['apple', 'apple', 'lemon', 'melon'], ['melon']]}
TD_KINDS, TD_XY = ['apple', 'lemon', 'apple'], [(2, 2), (3, 4), (4, 2)]  # td_run: three fruit and two instructions, 3 + 2 + 1 = 6 bits
TD_INSTRUCTIONS = [['apple', 'apple'], ['lemon']]


def instructions_for(policy):
    return CASE_INSTRUCTIONS['snake' if policy in ('greedy', 'sample') else 'wander']


def case_cells(W, xy):
    return [y * W + x for x, y in xy]


def case_plane(g, xy=None, kinds=CASE_KINDS):
    xy = xy or (CASE_XY_150 if g['W'] == 150 else CASE_XY)
    return plane_of(g['W'] * g['H'], case_cells(g['W'], xy), kinds)


def case_placement(g, plane, n):
    """int32[n] or None: where the envs of 'open150' are put after a reset -- free cells within two of the lava cell (5, 5), none of
    them a fruit cell (tests/_overlay_starts.py: placement)."""
    if g['W'] != 150:
        return None
    W = g['W']
    around = [y * W + x for y in range(3, 8) for x in range(3, 8) if (x, y) != (5, 5)]
    free = np.array([s for s in around if plane[s] == 0], np.int32)
    return free[np.random.RandomState(n).randint(0, len(free), n)]


def case_policy(g):
    """float64[S, 4]: every row leans 0.7 towards a row-by-row snake through bands of eight columns (right along even rows, left along
    odd ones, down at a band's end), so that greedy and sampling envs pass the fruit in a fixed order; every seventh row is one-hot."""
    UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3
    W, S = g['W'], g['W'] * g['H']
    x, y = np.arange(S) % W % 8, np.arange(S) // W
    act = np.where(y % 2 == 0, np.where(x == 7, DOWN, RIGHT), np.where(x == 0, DOWN, LEFT))
    pi = 0.3 * np.random.RandomState(1).dirichlet(np.ones(4), S) + 0.7 * np.eye(4)[act]
    pi[::7] = np.eye(4)[act[::7]]
    return pi
