"""CPU restatement of gu_td_evaluate (include/gu.h; csrc/gu_eval.hip): K greedy test episodes of at most L steps per env on its own
table.  Calm engines walk through the C oracle's look_step_ahead from the C oracle's reset with np.argmax; under an overlay the walk
drives a FRESH restatement of the kind (tests/_overlay_starts.py: oracle(kind, name, env_id0)) through its _move / _row from the
rule-1 start, so the caller's own oracle object is left untouched.  `disc` is summed with Python floats in the rule's order.  The
walk keeps a log of what it met (LOG), so that a comparison can show that it compared something.  Nothing here needs a device.

A table is anything indexed as q[idx, row] with int arrays idx (envs) and row -> float64 [m, 4]: an array [n, rows, 4], or Shared."""
import numpy as np

from oracle import c_oracle as C

from . import _overlay_starts as OS
from . import _td_oracle as TD

KEYS = ('ret', 'length', 'outcome', 'end', 'word', 'discounted')
DTYPES = dict(ret=np.int32, length=np.int32, outcome=np.int32, end=np.int32, word=np.uint32, discounted=np.float64)


class Shared(object):
    """n tables of `rows` rows that differ from one base table [rows, 4] by an offset per (env, action) [n, 4]: big tables without
    the memory of n of them."""

    def __init__(self, base, off):
        self.base, self.off = np.asarray(base, np.float64), np.asarray(off, np.float64)

    def __getitem__(self, key):
        idx, row = key
        return self.base[row] + self.off[idx]

    def table(self, e):
        return self.base + self.off[e]


def new_log():
    return dict(outcomes=set(), ties=0, starts=set(), gust_moved=0, drawn=set(), bumps_that_changed_row=0)


def _finish(out, k, grid, alive, done, pos, word):
    term = (np.asarray(grid.goal) | np.asarray(grid.lava)) != 0
    goal = np.asarray(grid.reward)[pos] > 0
    out['outcome'][k] = np.where(~done, 0, np.where(~term[pos], 3, np.where(goal, 1, 2)))
    out['end'][k] = pos
    out['word'][k] = word


def _empty(K, n):
    return {key: np.zeros((K, n), DTYPES[key]) for key in KEYS}


def _sum(out, k, who, r, w, disc, gamma):
    """Rule 5 for the envs of `who`: Python floats, one rounding per operation."""
    for e in np.flatnonzero(who):
        out['ret'][k, e] += r[e]
        out['length'][k, e] += 1
        disc[e] = disc[e] + w[e] * float(r[e])
        w[e] = w[e] * gamma


def evaluate_calm(grid, seed, n, env_id0, q, K, L, gamma=1.0, first_state=None, log=None):
    """n envs on the C.Grid `grid`, the first the global id env_id0.  Returns the dict of VecGridUniverse.evaluate."""
    log = new_log() if log is None else log
    out, idx, gamma = _empty(K, n), np.arange(n), float(gamma)
    term = (np.asarray(grid.goal) | np.asarray(grid.lava)) != 0
    for k in range(K):
        st = C.State(n, env_id0)
        st.episode[:] = k
        pos = C.reset(grid, seed, st)
        log['starts'] |= set(pos.tolist())
        if first_state is not None:
            pos = np.array(first_state[k], np.int32)
        done = term[pos].copy()
        disc, w = [0.0] * n, [1.0] * n
        for i in range(L):
            alive = ~done
            if not alive.any():
                break
            rows = q[idx, pos]
            log['ties'] += int(((rows == TD.row_max(rows)[:, None]).sum(axis=1)[alive] > 1).sum())
            act = np.argmax(rows, axis=1).astype(np.int32)
            s2, r, d = C.look_step_ahead(grid, pos, act, True)
            pos = np.where(alive, s2, pos).astype(np.int32)
            done = np.where(alive, d != 0, done)
            _sum(out, k, alive, r, w, disc, gamma)
        out['discounted'][k] = disc
        _finish(out, k, grid, None, done, pos, 0)
        log['outcomes'] |= set(out['outcome'][k].tolist())
    return out


def evaluate_overlay(kind, name, env_id0, q, K, L, gamma=1.0, first_state=None, n=OS.N, seed=OS.SEED, log=None):
    """n envs under `kind` on grid `name` of tests/_overlay_starts.py (plane and parameters as its oracle() gives them)."""
    # a restatement of our own: the caller's is not touched
    return evaluate_with(OS.oracle(kind, name, env_id0, n=n, seed=seed, q0=None), kind, q, K, L, gamma, first_state, log)


def evaluate_with(o, kind, q, K, L, gamma=1.0, first_state=None, log=None):
    """The walk on a fresh restatement `o` of `kind` (an OverlayOracle without tables), which it uses up."""
    log = new_log() if log is None else log
    grid, st, n = o.grid, o.state, o.n
    out, idx, gamma = _empty(K, n), np.arange(n), float(gamma)
    term = (np.asarray(grid.goal) | np.asarray(grid.lava)) != 0
    for k in range(K):
        st.episode[:] = k
        st.done[:] = 0
        o.reset()  # the kind's reset word (the errands' draw at count k), then the C oracle's start at count k
        log['starts'] |= set(st.pos.tolist())
        if first_state is not None:
            st.pos[:] = first_state[k]
        done = term[st.pos].copy()
        disc, w = [0.0] * n, [1.0] * n
        for i in range(L):
            alive = ~done
            if not alive.any():
                break
            st.tcount[:] = k * L + i
            before, pos0 = o._row(st.pos), st.pos.copy()
            rows = q[idx, before]
            log['ties'] += int(((rows == TD.row_max(rows)[:, None]).sum(axis=1)[alive] > 1).sum())
            act = np.argmax(rows, axis=1).astype(np.int32)
            pos, r, d = o._move(act, alive)
            log['bumps_that_changed_row'] += int((alive & (pos == pos0) & (o._row(st.pos) != before)).sum())
            done = np.where(alive, d != 0, done)
            _sum(out, k, alive, r, w, disc, gamma)
        out['discounted'][k] = disc
        masks = OS.masks_of(o, kind)
        _finish(out, k, grid, None, done, st.pos.copy(), 0 if masks is None else np.asarray(masks, np.uint32))
        log['outcomes'] |= set(out['outcome'][k].tolist())
    log['gust_moved'] += o.log.get('gust_moved', 0)
    log['drawn'] |= o.log.get('drawn', set())
    return out


def same(got, want):
    """All six arrays of an evaluation, compared as bytes."""
    for key in KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == DTYPES[key] and g.shape == w.shape, (key, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.astype(DTYPES[key]).tobytes(), '%s differs at %s' % (key, np.argwhere(g != w)[:6].tolist())


# ---- the learning claim (tests/test_gpu_eval.py): 64 distinct 7 x 7 mazes of the host generator, one Q-learner each, alpha 0.5, gamma
# 0.95, epsilon 0.1; after CLAIM_STEPS steps every learner's greedy walk reaches its goal on a shortest path.  Measured with the
# restated learners (tests/_td_oracle.py; measure_claim below): the smallest multiple of 100 steps at which that holds for all 64 ----
CLAIM_LEVELS, CLAIM_W, CLAIM_H, CLAIM_MAZE_SEED = 64, 7, 7, 23
CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16 = 0.5, 0.95, 6554  # eps 0.1
CLAIM_MEASURED = {0: 3200, 1: 3400, 2: 3200}  # seed: measure_claim(seed)
CLAIM_STEPS = 2 * max(CLAIM_MEASURED.values())  # 6800: twice the largest, the margin of the project's other claims


def claim_grids():
    """The first CLAIM_LEVELS DISTINCT mazes of the generator's sequence (a 7 x 7 maze has nine rooms: the sequence repeats itself early)."""
    grids, seen, k = [], set(), 0
    while len(grids) < CLAIM_LEVELS:
        wall, start, goal = C.generate_maze(CLAIM_MAZE_SEED, k, CLAIM_W, CLAIM_H)
        key = tuple(np.flatnonzero(wall).tolist())  # (distinct by their walls alone)
        if key not in seen:
            seen.add(key)
            grids.append(dict(W=CLAIM_W, H=CLAIM_H, starts=[start], goals=[goal], lava=[], walls=list(key)))
        k += 1
    return grids


def measure_claim(seed, every=100, cap=20000):
    """The smallest multiple of `every` steps at which every restated learner walks a shortest path to its goal."""
    from ._tabular_cases import _grid
    from ._walks import _shortest_from_start
    grids = [_grid(g) for g in claim_grids()]
    best = [_shortest_from_start(g) for g in grids]
    learners = [TD.TdOracle(g, seed, 1, env_id0=k) for k, g in enumerate(grids)]
    for o in learners:
        o.reset()
    for steps in range(every, cap + 1, every):
        ok = True
        for o, b in zip(learners, best):
            o.run(every, TD.Q_LEARNING, CLAIM_ALPHA, CLAIM_GAMMA, CLAIM_EPS_Q16)
            got = evaluate_calm(o.grid, seed, 1, int(o.env_ids[0]), o.q, 1, o.grid.S, CLAIM_GAMMA)
            ok = ok and got['outcome'][0, 0] == 1 and got['length'][0, 0] == b
        if ok:
            return steps
    return None
