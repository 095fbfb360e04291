"""The case scaffold of the rollout launch-shape tests (tests/test_gpu_wide_stores.py, tests/test_gpu_launch_shapes.py): an engine and
its oracle, one launch compared with the C oracle in the row layout the case asks for, the launches of a case on one engine, the forms
the planner is expected to report, and the planner's own arithmetic (csrc/gu_rollout_plan.hpp) on the device's CU count and LDS size.

Every comparison is byte equality with oracle.c_oracle -- never with another kernel, layout or shape."""
import numpy as np

from griduniverse_amd import Engine, GridSpec
from oracle import c_oracle as C
from tests._mazes import oracle_grid

LAUNCHES = (21, 67)
POLICIES = ['uniform', 'stream', 'greedy', 'sample']
STATE_KEYS = ('pos', 'done', 'episode', 'tcount')
TRIPLES = 'triples'  # the `layout` of int32 rows under the option traj_layout = 1 (read back like int32 rows)


def spec_of(meta):
    return GridSpec(meta['W'], meta['H'], meta['starts'], meta['goals'], meta['lava'], meta['walls'], meta['reward'])


def _policy_table(policy, S, seed=3):
    """greedy: a one-hot policy (the oracle follows `pi`, the engine its argmax); sample: rows with exact zeros and ones among them."""
    rs = np.random.RandomState(seed)
    if policy == 'greedy':
        return np.eye(4)[rs.randint(0, 4, S)]
    if policy == 'sample':
        pi = rs.dirichlet(np.ones(4) * 0.5, S)
        hot = rs.rand(S) < 0.35
        pi[hot] = np.eye(4)[rs.randint(0, 4, int(hot.sum()))]
        return pi
    return None


def _diff(got, want):
    """What differs, for the assertion message: how many words, and in which lanes of sixteen (the hazard's signature: 12 .. 15)."""
    bad = np.asarray(got) != np.asarray(want)
    lanes = np.bincount(np.nonzero(bad)[-1] % 16, minlength=16) if bad.ndim else bad
    return '%d of %d words differ; by env %% 16: %s' % (int(bad.sum()), bad.size, lanes.tolist())


def _oracle_and_engine(meta, N, seed, env_id0=0):
    grid = C.Grid.from_lists(**meta)
    st = C.State(N, env_id0)
    eng = Engine(N, spec_of(meta), seed=seed, env_id0=env_id0)
    assert np.array_equal(eng.reset(), C.reset(grid, seed, st))
    return grid, st, eng


def _multi_oracle_and_engine(specs, N, seed, env_id0=0):
    """Engine on several grids (env e on specs[e // (N // len(specs))]) and one oracle (grid, state, env slice) per grid."""
    group = N // len(specs)
    eng = Engine(N, specs[0], seed=seed, env_id0=env_id0)
    eng.set_grids(specs)
    first = eng.reset()
    parts = []
    for g, spec in enumerate(specs):
        sl = slice(g * group, (g + 1) * group)
        grid, st = oracle_grid(spec), C.State(group, env_id0 + g * group)
        assert np.array_equal(C.reset(grid, seed, st), first[sl]), g
        parts.append((grid, st, sl))
    return parts, eng


def _launch_and_compare(eng, parts, seed, T, policy, auto, expect, tag, table=None, acts_seed=0, layout=TRIPLES, stats=True):
    """One launch of T steps: the form is `expect`, rows / statistics / state are the oracle's (parts: (grid, state, env slice)).
    layout: TRIPLES or True -- int32 rows (which of the two the launch wrote is the traj_layout option's business and `expect`'s), read
    with read_trajectory; 'packed' -- one word per env-step, read with read_trajectory_packed; False -- no rows: statistics, state,
    read_outputs() and done_indices() are what is compared."""
    acts = None
    if policy == 'stream':
        acts = np.random.RandomState(1000 + acts_seed).randint(0, 4, (T, eng.N)).astype(np.int32)
        eng.upload_actions(acts)
    eng.rollout(T, policy, auto, True if layout == TRIPLES else layout, stats=stats)
    form = eng.rollout_last_form()
    assert {k: form[k] for k in expect} == expect, (tag, T, form)
    got = None if layout is False else eng.read_trajectory_packed(0, T) if layout == 'packed' else eng.read_trajectory(0, T)
    ret, eps = eng.read_stats() if stats else (None, None)
    state = eng.get_state()
    outputs = eng.read_outputs() if layout is False else None
    for grid, st, sl in parts:
        kw = dict(actions=acts[:, sl]) if acts is not None else dict(pi=table) if table is not None else {}
        want = C.rollout(grid, seed, st, T, auto, stats=True, **kw)
        if got is not None:
            for k in ('obs', 'reward', 'done'):
                assert np.array_equal(got[k][:, sl], want[k]), (tag, T, k, sl, _diff(got[k][:, sl], want[k]))
        if stats:
            assert np.array_equal(ret[sl], want['ret']) and np.array_equal(eps[sl], want['episodes']), (tag, T, 'statistics', sl)
        for k in STATE_KEYS:
            assert np.array_equal(state[k][sl], getattr(st, k)), (tag, T, k, sl)
        if outputs is not None:
            for k, o, w in zip(('obs', 'reward', 'done'), outputs, (st.pos, want['reward'][-1], st.done)):
                assert np.array_equal(o[sl], w), (tag, T, 'outputs', k, sl)
    if layout is False:
        done = np.zeros(eng.N, np.int32)
        for _, st, sl in parts:
            done[sl] = st.done
        assert np.array_equal(eng.done_indices(), np.flatnonzero(done)), (tag, T, 'done compaction')


def _run(eng, parts, seed, policy, auto, expect, tag, table=None, launches=LAUNCHES, layout=TRIPLES, stats=True, reserve=None, after=None):
    """The launches of every case on one engine, each continuing the one before; `expect`: the form, or launch index -> form.
    reserve: rows of the trajectory buffer (default: the longest launch; none for a case without rows); after(eng, parts): further
    checks on the engine behind the last launch."""
    with eng:
        if layout is not False:
            eng.reserve_trajectory(max(launches) if reserve is None else reserve)
        if table is not None:
            eng.vi_set(np.zeros(table.shape[0]), table)
        for i, T in enumerate(launches):
            _launch_and_compare(eng, parts, seed, T, policy, auto, expect(i) if callable(expect) else expect, tag, table, acts_seed=i, layout=layout,
                                stats=stats)
        if after is not None:
            after(eng, parts)


def _general(map_, block, **bits):
    form = dict(family='general', layout=3, map=map_, block=block, pair=False, half=False, per_wave=False, straddle=False)
    form.update(bits)
    return form


# ---- the planner's arithmetic (csrc/gu_rollout_plan.hpp), on what Engine.device_info() reports ------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def rows_shape(info, N, S, row_bytes, max_copies):
    """gu_rows_shape: (workgroup, copies) of the transition-row table of an S-cell grid, or None where it does not fit."""
    for bs in (256, 512):
        per_cu = ceil_div(ceil_div(N, bs), info['cus'])
        c = max_copies
        while c >= 1:
            if S * row_bytes * c * per_cu <= info['lds_per_cu'] - 2048:
                return bs, c
            c >>= 1
    return None


def kstep_shape(info, N, S, only_k=0):
    """gu_multi_shape with one copy of the table: (K, workgroup), or None."""
    for bs in (256, 512, 1024):
        per_cu = ceil_div(ceil_div(N, bs), info['cus'])
        for k in (4, 2):
            if only_k and only_k != k:
                continue
            if S * ((4 << (2 * k)) + 16) * per_cu <= info['lds_per_cu'] - 2048:
                return k, bs
    return None


def stream_words(info, N, S, block, T):
    """gu_plan_general, MAP 1, a caller's stream with rows: action words staged per lane (0: none are)."""
    lds = 2 * ((S + 15) & ~15)
    per_cu = min(8, max(1, ceil_div(ceil_div(N, block), info['cus'])))
    kw = min((info['lds_per_cu'] // per_cu - lds - 512) // (block * 4), 64, ceil_div(T, 16))
    return kw if kw >= 4 else 0


def staging_class(n_src, block, rows_written):
    """The straight-line variant by which gu_rollout_rows_kernel stages n_src source rows with a workgroup of `block`: 1, 2, 4 or 8
    rows per thread, 'wide' (the loop's first two stages cover the table) or 'wide+loop' (the loop iterates beyond them)."""
    rows_total = ceil_div(n_src, block)
    for nb in (1, 2, 4) + ((8,) if rows_written else ()):
        if rows_total <= nb:
            return nb
    return 'wide+loop' if n_src > 2 * (12 if rows_written else 4) * block else 'wide'
