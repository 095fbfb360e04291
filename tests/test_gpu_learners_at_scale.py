"""The batched learners where their other tests never go: on one shared grid too large for LDS, and with per-env stores larger than
2^32 bytes and 2^31 elements.  Every comparison is byte for byte against the learner's own CPU restatement (tests/_*_oracle.py).

Part A -- a shared grid beyond LDS, N = 130 (three waves, the last partial).  `big182` (182 x 182, 33 124 states: the smallest square
past GU_MAX_LDS_CELLS = 32 767) sends every learner to its L2 instantiation with the arithmetic move deltas; the cells where the envs
start lie past 32 767 and the table rows s * 4 past 2^17.  td_run also runs on 40 000 x 1 (W fits no int16 delta) and 33 000 x 2
(cells past 65 535).  No learner has a probe that reports the kernel chosen: the choice follows from gu_lds_block (gu_rollout_plan.hpp),
which returns 0 for S > GU_MAX_LDS_CELLS, and gu_tabular_launch, which then launches the L2 form; each case asserts S > 32 767.
sweep_run refuses big182 (its keys hold 16-bit pair indices: at most 16 384 states, include/gu.h) and test_gpu_sweep.py runs it at that
limit; no other learner refuses it.

Part B -- per-env stores across 2^32 bytes.  Each case picks the smallest batch at which the store named passes 2^32 bytes with room
for a group of envs on both sides of the crossing, asserts that arithmetic, and compares three or more groups of envs -- the first,
the last, and those around every crossing -- with a restatement built at the group's first env id: the group's slice of every store
(getter with (env0, n)), its columns of the statistics and its env state.  No store is read whole and no rows are written.
    store                                     owner                      bytes per env      grid        crossing near env
    Q                                         td_run (both methods)      32 S               big182      4 051
    Q through another kernel's TabLane        nstep_run                  32 S               big182      4 051
    cumulative weights c (and Q)              is_run                     32 S               big182      4 051
    feature weights w, one-hot (F = S)        fa_run                     32 F               big182      4 051
    model u64, list i32 (seen: S bytes)       dyna_run                   32 S, 16 S         big182      4 051, 8 103
    visit counts (and Q)                      explore_run                16 S               big182      8 103 (Q: 4 051)
    actor h, critic v                         ac_run                     32 S, 8 S          big182      4 051, 16 207
    heap u64 x (4 S + 2), model, Q            sweep_run                  524 304, 524 288   128 x 128   8 191, 8 192
    node pool, 64 B x 256 (mcts_init(255))    mcts_run                   16 384             4 x 4       262 144
    episode buffers [L][N] x 8 B, L = 1024    reinforce_run, is_run      step-major         5 x 5       entry 2^29: row 894
Part C -- 2^31 elements: td_run on big182 with 16 389 envs, whose tables hold more than 2^31 doubles (17.4 GB); the crossing is at
env 16 207.  (ac_run's actor in Part B passes it at the same env.)

Left out: the n-step windows (16 entries of 8 bytes per env: 2^32 bytes are 2^25 envs, the engine's cap, and the store has to pass
it), the search scores (32 bytes per env: 2^27 envs), the MCTS meta store (8 bytes x 256 per env: 2^21 envs, whose node pool alone
is 34 GB) and the lambda windows (64 entries of 4 bytes per env: 2^24 envs and more, half the engine's cap; a batch of that size
belongs to a test of its own).  All four are compared whole at N = 130 in Part A.  The sweep's positions (16 S bytes per env) cross
at 16 384 envs, where the whole engine would need 35 GB: they ride along below 2^32.

Peak device memory, from the shapes: Part A under 0.2 GB; Part B 22.0 GB (dyna_run: 81 S bytes x 8 200 envs) and 21.7 GB (ac_run);
Part C 17.4 GB.  One engine is alive at a time.  A case whose tables the library refuses for want of memory (GU_ERR_NOMEM) skips with
the library's message: it proves nothing then.

The adapters that say how to drive each learner and its restatement, and the two harnesses below them (_shared_grid_beyond_lds,
_stores_past_a_boundary), are in tests/_learners.py.
"""
import numpy as np
import pytest

import griduniverse_amd as gua

from ._learners import (LEARNERS, Q0, Ac, Dyna, Is, Mcts, Reinforce, Sweep, Td, _crossing, _shared_grid_beyond_lds, _stores_past_a_boundary,
                        big182, no_way_out, sweep128)
from ._tabular_cases import GRIDS, _grid, _spec, spread_grid

pytestmark = pytest.mark.gpu

ERR_INVALID = -1


def _heap_is_a_heap_of(raw, key, where):
    """diag_sweep_heap of some envs against their keys [n][S][4]: a 1-based max-heap of exactly the queued keys, pos its inverse."""
    key = key.reshape(len(key), -1)
    heap, pos = raw['heap'], raw['pos']
    assert heap.shape == (len(key), key.shape[1] + 2) and pos.shape == key.shape, where
    for e in range(len(key)):
        queued = np.flatnonzero(key[e])
        n = len(queued)
        i = np.arange(2, n + 1)
        assert (heap[e, i >> 1] >= heap[e, i]).all(), (where, e)
        assert sorted(heap[e, 1:n + 1].tolist()) == sorted(key[e, queued].tolist()), (where, e)
        assert (pos[e, queued] >= 1).all() and (pos[e, queued] <= n).all(), (where, e)
        assert ((heap[e, pos[e, queued]] & np.uint64(0xFFFF)) == queued.astype(np.uint64)).all(), (where, e)
        assert (np.delete(pos[e], queued) == -1).all(), (where, e)


# ---------------------------------------------------------------------------------------------------------------- Part A
# (not 'sweep': it refuses big182, below; 'expected_sarsa' and 'double_q' run from test_gpu_double.py)
PART_A = dict((name, LEARNERS[name]) for name in (
    'td-q_learning', 'td-sarsa', 'nstep-q_learning', 'nstep-sarsa', 'lambda-q_learning', 'lambda-sarsa', 'dyna', 'explore-ucb',
    'explore-thompson', 'search', 'mcts', 'is', 'ac', 'reinforce', 'fa-q_learning', 'fa-sarsa'))


@pytest.mark.parametrize('name', sorted(PART_A))
def test_a_shared_grid_beyond_lds(name):
    _shared_grid_beyond_lds(PART_A[name], big182(), 32768)


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('W,H,bar', [(40000, 1, 32768), (33000, 2, 65536)])
def test_a_td_on_wide_grids(W, H, bar, method):
    """40 000 x 1: a step down or up the rows is W cells, more than an int16 delta holds.  33 000 x 2: cells past 65 535."""
    _shared_grid_beyond_lds(Td(method), spread_grid(W, H), bar)


def test_a_sweep_refuses_a_grid_of_more_than_16384_states():
    """The queue's keys hold 16-bit pair indices (include/gu.h: gu_sweep_init); the largest grid it takes, 128 x 128, runs in
    test_gpu_sweep.py and, past 2^32 bytes, in Part B below."""
    vec = gua.VecGridUniverse(130, template=_spec(big182()), seed=3)
    try:
        vec._ensure_q(Q0)
        with pytest.raises(gua.GuError) as err:
            vec.sweep_run(10, 2)
        assert err.value.code == ERR_INVALID
        vec.dyna_run(10, 2)  # (the model alone has no such limit)
    finally:
        vec.close()


# ---------------------------------------------------------------------------------------------------------------- Part B, Part C
S182 = 182 * 182


@pytest.mark.parametrize('name', ['td-q_learning', 'td-sarsa', 'nstep-sarsa', 'is', 'fa-sarsa'])
def test_b_tables_of_32_S_bytes_per_env(name):
    """Q [N][S][4] under td_run's kernels and, through TabLane, under nstep_run's; is_run's cumulative weights beside it; fa_run's
    weights [N][F][4] with F = S.  4 165 envs: 4.41 GB per table."""
    N, per_env = 4165, 32 * S182
    e = _crossing(per_env, N)
    assert e == 4051 and _grid(big182()).S == S182
    _stores_past_a_boundary(PART_A[name], big182(), N, [e], (30, 20))


def test_b_dyna_model_and_list():
    """model uint64 [N][S][4] (and Q) cross at env 4 051, list int32 [N][4 S] at env 8 103; seen uint8 [N][S] rides along (it
    shows in the model the getter unpacks).  81 S bytes x 8 200 envs = 22.0 GB."""
    N = 8200
    crossings = [_crossing(32 * S182, N), _crossing(16 * S182, N)]
    assert crossings == [4051, 8103] and (32 + 32 + 16 + 1) * S182 * N < 24 << 30
    _stores_past_a_boundary(Dyna(), big182(), N, crossings, (20, 10))


def test_b_visit_counts():
    """counts uint32 [N][S][4] cross at env 8 103 (Q at 4 051).  48 S bytes x 8 200 envs = 13.0 GB."""
    N = 8200
    crossings = [_crossing(32 * S182, N), _crossing(16 * S182, N)]
    assert crossings == [4051, 8103]
    _stores_past_a_boundary(PART_A['explore-ucb'], big182(), N, crossings, (30, 20))


def test_b_actor_and_critic():
    """h float64 [N][S][4] crosses 2^32 bytes at env 4 051 (and 2^31 elements at 16 207), v float64 [N][S] crosses 2^32 bytes at
    env 16 207.  40 S bytes x 16 400 envs = 21.7 GB."""
    N = 16400
    crossings = [_crossing(32 * S182, N), _crossing(8 * S182, N)]
    assert crossings == [4051, 16207] and 4 * S182 * N > 2 ** 31 and 40 * S182 * N < 24 << 30
    _stores_past_a_boundary(Ac(), big182(), N, crossings, (30, 20))


def test_b_sweep_heap():
    """128 x 128, the largest grid sweep_run takes: heap uint64 [N][4 S + 2] crosses at env 8 191, the model and Q (32 S bytes per
    env) at 8 192: one group holds both.  The positions (16 S bytes per env) would cross at 16 384 envs, where the engine needs
    35 GB: left below 2^32.  129 S bytes x 8 270 envs = 17.5 GB."""
    S, N = 128 * 128, 8270
    e = _crossing(8 * (4 * S + 2), N)
    assert e == 8191 and _crossing(32 * S, N) == 8192 and 16 * S * N < 2 ** 32 and 129 * S * N < 24 << 30
    learner = Sweep()
    _stores_past_a_boundary(learner, sweep128(), N, [e], learner.T,
                            after=lambda tag, e0, o, got: _heap_is_a_heap_of(learner.raw, o.key, (tag, e0)))


def test_b_mcts_node_pool():
    """mcts_init(255): 256 nodes of 64 bytes per env, the pool crosses at env 262 144.  The meta store (8 bytes a node) would take
    eight times the envs and a pool of 34 GB: left out.  4.30 GB of pool."""
    N, P = 262346, 256
    e = _crossing(64 * P, N)
    assert e == 262144 and 8 * P * N < 2 ** 32
    _stores_past_a_boundary(Mcts(255), GRIDS['default4x4'](), N, [e], (6, 4))


@pytest.mark.parametrize('name', ['reinforce', 'is'])
def test_b_episode_buffers(name):
    """[L][N] entries of 8 bytes, step-major: entry k of env e at k * N + e, so byte 2^32 is entry 2^29, in row k* = 2^29 // N at
    env e* = 2^29 - k* N.  No episode ends on the grid, so every env's buffer fills: after 1 023 steps the getter shows L - 1
    entries (rows 0 .. 1 022, past k* = 894) -- a count never reads L, because the step that appends entry L - 1 runs the backward
    pass and empties the buffer --, and after 7 more the tables hold that pass over the rows and the buffer 6 new entries.
    reinforce_run's pass reads every row.  is_run's stops at the first action that is no longer greedy or where the weight
    passes w_cap, which tables of one value (every action tied: a ratio of 4 a step) reach within 32 rows: its groups get untied
    pessimistic tables and a greedy behaviour policy, under which the passes read down to row 0.  4.92 GB of buffers."""
    L, N = 1024, 600010
    assert 8 * L * N > 2 ** 32
    k, e = divmod(2 ** 29, N)
    assert k * N + e == 2 ** 29 and (k, e) == (894, 461972) and k < L - 2  # (the crossing lies in a row that every env writes)
    assert 192 <= e <= N - 192  # (the three groups are apart)
    learner = {'reinforce': Reinforce, 'is': Is}[name]()
    learner.L, learner.install = L, None
    before = None
    if name == 'is':
        learner.eps = 0.0

        def before(vec, e0, o):  # (these groups do not overlap: asserted below)
            q = -20.0 - 10.0 * np.random.RandomState(e0).random_sample(o.q.shape)
            vec.set_q_table(q, env0=e0)
            o.set_q(q)

    def after(tag, e0, o, got):
        assert (got['buffer.count'] == {'launch 0': L - 1, 'launch 1': 6}[tag]).all(), (tag, e0)
        if name == 'is' and tag == 'launch 1':
            assert o.passes == o.n and o.walked > o.passes * (L - k)  # some pass read rows below the crossing

    _stores_past_a_boundary(learner, no_way_out(), N, [e], (L - 1, 7), before=before, after=after)


def test_c_more_than_2_31_table_entries():
    """td_run on big182 with 16 389 envs: N S 4 > 2^31 doubles, 17.4 GB; entry 2^31 lies in the table of env 16 207."""
    N = 16389
    assert N * S182 * 4 > 2 ** 31
    e = 2 ** 31 // (4 * S182)
    assert e == 16207
    _stores_past_a_boundary(Td('q_learning'), big182(), N, [e], (30, 20))
