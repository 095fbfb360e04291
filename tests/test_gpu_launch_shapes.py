"""The launch shapes of the three rollout kernels that only batch size or options reach, each against the C oracle.

gu_rollout_plan() (csrc/gu_rollout_plan.hpp) picks the general kernel, the transition-row kernel (gu_rollout_rows.hip) or the K-step
kernel (gu_rollout_multi.hip) and a shape for it: workgroup size, copies of the table across the LDS banks, staging variant, env-block
order, staged stream words.  tests/test_rollout_plan.py pins the planner on the host; tests/test_gpu_wide_stores.py runs the shapes of
the int32 triples.  This file runs what was left: the row kernel at a workgroup of 512, the K-step kernel at 512 and 1024, every copy
count of the row tables and the store form and staging variant each selects, the XCD env-block order (rollout_xcd = 1) on all three
kernels, staged action words at workgroups other than 256, and the general kernel's planes, packed rows and statistics-only launches
at workgroups other than 256.

Every case: byte equality with oracle.c_oracle (integers, no tolerance; never another kernel, layout or shape as the reference) of
rows, statistics and final state, and without rows of read_outputs() and the done compaction; two launches on one engine, T = 21 and
then T = 67 continuing it (the stream and K-step cases state their own), auto-reset on and off; a non-zero env_id0; a fresh engine per
shape; options through the gu_option fixture.  After each launch Engine.rollout_last_form() must name the shape the case is about --
family, workgroup, workgroups, K, row_shift, the xcd_remap flag, stream words: a case whose shape the planner does not produce FAILS.
Batch sizes and expected forms come from Engine.device_info() by the planner's own arithmetic (tests/_rollout_shapes.py); where a
staging variant of the row kernel is the target, the test computes the class its source rows per thread fall in and asserts it.

A distinct walk per env: the uniform, stream and sample policies draw per env; under the greedy policy the envs are placed on cells of
their own (set_state) -- one start cell would be one walk N times over, and a permuted or dropped env block would not show.

FOUND by the first run of this file: test_general_kernel_layouts_at_other_workgroup_sizes[1024-stream-stats] -- the general kernel's
statistics-only stream launch without auto-reset lost envs at workgroups of 512 and 1024 (never at 64 or 256), in some launches only:
2 .. 24 of 40 fresh engines, depending on the grid; 6 .. 61 envs of one or two waves left the grid in the 45th step of the 67-step
launch, by lut >> lane.  That instantiation kept the amount of one of its 84 64-bit LUT shifts in v63, the last of its 64 registers, and
gfx950 now and then shifts by what lies behind the allocation instead (csrc/gu_map.hpp, gu_delta; docs/HISTORY.md).  The same build
with one more register allocated, the instruction unchanged, failed 0 of 120 times against 39 of 120.  The launches without int32 rows
now look the delta up in 32-bit halves, and tests/test_shift_amount_register.py reads every build back for such a shift."""
import numpy as np
import pytest

from griduniverse_amd import Engine, GridSpec
from oracle import c_oracle as C
from tests import _golden as G
from tests._mazes import oracle_grid
from tests._rollout_shapes import (LAUNCHES, POLICIES, STATE_KEYS, TRIPLES, _general, _policy_table, _run, ceil_div, kstep_shape, rows_shape, spec_of,
                                   staging_class, stream_words)

pytestmark = pytest.mark.gpu

LAYOUT_CODE = {False: 0, True: 1, 'packed': 2, TRIPLES: 3}  # Engine.rollout_last_form()['layout']
LAYOUT_ID = {False: 'stats', True: 'planes', 'packed': 'packed', TRIPLES: 'triples'}
ROW_LOG2 = dict(uniform=4, stream=4, greedy=2, sample=5)    # log2 of the bytes of one transition row (gu_plan_rows)
MAX_COPIES = dict(uniform=8, stream=8, greedy=16, sample=4)  # gu_rows_max_copies
BIG_W, BIG_H = 182, 181  # the grid of tests/test_gpu_wide_stores.py that is too big for two planes in 64 KiB
SEED, ENV_ID0 = 41, 70007


def _log2(v):
    assert v > 0 and v & (v - 1) == 0, v
    return v.bit_length() - 1


def _grid(W, H):
    """W x H, one start cell in the middle, the goal two moves to its right and a lava cell above it (random walks end within a few
    steps, again and again), S // 16 walls anywhere else."""
    S, start = W * H, (H // 2) * W + W // 2
    keep = {start, start + 1, start + 2, start - W, start - 1, start + W}
    rs = np.random.RandomState(S)
    walls = [int(c) for c in rs.choice(S, S // 16, replace=False) if int(c) not in keep]
    return GridSpec(W, H, [start], [start + 2], [start - W], walls)


def _golden_spec(name):
    return spec_of(G.load_traj(name)[0])


def _place(eng, st, spec, seed):
    """Every env on a non-terminal open cell of its own choice (distinct cells while the grid has enough of them), every fourth on a
    cell next to a start, goal or lava cell, so that episodes end and begin under a table policy too."""
    N = st.n
    free = np.flatnonzero(~(spec.wall | spec.goal | spec.lava))
    rs = np.random.RandomState(seed)
    pos = rs.choice(free, N, replace=N > free.size)
    hubs = np.concatenate([np.flatnonzero(spec.goal | spec.lava), np.asarray(spec.starts)])
    near = np.intersect1d(free, np.concatenate([hubs + d for d in (1, -1, spec.W, -spec.W)]))
    if near.size:
        pos[1::4] = rs.choice(near, pos[1::4].size)
    st.pos[:] = pos
    eng.set_state(pos=st.pos)


def _table(policy, spec):
    """The policy table of a case; the greedy one leads from every open cell beside a goal or lava cell into it (a one-hot table drawn
    at random may reach no terminal cell at all, and the placed envs next to one should end their episodes)."""
    table = _policy_table(policy, spec.S)
    if policy == 'greedy':
        open_ = ~(spec.wall | spec.goal | spec.lava)
        for hub in np.flatnonzero(spec.goal | spec.lava):
            for act, delta in enumerate((-spec.W, 1, spec.W, -1)):  # up, right, down, left
                cell = int(hub) - delta
                if 0 <= cell < spec.S and open_[cell] and (abs(delta) != 1 or cell // spec.W == hub // spec.W):
                    table[cell] = np.eye(4)[act]
    return table


def _case(spec, N, policy, place_seed=0):
    """(parts, engine, policy table) of one shape: a fresh engine behind reset(), its oracle, the envs placed under the greedy policy."""
    grid, st = oracle_grid(spec), C.State(N, ENV_ID0)
    eng = Engine(N, spec, seed=SEED, env_id0=ENV_ID0)
    assert np.array_equal(eng.reset(), C.reset(grid, SEED, st))
    if policy == 'greedy':
        _place(eng, st, spec, N + place_seed)
    return [(grid, st, slice(None))], eng, _table(policy, spec)


def _rows_form(layout, block, workgroups, row_shift, pair=False, half=False, xcd=False):
    return dict(family='rows', layout=LAYOUT_CODE[layout], map=-1, block=block, workgroups=workgroups, K=0, row_shift=row_shift, stream_words=0, pair=pair,
                half=half, per_wave=False, straddle=False, xcd_remap=xcd)


def _kstep_form(K, block, workgroups, xcd=False):
    return dict(family='kstep', layout=0, map=-1, block=block, workgroups=workgroups, K=K, row_shift=2 * K + 2, stream_words=0, pair=False, half=False,
                per_wave=False, straddle=False, xcd_remap=xcd)


def _general_form(layout, map_, block, N, words=0, xcd=False):
    return _general(map_, block, layout=LAYOUT_CODE[layout], workgroups=ceil_div(N, block), K=0, row_shift=0, stream_words=words, xcd_remap=xcd)


def _options(gu_option, **values):
    for name, value in values.items():
        gu_option(name, value)


# ---- 1. the transition-row kernel at a workgroup of 512 -----------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [False, 'packed', True, TRIPLES], ids=LAYOUT_ID.get)
@pytest.mark.parametrize('policy,W', [('uniform', 72), ('stream', 72), ('sample', 51), ('greedy', 150)])
def test_row_kernel_at_a_workgroup_of_512(gu_option, policy, W, layout):
    """gu_rows_shape grows the workgroup to 512 when one table takes more than half a CU's LDS and the batch needs more than one
    256-lane workgroup per CU: 256 x CUs + 64 envs on 72 x 72 (16-byte rows), 51 x 51 (the sampled policy's 32-byte rows) and 150 x 150
    (the greedy policy's dword rows: one copy, so also the dword-by-dword staging at 512).  The staging derives its rows per thread from
    blockDim.x: eleven per thread at 512 -- the wide variant, whose loop iterates when no rows are written (four rows in flight)."""
    _options(gu_option, rollout_rows=1, rollout_multi=0, traj_layout=1 if layout == TRIPLES else 0)
    info = Engine.device_info(0)
    N = 256 * info['cus'] + 64
    spec = _grid(W, W)
    shape = rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], MAX_COPIES[policy])
    assert shape is not None and shape[0] == 512, (shape, info)
    if policy == 'greedy':
        assert shape[1] < 4  # (fewer than four copies of a dword row: staged dword by dword)
    else:
        n_src = spec.S * (2 if policy == 'sample' else 1)
        assert staging_class(n_src, 512, layout is not False) == ('wide+loop' if layout is False else 'wide'), n_src
    expect = _rows_form(layout, 512, ceil_div(N, 512), ROW_LOG2[policy] + _log2(shape[1]))
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (policy, W, layout, auto), table, layout=layout)


# ---- 2. the K-step kernel at workgroups of 512 and 1024 ---------------------------------------------------------------------------
KSTEP_LAUNCHES = LAUNCHES + (130,)  # single steps, partial words and whole 16-step words


@pytest.mark.parametrize('policy,stats', [('uniform', True), ('uniform', False), ('stream', True)])
@pytest.mark.parametrize('factor,block', [(1, 512), (2, 1024)])
@pytest.mark.parametrize('grid,K', [('c3_maze32', 2), ('open12', 4)])
def test_k_step_kernel_at_workgroups_of_512_and_1024(gu_option, grid, K, factor, block, policy, stats):
    """gu_multi_shape grows the workgroup while the batch needs more workgroups per CU than tables fit its LDS: 32 x 32 at K = 2
    (80 bytes per cell) and 12 x 12 at a forced K = 4 (1040 bytes per cell) admit one table per CU, so 256 x CUs + 64 envs run at 512
    and twice as many at 1024.  Statistics, state, outputs and done compaction as in tests/test_gpu_kstep_kernel.py."""
    _options(gu_option, rollout_multi=1, rollout_multi_k=4 if K == 4 else None)
    info = Engine.device_info(0)
    N = factor * (256 * info['cus'] + 64)
    spec = _golden_spec(grid) if grid != 'open12' else _grid(12, 12)
    assert kstep_shape(info, N, spec.S, 4 if K == 4 else 0) == (K, block), info
    expect = _kstep_form(K, block, ceil_div(N, block))
    for auto in (True, False):
        parts, eng, _ = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (grid, N, policy, stats, auto), launches=KSTEP_LAUNCHES, layout=False, stats=stats)


# ---- 3. copies of the row table across the LDS banks ------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('copies', [1, 2, 4, 8, 16, 32])
def test_row_table_at_every_copy_count(gu_option, copies, policy):
    """rows_copies = 1 .. 32 on the one-step table of an 8 x 8 grid: the 16-byte places per source row (copies; a quarter of them for
    the greedy policy's dword rows) select the unrolled eight-way store, the unrolled four-way store or the loop (1, 2, 16, 32), and a
    greedy table of fewer than four copies is staged dword by dword.  Each lane then reads the copy its lane index names."""
    _options(gu_option, rollout_rows=2, rollout_multi=0, traj_layout=0, rows_copies=copies)
    info, N, spec = Engine.device_info(0), 2120, _golden_spec('c2_open8x8')
    assert rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], copies) == (256, copies), info
    expect = _rows_form(True, 256, ceil_div(N, 256), ROW_LOG2[policy] + _log2(copies))
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (copies, policy, auto), table, layout=True)


@pytest.mark.parametrize('policy', ['uniform', 'greedy'])
@pytest.mark.parametrize('copies', [1, 32])
def test_row_table_copies_under_half_waves(gu_option, copies, policy):
    """The smallest and the largest copy count with 32 envs per wave (rollout_half_waves = 1, 2080 = 65 x 32 envs): the lane's copy comes
    from threadIdx.x, its env from the half-wave slot."""
    _options(gu_option, rollout_rows=2, rollout_multi=0, traj_layout=0, rows_copies=copies, rollout_half_waves=1)
    info, N, spec = Engine.device_info(0), 2080, _golden_spec('c2_open8x8')
    assert rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], copies) == (256, copies), info
    expect = _rows_form(True, 256, ceil_div(N, 128), ROW_LOG2[policy] + _log2(copies), half=True)
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (copies, policy, auto), table, layout=True)


@pytest.mark.parametrize('W,copies', [(101, 2), (150, 1)])
def test_greedy_rows_staged_dword_by_dword_on_big_grids(gu_option, W, copies):
    """Without rows_copies the greedy table has fewer than four copies only where four do not fit a CU's LDS: above ~10 100 cells.
    101 x 101 keeps two copies, 150 x 150 one."""
    _options(gu_option, rollout_rows=1, rollout_multi=0, traj_layout=0)
    info, N, spec = Engine.device_info(0), 2120, _grid(W, W)
    assert rows_shape(info, N, spec.S, 4, MAX_COPIES['greedy']) == (256, copies), info
    expect = _rows_form(True, 256, ceil_div(N, 256), 2 + _log2(copies))
    for auto in (True, False):
        parts, eng, table = _case(spec, N, 'greedy')
        _run(eng, parts, SEED, 'greedy', auto, expect, (W, auto), table, layout=True)


# ---- 4. staging variants of the row kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [False, True], ids=LAYOUT_ID.get)
@pytest.mark.parametrize('policy,W', [('uniform', 20), ('sample', 14)])
def test_row_kernel_stages_two_rows_per_thread(gu_option, policy, W, layout):
    """257 .. 512 source rows under a workgroup of 256 (400 cells under the uniform policy, 2 x 196 units under the sampled one): the
    variant NB = 2 of the staging, which no other grid of the suite reaches."""
    _options(gu_option, rollout_rows=2, rollout_multi=0, traj_layout=0)
    info, N, spec = Engine.device_info(0), 2120, _grid(W, W)
    assert staging_class(spec.S * (2 if policy == 'sample' else 1), 256, layout is not False) == 2
    shape = rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], MAX_COPIES[policy])
    assert shape is not None and shape[0] == 256, info
    expect = _rows_form(layout, 256, ceil_div(N, 256), ROW_LOG2[policy] + _log2(shape[1]))
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (policy, W, layout, auto), table, layout=layout)


@pytest.mark.parametrize('policy,grid,layout', [('uniform', 'open80', True), ('sample', 'c5_maze64', True), ('uniform', 'c4_lava32', 'packed'),
                                                ('stream', 'c4_lava32', 'packed')])
def test_row_kernel_stages_in_a_loop_with_rows_written(gu_option, policy, grid, layout):
    """More than 24 source rows per thread of a launch that writes rows (twelve in flight): the loop behind the first two stages
    iterates -- 6400 one-step rows at 80 x 80, 8192 units of the sampled policy at 64 x 64, and the 9 S = 9216 units of the pair
    tables at 32 x 32 (packed rows; the image is copied as it stands, pair table and one-step table behind it)."""
    pair = layout == 'packed'
    _options(gu_option, rollout_rows=1 if pair else 2, rollout_multi=0, traj_layout=0)
    info, N = Engine.device_info(0), 2120
    spec = _grid(80, 80) if grid == 'open80' else _golden_spec(grid)
    assert staging_class(spec.S * (9 if pair else 2 if policy == 'sample' else 1), 256, True) == 'wide+loop'
    if pair:
        assert spec.S * 144 <= info['lds_per_cu'] - 2048 and ceil_div(N, 256) <= info['cus'], info
        expect = _rows_form(layout, 256, ceil_div(N, 256), 7, pair=True)
    else:
        shape = rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], MAX_COPIES[policy])
        assert shape is not None and shape[0] == 256, info
        expect = _rows_form(layout, 256, ceil_div(N, 256), ROW_LOG2[policy] + _log2(shape[1]))
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (policy, grid, auto), table, layout=layout)


# ---- 5. the XCD env-block order ----------------------------------------------------------------------------------------------------
def _step_behind(auto):
    """One step() with random actions behind the launches, against the oracle: the entry path behind a remapped launch."""
    def after(eng, parts):
        acts = np.random.RandomState(77).randint(0, 4, eng.N).astype(np.int32)
        got = eng.step(acts, auto_reset=auto)
        state = eng.get_state()
        for grid, st, sl in parts:
            want = C.rollout(grid, SEED, st, 1, auto, actions=acts[None, sl])
            for k, g in zip(('obs', 'reward', 'done'), got):
                assert np.array_equal(g[sl], want[k][0]), ('step', k)
            for k in STATE_KEYS:
                assert np.array_equal(state[k][sl], getattr(st, k)), ('step', k)
    return after


# shape -> (options, grid, (N with a multiple of eight workgroups, N without), layout, policies)
XCD_SHAPES = {
    'general-64': (dict(rollout_rows=0, rollout_block=64), 'c2_open8x8', (2040, 2120), True, POLICIES),
    'general-256': (dict(rollout_rows=0, rollout_block=256), 'c2_open8x8', (2040, 2120), True, POLICIES),
    'general-big': (dict(rollout_rows=0, rollout_block=256), 'big', (2040, 2120), True, POLICIES),
    'rows': (dict(rollout_rows=2), 'c2_open8x8', (2040, 2120), True, POLICIES),
    'rows-pair-half': (dict(rollout_rows=3, rollout_half_waves=1), 'c2_open8x8', (2016, 2080), 'packed', ['uniform', 'stream']),
    'kstep': (dict(rollout_multi=1), 'c2_open8x8', (2040, 2120), False, ['uniform', 'stream']),
}


@pytest.mark.parametrize('remap', [True, False], ids=['remap', 'ragged'])
@pytest.mark.parametrize('shape,policy', [(s, p) for s, v in XCD_SHAPES.items() for p in v[4]])
def test_xcd_env_block_order(gu_option, shape, policy, remap):
    """rollout_xcd = 1: workgroup b works on env block (b % 8) * (workgroups / 8) + b / 8 (gu_env_block) in all three kernels -- the
    general kernel on one grid in LDS at workgroups of 64 and 256 and on the 182 x 181 grid (its flags plane in LDS, or the records
    from L2 under the table policies), the row kernel on the one-step table and on pair tables under half waves (sixteen workgroups of
    128 envs), the K-step kernel.  2040 envs leave a ragged last workgroup and still a multiple of eight workgroups; 2120 (2080 under
    half waves) make nine (seventeen; 34 of 64 lanes): the planner must then clear the flag, and the results are the same."""
    options, grid, sizes, layout, _ = XCD_SHAPES[shape]
    _options(gu_option, rollout_xcd=1, rollout_multi=0, traj_layout=0)
    _options(gu_option, **options)
    info, N = Engine.device_info(0), sizes[0 if remap else 1]
    spec = GridSpec(BIG_W, BIG_H, [BIG_W * BIG_H - 3], [BIG_W * BIG_H - 1], [BIG_W * BIG_H - 3 - BIG_W], []) if grid == 'big' else _golden_spec(grid)
    if shape.startswith('general'):
        block = options['rollout_block']
        map_ = 1 if grid != 'big' else 3 if policy in ('uniform', 'stream') else 0
        assert (ceil_div(N, block) % 8 == 0) == remap
        words = {T: stream_words(info, N, spec.S, block, T) if policy == 'stream' and map_ == 1 else 0 for T in LAUNCHES}
        expect = lambda i: _general_form(layout, map_, block, N, words[LAUNCHES[i]], xcd=remap)  # noqa: E731
    elif shape == 'rows':
        assert rows_shape(info, N, spec.S, 1 << ROW_LOG2[policy], MAX_COPIES[policy]) == (256, MAX_COPIES[policy]), info
        assert (ceil_div(N, 256) % 8 == 0) == remap
        expect = _rows_form(layout, 256, ceil_div(N, 256), ROW_LOG2[policy] + _log2(MAX_COPIES[policy]), xcd=remap)
    elif shape == 'rows-pair-half':
        assert N % 32 == 0 and (ceil_div(N, 128) % 8 == 0) == remap
        expect = _rows_form(layout, 256, ceil_div(N, 128), 7, pair=True, half=True, xcd=remap)
    else:
        assert kstep_shape(info, N, spec.S) == (4, 256) and (ceil_div(N, 256) % 8 == 0) == remap, info
        expect = _kstep_form(4, 256, ceil_div(N, 256), xcd=remap)
    for auto in (True, False):
        parts, eng, table = _case(spec, N, policy)
        _run(eng, parts, SEED, policy, auto, expect, (shape, policy, N, auto), table, layout=layout, after=_step_behind(auto))


# ---- 6. staged action words at workgroups other than 256 -----------------------------------------------------------------------------
@pytest.mark.parametrize('layout', [True, 'packed'], ids=LAYOUT_ID.get)
@pytest.mark.parametrize('block', [64, 512, 1024])
@pytest.mark.parametrize('T', [2100, 1025])
def test_staged_action_words_at_other_workgroup_sizes(gu_option, T, block, layout):
    """A caller's stream with rows on the general kernel keeps its action words in LDS, as many per lane as the workgroup's share of a
    CU's LDS admits, 64 at most: 64 at workgroups of 64 and 512, fewer at 1024 (39 on 160 KiB: no power of two, the groups' boundaries
    fall elsewhere).  2100 steps are several groups and a partial last word, 1025 one group and one step (or 39 words, 26 and one
    step); a launch of 21 steps behind it stages nothing."""
    _options(gu_option, rollout_rows=0, traj_layout=0, rollout_block=block)
    info, N, spec = Engine.device_info(0), 300, _golden_spec('c3_maze32')
    launches = (T, 21)
    words = [stream_words(info, N, spec.S, block, t) for t in launches]
    assert 4 <= words[0] <= 64 and words[1] == 0 and (words[0] < 64 if block == 1024 else words[0] == 64), (words, info)
    for auto in (True, False):
        parts, eng, _ = _case(spec, N, 'stream')
        _run(eng, parts, SEED, 'stream', auto, lambda i: _general_form(layout, 1, block, N, words[i]), (T, block, layout, auto), launches=launches, layout=layout)


# ---- 7. the general kernel's other layouts at workgroups other than 256 ----------------------------------------------------------
@pytest.mark.parametrize('layout', [False, True, 'packed'], ids=LAYOUT_ID.get)
@pytest.mark.parametrize('block,policy', [(b, p) for b in (64, 1024) for p in POLICIES] + [(128, 'uniform'), (512, 'uniform')])
def test_general_kernel_layouts_at_other_workgroup_sizes(gu_option, block, policy, layout):
    """Plane rows, packed rows and statistics only on MAP 1 at workgroups of 64 and 1024 under every policy kind (128 and 512 under
    the uniform one), onto one start cell and onto one of several, 2120 envs: ragged last workgroups at every size."""
    _options(gu_option, rollout_rows=0, rollout_multi=0, traj_layout=0, rollout_block=block)
    info, N = Engine.device_info(0), 2120
    for name in ('c2_open8x8', 'multistart_test_env'):
        spec = _golden_spec(name)
        words = [stream_words(info, N, spec.S, block, T) if policy == 'stream' and layout is not False else 0 for T in LAUNCHES]
        for auto in (True, False):
            parts, eng, table = _case(spec, N, policy)
            _run(eng, parts, SEED, policy, auto, lambda i: _general_form(layout, 1, block, N, words[i]), (name, block, policy, layout, auto), table, layout=layout)


@pytest.mark.parametrize('block', [512, 1024])
def test_stream_statistics_without_auto_reset_on_c3_maze32(gu_option, block):
    """The launch that showed the fault of the 64-bit shift (module docstring, FOUND) where it showed most often: a caller's stream,
    statistics only, no auto-reset, c3_maze32, 2120 envs -- before the fix 24 of 40 fresh engines at a workgroup of 1024 left the oracle's
    walk in the 45th step of the 67-step launch.  Three fresh engines per workgroup size."""
    _options(gu_option, rollout_rows=0, rollout_multi=0, traj_layout=0, rollout_block=block)
    N, spec = 2120, _golden_spec('c3_maze32')
    for rep in range(3):
        parts, eng, _ = _case(spec, N, 'stream')
        _run(eng, parts, SEED, 'stream', False, _general_form(False, 1, block, N), (block, rep), layout=False)
