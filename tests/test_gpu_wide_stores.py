"""The 12-byte row stores of the int32 TRIPLES layout (option traj_layout = 1, TRAJ == 3: one raw_buffer_store_b96 per lane and
step) at every workgroup size, map and wave shape the planner can produce, against the C oracle.

There are two store sites -- emit() in csrc/gu_rollout.hpp (the general kernel) and the row stores of csrc/gu_rollout_rows.hip (the
transition-row kernel) -- and each is followed by GU_WIDE_STORE_PAD() (csrc/gu_internal.hpp): on gfx950 such a store reads its data
registers late, and without the pad lanes 12 .. 15 of every sixteen got wrong first words at every workgroup size but 256 and under
half-wave launches (docs/HISTORY.md, profiles/r06t_triples_race.txt).  tests/test_gpu_traj_layout.py compares the layouts with each
other at the default workgroup; this file runs the shapes that only options reach.

Every case: rows, final state (pos, done, episode, tcount) and per-env statistics are the oracle's, byte for byte (integers: no
tolerance; never another layout or kernel as the reference); two launches on one engine, T = 21 and then T = 67 continuing it (head
and tail of the 16-step action words, the entry path behind a rollout, a rebase of the buffer resource); and after each launch
Engine.rollout_last_form() must name the shape the case is about -- a case whose shape the planner does not produce FAILS.
Every shape gets a fresh engine, the options are process defaults for the duration of the test (the gu_option fixture).

What the file was seen to catch: built with the pad defined away (make -C griduniverse_amd/csrc variant VARIANT=_nopad
EXTRA="-D'GU_WIDE_STORE_PAD()='", run once with GU_LIB_PATH on that library), 12 of its cases went red, all on the general kernel's
site on one grid in LDS (MAP 1) under the uniform and greedy policies: workgroups of 512 and 1024 at 2120 envs already, 64 and 128
at 65 536 envs (test 4 has the counts).  The same build passed every case of the row kernel (pairs, half waves, every policy), of
MAP 0 / 3 / 5, of per-wave staging and of the straddling launches: there the comparisons stand as oracle tests of shapes that ran
nowhere before -- they would see a row that is wrong, held back too long or stored twice, but no run has shown them red for
want of the pad."""
import numpy as np
import pytest

from griduniverse_amd import Engine, GridSpec
from oracle import c_oracle as C
from tests import _golden as G
from tests._mazes import oracle_grid, random_specs
from tests._rollout_shapes import LAUNCHES, POLICIES, STATE_KEYS, _diff, _general, _multi_oracle_and_engine, _oracle_and_engine, _policy_table, _run, spec_of

pytestmark = pytest.mark.gpu


# ---- 1. the general kernel, one grid in LDS (MAP 1) -----------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('block', [64, 128, 256, 512, 1024])
def test_general_kernel_on_one_grid_in_lds_at_every_workgroup_size(gu_option, block, policy):
    """emit() on MAP 1 at workgroups of 64 .. 1024, every policy kind, auto-reset on and off, onto one start cell (c2_open8x8: auto
    mode 1) and onto one of several (multistart_test_env: mode 2, the reset draws from the RNG).  2120 envs: three workgroups of
    1024, the last of one full wave and one of eight lanes; ragged last workgroups at every other size.  At 512 and 64 also with
    the store pacer's instantiation switched off (rollout_pace = 0) and on a fixed 0.2 us period (= 20): include/gu.h promises
    results that do not depend on pacing."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    gu_option('rollout_block', block)
    N, seed = 2120, 11
    for name in ('c2_open8x8', 'multistart_test_env'):
        meta, _ = G.load_traj(name)
        table = _policy_table(policy, meta['W'] * meta['H'])
        for auto in (True, False):
            for pace in ((None, 0, 20) if block in (512, 64) else (None,)):
                gu_option('rollout_pace', pace)
                grid, st, eng = _oracle_and_engine(meta, N, seed, env_id0=5)
                expect = _general(1, block)
                if pace is not None:
                    expect['pace_mode'] = 2 if pace else 0
                _run(eng, [(grid, st, slice(None))], seed, policy, auto, expect, (name, block, policy, auto, pace), table)


# ---- 2. the general kernel on its other maps --------------------------------------------------------------------------------------
BIG_W, BIG_H = 182, 181  # S = 32 942 > 32 767: no two planes in 64 KiB; the flags plane alone fits a CU's LDS


def _big_open_grid():
    S = BIG_W * BIG_H
    return GridSpec(BIG_W, BIG_H, [S - 3], [S - 1], [S - 3 - BIG_W], [])  # no walls; two moves from the goal, lava next door: episodes end


@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('block', [64, 1024])
def test_general_kernel_on_a_grid_too_big_for_two_planes(gu_option, block, policy):
    """One open 182 x 181 grid on the general kernel (rollout_rows = 0: the default would hand the greedy policy to the row
    kernel): the uniform and stream policies keep its flags plane in LDS (MAP 3), greedy and sample read the records from L2 (MAP 0)."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    gu_option('rollout_block', block)
    spec, N, seed = _big_open_grid(), 200, 13
    table = _policy_table(policy, spec.S)
    for auto in (True, False):
        grid, st = oracle_grid(spec), C.State(N, 9)
        eng = Engine(N, spec, seed=seed, env_id0=9)
        assert np.array_equal(eng.reset(), C.reset(grid, seed, st))
        # every env on a cell of its own (a table policy from the one start cell is one walk N times over): half of them anywhere,
        # half within a few moves of the goal, none on a terminal cell
        rs = np.random.RandomState(block)
        st.pos[:] = np.where(np.arange(N) % 2, rs.randint(0, spec.S - 4 * BIG_W, N), spec.S - 1 - BIG_W * rs.randint(0, 3, N) - rs.randint(1, 4, N))
        st.pos[st.pos == spec.S - 3 - BIG_W] = spec.S - 3
        eng.set_state(pos=st.pos)
        expect = _general(3 if policy in ('uniform', 'stream') else 0, block)
        _run(eng, [(grid, st, slice(None))], seed, policy, auto, expect, (block, policy, auto), table)


@pytest.mark.parametrize('block', [64, 1024])
def test_general_kernel_without_lds_on_one_wide_grid_per_env(gu_option, block):
    """192 grids of 1023 x 1, one per env: no group fills a workgroup (no LDS planes) and W > 1022 rules out the four-bit image --
    MAP 0 on a multi-grid engine."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    gu_option('rollout_block', block)
    N, seed = 192, 17
    specs = random_specs(np.random.RandomState(block), N, 1023, 1)
    for auto in (True, False):
        parts, eng = _multi_oracle_and_engine(specs, N, seed, env_id0=N)
        _run(eng, parts, seed, 'uniform', auto, _general(0, block), (block, auto))


def _quirk_specs(rs, N, W, H):
    """One grid per env as tests/test_gpu_multigrid.py::test_one_grid_per_env_on_the_four_bit_image builds them: starts on
    terminal cells and on walls, goals that are walls, cells both goal and lava, several starts."""
    S = W * H
    specs = random_specs(rs, N, W, H)
    for i, sp in enumerate(specs[:64]):
        cells = [int(c) for c in rs.choice(S, size=4, replace=False)]
        goals, lava, walls = (np.flatnonzero(m).tolist() for m in (sp.goal, sp.lava, sp.wall))
        kind = i % 4
        if kind == 0:
            specs[i] = GridSpec(W, H, [cells[0]], [cells[0]], lava, walls)                                   # start on a goal: absorbing at once
        elif kind == 1:
            specs[i] = GridSpec(W, H, [cells[0]], goals, [], sorted(set(walls) | {cells[0]}))               # start on a wall
        elif kind == 2:
            specs[i] = GridSpec(W, H, list(sp.starts), [cells[-1]], [cells[-1]], sorted(set(walls) | {cells[-1]}))  # goal = lava = wall
    return specs


@pytest.mark.parametrize('policy', ['uniform', 'stream'])
@pytest.mark.parametrize('W,H,block', [(9, 7, 256), (64, 64, 64)])
def test_held_rows_on_the_four_bit_image(gu_option, W, H, block, policy):
    """MAP 5, one maze per env: every row is held back behind the next step's gather (held_*, release() in gu_rollout.hpp) and
    stored from there -- a row released late, early or twice shows here.  The planner sizes the workgroup by the images that fit a
    CU's LDS, not by rollout_block: four waves at 9 x 7, one at 64 x 64 (asserted)."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    N, seed = 192, 23
    specs = _quirk_specs(np.random.RandomState(W * 100 + H), N, W, H)
    for auto in (True, False):
        parts, eng = _multi_oracle_and_engine(specs, N, seed)
        _run(eng, parts, seed, policy, auto, _general(5, block), (W, H, policy, auto))


@pytest.mark.parametrize('policy', ['uniform', 'stream'])
@pytest.mark.parametrize('group,block,per_wave', [(64, 256, True), (128, 256, True), (64, 64, False)])
def test_every_wave_stages_its_own_grid(gu_option, group, block, per_wave, policy):
    """Multi-grid 8 x 8, 384 envs: groups of 64 and 128 under a workgroup of 256 (every wave stages its own grid's planes:
    per_wave), and groups of 64 under a workgroup of 64 (one grid per workgroup)."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    gu_option('rollout_block', block)
    N, seed = 384, 29
    specs = random_specs(np.random.RandomState(group), N // group, 8, 8)
    for auto in (True, False):
        parts, eng = _multi_oracle_and_engine(specs, N, seed, env_id0=2 * N)
        _run(eng, parts, seed, policy, auto, _general(1, block, per_wave=per_wave), (group, block, policy, auto))


@pytest.mark.parametrize('policy', ['uniform', 'sample'])
@pytest.mark.parametrize('block', [64, 1024])
def test_the_launches_that_straddle_2_pow_32_steps(gu_option, block, policy):
    """Step counts of 2^32 - 30 plus 0 .. 40 per env: the launch of 21 steps has envs on both sides of the boundary, and so has the
    one of 67 behind it (the envs that began at 2^32 - 30 .. - 22 are still 9 .. 1 steps short of it), so both must report
    `straddle`; a third launch of 21 steps lies wholly in epoch 1 and must not."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', 0)
    gu_option('rollout_block', block)
    meta, _ = G.load_traj('c2_open8x8')
    N, seed = 2120, 31
    table = _policy_table(policy, meta['W'] * meta['H'])
    for auto in (True, False):
        grid, st, eng = _oracle_and_engine(meta, N, seed, env_id0=5)
        st.tcount[:] = (2 ** 32 - 30 + np.random.RandomState(4).randint(0, 41, N)).astype(np.uint64)
        assert st.tcount.min() == 2 ** 32 - 30 and st.tcount.max() == 2 ** 32 + 10
        eng.set_state(tcount=st.tcount)
        _run(eng, [(grid, st, slice(None))], seed, policy, auto, lambda i: _general(1, block, straddle=i < 2), (block, policy, auto), table,
             launches=LAUNCHES + (21,))
        assert st.tcount.min() == 2 ** 32 - 30 + sum(LAUNCHES) + 21


# ---- 3. the transition-row kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('rows', [1, 2, 3])
def test_row_kernel_with_and_without_pairs_and_half_waves(gu_option, rows, policy):
    """The row stores of gu_rollout_rows.hip: one-step tables and pair tables (rollout_rows = 2: no pairs, 3: pairs forced, 1: the
    planner's rule, gu_plan_rows -- triples go to the pairs under the uniform policy up to a workgroup per four CUs), whole waves
    and half waves (rollout_half_waves).  2080 = 65 x 32 envs: with half waves 128 envs per workgroup, an odd number of half waves,
    the last workgroup holds one; 2120 is no multiple of 32, the planner must then refuse half waves and the rows are right all the
    same.  The row kernel's workgroup stays at 256 here: it grows to 512 when one table takes more than half a CU's LDS and the batch
    needs more than one 256-lane workgroup per CU -- 256 x CUs + 64 envs on a 72 x 72 grid already; tests/test_gpu_launch_shapes.py
    runs that shape, the triples among its row layouts."""
    gu_option('traj_layout', 1)
    gu_option('rollout_rows', rows)
    info = Engine.device_info(0)
    seed = 37
    for name in ('c2_open8x8', 'c4_lava32'):
        meta, _ = G.load_traj(name)
        S = meta['W'] * meta['H']
        table = _policy_table(policy, S)
        pairs_fit = S * 144 <= info['lds_per_cu'] - 2048
        for N, half_opt in ((2080, 0), (2080, 1), (2120, 1)):
            gu_option('rollout_half_waves', half_opt)
            pair = policy in ('uniform', 'stream') and rows != 2 and pairs_fit and (rows == 3 or (policy == 'uniform' and -(-N // 256) * 4 <= info['cus']))
            half = bool(half_opt) and N % 32 == 0
            expect = dict(family='rows', layout=3, map=-1, block=256, workgroups=-(-N // (128 if half else 256)), pair=pair, half=half,
                          per_wave=False, straddle=False)
            for auto in (True, False):
                grid, st, eng = _oracle_and_engine(meta, N, seed, env_id0=5)
                _run(eng, [(grid, st, slice(None))], seed, policy, auto, expect, (name, rows, policy, N, half_opt, auto), table)


# ---- 4. the hazard at the scale where it was seen ----------------------------------------------------------------------------------
SCALE_LAUNCHES = LAUNCHES + (120,)
SCALE_SEED = 11


@pytest.fixture(scope='module')
def scale_reference():
    """The oracle's rows and final state of c3_maze32 under the uniform policy with auto-reset, per batch size: computed once,
    shared by the shapes of that size, never written to."""
    cache = {}

    def get(N):
        if N not in cache:
            meta, _ = G.load_traj('c3_maze32')
            grid, st = C.Grid.from_lists(**meta), C.State(N, 5)
            first = C.reset(grid, SCALE_SEED, st)
            outs = [C.rollout(grid, SCALE_SEED, st, T, True, stats=True) for T in SCALE_LAUNCHES]
            for a in [first] + [x for o in outs for x in o.values()] + [getattr(st, k) for k in STATE_KEYS]:
                a.setflags(write=False)
            cache[N] = (first, outs, {k: getattr(st, k) for k in STATE_KEYS})
        return cache[N]

    yield get
    cache.clear()


SCALE_SHAPES = [dict(rollout_rows=0, rollout_block=64), dict(rollout_rows=0, rollout_block=128), dict(rollout_rows=0, rollout_block=512),
                dict(rollout_rows=0, rollout_block=1024), dict(rollout_rows=3, rollout_half_waves=1)]


@pytest.mark.parametrize('shape', SCALE_SHAPES, ids=lambda s: '-'.join('%s%d' % (k.split('_', 1)[1], v) for k, v in s.items()))
@pytest.mark.parametrize('N', [2120, 65536])
def test_triples_at_the_batch_sizes_of_the_recorded_race(gu_option, scale_reference, N, shape):
    """Uniform policy, auto-reset, c3_maze32, launches of 21, 67 and 120 steps against the full-batch oracle, on the general kernel
    at workgroups of 64, 128, 512 and 1024 and on the row kernel's pair tables under half waves (there with 2080 envs in place of
    2120: half waves want a multiple of 32).  The recorded race -- 2 000 .. 14 000 wrong words among 7.8 M rows of 65 536 envs x 120
    steps, different from run to run -- was found at that size; tests/test_gpu_traj_layout.py runs it at the workgroup of 256.

    MEASURED, one run of this file on a build with the pad defined away (see the module docstring): the general kernel's store site
    goes red from the smallest batch on -- 2120 envs at workgroups of 512 (112 wrong obs words among the 142 040 of the 67-step
    launch) and 1024 (96) -- and at workgroups of 64 and 128 only at 65 536 envs (288 and 912 wrong obs words among 4.39 M; 1648 and
    3152 at 512 and 1024); every wrong word sat in lanes 12 .. 15 of a row of sixteen.  16 384 envs showed nothing that the two
    sizes kept here do not (red at 512 and 1024, green at 64 and 128).  The row kernel's shape stayed GREEN without the pad at every
    size: for that store site this test is an oracle comparison, not a demonstrated guard."""
    rows_kernel = shape['rollout_rows'] != 0
    if rows_kernel and N == 2120:
        N = 2080
    gu_option('traj_layout', 1)
    for name, value in shape.items():
        gu_option(name, value)
    first, outs, final = scale_reference(N)
    meta, _ = G.load_traj('c3_maze32')
    if rows_kernel:
        expect = dict(family='rows', layout=3, map=-1, block=256, workgroups=N // 128, pair=True, half=True, per_wave=False, straddle=False)
        if N % 128:
            expect['workgroups'] += 1
    else:
        expect = _general(1, shape['rollout_block'])
    with Engine(N, spec_of(meta), seed=SCALE_SEED, env_id0=5) as eng:
        assert np.array_equal(eng.reset(), first)
        eng.reserve_trajectory(max(SCALE_LAUNCHES))
        for T, want in zip(SCALE_LAUNCHES, outs):
            eng.rollout(T, 'uniform', True, True, stats=True)
            form = eng.rollout_last_form()
            assert {k: form[k] for k in expect} == expect, (N, shape, T, form)
            got = eng.read_trajectory(0, T)
            for k in ('obs', 'reward', 'done'):
                assert np.array_equal(got[k], want[k]), (N, shape, T, k, _diff(got[k], want[k]))
            ret, eps = eng.read_stats()
            assert np.array_equal(ret, want['ret']) and np.array_equal(eps, want['episodes']), (N, shape, T)
        state = eng.get_state()
        for k in STATE_KEYS:
            assert np.array_equal(state[k], final[k]), (N, shape, k)
