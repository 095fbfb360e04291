"""The overlay kernels -- wind (with and without gusts), fruit, doors, boxes and errands: each kind's step kernel, its rollout kernel
under four policies and in both memory forms, and its gu_td_kernel instantiation -- where their other tests never go: on grids past
LDS and at the edge of it, in batches of more workgroups than the device has CUs, and with masked Q tables larger than 2^32 bytes
and 2^31 elements.  Every comparison is byte for byte against the kind's CPU restatement (tests/_{wind,fruit,doors,boxes,errands}_oracle.py
on _overlay_oracle.py), never one kernel against another.  The cases are in tests/_overlay_scale.py; tests/test_overlay_scale_host.py
holds without a device that every restatement's run met what its case is about (fruit eaten, a door opened and one found shut, a box
pushed and a push refused, a gust that changed a push, an errand completed and a wrong fruit, every start drawn under auto-reset, an
absorbed step without it), and every case here asserts the same on the run it compares against.

Part A -- grids.  Every kind, N = 130 (three waves, the last partial), T = 33, env_id0 = 2^31 - 40, three start cells, the envs put
around the lava cell that the planes lie next to.
    grid        shape       cells     3 x cell_bytes   form asserted after each rollout (rollout_last_form)
    big182      182 x 182   33 124    99 408           lds_bytes 0: S > GU_MAX_LDS_CELLS; planes, starts and envs past cell 32 767
    fit156      140 x 156   21 840    65 520           lds_bytes 65 520: the largest three-plane LDS image
    over32      683 x 32    21 856    65 568           lds_bytes 0: 32 bytes too many (two planes still fit: the calm kernels stage them)
    line40000   40 000 x 1  40 000    120 000          lds_bytes 0: W fits no int16 delta, up and down never move
Per kind and grid: rollout under uniform, stream, greedy and sample with auto-reset on and off, rows and statistics, as one launch and
as launches of 16 and 17 (the per-env word goes through memory); step with pinned outputs and, twice, rejected actions; td_run under
both methods in launches of 150 and 151 steps -- with 130 learners where their tables stay below 400 MB and six where they do not, and
under errands with three mask bits on big182 and line40000 and six on the other two.  The boxes take 30 or 32 bits there: gu_td_init
refuses them with GU_ERR_INVALID and leaves the engine as it was, and that is their case.  After every call the env state and the
per-env words are compared.

Part B -- batch.  'starts8' (LDS) and 'open150' (L2) of tests/_overlay_starts.py with N = 65 536 + 70 envs: 257 workgroups of
GU_BLOCK = 256, the last of one full wave and one wave of six lanes.  Every kind: rollout under uniform and stream, auto-reset on
and off, all rows, statistics, state and all N words; one gu_step with lazy resets due, one gu_step_device read through
read_outputs(), and the done compaction.

Part C -- masked tables past 2^32 bytes, both methods, through tests/_learners.py's _stores_past_a_boundary with the overlay-aware
adapter OverlayTd: the smallest batch at which Q passes 2^32 bytes INSIDE an env's table with a group of envs on each side; the first
group, the last and the one around the crossing each against a restatement built at the group's first env id -- its slice of
q_table(env0, n), its words, its statistics columns and its env state, after each of two launches (60 and 41 steps), nothing read
whole.
    kind      grid                  bits   rows per env   bytes per env   crossing in env   N       group   device
    fruit     big182, three fruit   3      264 992        8 479 744       506               520     8       4.4 GB
    doors     big182, three slots   3      264 992        8 479 744       506               520     8       4.4 GB
    boxes     31 x 33, one box      10     1 047 552      33 521 664      128               136     4       4.6 GB
    errands   8 x 9, five fruit     10     73 728         2 359 296       1 820             1 830   16      4.3 GB
    fruit, Q-learning: 2^31 ELEMENTS -- N = 2 040, entry 2^31 lies in env 2 025's table, 2 880 rows before its end; 17.3 GB
One engine is alive at a time.  A case whose tables the library refuses for want of memory (GU_ERR_NOMEM) skips with the library's
message: it proves nothing then, and on a 288 GB device none skips.  Peak device memory, from the shapes: Part A 0.3 GB (130 tables of
2.6 MB under doors on line40000), Part B under 0.1 GB (33 rows of 65 606 envs), Part C 17.3 GB.

Left out, on purpose.  One env's masked table of more than 2^31 entries: S << bits > 2^29 rows are 17 GB for one env and a host table to
match.  Trajectory planes past 2^31 rows under an overlay: 26 GB of rows; the index is formed in 64 bits in all five kernels, and the
case belongs with the calm kernels' own, if ever."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.grid import GridSpec

from . import _overlay_scale as X
from . import _overlay_starts as S
from ._learners import _crossing, _stores_past_a_boundary
from ._overlays import METHODS, overlay, same_state
from ._tabular_cases import _eps, _same, code

pytestmark = pytest.mark.gpu

N, T, ID0 = X.N, X.T, X.ID0
GRIDS = sorted(X.GRIDS)


def _spec(name):
    g = S.grid_dict(name)
    return GridSpec(g['W'], g['H'], g['starts'], g['goals'], g['lava'], g['walls'])


def _again(vec, kind, name, q0=None):
    """The batch seeded and reset anew and put in place, next to a fresh restatement of it."""
    o = S.oracle(kind, name, ID0, n=vec.num_envs, q0=q0)
    vec.seed(S.SEED)
    assert np.array_equal(vec.reset(), o.reset())
    S.place(kind, name, o, vec)
    return o


def _batch(kind, name, n=N, q0=None):
    vec = gua.VecGridUniverse(n, template=_spec(name), seed=S.SEED, env_id0=ID0)
    try:
        overlay(kind).install(vec.engine, S.plane(kind, name), *S.extra(kind, name))
        if q0 is not None:
            vec._ensure_q(q0)
        return vec
    except BaseException:
        vec.close()
        raise


def _rollouts(vec, kind, name, policy, lds_bytes, split=True):
    """One launch of T steps and (`split`) launches of 16 and 17, auto-reset on and off: rows, statistics, state and words."""
    acts = S.stream_actions(vec.num_envs) if policy == 'stream' else None
    if policy in ('greedy', 'sample'):
        vec.engine.vi_set(np.zeros(vec.spec.S), S.policy_table(name))
    for auto in (True, False):
        o = _again(vec, kind, name)
        want = S.rollout_of(o, name, policy, auto=auto)
        X.met(kind, o, auto)
        if not auto:
            X.absorbed(want)
        _same(vec.rollout(T, policy, actions=acts, auto_reset=auto, stats=True), want)  # one launch ...
        form = vec.engine.rollout_last_form()
        assert form['family'] == X.family(kind) and form['lds_bytes'] == lds_bytes, form
        same_state(vec, o, kind)
        if not split:
            continue
        o = _again(vec, kind, name)  # ... and launches of 16 and 17: the word goes through memory
        parts = []
        for t0, n in ((0, 16), (16, 17)):
            parts.append(vec.rollout(n, policy, actions=None if acts is None else acts[t0:t0 + n], auto_reset=auto, stats=True))
            S.rollout_of(o, name, policy, n, auto, t0=t0)
            same_state(vec, o, kind)
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(np.concatenate([h[k] for h in parts]), want[k]), (auto, k)
        assert np.array_equal(parts[0]['ret'] + parts[1]['ret'], want['ret']) and np.array_equal(parts[0]['episodes'] + parts[1]['episodes'], want['episodes'])


# ---------------------------------------------------------------------------------------------------------------- Part A
@pytest.mark.parametrize('policy', S.POLICIES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_a_rollout_equals_the_oracle(kind, grid, policy):
    X.arithmetic(grid)
    vec = _batch(kind, grid)
    try:
        _rollouts(vec, kind, grid, policy, X.LDS_BYTES[grid])
    finally:
        vec.close()


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_a_step_pinned_and_rejected_actions_equal_the_oracle(kind, grid):
    X.arithmetic(grid)
    vec = _batch(kind, grid)
    try:
        o = _again(vec, kind, grid)
        vec.auto_reset = True
        refusals = 0
        for i, a, refused, (w_obs, w_rew, w_don) in X.steps(o):
            if refused:  # gu_step names the invalid actions and steps the other envs all the same
                assert code(lambda: vec.step(a)) == -1
                refusals += 1
            else:
                obs, rew, don, _ = vec.step(a, zero_copy=(i % 2 == 1))
                assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0), i
            same_state(vec, o, kind)
        assert refusals == 2
        X.met(kind, o)
    finally:
        vec.close()


TD = [(kind, grid) for kind in X.KINDS for grid in GRIDS if kind != 'boxes']


@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('kind,grid', TD)
def test_a_td_run_tables_rows_and_state_equal_the_oracle(kind, grid, method):
    X.arithmetic(grid)
    td, n = X.td_case(kind, grid)
    vec = _batch(kind, td, n, q0=S.Q0)
    try:
        o = _again(vec, kind, td, q0=S.Q0)
        b = X.bits(kind, td)
        assert vec.engine.stores()['overlay_bits'] == b and vec.engine.td_rows == o.grid.S << b == o.q.shape[1]
        for steps in X.TD_STEPS:
            want = o.td_run(steps, METHODS[method], X.ALPHA, X.GAMMA, _eps(X.EPS))
            _same(vec.td_run(steps, method, alpha=X.ALPHA, discount_factor=X.GAMMA, epsilon=X.EPS, trajectory=True, stats=True), want)
            q = vec.q_table()
            assert q.shape == o.q.shape and np.array_equal(q.view(np.int64), o.q.view(np.int64))  # by bits
            same_state(vec, o, kind)
        X.learned_on_masked_rows(kind, td, o)
        X.met(kind, o, starts=(n == N))
    finally:
        vec.close()


@pytest.mark.parametrize('grid', GRIDS)
def test_a_td_init_refuses_the_boxes_and_leaves_the_engine_as_it_was(grid):
    """Two boxes of 15 or 16 bits: more than the 10 that gu_td_init admits.  The refusal changes no plane, word, store or env."""
    td, n = X.td_case('boxes', grid)
    assert n is None and X.bits('boxes', td) in (30, 32)
    K = overlay('boxes')
    vec = _batch('boxes', td)
    try:
        eng = vec.engine
        o = _again(vec, 'boxes', td)
        _same(vec.rollout(16, 'uniform', auto_reset=True, stats=True), S.rollout_of(o, td, 'uniform', 16))  # (words that are not the reset value)
        assert (o.words != K.reset_value(S.plane('boxes', td))).any()

        def snapshot():
            return K.plane(eng).tobytes(), K.params(eng), K.masks(eng).tobytes(), sorted(eng.stores().items()), [v.tobytes() for _, v in sorted(eng.get_state().items())]

        before = snapshot()
        assert code(lambda: eng.td_init(0.0)) == -1
        assert code(lambda: vec.td_run(5, 'q_learning')) == -1
        assert snapshot() == before and eng.stores()['td_rows'] == 0
        _same(vec.rollout(17, 'uniform', auto_reset=True, stats=True), S.rollout_of(o, td, 'uniform', 17))  # the engine goes on where it was
        same_state(vec, o, 'boxes')
    finally:
        vec.close()


# ---------------------------------------------------------------------------------------------------------------- Part B
@pytest.mark.parametrize('policy', X.BATCH_POLICIES)
@pytest.mark.parametrize('grid', X.BATCH_GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_b_rollout_of_257_workgroups_equals_the_oracle(kind, grid, policy):
    vec = _batch(kind, grid, X.BIG_N)
    try:
        _rollouts(vec, kind, grid, policy, 3 * X.cell_bytes(64) if grid == 'starts8' else 0, split=False)
    finally:
        vec.close()


@pytest.mark.parametrize('grid', X.BATCH_GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_b_step_of_257_workgroups_equals_the_oracle(kind, grid):
    """Sixteen steps without auto-reset leave envs done in every workgroup; then one gu_step with auto-reset (their lazy resets), one
    gu_step_device read back through read_outputs(), and the done compaction."""
    n = X.BIG_N
    vec = _batch(kind, grid, n)
    try:
        eng = vec.engine
        o = _again(vec, kind, grid)
        want = X.batch_step_case(kind, grid, o)
        acts = S.step_actions(n)
        _same(vec.rollout(16, 'uniform', auto_reset=False, stats=True), want['rows'])
        vec.auto_reset = True
        obs, rew, don, _ = vec.step(acts[0])
        w_obs, w_rew, w_don = want['step']
        assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0)
        eng.upload_actions(acts[1:3])
        eng.step_device(1, True)
        w_obs, w_rew, w_don = want['step_device']
        obs, rew, don = eng.read_outputs()
        assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don != 0, w_don != 0)
        assert np.array_equal(eng.done_indices(), np.flatnonzero(w_don != 0))
        same_state(vec, o, kind)
    finally:
        vec.close()


# ---------------------------------------------------------------------------------------------------------------- Part C
def _masked_tables(case, method, at):
    kind, name, b, n, e, width = case
    per_env = X.bytes_per_env(name, b)
    assert X.bits(kind, name) == b and _crossing(per_env, n, at) == e and at % per_env != 0  # byte `at` lies inside env e's table
    learner = X.OverlayTd(kind, name, method)

    def after(tag, e0, o, got):
        assert got['q'].shape == (width, S.grid_dict(name)['W'] * S.grid_dict(name)['H'] << b, 4)
        if tag == 'launch 1':
            X.learned_on_masked_rows(kind, name, o)

    _stores_past_a_boundary(learner, S.grid_dict(name), n, [e], X.C_LAUNCHES, seed=X.C_SEED, width=width, before=X.put_in_place(kind, name, n), after=after)


@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('case', sorted(X.MASKED))
def test_c_masked_tables_across_2_32_bytes(case, method):
    _masked_tables(X.MASKED[case], method, 2 ** 32)


def test_c_more_than_2_31_masked_table_entries():
    """Fruit on big182 under Q-learning with 2 040 envs: N x (S << 3) x 4 > 2^31 doubles, 17.3 GB; entry 2^31 lies in env 2 025's table."""
    kind, name, b, n, e, width = X.ELEMENTS
    assert n * (33124 << b) * 4 > 2 ** 31 > (n - 2 * width) * (33124 << b) * 4
    _masked_tables(X.ELEMENTS, 'q_learning', 8 * 2 ** 31)
