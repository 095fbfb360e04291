"""Wind, fruit, doors, boxes and errands on grids with THREE start cells, and on an engine that is a shard (env_id0 = 2^31 - 40: the
batch straddles bit 31), against the CPU restatements tests/_{wind,fruit,doors,boxes,errands}_oracle.py built at the same id, byte for
byte: rows, statistics, positions, masks or words, episode counts, tables.

The fruit, door, box and errand step kernels each carry their own copy of the lazy reset, their rollout kernels another (start_prefix beside
the policy's epoch-folded prefix), and every overlay kernel writes a.env_id0 + e out by itself.  Every other overlay test runs at
env_id0 = 0 on a grid with one start cell, where gu_rng_start_index(...) is always 0: a wrong prefix, a wrong episode count or the
policy's prefix in place of the stream-1 prefix gives the same bytes there.  Here every case asserts on the restatement's log
(tests/_start_log.py) that lazy resets drew every one of the three cells and that some step reset two envs to different cells.

The grids, planes, placement and policy table are in tests/_overlay_starts.py (and its conditions are held without a device by
tests/test_env_ids_host.py).  N = 130 (three waves, the last partial), T = 33 (two full action words and a tail of one step)."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.grid import GridSpec

from . import _overlay_starts as S
from ._overlay_starts import IDS, KINDS, N, POLICIES, SEED, T
from ._overlays import METHODS, overlay, same_state as _same_state
from ._tabular_cases import _eps, _same, code, counts_near_2_32

pytestmark = pytest.mark.gpu

GRIDS = ('starts8', 'open150')
ALPHA, GAMMA, EPS = 0.25, 0.9, 0.3


def _spec(name):
    g = S.grid_dict(name)
    return GridSpec(g['W'], g['H'], g['starts'], g['goals'], g['lava'], g['walls'])


def _install(vec, kind, name):
    overlay(kind).install(vec.engine, S.plane(kind, name), *S.extra(kind, name))


def _again(vec, kind, name, env_id0, q0=None):
    """The batch seeded and reset anew and put in place, next to a fresh restatement of it."""
    o = S.oracle(kind, name, env_id0, q0=q0)
    vec.seed(SEED)
    assert np.array_equal(vec.reset(), o.reset())
    S.place(kind, name, o, vec)
    return o


def _pair(kind, name, env_id0, q0=None):
    vec = gua.VecGridUniverse(N, template=_spec(name), seed=SEED, env_id0=env_id0)
    try:
        _install(vec, kind, name)
        if q0 is not None:
            vec._ensure_q(q0)
        return vec, _again(vec, kind, name, env_id0, q0)
    except BaseException:
        vec.close()
        raise


def _same_tables(vec, o):
    q = vec.q_table()
    assert q.shape == o.q.shape and np.array_equal(q.view(np.int64), o.q.view(np.int64))  # by bits, without a copy of either


# ---- 1: step and step_device ----
@pytest.mark.parametrize('env_id0', IDS)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', KINDS)
def test_step_and_step_device_equal_the_oracle(kind, grid, env_id0):
    vec, o = _pair(kind, grid, env_id0)
    try:
        acts = S.step_actions()
        vec.auto_reset = True
        for i in range(T):
            obs, rew, don, _ = vec.step(acts[i])
            w_obs, w_rew, w_don, rejected = o.step(acts[i], True)
            assert not rejected.any()
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0), i
        S.drew_every_start(o)
        _same_state(vec, o, kind)
        o2 = _again(vec, kind, grid, env_id0)  # the same rows from the device-resident stream
        vec.engine.upload_actions(acts)
        for i in range(T):
            vec.engine.step_device(i, True)
            obs, rew, don = vec.engine.read_outputs()
            w_obs, w_rew, w_don, _ = o2.step(acts[i], True)
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don != 0, w_don != 0), i
        _same_state(vec, o2, kind)
        assert np.array_equal(o2.state.pos, o.state.pos) and np.array_equal(o2.starts.drawn, o.starts.drawn)
    finally:
        vec.close()


# ---- 2: rollout ----
@pytest.mark.parametrize('env_id0', IDS)
@pytest.mark.parametrize('policy', POLICIES)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', KINDS)
def test_rollout_equals_the_oracle(kind, grid, policy, env_id0):
    vec, o = _pair(kind, grid, env_id0)
    try:
        acts = S.stream_actions() if policy == 'stream' else None
        if policy in ('greedy', 'sample'):
            vec.engine.vi_set(np.zeros(o.grid.S), S.policy_table(grid))
        want = S.rollout_of(o, grid, policy)
        S.drew_every_start(o)
        _same(vec.rollout(T, policy, actions=acts, auto_reset=True, stats=True), want)  # one launch ...
        form = vec.engine.rollout_last_form()
        assert form['family'] == {'gusts': 'wind'}.get(kind, kind) and (form['lds_bytes'] > 0) == (grid == 'starts8')
        _same_state(vec, o, kind)
        _again(vec, kind, grid, env_id0)  # ... and launches of 16 and 17
        parts = [vec.rollout(n, policy, actions=None if acts is None else acts[t0:t0 + n], auto_reset=True, stats=True) for t0, n in ((0, 16), (16, 17))]
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(np.concatenate([h[k] for h in parts]), want[k]), k
        assert np.array_equal(parts[0]['ret'] + parts[1]['ret'], want['ret'])
        assert np.array_equal(parts[0]['episodes'] + parts[1]['episodes'], want['episodes'])
        _same_state(vec, o, kind)
    finally:
        vec.close()


# ---- 3: td_run ----
# (every kind that learns on the grid, S.td_grid: the boxes refuse 'open150', their word takes more than 10 bits, and their learners
# run on 'learn4' in the place of 'starts8'; the errands learn under the planes ':td' -- six bits on 'starts8', three on 'open150', where
# the six bits of tests/test_gpu_errands.py are 46 MB a table and run with six learners there)
TD_CASES = [(kind, S.td_grid(kind, grid)) for kind in KINDS for grid in GRIDS if (kind, grid) != ('boxes', 'open150')]
assert len(TD_CASES) == 2 * len(KINDS) - 1 and ('boxes', 'learn4') in TD_CASES and ('errands', 'open150:td') in TD_CASES


@pytest.mark.parametrize('env_id0', IDS)
@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('kind,grid', TD_CASES)
def test_td_run_tables_rows_and_state_equal_the_oracle(kind, grid, method, env_id0):
    vec, o = _pair(kind, grid, env_id0, q0=S.Q0)
    try:
        want = o.td_run(300, METHODS[method], ALPHA, GAMMA, _eps(EPS))
        S.drew_every_start(o)
        assert (o.q != S.Q0).any()
        _same(vec.td_run(300, method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, trajectory=True, stats=True), want)
        _same_tables(vec, o)
        _same_state(vec, o, kind)
    finally:
        vec.close()


def test_the_boxes_refuse_the_learners_on_open150():
    vec, _ = _pair('boxes', 'open150', IDS[1])
    try:
        assert code(lambda: vec.engine.td_init(0.0)) == -1  # more than 10 bits
    finally:
        vec.close()


# ---- 4: reset(mask) and reset_done() halfway ----
@pytest.mark.parametrize('env_id0', IDS)
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', KINDS)
def test_reset_paths_halfway_equal_the_oracle(kind, grid, env_id0):
    vec, o = _pair(kind, grid, env_id0)
    try:
        _same(vec.rollout(16, 'uniform', auto_reset=False, stats=True), S.rollout_of(o, grid, 'uniform', 16, auto=False))
        done = o.state.done != 0
        assert done.any() and not done.all()
        _same_state(vec, o, kind)
        before = None if S.masks_of(o, kind) is None else S.masks_of(o, kind).copy()
        vec.engine.reset_done()  # the done envs only, each to the start its own stream and episode count name
        d = o.reset_done()
        assert np.array_equal(d, done) and len(set(o.state.pos[d].tolist())) > 1
        if before is not None:
            assert np.array_equal(S.masks_of(o, kind)[~d], before[~d])
        _same_state(vec, o, kind)
        mask = (np.arange(N) % 3 == 0).astype(np.uint8)
        assert np.array_equal(vec.reset(mask), o.reset(mask))  # the masked envs only
        assert len(set(o.state.pos[mask != 0].tolist())) == 3
        _same_state(vec, o, kind)
        _same(vec.rollout(17, 'uniform', auto_reset=True, stats=True), S.rollout_of(o, grid, 'uniform', 17))  # the lazy reset
        S.drew_every_start(o)
        _same_state(vec, o, kind)
    finally:
        vec.close()


# ---- 5: a box on a start cell ----
@pytest.mark.parametrize('grid', GRIDS)
def test_set_boxes_refuses_a_box_on_the_second_and_on_the_third_start(grid):
    g = S.grid_dict(grid)
    boxes, targets = S.box_cells(grid)
    vec = gua.VecGridUniverse(8, template=_spec(grid))
    try:
        eng = vec.engine
        eng.set_boxes(S.plane('boxes', grid), S.ON_TARGET)
        before = eng.get_boxes()[0].copy()
        for start in g['starts'][1:]:
            bad = S.BO.plane_of(g['W'] * g['H'], boxes[:-1] + [start], targets)
            assert code(lambda: eng.set_boxes(bad, S.ON_TARGET)) == -1, start
        assert np.array_equal(eng.get_boxes()[0], before)  # a refused call changes nothing
    finally:
        vec.close()


# ---- 6: the step count crosses 2^32 inside a launch ----
@pytest.mark.parametrize('env_id0', IDS)
@pytest.mark.parametrize('kind,grid', [('fruit', 'starts8'), ('doors', 'starts8'), ('boxes', 'one_box8'), ('errands', 'starts8')])
def test_the_epoch_changes_inside_a_launch(kind, grid, env_id0):
    """Streams 0, 2 and 4 are re-keyed in the step that crosses a multiple of 2^32; stream 1, which draws the start cell, and stream
    11, which draws the instruction, have no epoch: resets behind the crossing still draw with the prefix of epoch 0.  ('one_box8':
    the boxes' learners take 10 bits, as the errands' five fruit and three instructions do.)"""
    vec, o = _pair(kind, grid, env_id0, q0=0.0)
    try:
        tc = counts_near_2_32(vec, o, N, 2 ** 32 - 20)
        for method in sorted(METHODS):
            got = vec.td_run(60, method, alpha=0.2, discount_factor=0.9, epsilon=0.5, trajectory=True, stats=True)
            want = o.td_run(60, METHODS[method], 0.2, 0.9, _eps(0.5))
            assert (want['done'][40:] != 0).sum() > 10  # (episodes end, and so resets draw, behind the crossing)
            _same(got, want)
            _same_tables(vec, o)
            _same_state(vec, o, kind)
            vec.set_state(tcount=tc)
            o.set_state(tcount=tc)
        vec.engine.vi_set(np.zeros(o.grid.S), S.policy_table(grid))
        for policy in ('uniform', 'sample'):
            want = S.rollout_of(o, grid, policy, 40)
            assert (want['done'][28:] != 0).sum() > 10
            _same(vec.rollout(40, policy, auto_reset=True, stats=True), want)
            _same_state(vec, o, kind)
            vec.set_state(tcount=tc)  # (every launch crosses)
            o.set_state(tcount=tc)
        S.drew_every_start(o)
        assert (o.state.tcount == tc).all() and (tc < 2 ** 32).all()
    finally:
        vec.close()
