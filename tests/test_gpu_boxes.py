"""Pushable boxes on the device (gu_set_boxes; csrc/gu_boxes.hip and the box gu_td_kernel instantiations) against the CPU restatement
tests/_boxes_oracle.py: step, step_device, rollout and td_run compared byte for byte -- rows, statistics, positions, WORDS, tables --,
twins on engines without boxes that do not rest on the restatement, every reset path, the library's own refusals, and the engine after
the boxes have been taken away against one that never had any.  (The calls that have no box form: tests/test_gpu_overlay.py.)

Shapes: N = 64 and 130 (three waves, the last one partial), T = 33 (two full action words and a tail of one step).  'b8': 8 x 8 with 5
boxes, b * B = 30, planes in LDS, S = 64 (b = 6).  's65': 13 x 5, S = 65 (b = 7).  'open150': 150 x 150 with 2 boxes, b = 15, three
planes do not fit 64 KiB: the L2 kernels.  'wide': 256 x 200 = 51 200 cells with 2 boxes, b * B = 32.  'claim' (4 x 4, one box) and
'two' (5 x 5, two boxes: b * B = 10, the most gu_td_init takes) carry the learners.

The runs on 'b8' assert on the restatement's own log that they met every event.  The envs are PLACED for that (`SETUPS`): each setup
is one move away from one event, and its env is handed that move (step, stream), finds it in its row of the policy table (greedy,
sample) or by chance (uniform, td_run: checked with the restatement alone).  Without auto-reset no env is ever reset, so the log
cannot show a reset there."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms.temporal_difference import q_learning
from griduniverse_amd.grid import box_plane, pack_boxes

from . import _boxes_oracle as O
from ._overlays import METHODS, same_state
from ._tabular_cases import _eps, _same, _spec, code

pytestmark = pytest.mark.gpu

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3
T = 33

# 'b8': start 9; boxes 1 (against the border above the start), 10 and 12 (a row right of the start), 17 and 25 (a column below it);
# lava 27 right of target 26; (agent, box cells, the move, what it meets)
B8_INIT = [1, 10, 12, 17, 25]
SETUPS = [(9, B8_INIT, UP, 'refused_wall'), (10, [1, 11, 12, 17, 25], RIGHT, 'refused_box'), (25, [1, 10, 12, 17, 26], RIGHT, 'refused_terminal'),
          (34, [1, 10, 12, 17, 26], UP, 'off_target'), (24, [2, 11, 13, 19, 25], RIGHT, 'solved'), (40, [2, 11, 13, 19, 26], DOWN, 'absorbing')]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid dict, boxes, targets)"""
    if name == 'b8':
        return dict(W=8, H=8, starts=[9], goals=[63], lava=[27], walls=[]), B8_INIT, [2, 11, 13, 19, 26]
    if name == 's65':
        return dict(W=13, H=5, starts=[14], goals=[64], lava=[40], walls=[30]), [15, 27], [16, 28, 3]
    if name == 'open150':
        W = 150
        assert 2 * ((W * W + 15) & ~15) <= 65536 < 3 * ((W * W + 15) & ~15)
        return dict(W=W, H=W, starts=[W + 1], goals=[W * W - 1], lava=[5 * W + 5], walls=[]), [W + 2, 2 * W + 1], [W + 3, 3 * W + 1]
    if name == 'wide':
        W, H = 256, 200
        assert 32768 < W * H <= 65536
        return dict(W=W, H=H, starts=[W + 1], goals=[W * H - 1], lava=[5 * W + 5], walls=[]), [W + 2, 2 * W + 1], [W + 3, 3 * W + 1]
    if name == 'two':
        return dict(W=5, H=5, starts=[6], goals=[24], lava=[20], walls=[]), [7, 11], [8, 16]
    assert name == 'claim'
    return O.CLAIM, O.CLAIM_BOXES['boxes'], O.CLAIM_BOXES['targets']


def _plane(name):
    g, boxes, targets = _case(name)
    return O.plane_of(g['W'] * g['H'], boxes, targets)


def _place(name, vec, o):
    """'b8': env e stands in setup e % 6 (env 0: the start, the boxes where they began); returns the setups' moves per env."""
    if name != 'b8':
        return None
    N = o.n
    pos, cells, acts = np.empty(N, np.int32), np.empty((N, 5), np.int32), np.empty(N, np.int32)
    for e in range(N):
        pos[e], cells[e], acts[e], _ = SETUPS[e % len(SETUPS)]
    vec.set_state(pos=pos)
    o.state.pos[:] = pos
    vec.set_box_cells(cells)
    o.set_cells(cells)
    return acts


def _pair(name, N, seed, q0=None, v=5):
    g, boxes, targets = _case(name)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    o = O.BoxesOracle(O.grid_of(g), seed, N, _plane(name), v, q0=q0)
    vec.set_boxes(boxes, targets, on_target=v)
    got = vec.engine.get_boxes()
    assert np.array_equal(got[0], _plane(name)) and got[1:] == (v, len(boxes), O.bits_of(g['W'] * g['H']))
    if q0 is not None:
        vec._ensure_q(q0)
    assert np.array_equal(vec.reset(), o.reset())
    return vec, o, _place(name, vec, o)


def _same_state(vec, o):
    same_state(vec, o, 'boxes')
    assert np.array_equal(vec.box_cells(), o.cells)


def _saw(o, auto):
    assert o.saw_everything(resets=auto), o.log


# ---- 1: round trip and errors ----
def test_set_boxes_round_trip_and_errors():
    g, boxes, targets = _case('b8')
    plane = _plane('b8')
    vec = gua.VecGridUniverse(8, template=_spec(g))
    try:
        eng = vec.engine
        assert vec.boxes() is None and eng.get_boxes() is None
        assert code(lambda: eng.get_boxes_state()) == -4 and code(lambda: eng.set_boxes_state(np.zeros(8, np.uint32))) == -4
        vec.set_boxes(boxes[::-1], targets, on_target=7)
        got = vec.boxes()
        assert got['boxes'].tolist() == boxes and got['targets'].tolist() == sorted(targets) and got['on_target'] == 7
        st = eng.stores()
        assert st['overlay'] == 4 and st['overlay_bits'] == 30 and eng.td_rows == 64 << 30
        assert np.array_equal(vec.box_cells(), np.tile(boxes, (8, 1))) and vec.box_cells(2, 3).shape == (3, 5)
        vec.set_box_cells([[2, 11, 13, 19, 26], [3, 4, 5, 6, 7]], env0=2)
        assert vec.box_cells(2, 2).tolist() == [[2, 11, 13, 19, 26], [3, 4, 5, 6, 7]]
        word = lambda cells: np.array([sum(c << (6 * k) for k, c in enumerate(cells))], np.uint32)  # noqa: E731
        for bad in (np.array([1 << 30], np.uint32), word([1, 1, 12, 17, 25]), word([63, 10, 12, 17, 25]), word([27, 10, 12, 17, 25])):
            assert code(lambda: eng.set_boxes_state(bad, 0)) == -1  # a bit above b * B; two fields equal; a goal cell; a lava cell
        on = lambda p, s, byte: np.where(np.arange(64) == s, byte, p).astype(np.uint8)  # noqa: E731
        bad_planes = [on(plane, 40, 4), on(plane, 40, 128), on(plane, 63, 1), on(plane, 27, 2), on(plane, 9, 2),  # bits 2, 7; goal; lava; start
                      on(on(plane, 2, 0), 11, 0), O.plane_of(64, [2, 11], [2, 11, 13]), O.plane_of(64, [], [5]),  # 3 targets for 5 boxes; all on target; no box
                      O.plane_of(64, [1, 10, 12, 17, 25, 30], [2, 11, 13, 19, 26, 31])]  # 6 boxes of 6 bits
        for i, bad in enumerate(bad_planes):
            assert code(lambda: eng.set_boxes(bad, 5)) == -1, i
        for v in (-1, 17):
            assert code(lambda: eng.set_boxes(plane, v)) == -1
        assert np.array_equal(eng.get_boxes()[0], plane) and eng.get_boxes()[1] == 7  # a refused call changes nothing
        assert vec.box_cells(2, 2).tolist() == [[2, 11, 13, 19, 26], [3, 4, 5, 6, 7]]
        vec.set_boxes(boxes, targets)  # set_boxes puts every env's boxes back
        assert np.array_equal(vec.box_cells(), np.tile(boxes, (8, 1))) and vec.boxes()['on_target'] == 5
        vec.set_boxes(None)
        assert vec.boxes() is None and eng.stores()['overlay'] == 0
    finally:
        vec.close()


def test_walls_and_fields_outside_the_grid_are_refused_by_the_library_itself():
    """S = 65, b = 7: a field can hold 65 .. 127, cells that do not exist -- the check that keeps a caller's word inside the planes --,
    and the grid has a wall.  The facade refuses all of these before the library is called, so they go through the Engine."""
    g, boxes, targets = _case('s65')
    wall, S = g['walls'][0], 65
    vec = gua.VecGridUniverse(8, template=_spec(g))
    try:
        eng = vec.engine
        vec.set_boxes(boxes, targets)
        vec.set_box_cells([[16, 28], [3, 4]], env0=2)
        plane, words = eng.get_boxes()[0].copy(), eng.get_boxes_state()
        word = lambda a, b: np.array([a | b << 7], np.uint32)  # noqa: E731
        bad_words = [word(100, 27), word(15, 65), word(15, 127), word(wall, 27), word(15, wall)]  # a field >= S (first, second, all ones); a wall
        for i, bad in enumerate(bad_words):
            for env0 in (0, 7):
                assert code(lambda: eng.set_boxes_state(bad, env0)) == -1, i
        assert code(lambda: eng.set_boxes_state(np.concatenate([word(15, 27), word(100, 27)]), 3)) == -1  # ... behind a valid one: none is installed
        bad_planes = [O.plane_of(S, boxes + [wall], targets), O.plane_of(S, boxes, targets + [wall]), O.plane_of(S, [wall], targets)]
        for i, bad in enumerate(bad_planes):
            assert code(lambda: eng.set_boxes(bad, 5)) == -1, i
        assert np.array_equal(eng.get_boxes()[0], plane) and np.array_equal(eng.get_boxes_state(), words)
        eng.set_boxes_state(word(63, 0), 0)  # the last free cell and cell 0 are cells
        assert vec.box_cells(0, 1).tolist() == [[63, 0]]
    finally:
        vec.close()


# ---- 2: step and step_device ----
@pytest.mark.parametrize('N', [64, 130])
@pytest.mark.parametrize('auto', [True, False])
def test_step_and_step_device_equal_the_oracle(auto, N):
    vec, o, first = _pair('b8', N, 4)
    try:
        vec.auto_reset = auto
        acts = np.random.RandomState(11).randint(-4, 4, (T, N)).astype(np.int32)
        acts[0] = first
        for i in range(T):
            a = acts[i].copy()
            if i == 20:  # env 5 is given a rejected action: it does not step, and its word and position stay
                before = (vec.get_state()['pos'][5], vec.box_cells(5, 1).tolist())
                a[5] = 7
                assert code(lambda: vec.step(a)) == -1
                o.step(a, auto)
                _same_state(vec, o)
                assert (vec.get_state()['pos'][5], vec.box_cells(5, 1).tolist()) == before
                continue
            obs, rew, don, _ = vec.step(a, zero_copy=(i % 2 == 1))
            w_obs, w_rew, w_don, rejected = o.step(a, auto)
            assert not rejected.any()
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0), i
        _saw(o, auto)
        _same_state(vec, o)
        # the same rows from the device-resident stream
        vec.seed(4)
        o2 = O.BoxesOracle(o.grid, 4, N, o.box, o.v, q0=None)
        assert np.array_equal(vec.reset(), o2.reset())
        assert np.array_equal(vec.box_cells(), o2.cells)
        _place('b8', vec, o2)
        acts[20, 5] = 0
        vec.engine.upload_actions(acts)
        for i in range(T):
            vec.engine.step_device(i, auto)
            obs, rew, don = vec.engine.read_outputs()
            w_obs, w_rew, w_don, _ = o2.step(acts[i], auto)
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don != 0, w_don != 0), i
        _saw(o2, auto)
        _same_state(vec, o2)
    finally:
        vec.close()


# ---- 3: rollout ----
def _policy_table(S):
    pi = np.random.RandomState(1).dirichlet(np.ones(4), S)
    for s, _, a, _ in SETUPS:  # one-hot rows on the setups' cells: thresholds that no word reaches
        pi[s] = np.eye(4)[a]
    return pi


@pytest.mark.parametrize('N', [130, 64])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('policy', ['uniform', 'stream', 'greedy', 'sample'])
def test_rollout_equals_the_oracle(policy, auto, N):
    seed = 6
    vec, o, first = _pair('b8', N, seed)
    try:
        S = o.grid.S
        pi = _policy_table(S) if policy in ('greedy', 'sample') else None
        acts = None
        if policy == 'stream':
            acts = np.random.RandomState(2).randint(0, 4, (T, N)).astype(np.int32)
            acts[0] = first
        if pi is not None:
            vec.engine.vi_set(np.zeros(S), pi)
        want = o.rollout(T, policy, auto, actions=acts, pi=pi)
        _saw(o, auto)
        # launches of 16 and 17 ...
        parts = [vec.rollout(n, policy, actions=None if acts is None else acts[t0:t0 + n], auto_reset=auto, stats=True) for t0, n in ((0, 16), (16, 17))]
        form = vec.engine.rollout_last_form()
        assert form['family'] == 'boxes' and form['lds_bytes'] > 0
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(np.concatenate([h[k] for h in parts]), want[k]), k
        assert np.array_equal(parts[0]['ret'] + parts[1]['ret'], want['ret'])
        assert np.array_equal(parts[0]['episodes'] + parts[1]['episodes'], want['episodes'])
        _same_state(vec, o)
        # ... equal one of 33, and statistics alone
        for traj in (True, False):
            vec.seed(seed)
            vec.reset()
            _place('b8', vec, o)  # (moves o's envs too: its state is compared only behind the last launch)
            got = vec.rollout(T, policy, actions=acts, auto_reset=auto, trajectory=traj, stats=True)
            _same(got, want, ('obs', 'reward', 'done', 'ret', 'episodes') if traj else ('ret', 'episodes'))
        with pytest.raises(gua.GuError) as err:
            vec.engine.rollout(8, 'uniform', True, 'packed')
        assert err.value.code == -6 and 'boxes' in str(err.value)
    finally:
        vec.close()


@pytest.mark.parametrize('case', ['s65', 'open150', 'wide'])
def test_other_widths_and_the_l2_path_equal_the_oracle(case):
    N = 130
    vec, o, _ = _pair(case, N, 3)
    try:
        g = _case(case)[0]
        S = g['W'] * g['H']
        bits = O.bits_of(S) * 2
        assert vec.engine.stores()['overlay_bits'] == bits == {'s65': 14, 'open150': 30, 'wide': 32}[case]
        for policy, auto in (('uniform', True), ('stream', False)):
            acts = np.random.RandomState(5).randint(0, 4, (T, N)).astype(np.int32) if policy == 'stream' else None
            got = vec.rollout(T, policy, actions=acts, auto_reset=auto, stats=True)
            form = vec.engine.rollout_last_form()
            assert form['family'] == 'boxes' and (form['lds_bytes'] == 0) == (case != 's65')
            _same(got, o.rollout(T, policy, auto, actions=acts))
            _same_state(vec, o)
        assert o.log['push'] > 0 and o.log['refused_wall'] + o.log['refused_box'] > 0, o.log
        assert (o.cells != o.init).any()
        vec.auto_reset = True
        for i in range(8):  # the step kernel on the same planes
            a = np.random.RandomState(i).randint(0, 4, N).astype(np.int32)
            obs, rew, don, _ = vec.step(a)
            w = o.step(a, True)
            assert np.array_equal(obs, w[0]) and np.array_equal(rew, w[1]) and np.array_equal(don, w[2] != 0)
        _same_state(vec, o)
        assert code(lambda: vec.engine.td_init(0.0)) == -1  # more than 10 bits
    finally:
        vec.close()


# ---- 4: twins that do not rest on the oracle ----
@pytest.mark.parametrize('kind', ['walled_in', 'immovable'])
def test_twins_on_engines_without_boxes(kind):
    """walled_in: the box in the corner 7 behind walls on 6 and 15 -- no agent reaches it: the engine walks as the one without boxes.
    immovable: the box in the open corner 7 -- both approaches push it against the border: the engine walks as one with a wall there."""
    N, S = 130, 64
    g = dict(W=8, H=8, starts=[9], goals=[63], lava=[27], walls=[6, 15] if kind == 'walled_in' else [])
    twin_g = g if kind == 'walled_in' else dict(g, walls=[7])
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=5)
    twin = gua.VecGridUniverse(N, template=_spec(twin_g), seed=5)
    try:
        vec.set_boxes([7], [20])
        assert np.array_equal(vec.reset(), twin.reset())
        free = np.array([s for s in O.free_cells(twin_g) if s != 7], np.int32)
        pos = free[np.random.RandomState(N).randint(0, len(free), N)]
        pos[:8] = [5, 14, 6, 15, 5, 14, 13, 4][:8] if kind == 'immovable' else 9  # (beside the box)
        for v in (vec, twin):
            v.set_state(pos=pos)
        for auto in (True, False):
            got = vec.rollout(60, 'uniform', auto_reset=auto, stats=True)
            assert vec.engine.rollout_last_form()['family'] == 'boxes'
            _same(got, twin.rollout(60, 'uniform', auto_reset=auto, stats=True))
            assert not (got['obs'] == 7).any()
        for v in (vec, twin):
            v.reset()
            v._ensure_q(0.25)
        kw = dict(alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        for method in ('q_learning', 'sarsa'):
            _same(vec.td_run(120, method, **kw), twin.td_run(120, method, **kw))
        q, want = vec.q_table(), twin.q_table()
        assert q.shape == (N, S << 6, 4) and want.shape == (N, S, 4)
        assert q[:, 7 * S:8 * S].tobytes() == want.tobytes() and (want != 0.25).any()
        assert (np.delete(q, np.s_[7 * S:8 * S], axis=1) == 0.25).all()
        a, b = vec.get_state(), twin.get_state()
        assert all(np.array_equal(a[k], b[k]) for k in ('pos', 'done', 'episode', 'tcount'))
        assert (vec.box_cells() == 7).all()
    finally:
        vec.close()
        twin.close()


# ---- 5: td_run ----
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('case,N,steps', [('claim', 130, 300), ('two', 64, 100)])
def test_td_run_tables_rows_and_words_equal_the_oracle(case, N, steps, method):
    vec, o, _ = _pair(case, N, 3, q0=0.5)
    try:
        S, bits = o.grid.S, o.b * o.B
        assert vec.engine.td_rows == S << bits
        if case == 'claim':  # tables of [n, S << bits, 4] through set_q_table / q_table
            q = np.random.RandomState(7).uniform(-1, 1, (N, S << bits, 4))
            vec.set_q_table(q)
            o.q[:] = q
            assert vec.q_table(3, 2).tobytes() == q[3:5].tobytes()
        want = o.td_run(steps, METHODS[method], 0.25, 0.9, _eps(0.3))
        assert all(o.log[k] > 0 for k in ('push', 'refused_wall', 'reset_restored')), o.log
        assert all(o.log[k] > 0 for k in ('onto_target', 'solved', 'refused_terminal')), o.log
        assert case != 'two' or (o.log['refused_box'] > 0 and o.log['off_target'] > 0), o.log  # (one box, one target: on target is solved)
        got = vec.td_run(steps, method, alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        _same(got, want)
        assert vec.q_table().shape == (N, S << bits, 4) and vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()


def test_sarsa_split_in_two_carries_its_action_and_set_boxes_and_set_box_cells_drop_it():
    vec, o, _ = _pair('claim', 130, 8, q0=0.0)
    twin, o1, _ = _pair('claim', 130, 8, q0=0.0)
    try:
        kw = dict(alpha=0.5, discount_factor=0.95, epsilon=0.3, trajectory=True, stats=True)
        for n in (100, 100):  # the second launch starts with the first one's a'
            _same(vec.td_run(n, 'sarsa', **kw), o.td_run(n, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert o.carry_valid and (o.carry >= 0).any()
        _same(twin.td_run(200, 'sarsa', **kw), o1.td_run(200, O.SARSA, 0.5, 0.95, _eps(0.3)))  # ... and equals one launch
        assert vec.q_table().tobytes() == twin.q_table().tobytes() == o.q.tobytes()
        cells = o.cells.copy()
        vec.set_box_cells(cells)  # the same cells again: the carry goes
        o.set_cells(cells)
        _same(vec.td_run(50, 'sarsa', **kw), o.td_run(50, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert o.carry_valid
        vec.engine.set_boxes(o.box, o.v)  # the same boxes again: tables, positions and counts stay, the words and the carry go
        q = o.q.copy()
        o.set_boxes(o.box, o.v)
        assert o.q.tobytes() == q.tobytes()
        _same(vec.td_run(50, 'sarsa', **kw), o.td_run(50, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()
        twin.close()


# ---- 6: reset paths ----
def test_every_reset_path_restores_the_boxes_of_the_envs_it_resets():
    N = 130
    vec, o, _ = _pair('b8', N, 2)
    try:
        _same(vec.rollout(40, 'uniform', auto_reset=False, stats=True), o.rollout(40, 'uniform', False))
        moved = (o.cells != o.init).any(axis=1)
        done = o.state.done != 0
        assert (moved & done).any() and (moved & ~done).any()
        _same_state(vec, o)
        before = o.cells.copy()
        vec.set_state(pos=o.state.pos)  # set_state and seed leave the words alone
        vec.seed(2)
        o.state.episode[:] = 0
        o.state.tcount[:] = 0
        assert np.array_equal(vec.box_cells(), before)
        vec.engine.reset_done()  # the done envs only
        d = o.reset_done()
        assert d.any() and (o.cells[d] == o.init).all() and np.array_equal(o.cells[~d], before[~d])
        _same_state(vec, o)
        mask = (np.arange(N) % 3 == 0).astype(np.uint8)
        assert np.array_equal(vec.reset(mask), o.reset(mask))  # the masked envs only
        assert (o.cells[mask == 0] != o.init).any() and (o.cells[mask != 0] == o.init).all()
        _same_state(vec, o)
        _same(vec.rollout(60, 'uniform', auto_reset=True, stats=True), o.rollout(60, 'uniform', True))  # the lazy reset
        assert o.log['reset_restored'] > 0
        _same_state(vec, o)
        cells = np.tile([1, 11, 12, 17, 26], (N, 1))
        flags = np.zeros(N, np.int32)
        flags[::2] = 1
        vec.set_box_cells(cells)
        vec.set_state(done=flags)
        o.set_cells(cells)
        o.state.done[:] = flags
        acts = np.full(N, LEFT, np.int32)
        vec.auto_reset = True
        obs, _, _, _ = vec.step(acts)  # the step kernel's lazy reset
        assert np.array_equal(obs, o.step(acts, True)[0])
        assert (o.cells[::2] == o.init).all() and (o.cells[1::2, 4] == 26).all()  # (an env that was not done keeps its boxes, but for one it may push)
        _same_state(vec, o)
        assert np.array_equal(vec.reset(), o.reset()) and np.array_equal(vec.box_cells(), np.tile(B8_INIT, (N, 1)))
    finally:
        vec.close()


# ---- 7: refusals (the calls without a box form: tests/test_gpu_overlay.py) ----
def test_a_refused_plane_or_word_leaves_plane_words_and_q_tables_as_they_were():
    g, boxes, targets = _case('claim')
    N, S = 64, 16
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=1)
    try:
        eng = vec.engine
        vec.reset()
        vec.set_boxes(boxes, targets)
        plane = eng.get_boxes()[0]
        vec._ensure_q()
        vec.td_run(50, 'q_learning')
        words, q, rows = eng.get_boxes_state(), vec.q_table(), eng.td_rows
        assert rows == S << 4 and q.any()
        assert code(lambda: eng.set_boxes(O.plane_of(S, [12], [10]), 5)) == -1  # a box on the lava cell
        assert code(lambda: eng.set_boxes_state(np.array([12], np.uint32))) == -1
        assert np.array_equal(eng.get_boxes()[0], plane) and np.array_equal(eng.get_boxes_state(), words)
        assert eng.td_rows == rows and vec.q_table().tobytes() == q.tobytes()
    finally:
        vec.close()


# ---- 8: the slot ----
def test_an_engine_without_its_boxes_again_is_the_engine_that_never_had_any_and_the_slot_takes_the_next_kind():
    g, boxes, targets = _case('b8')
    N, seed = 130, 9
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    ref = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    try:
        vec.set_boxes(boxes, targets)
        vec.reset()
        vec.rollout(20, 'uniform', auto_reset=True)
        assert vec.engine.rollout_last_form()['family'] == 'boxes'
        vec.set_boxes(None)
        vec.set_boxes([10], [11])  # ten bits: tables
        vec.td_run(20, 'q_learning')
        vec.set_boxes(None)
        assert code(lambda: vec.engine.td_run(5)) == -4  # the tables of S << 6 rows went with the boxes
        # the slot after boxes: fruit's and doors' masks are zero at reset, not the boxes' word
        vec.set_fruit([10, 12])
        vec.reset()
        assert not vec.fruit_eaten().any()
        vec.set_fruit(None)
        vec.set_doors({0: 10}, keys={0: 12})
        vec.set_doors_open(np.ones(N, np.uint32))
        vec.reset()
        assert not vec.doors_open().any()
        vec.set_doors(None)
        vec.seed(seed)
        assert np.array_equal(vec.reset(), ref.reset())
        for auto in (True, False):
            _same(vec.rollout(100, 'uniform', auto_reset=auto, stats=True), ref.rollout(100, 'uniform', auto_reset=auto, stats=True))
            a, b = vec.engine.rollout_last_form(), ref.engine.rollout_last_form()
            assert a['family'] == b['family'] != 'boxes' and a['words'] == b['words']
        acts = np.random.RandomState(3).randint(0, 4, (8, N)).astype(np.int32)
        for i in range(8):
            a, b = vec.step(acts[i]), ref.step(acts[i])
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        for method in ('q_learning', 'sarsa'):
            kw = dict(alpha=0.3, discount_factor=0.9, epsilon=0.2, trajectory=True, stats=True)
            _same(vec.td_run(120, method, **kw), ref.td_run(120, method, **kw))
            assert vec.q_table().shape == (N, 64, 4) and vec.q_table().tobytes() == ref.q_table().tobytes()
        a, b = vec.get_state(), ref.get_state()
        assert all(np.array_equal(a[k], b[k]) for k in ('pos', 'done', 'episode', 'tcount'))
    finally:
        vec.close()
        ref.close()


# ---- 9: the learning claim ----
def test_q_learning_end_to_end_solves_the_level_along_a_shortest_solution():
    """64 learners, O.CLAIM_STEPS steps, alpha 0.5, gamma 0.95, epsilon 0.1 on the 4 x 4 grid of tests/test_boxes_host.py: every greedy
    walk over (cell, word) rows is a shortest solution -- 4 moves, return 7, the box on its target."""
    L = O.CLAIM_LEARNERS
    env = _spec(O.CLAIM)  # (a GridSpec: the level has no goal cell, and a GridUniverseEnv always has one)
    q = q_learning(env, O.CLAIM_STEPS, alpha=O.CLAIM_ALPHA, discount_factor=O.CLAIM_GAMMA, epsilon=0.1, num_learners=L, seed=1, boxes=O.CLAIM_BOXES)
    grid, plane = O.grid_of(O.CLAIM), box_plane(4, 4, O.CLAIM_BOXES['boxes'], O.CLAIM_BOXES['targets'])
    assert q.shape == (L, 16 << 4, 4)
    assert O.shortest_solution(grid, plane, 5, 4) == O.CLAIM_WALK[:2]
    walks = [O.greedy_walk(grid, plane, 5, q[e]) for e in range(L)]
    assert walks == [O.CLAIM_WALK] * L, walks
    assert int(pack_boxes(16, [10])) == 10
