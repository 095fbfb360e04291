"""Pushable boxes, the parts that need no GPU: the box plane, the words, the XSB parser, the argument checks, the library's symbols, the
CPU restatement against the calm C oracle in two identities that do not rest on the new code, rules 2-6 on hand-written walks, and the
learning claim on the 4 x 4 grid."""
import re
import subprocess

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import q_learning, sarsa
from griduniverse_amd.grid import GridSpec, box_bits, box_plane, pack_boxes, sokoban_level, unpack_boxes
from oracle import c_oracle as C

from . import _boxes_oracle as O
from ._tabular_cases import _spec

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


def test_box_plane_pack_and_unpack_shapes_round_trip_and_errors():
    p = box_plane(5, 3, [7, 3], [3, 11, 14])
    assert p.dtype == np.uint8 and p.shape == (15,)
    want = np.zeros(15, np.uint8)
    want[7], want[3], want[11], want[14] = 2, 3, 1, 1
    assert np.array_equal(p, want) and np.array_equal(p, O.plane_of(15, [7, 3], [3, 11, 14]))
    assert np.array_equal(box_plane(5, 3, 7, np.array([11])), box_plane(5, 3, [7], [11]))
    assert [box_bits(S) for S in (1, 2, 3, 64, 65, 256, 257, 1024, 32768, 32769, 65536)] == [1, 1, 2, 6, 7, 8, 9, 10, 15, 16, 16]
    for kw in (dict(boxes=[], targets=[1]), dict(boxes=[1], targets=[]), dict(boxes=[1, 2], targets=[3]), dict(boxes=[1], targets=[1]),  # none; too few targets; solved
               dict(boxes=[1, 2], targets=[1, 2, 3]), dict(boxes=[15], targets=[1]), dict(boxes=[1], targets=[-1]), dict(boxes=[1, 1], targets=[2, 3]),
               dict(boxes=[1.5], targets=[2]), dict(boxes=[[1]], targets=[2]), dict(boxes=[True], targets=[2]), dict(boxes=None, targets=[2])):
        with pytest.raises(ValueError):
            box_plane(5, 3, **kw)
    box_plane(8, 8, [1, 2, 3, 4, 5], [11, 12, 13, 14, 15])  # 5 x 6 bits
    with pytest.raises(ValueError):
        box_plane(8, 8, [1, 2, 3, 4, 5, 6], [11, 12, 13, 14, 15, 16])  # 6 x 6 bits
    box_plane(256, 256, [1, 2], [3, 4])  # 2 x 16 bits: all 32
    with pytest.raises(ValueError):
        box_plane(256, 256, [1, 2, 5], [3, 4, 6])
    cells = np.array([[1, 10, 63], [63, 0, 5]])
    words = pack_boxes(64, cells)
    assert words.dtype == np.uint32 and words.tolist() == [1 | 10 << 6 | 63 << 12, 63 | 0 << 6 | 5 << 12]
    assert np.array_equal(unpack_boxes(64, words, 3), cells) and unpack_boxes(64, words, 3).dtype == np.int32
    assert int(pack_boxes(64, [1, 10, 63])) == words[0] and unpack_boxes(64, words[0], 3).tolist() == [1, 10, 63]
    top = pack_boxes(65536, [[65535, 65534]])  # b * B = 32: the top bit is in use
    assert top.tolist() == [65535 | 65534 << 16] and unpack_boxes(65536, top, 2).tolist() == [[65535, 65534]]
    assert np.array_equal(words, O.pack(64, cells))
    for bad in ([[1, 1, 2]], [[64, 1, 2]], [[-1, 1, 2]], [[1, 2, 3, 4, 5, 6]], [[1.0, 2.0]], 5, [[]]):
        with pytest.raises(ValueError):
            pack_boxes(64, bad)
    for B in (0, 6):
        with pytest.raises(ValueError):
            unpack_boxes(64, words, B)


def test_sokoban_level_parses_the_xsb_characters_and_pads_ragged_rows():
    spec, boxes, targets = sokoban_level('''
#####
#@$.#
# *.
#-
''')
    assert isinstance(spec, GridSpec) and (spec.W, spec.H) == (5, 4)
    assert np.flatnonzero(spec.wall).tolist() == [0, 1, 2, 3, 4, 5, 9, 10, 15] and not spec.goal.any() and not spec.lava.any()
    assert boxes == [7, 12] and targets == [8, 12, 13]
    assert spec.starts == [6]
    spec2, boxes2, targets2 = sokoban_level('#+$ ')
    assert spec2.starts == [1] and boxes2 == [2] and targets2 == [1]
    box_plane(spec.W, spec.H, boxes, targets)
    for bad in ('', '\n\n', '#@@#', '#$.#', '#@x#'):
        with pytest.raises(ValueError):
            sokoban_level(bad)


class _NoEngine(object):
    """Stands in for Engine: any call on it is a library call that must not have been made."""

    def __init__(self, *a, **kw):
        self.calls, self.held = [], {'overlay': 4, 'overlay_bits': 12}

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
        return call

    def stores(self):
        return self.held


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    g = dict(W=8, H=8, starts=[9], goals=[63], lava=[27], walls=[5])
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    for kw in (dict(boxes=[5], targets=[1]), dict(boxes=[1], targets=[5]), dict(boxes=[63], targets=[1]), dict(boxes=[1], targets=[27]),  # wall, goal, lava
               dict(boxes=[9], targets=[1]), dict(boxes=[1], targets=[1]), dict(boxes=[1, 2], targets=[3]), dict(boxes=[64], targets=[1]),  # a start; solved; few targets; outside
               dict(boxes=[1], targets=[2], on_target=17), dict(boxes=[1], targets=[2], on_target=-1), dict(boxes=[1], targets=[2], on_target=2.5),
               dict(boxes=[1], targets=[2], on_target=True), dict(boxes=None, targets=[2]), dict(boxes=[1], targets=None)):
        with pytest.raises(ValueError):
            vec.set_boxes(**kw)
    for cells in ([[1, 1]], [[1, 64]], [[1, 5]], [[1, 63]], [[1, 27]], [[1, 2, 3]], [[1]], [[1.0, 2.0]], 3):  # equal; outside; wall; goal; lava; not two boxes
        with pytest.raises(ValueError):
            vec.set_box_cells(cells)
    assert vec.engine.calls == []
    vec.set_boxes([1], [9], on_target=0)  # (a target may lie on a start cell)
    vec.set_box_cells([[1, 2], [3, 4]], env0=1)
    vec.set_box_cells([9, 2])  # (a box may be put on a start cell later)
    vec.set_boxes(None)
    assert vec.engine.calls == ['set_boxes', 'set_boxes_state', 'set_boxes_state', 'set_boxes']
    vec.engine.held = {'overlay': 3, 'overlay_bits': 2}  # doors are set, not boxes
    with pytest.raises(ValueError, match='no boxes set: call set_boxes first'):
        vec.set_box_cells([[1, 2]])
    assert len(vec.engine.calls) == 4
    env = gua.GridUniverseEnv(grid_shape=(4, 4))
    ok = dict(boxes=[5], targets=[10])
    for f in (q_learning, sarsa):
        for kw, message in ((dict(boxes=ok, wind=np.zeros(4, int)), 'boxes exclude wind, fruit and doors'), (dict(boxes=ok, fruit=([1], 'apple', (1, 2, 3))), 'boxes exclude'),
                            (dict(boxes=ok, doors=dict(doors={0: 1}, keys={0: 2})), 'boxes exclude'), (dict(boxes=dict(boxes=[5])), 'boxes must be dict'),
                            (dict(boxes=dict(boxes=[5], targets=[10], value=3)), 'boxes must be dict'), (dict(boxes=[5]), 'boxes must be dict')):
            with pytest.raises(ValueError, match=message):
                f(env, 10, **kw)


def test_header_binding_and_library_hold_the_box_entry_points_and_kernels():
    names = ('gu_set_boxes', 'gu_get_boxes', 'gu_get_boxes_state', 'gu_set_boxes_state')
    header = open(_lib.LIB_PATH.rsplit('/griduniverse_amd/', 1)[0] + '/include/gu.h').read() if '/griduniverse_amd/' in _lib.LIB_PATH else None
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in names:
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
        assert header is None or 'int ' + name + '(gu_handle h' in header, name
    blob = open(_lib.LIB_PATH, 'rb').read()
    for frame in (b'gu_overlay_step_kernel', b'gu_overlay_rollout_kernel'):  # the frame's name and the kind's rule type in ONE mangled symbol
        assert re.search(frame + rb'I\d+BoxRule', blob), frame
    assert b'gu_overlay_reset_kernel' in blob
    assert gua.Engine.ROLLOUT_FAMILIES[7] == 'boxes'


# ---- rules 2-6 on hand-written walks: 4 x 4, start 0, goal 15, lava 12, on_target 5 ----
_G = dict(W=4, H=4, starts=[0], goals=[15], lava=[12], walls=[])


def _walk(acts, boxes, targets, pos=None, cells=None, g=_G, v=5):
    """[(cell, box cells, reward, done)] of one env."""
    o = O.BoxesOracle(O.grid_of(g), 0, 1, O.plane_of(g['W'] * g['H'], boxes, targets), v, q0=None)
    o.reset()
    if pos is not None:
        o.state.pos[0] = pos
    if cells is not None:
        o.set_cells([cells])
    out = []
    for a in acts:
        s, r, d = o._move(np.array([a], np.int32))
        out.append((int(s[0]), o.cells[0].tolist(), int(r[0]), int(d[0])))
    return out, o


def test_rule_4_a_push_moves_the_box_and_the_agent_and_the_border_a_terminal_cell_and_a_box_refuse_it():
    out, o = _walk([RIGHT, RIGHT, RIGHT], [1], [10])  # 1 -> 2 -> 3, then the border
    assert out == [(1, [2], -1, 0), (2, [3], -1, 0), (2, [3], -1, 0)]
    assert o.log['push'] == 2 and o.log['refused_wall'] == 1
    out, o = _walk([DOWN, DOWN], [4], [10])  # 4 -> 8, then lava at 12
    assert out == [(4, [8], -1, 0), (4, [8], -1, 0)] and o.log['refused_terminal'] == 1
    out, o = _walk([RIGHT], [1, 2], [10, 11])  # a second box behind the first
    assert out == [(0, [1, 2], -1, 0)] and o.log['refused_box'] == 1
    out, o = _walk([RIGHT], [1], [10], g=dict(_G, walls=[2]))  # a wall behind the box
    assert out == [(0, [1], -1, 0)] and o.log['refused_wall'] == 1
    out, o = _walk([RIGHT], [14], [10], pos=13)  # the goal cell behind the box
    assert out == [(13, [14], -1, 0)] and o.log['refused_terminal'] == 1


def test_rule_5_an_agent_on_a_box_cell_leaves_it_like_any_cell():
    out, o = _walk([RIGHT, LEFT, LEFT], [5], [10], pos=5)  # (after gu_set_state): leaves, comes back pushing
    assert out == [(6, [5], -1, 0), (5, [4], -1, 0), (5, [4], -1, 0)]  # ... and the third move is refused by the border
    assert o.log['push'] == 1 and o.log['refused_wall'] == 1
    out, o = _walk([UP], [1], [10], pos=1)  # a wall bump on the box cell is no push
    assert out == [(1, [1], -1, 0)] and o.log['push'] == o.log['refused_wall'] == 0


def test_rule_6_a_push_onto_a_target_pays_and_the_push_off_takes_it_back():
    out, o = _walk([RIGHT, RIGHT], [1, 9], [2, 6])  # 1 -> 2 (target): -1 + 5; 2 -> 3: -1 - 5
    assert out == [(1, [2, 9], 4, 0), (2, [3, 9], -6, 0)]
    assert o.log['onto_target'] == 1 and o.log['off_target'] == 1 and o.log['solved'] == 0
    out, o = _walk([RIGHT], [1, 9], [2, 3], cells=[2, 9], pos=1)  # target to target pays nothing extra
    assert out == [(2, [3, 9], -1, 0)]
    out, _ = _walk([RIGHT], [1], [2], v=0, g=dict(_G))  # v = 0: only the solving step pays
    assert out == [(1, [2], 10, 1)]


def test_rules_2_and_6_the_solving_step_pays_exactly_10_and_a_solved_word_is_absorbing():
    out, o = _walk([RIGHT, RIGHT, DOWN, LEFT], [1, 9], [2, 9])  # box 9 is on its target already; 1 -> 2 solves: +10, not -1 + 5
    assert out == [(1, [2, 9], 10, 1), (1, [2, 9], 10, 1), (1, [2, 9], 10, 1), (1, [2, 9], 10, 1)]
    assert o.log['solved'] == 1 and o.log['absorbing'] == 3 and o.log['onto_target'] == 1 and (o.state.tcount == 4).all()
    out, _ = _walk([DOWN], [1], [2], cells=[2], pos=8)  # solved is a property of the word: the lava below does not matter
    assert out == [(8, [2], 10, 1)]
    # ... and the lazy reset puts the boxes back
    o.state.done[0] = 1
    o._lazy_reset()
    assert o.cells[0].tolist() == [1, 9] and o.log['reset_restored'] == 1 and not o.solved()[0]


def test_a_rejected_action_moves_nothing_and_resets_nothing():
    o = O.BoxesOracle(O.grid_of(_G), 0, 2, O.plane_of(16, [1], [10]), q0=None)
    o.reset()
    o.set_cells([[2], [2]])
    o.state.done[:] = 1
    obs, _, _, rejected = o.step([7, RIGHT], auto_reset=True)
    assert rejected.tolist() == [True, False] and o.cells.tolist() == [[2], [2]] and o.state.tcount.tolist() == [0, 1]
    assert o.state.done.tolist() == [1, 0] and obs.tolist() == [0, 1]  # env 1 was reset and pushed its box 1 -> 2 again


# ---- two identities that rest on the calm C oracle alone ----
def _calm(g, seed, N, T, auto):
    grid = O.grid_of(g)
    st = C.State(N)
    C.reset(grid, seed, st)
    return C.rollout(grid, seed, st, T, auto_reset=auto, trajectory=True, stats=True), st


@pytest.mark.parametrize('kind', ['walled_in', 'immovable'])
def test_boxes_nobody_reaches_or_moves_leave_the_calm_oracles_rows(kind):
    """(a) the box in the corner 7 behind walls on 6 and 15: rows equal the calm oracle's on the same grid.  (b) the box in the open
    corner 7, which both approaches push against the border: rows equal the calm oracle's on the twin grid with a wall on 7."""
    g = dict(W=8, H=8, starts=[9], goals=[63], lava=[27], walls=[6, 15] if kind == 'walled_in' else [])
    twin = g if kind == 'walled_in' else dict(g, walls=[7])
    for N, seed in ((1, 2), (64, 9), (37, 5)):
        for auto in (True, False):
            o = O.BoxesOracle(O.grid_of(g), seed, N, O.plane_of(64, [7], [20]), q0=None)
            o.reset()
            got = o.rollout(200, 'uniform', auto)
            want, st = _calm(twin, seed, N, 200, auto)
            for k in ('obs', 'reward', 'done'):
                assert np.array_equal(got[k], want[k]), (k, N, auto)
            assert np.array_equal(o.state.pos, st.pos) and np.array_equal(o.state.episode, st.episode)
            assert (o.cells == 7).all() and o.log['push'] == 0
            assert kind != 'walled_in' or o.log['refused_wall'] == 0


# ---- the learning claim ----
def _claim():
    return O.grid_of(O.CLAIM), O.plane_of(16, O.CLAIM_BOXES['boxes'], O.CLAIM_BOXES['targets'])


def test_the_claims_shortest_solution_pushes_right_walks_round_and_pushes_down():
    grid, plane = _claim()
    assert O.shortest_solution(grid, plane, 5, 4) == O.CLAIM_WALK[:2] == (4, 7)
    out, o = _walk([RIGHT, UP, RIGHT, DOWN], [5], [10], g=O.CLAIM)
    assert out == [(5, [6], -1, 0), (1, [6], -1, 0), (2, [6], -1, 0), (6, [10], 10, 1)]
    assert O.shortest_solution(grid, O.plane_of(16, [3], [10]), 5, 4) is None  # a box in the corner is a deadlock
    q = np.zeros((16 << 4, 4))
    for (s, w), a in {(4, 5): RIGHT, (5, 6): UP, (1, 6): RIGHT, (2, 6): DOWN}.items():
        q[w * 16 + s, a] = 1.0
    assert O.greedy_walk(grid, plane, 5, q) == O.CLAIM_WALK


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_restated_q_learners_all_walk_a_shortest_solution(seed):
    """64 learners, alpha 0.5, gamma 0.95, epsilon 0.1, tables of 16 << 4 = 256 rows.  Measured with BoxesOracle.td_run: all 64 greedy
    walks are shortest solutions (4 moves, return 7) from 3100 steps on for seed 0, from 2400 for seed 1 and from 2800 for seed 2 (61, 61
    and 62 of 64 two hundred steps earlier), and at every multiple of 100 from there to ten times that.  The budget is twice the
    largest, O.CLAIM_STEPS = 6200 steps."""
    grid, plane = _claim()
    o = O.BoxesOracle(grid, seed, O.CLAIM_LEARNERS, plane, O.CLAIM_BOXES['on_target'], q0=0.0)
    o.reset()
    o.td_run(O.CLAIM_STEPS, O.Q_LEARNING, O.CLAIM_ALPHA, O.CLAIM_GAMMA, O.CLAIM_EPS_Q16)
    assert all(o.log[k] > 0 for k in ('push', 'refused_wall', 'refused_terminal', 'onto_target', 'solved', 'reset_restored')), o.log
    walks = [O.greedy_walk(grid, plane, 5, o.q[e]) for e in range(O.CLAIM_LEARNERS)]
    assert walks == [O.CLAIM_WALK] * O.CLAIM_LEARNERS, walks
