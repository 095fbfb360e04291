"""Doors, keys and levers, the parts that need no GPU: the door plane, the argument checks, the library's symbols, the CPU restatement
against the calm C oracle in two identities that do not rest on the new code, rule 5 on hand-written walks, and the learning claim on
the 7 x 3 grid."""
import re
import subprocess

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.grid import DOOR_KINDS, DOOR_SLOTS_MAX, door_plane
from oracle import c_oracle as C

from . import _doors_oracle as O
from ._tabular_cases import GRIDS, _grid, _spec

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


def test_door_plane_shapes_slot_order_and_errors():
    assert DOOR_KINDS == {'door': 1, 'key': 2, 'lever': 3} and DOOR_SLOTS_MAX == 8
    p = door_plane(5, 3, {0: 7, 1: [11, 3]}, keys={0: 2}, levers={1: [14]})
    assert p.dtype == np.uint8 and p.shape == (15,)
    want = np.zeros(15, np.uint8)
    want[7], want[11], want[3], want[2], want[14] = 0 | 16, 1 | 16, 1 | 16, 0 | 32, 1 | 48
    assert np.array_equal(p, want)
    assert np.array_equal(door_plane(5, 3, {0: np.array([1, 2])}, None, {0: np.int64(9)}), door_plane(5, 3, {0: [2, 1]}, levers={0: 9}))
    full = door_plane(8, 8, {k: k for k in range(8)}, keys={k: 8 + k for k in range(8)})  # eight slots: slot 7 is in range
    assert np.array_equal(full[:16], np.concatenate([np.arange(8) | 16, np.arange(8) | 32]).astype(np.uint8)) and not full[16:].any()
    for bad in (dict(doors={8: 1}, keys={8: 2}), dict(doors={-1: 1}, keys={-1: 2}), dict(doors={True: 1}, keys={True: 2}),  # a slot outside 0 .. 7
                dict(doors={0: 1, 2: 3}, keys={0: 4, 2: 5}), dict(doors={1: 1}, keys={1: 2}),  # a gap in the slots
                dict(doors={0: 1}), dict(doors={0: 1, 1: 2}, keys={0: 3}), dict(doors={0: 1}, keys={0: 2, 1: 3}), dict(doors={}, keys={}),  # no door / no opener
                dict(doors={0: 1}, keys={0: 1}), dict(doors={0: [1, 1]}, keys={0: 2}), dict(doors={0: 1}, keys={0: 2}, levers={0: 2}),  # a cell twice
                dict(doors={0: 64}, keys={0: 2}), dict(doors={0: 1}, keys={0: -1}), dict(doors={0: 1}, levers={0: [3, 99]}),  # outside the grid
                dict(doors={0: 1.5}, keys={0: 2}), dict(doors={0: []}, keys={0: 2}), dict(doors=[1], keys={0: 2}), dict(doors={0: [[1]]}, keys={0: 2})):
        with pytest.raises(ValueError):
            door_plane(8, 8, **bad)


class _NoEngine(object):
    """Stands in for Engine: any call on it is a library call that must not have been made."""

    def __init__(self, *a, **kw):
        self.calls, self.args, self.held = [], [], {}

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            self.args.append(a)
        return call

    def stores(self):
        """What the library would report (Engine.stores): the test sets `held`.  A query, so it is not recorded."""
        return self.held


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    free = O.free_cells(g)
    for kw in (dict(doors={0: g['walls'][0]}, keys={0: free[0]}), dict(doors={0: free[0]}, keys={0: g['goals'][0]}),
               dict(doors={0: free[0]}, levers={0: g['walls'][1]}), dict(doors={0: free[0]}), dict(doors={0: free[0]}, keys={0: free[0]}),
               dict(doors={1: free[0]}, keys={1: free[1]}), dict(doors={0: 121}, keys={0: free[1]}), dict(doors=None, keys={0: free[1]})):
        with pytest.raises(ValueError):
            vec.set_doors(**kw)
    assert vec.engine.calls == []
    vec.set_doors({0: free[0], 1: free[1]}, keys={0: free[2]}, levers={1: free[3]})
    vec.engine.held = dict(overlay=3, overlay_bits=2)
    for bad in ([4], [-1], [0.5], [[1]], [True]):  # two slots: bits 0 and 1
        with pytest.raises(ValueError):
            vec.set_doors_open(bad)
    assert vec.engine.calls == ['set_doors']
    vec.set_doors_open([3, 0], env0=1)
    vec.set_doors(None)
    assert vec.engine.calls == ['set_doors', 'set_doors_state', 'set_doors']
    from griduniverse_amd.algorithms.temporal_difference import q_learning, sarsa
    doors = dict(doors={0: free[0]}, keys={0: free[1]})
    for learn in (q_learning, sarsa):
        with pytest.raises(ValueError):  # doors exclude wind ...
            learn(None, 10, wind=np.zeros(11, int), doors=doors)
        with pytest.raises(ValueError):  # ... and fruit
            learn(None, 10, fruit=(free[:1], 'apple', (1, 5, -5)), doors=doors)
        for bad in (({0: free[0]}, {0: free[1]}), dict(keys={0: free[1]}), dict(doors, door={})):
            with pytest.raises(ValueError):
                learn(None, 10, doors=bad)


def test_the_facade_asks_the_library_for_the_tables_after_set_doors():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    free = O.free_cells(g)
    # The facade keeps no flag of its own: after set_doors it asks the library, which drops tables of another row count
    # (tests/test_gpu_stores.py checks that half) and says so in stores().
    def inits():
        return [(c, a) for c, a in zip(vec.engine.calls, vec.engine.args) if c != 'set_doors']

    vec.set_doors({0: free[0], 1: free[1]}, keys={0: free[2], 1: free[3]})
    vec.engine.held = dict(td_rows=0)  # another row count: the tables went
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))]
    vec.set_doors({0: [free[5], free[6]], 1: free[7]}, levers={0: free[8], 1: free[9]})  # two slots again: the rows stay, and so do the tables
    vec.engine.held = dict(td_rows=121 << 2)
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))]
    vec.set_doors({0: free[5]}, keys={0: free[6]})
    vec.engine.held = dict(td_rows=0)
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))] * 2
    vec.set_doors(None)
    vec._ensure_q()
    assert inits() == [('td_init', (0.0,))] * 3
    assert vec.engine.calls == ['set_doors', 'td_init', 'set_doors', 'set_doors', 'td_init', 'set_doors', 'td_init']


def test_library_exports_the_door_entry_points_and_kernels():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_set_doors', 'gu_get_doors', 'gu_get_doors_state', 'gu_set_doors_state'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    blob = open(_lib.LIB_PATH, 'rb').read()
    for frame in (b'gu_overlay_step_kernel', b'gu_overlay_rollout_kernel'):  # the frame's name and the kind's rule type in ONE mangled symbol
        assert re.search(frame + rb'I\d+DoorRule', blob), frame
    assert b'gu_overlay_reset_kernel' in blob
    assert gua.Engine.ROLLOUT_FAMILIES[6] == 'doors'


def _equal_c_oracle(o, grid, seed, N, T, auto):
    st = C.State(N)
    assert np.array_equal(o.reset(), C.reset(grid, seed, st))
    return o.rollout(T, 'uniform', auto_reset=auto), C.rollout(grid, seed, st, T, auto, stats=True), st


def _same_run(got, want, o, st):
    for k in ('obs', 'reward', 'done', 'ret', 'episodes'):
        assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), k
    assert np.array_equal(o.state.pos, st.pos) and np.array_equal(o.state.done, st.done)
    assert np.array_equal(o.state.episode, st.episode) and np.array_equal(o.state.tcount, st.tcount)


@pytest.mark.parametrize('name', ['default4x4', 'maze11'])
def test_doors_that_never_open_are_walls_for_the_c_oracle(name):
    g, plane, twin = O.walled_in_case(GRIDS[name]())
    for N, seed in ((1, 2), (64, 9), (37, 5)):
        for auto in (True, False):
            o = O.DoorsOracle(_grid(g), seed, N, plane, q0=None)
            got, want, st = _equal_c_oracle(o, _grid(twin), seed, N, 150, auto)
            _same_run(got, want, o, st)
            assert not o.open.any() and o.log['key'] == o.log['passage'] == 0
            assert N == 1 or o.log['bump'] > 0


@pytest.mark.parametrize('name', ['default4x4', 'maze11'])
def test_doors_that_are_all_open_are_free_cells_for_the_c_oracle(name):
    g, plane = O.keys_only_case(GRIDS[name]())
    for N, seed in ((1, 2), (64, 9), (37, 5)):
        o = O.DoorsOracle(_grid(g), seed, N, plane, q0=None)
        st = C.State(N)
        assert np.array_equal(o.reset(), C.reset(_grid(g), seed, st))
        o.set_open(np.full(N, 3, np.uint32))  # (behind the reset, which clears the masks)
        got = o.rollout(150, 'uniform', auto_reset=False)
        want = C.rollout(_grid(g), seed, st, 150, False, stats=True)
        _same_run(got, want, o, st)
        assert (o.open == 3).all() and o.log['bump'] == 0
        assert N == 1 or o.log['passage'] > 0


# ---- rule 5 on hand-written walks: an open 4 x 4 grid, start 0, goal 15; lever of slot 0 at cell 1 with its door at 10, key of slot 1 at
# cell 4 with its door at 6 ----
_RULE5 = dict(W=4, H=4, starts=[0], goals=[15], lava=[], walls=[])
_RULE5_PLANE = dict(doors={0: 10, 1: 6}, levers={0: 1}, keys={1: 4})


def _walk(actions, g=_RULE5, plane=None):
    plane = door_plane(4, 4, **_RULE5_PLANE) if plane is None else plane
    o = O.DoorsOracle(_grid(g), 0, 1, plane, q0=None)
    o.reset()
    out = []
    for a in actions:
        obs, r, d, _ = o.step([a])
        out.append((int(obs[0]), int(o.open[0]), int(r[0]), int(d[0])))
    return out, o


def test_rule_5_a_wall_bump_on_a_lever_does_not_toggle_and_re_entering_toggles_back():
    out, o = _walk([RIGHT, UP, UP, LEFT, RIGHT])
    assert out == [(1, 1, -1, 0), (1, 1, -1, 0), (1, 1, -1, 0), (0, 1, -1, 0), (1, 0, -1, 0)]
    assert o.log['lever_open'] == 1 and o.log['lever_shut'] == 1


def test_rule_5_a_key_is_one_way_and_its_door_lets_through_afterwards():
    # cell 5 lies beside door 6: shut at first (a bump that pays -1 and keeps the cell), open behind the key at 4
    out, o = _walk([RIGHT, DOWN, RIGHT, LEFT, UP, DOWN, RIGHT, RIGHT, LEFT, LEFT, RIGHT])
    assert out[:3] == [(1, 1, -1, 0), (5, 1, -1, 0), (5, 1, -1, 0)]  # over the lever (slot 0) to cell 5, then the bump on door 6
    assert out[3:6] == [(4, 3, -1, 0), (0, 3, -1, 0), (4, 3, -1, 0)]  # the key sets bit 1, and entering it again changes nothing
    assert out[6:] == [(5, 3, -1, 0), (6, 3, -1, 0), (5, 3, -1, 0), (4, 3, -1, 0), (5, 3, -1, 0)]  # through the door, and back out of it
    assert o.log['bump'] == 1 and o.log['passage'] == 1 and o.log['key'] == 1


def test_rule_5_a_door_bump_on_a_lever_does_not_pull_it_and_standing_on_a_door_is_free():
    # lever of slot 0 at cell 5 beside its own door at 6: the bump from the lever keeps the mask; after set_state onto the door, the agent leaves
    plane = door_plane(4, 4, {0: 6}, levers={0: 5})
    out, o = _walk([RIGHT, DOWN, LEFT, RIGHT, RIGHT, RIGHT], plane=plane)
    assert out == [(1, 0, -1, 0), (5, 1, -1, 0), (4, 1, -1, 0), (5, 0, -1, 0), (5, 0, -1, 0), (5, 0, -1, 0)]
    o.state.pos[0] = 6  # standing on a closed door
    obs, r, d, _ = o.step([RIGHT])
    assert (int(obs[0]), int(o.open[0])) == (7, 0)
    obs, r, d, _ = o.step([LEFT])  # ... which refuses entry again
    assert (int(obs[0]), int(o.open[0])) == (7, 0) and o.log['bump'] == 3


def test_rule_5_a_reset_onto_a_key_cell_does_not_pick_it_up():
    g = dict(_RULE5, starts=[4])
    out, o = _walk([RIGHT], g=g)
    assert o.log['key'] == 0 and out == [(5, 0, -1, 0)]  # the start cell held the key of slot 1
    out, o = _walk([RIGHT, LEFT, 7], g=g)
    assert out[1] == (4, 2, -1, 0) and out[2] == (4, 2, -1, 0)  # entering it does; a rejected action changes nothing
    o.state.done[0] = 1
    o.step([RIGHT], auto_reset=True)  # the lazy reset puts the key back
    assert (int(o.state.pos[0]), int(o.open[0])) == (5, 0)


# ---- the learning claim ----
def _claim():
    return _grid(O.CLAIM), door_plane(O.CLAIM_W, O.CLAIM_H, **O.CLAIM_DOORS)


def test_the_claims_shortest_walk_fetches_the_key_and_without_it_the_goal_is_unreachable():
    grid, plane = _claim()
    assert O.shortest_walk(grid, plane, O.CLAIM['starts'][0]) == O.CLAIM_WALK == (8, 3)
    no_key = plane.copy()
    no_key[2] = 0
    assert O.shortest_walk(grid, no_key, O.CLAIM['starts'][0]) is None
    assert O.shortest_walk(grid, np.zeros(21, np.uint8), O.CLAIM['starts'][0]) == (6, 5)  # ... and without the door it is a straight line


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_restated_q_learners_all_walk_a_shortest_walk(seed):
    """64 learners, alpha 0.5, gamma 0.95, epsilon 0.1, tables of 21 << 1 = 42 rows.  Measured with DoorsOracle.td_run: all 64 greedy
    walks are shortest walks (8 moves, return 3) from 700 steps on for seed 0, from 700 for seed 1 and from 700 for seed 2 (51, 51 and
    55 of 64 at 600 steps), and at every multiple of 100 from there to 6000.  The budget is twice that, B = 1400 steps."""
    grid, plane = _claim()
    assert O.CLAIM_STEPS == 1400
    o = O.DoorsOracle(grid, seed, O.CLAIM_LEARNERS, plane, q0=0.0)
    o.reset()
    o.td_run(O.CLAIM_STEPS, O.Q_LEARNING, O.CLAIM_ALPHA, O.CLAIM_GAMMA, O.CLAIM_EPS_Q16)
    assert o.q.shape == (O.CLAIM_LEARNERS, 42, 4)
    walks = [O.greedy_walk(grid, plane, o.q[e]) for e in range(O.CLAIM_LEARNERS)]
    assert walks == [O.CLAIM_WALK] * O.CLAIM_LEARNERS, walks
