"""Errands, the parts that need no GPU: the restatement (tests/_errands_oracle.py) against hand-written walks, the instructions in
words, the packing and the word's fields, the argument checks of the facade, the conditions that keep the device cases from being
vacuous, the library's symbols and the learning claim on the 5 x 3 grid."""
import re
import subprocess

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib, rng
from griduniverse_amd.grid import errand_bytes, errand_fields, errand_words, fruit_plane, instruction_text, pack_errands, parse_instruction
from oracle import gu_rng as R

from . import _errands_oracle as O
from . import _overlay_starts as S
from ._tabular_cases import GRIDS, _grid, _spec

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3

# the walks' grid: 5 x 3, start (0, 1) = cell 5, goal (4, 1) = cell 9; apple 2, lemon 12, melon 7, a second apple on 6, a lemon on the start
W5 = dict(W=5, H=3, starts=[5], goals=[9], lava=[], walls=[])
CELLS, KINDS = [2, 12, 7, 6, 5], ['apple', 'lemon', 'melon', 'apple', 'lemon']  # slots by ascending cell: 2 -> 0, 5 -> 1, 6 -> 2, 7 -> 3, 12 -> 4
PAY = (5, -8, 10)


def _one(instructions, j=0, pay=PAY, grid=W5, cells=CELLS, kinds=KINDS):
    """One env on the walks' grid, reset, under instruction j."""
    o = O.ErrandsOracle(_grid(grid), 0, 1, O.plane_of(grid['W'] * grid['H'], cells, kinds), instructions, pay, q0=None)
    o.reset()
    o.set_words([j << (o.F + o.pb)])
    return o


def _walk(o, acts):
    """[(cell, reward, done, eaten, p)] of the moves."""
    out = []
    for a in acts:
        s, r, d = o._move(np.array([a], np.int32))
        out.append((int(s[0]), int(r[0]), int(d[0]), int(o.eaten[0]), int(o.p[0])))
    return out


# ---- the restatement against hand-written walks ----
def test_the_plane_is_fruit_planes():
    assert np.array_equal(O.plane_of(15, CELLS, KINDS), fruit_plane(5, 3, CELLS, KINDS))


def test_right_order_pays_right_then_finish_and_a_reset_onto_a_fruit_eats_nothing():
    o = _one([['apple', 'melon']])
    assert int(o.state.pos[0]) == 5 and int(o.eaten[0]) == 0  # the start cell holds a lemon: the reset did not eat it
    # RIGHT to 6 (apple: right, -1 + 5), RIGHT to 7 (melon: completes, finish alone, done)
    assert _walk(o, [RIGHT, RIGHT]) == [(6, 4, 0, 0b00100, 1), (7, 10, 1, 0b01100, 2)]
    assert o.log == dict(right=2, wrong=0, completed=1, absorbed=0, drawn={0})


def test_wrong_order_pays_wrong_keeps_p_and_the_fruit_is_gone():
    o = _one([['melon', 'apple']])
    # 6 is an apple, wanted is the melon: wrong; 7 melon: right; back LEFT onto 6: eaten already, nothing; UP to 1, RIGHT to 2: apple, completes
    assert _walk(o, [RIGHT, RIGHT, LEFT, UP, RIGHT]) == [(6, -9, 0, 0b00100, 0), (7, 4, 0, 0b01100, 1), (6, -1, 0, 0b01100, 1), (1, -1, 0, 0b01100, 1),
                                                         (2, 10, 1, 0b01101, 2)]
    assert o.log['wrong'] == 1 and o.log['completed'] == 1


def test_an_impossible_instruction_ends_at_the_goal_only():
    o = _one([['melon']], cells=[2, 7], kinds=['apple', 'melon'], grid=W5)
    o2 = _one([['apple', 'melon']], cells=[2, 7], kinds=['apple', 'melon'])
    # the melon first: wrong, and now [apple, melon] cannot be carried out; the goal ends the episode with its own reward
    assert _walk(o2, [RIGHT, RIGHT, RIGHT, RIGHT]) == [(6, -1, 0, 0, 0), (7, -9, 0, 0b10, 0), (8, -1, 0, 0b10, 0), (9, 10, 1, 0b10, 0)]
    assert o2.log['completed'] == 0
    assert _walk(o, [RIGHT, RIGHT]) == [(6, -1, 0, 0, 0), (7, 10, 1, 0b10, 1)]  # (finish equals the goal's 10 here; done comes from the word)


def test_a_kind_named_twice_takes_two_fruit_of_it():
    o = _one([['apple', 'apple']])
    got = _walk(o, [RIGHT, UP, RIGHT])  # 6 apple (right), 1, 2 apple (completes)
    assert got == [(6, 4, 0, 0b00100, 1), (1, -1, 0, 0b00100, 1), (2, 10, 1, 0b00101, 2)]


def test_a_list_of_four_has_no_end_mark_and_completes_at_p_4():
    o = _one([['apple', 'melon', 'lemon', 'apple']], pay=(3, -2, 7))
    assert o.pb == 3 and pack_errands([['apple', 'melon', 'lemon', 'apple']]) == 1 | (3 << 2) | (2 << 4) | (1 << 6)
    got = _walk(o, [RIGHT, RIGHT, DOWN, UP, UP])  # 6 apple, 7 melon, 12 lemon, 7, 2 apple
    assert got == [(6, 2, 0, 0b00100, 1), (7, 2, 0, 0b01100, 2), (12, 2, 0, 0b11100, 3), (7, -1, 0, 0b11100, 3), (2, 7, 1, 0b11101, 4)]
    assert int(o.words[0]) == 0b11101 | (4 << 5)


def test_a_completed_word_is_absorbing():
    o = _one([['apple']])
    assert _walk(o, [RIGHT]) == [(6, 10, 1, 0b00100, 1)]
    # nothing moves, whatever the action, and nothing is eaten: finish and done every step
    assert _walk(o, [RIGHT, UP, LEFT]) == [(6, 10, 1, 0b00100, 1)] * 3
    assert o.log['absorbed'] == 3 and int(o.state.tcount[0]) == 4
    # absorbing is a property of the word: set on a fresh env that stands on an uneaten fruit, it still eats nothing
    o = _one([['apple']])
    o.set_words([1 << o.F])
    assert _walk(o, [LEFT]) == [(5, 10, 1, 0, 1)]


def test_a_wall_bump_onto_a_fruit_eats_it():
    o = _one([['lemon', 'apple']])
    # LEFT from the start cell bumps the border: the agent stays on cell 5, whose lemon the reset did not eat
    assert _walk(o, [LEFT, LEFT]) == [(5, 4, 0, 0b00010, 1), (5, -1, 0, 0b00010, 1)]


def test_the_draw_is_stream_11_at_the_count_before_the_reset_for_reset_and_lazy_reset():
    grid, n, seed, id0 = _grid(W5), 40, 3, 2 ** 31 - 7
    ins = [['apple'], ['lemon'], ['melon']]
    o = O.ErrandsOracle(grid, seed, n, O.plane_of(15, CELLS, KINDS), ins, PAY, env_id0=id0, q0=None)
    ids = np.arange(id0, id0 + n, dtype=np.uint64)
    want = lambda ep: ((R.word_v(seed, ids, 11, ep).astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)  # noqa: E731
    assert np.array_equal(rng.errand_words(seed, ids, 0), R.word_v(seed, ids, 11, 0))
    o.reset()
    assert (o.state.episode == 1).all() and np.array_equal(o.j, want(0))
    o.reset()
    assert np.array_equal(o.j, want(1))
    o.rollout(40, 'uniform', auto_reset=True)
    assert (o.state.episode > 2).any()
    # every env's instruction is the one of its last reset: episode - 1
    assert np.array_equal(o.j, want(o.state.episode.astype(np.uint64) - np.uint64(1)))
    assert o.log['drawn'] == {0, 1, 2}
    before = o.j.copy()
    mask = (np.arange(n) % 2).astype(np.uint8)
    ep = o.state.episode.astype(np.uint64).copy()
    o.reset(mask)
    assert np.array_equal(o.j[mask == 0], before[mask == 0]) and np.array_equal(o.j[mask != 0], want(ep)[mask != 0])
    one = O.ErrandsOracle(grid, seed, n, O.plane_of(15, CELLS, KINDS), [['apple']], PAY, q0=None)
    one.reset()
    assert not one.j.any() and one._bits() == 5 + 1 + 0


def test_a_rejected_action_moves_eats_and_draws_nothing():
    o = _one([['lemon'], ['apple']])
    o.state.done[:] = 1
    w, ep = o.words.copy(), o.state.episode.copy()
    obs, rew, don, rej = o.step(np.array([4]), auto_reset=True)
    assert rej.all() and np.array_equal(o.words, w) and np.array_equal(o.state.episode, ep) and int(o.state.tcount[0]) == 0


# ---- the instructions in words ----
def test_parse_instruction_and_its_inverse():
    assert parse_instruction('Collect the lemon and then the apple') == ['lemon', 'apple']
    assert parse_instruction('First get a MELON, then eat an apple; finally pick up the melon.') == ['melon', 'apple', 'melon']
    assert parse_instruction('apple') == ['apple'] and parse_instruction('take the') == []
    for bad in ('collect the apple after the lemon', 'the lemon before the apple', 'collect the pear', 'apples', 'lemon two', 'collect thelemon', 7, None, ['apple']):
        with pytest.raises(ValueError):
            parse_instruction(bad)
    assert parse_instruction('lemon 2 apple') == ['lemon', 'apple']  # (digits split words, they are no words)
    for kinds in (['lemon', 'apple'], ['apple'], ['melon', 'melon', 'apple', 'lemon']):
        assert parse_instruction(instruction_text(kinds)) == kinds
    assert instruction_text(['lemon', 'apple']) == 'collect the lemon and then the apple'
    for text in O.CLAIM_TEXTS:
        assert instruction_text(parse_instruction(text)) == text
    assert [parse_instruction(t) for t in O.CLAIM_TEXTS] == O.CLAIM_INSTRUCTIONS
    for bad in ([], ['pear'], ['apple'] * 5):
        with pytest.raises(ValueError):
            instruction_text(bad)


# ---- packing and fields ----
def test_packing_and_fields():
    ins = [['lemon', 'apple'], 'collect the apple, then the apple, then the melon and then the lemon', ['melon']]
    assert errand_bytes(ins).tolist() == [2 | (1 << 2), 1 | (1 << 2) | (3 << 4) | (2 << 6), 3, 0]
    assert pack_errands(ins) == 0x06 | (0xB5 << 8) | (0x03 << 16)
    assert pack_errands([[1, 2]]) == pack_errands([['apple', 'lemon']]) == 0x09
    for bad in ([], [['apple']] * 5, [[]], [['apple'] * 5], [['pear']], [[0]], [[4]], [[True]], 'apple', [['apple'], 'the lemon before the apple']):
        with pytest.raises(ValueError):
            pack_errands(bad)
    F = 5  # pb = bit_length(4) = 3, ib = bit_length(2) = 2
    words = np.array([0, 0b10011 | (2 << 5) | (1 << 8), 0b11111 | (4 << 5) | (1 << 8), 1 << 9], np.uint32)
    e, p, j = errand_fields(words, F, ins)
    assert e.tolist() == [0, 0b10011, 0b11111, 0] and p.tolist() == [0, 2, 4, 0] and j.tolist() == [0, 1, 1, 2]
    assert np.array_equal(errand_words(e, p, j, F, ins), words)
    e, p, j = errand_fields([0b1 | (1 << 1)], 1, [['apple']])  # one instruction: no index bits
    assert (e.tolist(), p.tolist(), j.tolist()) == ([1], [1], [0])
    # the restatement keeps the same layout
    o = O.ErrandsOracle(_grid(W5), 0, 4, O.plane_of(15, CELLS, KINDS), [parse_instruction(i) if isinstance(i, str) else i for i in ins], PAY, q0=None)
    o.set_words(words)
    assert np.array_equal(o.words, words) and (o.F, o.pb, o.ib, o._bits()) == (5, 3, 2, 10)
    e, p, j = errand_fields(words, F, ins)
    assert e.dtype == np.uint32 and np.array_equal(o.eaten, e) and np.array_equal(o.p, p) and np.array_equal(o.j, j)


# ---- the facade's checks ----
class _NoEngine(object):
    """Stands in for Engine: any call on it is a library call that must not have been made."""

    def __init__(self, *a, **kw):
        self.calls, self.args, self.got = [], [], None

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            self.args.append(a)
        return call

    def get_errands(self):
        return self.got


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    g = GRIDS['maze11']()
    vec = gua.VecGridUniverse(4, template=_spec(g), engine_factory=_NoEngine)
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    free = [s for s in range(121) if s not in taken]
    ok = dict(cells=free[:3], kinds=['apple', 'lemon', 'apple'], instructions=['collect the lemon and then the apple'])
    one = dict(kinds='apple', instructions=[['apple']])
    for kw in (dict(one, cells=[g['walls'][0]]), dict(one, cells=[g['goals'][0]]), dict(one, cells=[free[0], free[0]]), dict(one, cells=[]), dict(one, cells=free[:9]),
               dict(one, cells=[121]), dict(kinds='pear'), dict(instructions=None), dict(instructions=[]), dict(instructions=['apple'] * 5),
               dict(instructions=['collect the apple after the lemon']), dict(instructions=[['apple'] * 5]), dict(instructions=[[]]),
               dict(instructions=['the melon']),  # no melon in the plane
               dict(instructions=[['lemon', 'lemon']]),  # one lemon only
               dict(instructions=[['apple', 'apple', 'apple']]), dict(right=17), dict(right=-1), dict(wrong=1), dict(wrong=-17), dict(finish=17), dict(finish=-1),
               dict(right=1.5), dict(finish=True)):
        with pytest.raises(ValueError):
            vec.set_errands(**dict(ok, **kw))
    assert vec.engine.calls == []
    with pytest.raises(ValueError):
        vec.errand_state()  # none set
    with pytest.raises(ValueError):
        vec.set_errand_state(0, 0, 0)
    vec.set_errands(**ok)
    vec.set_errands(free[:3], ['apple', 'lemon', 'apple'], [['apple', 'apple'], 'lemon'], right=0, wrong=0, finish=0)
    assert vec.engine.calls == ['set_errands'] * 2
    plane, instr, n, pay = vec.engine.args[1]
    assert np.array_equal(plane, fruit_plane(11, 11, free[:3], ['apple', 'lemon', 'apple'])) and instr.tolist() == [5, 2, 0, 0] and n == 2 and pay.tolist() == [0, 0, 0]
    vec.engine.got = (plane, instr, n, pay, 3)  # what the library would hand back
    got = vec.errands()
    assert got.pop('cells').tolist() == free[:3]
    assert got == dict(kinds=['apple', 'lemon', 'apple'], instructions=[['apple', 'apple'], ['lemon']], right=0, wrong=0, finish=0)
    for bad in (dict(eaten=8), dict(eaten=-1), dict(instruction=2), dict(progress=3), dict(progress=2, instruction=1), dict(eaten=0.5), dict(eaten=[[1]]),
                dict(eaten=[1, 2], progress=[0, 0, 0])):
        with pytest.raises(ValueError):
            vec.set_errand_state(**bad)
    assert vec.engine.calls == ['set_errands'] * 2
    vec.set_errand_state(eaten=[7, 0], progress=[2, 1], instruction=[0, 1], env0=1)  # F = 3, pb = 2, ib = 1
    assert vec.engine.calls[-1] == 'set_errands_state' and vec.engine.args[-1][0].tolist() == [7 | (2 << 3), (1 << 3) | (1 << 5)] and vec.engine.args[-1][1] == 1
    vec.set_errands(None)
    assert vec.engine.calls[-1] == 'set_errands' and vec.engine.args[-1] == (None,)
    from griduniverse_amd.algorithms.temporal_difference import q_learning, sarsa
    e = dict(cells=free[:1], instructions=['apple'])
    for learn in (q_learning, sarsa):
        for other in (dict(wind=np.zeros(11, int)), dict(fruit=(free[:1], 'apple', (1, 5, -5))), dict(doors=dict(doors={0: free[0]}, keys={0: free[1]})),
                      dict(boxes=dict(boxes=[free[2]], targets=[free[3]]))):
            with pytest.raises(ValueError):  # the new keyword excludes the other four
                learn(None, 10, errands=e, **other)
        for bad in ((free[:1], 'apple'), dict(cells=free[:1]), dict(e, values=(1, 2, 3))):
            with pytest.raises(ValueError):
                learn(None, 10, errands=bad)


def test_library_exports_the_errands_entry_points_and_kernels():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_set_errands', 'gu_get_errands', 'gu_get_errands_state', 'gu_set_errands_state'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    blob = open(_lib.LIB_PATH, 'rb').read()
    for frame in (b'gu_overlay_step_kernel', b'gu_overlay_rollout_kernel'):  # the frame's name and the kind's rule type in ONE mangled symbol
        assert re.search(frame + rb'I\d+ErrandRule', blob), frame
    assert b'gu_errands_reset_kernel' in blob
    assert gua.Engine.ROLLOUT_FAMILIES[8] == 'errands'


# ---- the device cases are not vacuous (tests/test_gpu_errands.py compares against exactly these runs) ----
@pytest.mark.parametrize('policy', S.POLICIES)
@pytest.mark.parametrize('name', ['starts8', 'open150'])
def test_the_device_cases_complete_eat_wrongly_draw_every_index_and_absorb(name, policy):
    g, grid = S.grid_dict(name), S.c_grid(name)
    plane = O.case_plane(g)
    assert np.count_nonzero(plane) == 5 and sorted(((plane[plane != 0] >> 5) & 3).tolist()) == [1, 1, 2, 2, 3]
    if name == 'starts8':
        assert np.flatnonzero(plane).tolist() == [18, 20, 35, 45, 50]
    ins = O.instructions_for(policy)
    assert len(ins) == 3 and sorted(len(i) for i in ins) == [1, 2, 4] and any(len(set(i)) < len(i) for i in ins)
    for auto in (True, False):
        o = O.ErrandsOracle(grid, S.SEED, S.N, plane, ins, O.CASE_PAY, env_id0=S.IDS[1], q0=None)
        assert (o.F, o.pb, o.ib) == (5, 3, 2)
        o.reset()
        pos = O.case_placement(g, plane, S.N)
        if pos is not None:
            o.state.pos[:] = pos
        o.rollout(S.T, policy, auto, actions=S.stream_actions() if policy == 'stream' else None, pi=O.case_policy(g))
        assert o.log['completed'] >= 1 and o.log['wrong'] >= 1 and o.log['drawn'] == {0, 1, 2}, o.log
        if auto:
            S.drew_every_start(o)
        else:
            assert o.log['absorbed'] >= 1


# ---- the learning claim ----
def test_the_claims_shortest_walk_has_five_moves_and_returns_17():
    """Breadth-first over (cell, eaten, p) under each instruction: the fewest moves that complete it, and the best return among them."""
    grid, plane = _grid(O.CLAIM), O.plane_of(15, O.CLAIM_CELLS, O.CLAIM_KINDS)
    for j in (0, 1):
        best = {}
        frontier = [((), 0)]
        for depth in range(1, 7):
            nxt = []
            for acts, _ in frontier:
                for a in range(4):
                    o = O.ErrandsOracle(grid, 0, 1, plane, O.CLAIM_INSTRUCTIONS, O.CLAIM_PAY, q0=None)
                    o.reset()
                    o.set_words([j << (o.F + o.pb)])
                    got = _walk(o, list(acts) + [a])
                    if got[-1][2]:
                        if o.log['completed']:
                            best.setdefault(depth, []).append(sum(r for _, r, _, _, _ in got))
                    else:
                        nxt.append((acts + (a,), 0))
            frontier = nxt
            if best:
                break
        assert min(best) == O.CLAIM_SHORTEST == 5 and max(best[5]) == O.CLAIM_RETURN == 17, (j, best)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_restated_q_learners_all_complete_each_instruction(seed):
    """K = CLAIM_STEPS = 6000 is twice what the restatement needed (3000, 3000, 1500 for the seeds 0, 1, 2: _errands_oracle.py).  Every
    learner reaches the SHORTEST walk (5 moves, return 17) only after up to 15000 steps: recorded there, not asserted."""
    grid, plane = _grid(O.CLAIM), O.plane_of(15, O.CLAIM_CELLS, O.CLAIM_KINDS)
    assert O.CLAIM_STEPS == 2 * max(O.CLAIM_MEASURED.values()) == 6000
    o = O.ErrandsOracle(grid, seed, O.CLAIM_LEARNERS, plane, O.CLAIM_INSTRUCTIONS, O.CLAIM_PAY, q0=0.0)
    o.reset()
    o.td_run(O.CLAIM_STEPS, O.Q_LEARNING, O.CLAIM_ALPHA, O.CLAIM_GAMMA, O.CLAIM_EPS_Q16)
    assert o.q.shape == (O.CLAIM_LEARNERS, 15 << 5, 4) and o.log['drawn'] == {0, 1}
    for j in (0, 1):
        walks = [O.greedy_walk(grid, plane, o.q[e], j) for e in range(O.CLAIM_LEARNERS)]
        assert all(w[0] for w in walks), (j, walks)
