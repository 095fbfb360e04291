"""Greedy evaluation (include/gu.h: gu_td_evaluate) without a device: the restatement tests/_eval_oracle.py on walks written out by
hand, the facade's argument checks against an engine double, algorithms.evaluation's helpers, and the conditions that keep the device
cases of tests/test_gpu_eval.py from being vacuous, shown on the restatement alone."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms import evaluation
from griduniverse_amd.grid import GridSpec, box_plane, door_plane, fruit_plane

from . import _boxes_oracle as BO
from . import _doors_oracle as DO
from . import _errands_oracle as ER
from . import _eval_cases as EC
from . import _eval_oracle as EO
from . import _fruit_oracle as FO
from ._fake_engine import PRESENT, Scripted

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3
W = H = 4
S = W * H
OPEN = dict(W=W, H=H, starts=[0], goals=[15], lava=[], walls=[])


def _calm(q, L, first=None, g=OPEN, gamma=1.0, K=1):
    out = EO.evaluate_calm(BO.grid_of(g), 0, 1, 0, np.asarray(q, np.float64)[None], K, L, gamma, None if first is None else [[first]] * K)
    return {k: v[:, 0] for k, v in out.items()}


def _best(rows, pairs):
    """A table of `rows` rows of zeros in which action a is the one maximum of row r for every (r, a) of `pairs`."""
    q = np.zeros((rows, 4))
    for r, a in pairs:
        q[r, a] = 1.0
    return q


def _one(got, **want):
    for k, v in want.items():
        assert got[k][0] == v, (k, got[k][0], v)


# ---- walks written out by hand ----
def test_a_tie_is_taken_at_the_lowest_action():
    q = np.zeros((S, 4))
    q[0] = [1, 5, 5, 0]
    _one(_calm(q, 1), end=1, length=1, ret=-1, outcome=0)
    q[0] = [5, 1, 5, 5]
    _one(_calm(q, 1), end=0, length=1)  # UP from the top row: a bump


def test_a_row_whose_first_entry_is_nan_takes_action_0():
    q = np.zeros((S, 4))
    q[5] = [np.nan, 1, 2, 3]
    _one(_calm(q, 1, first=5), end=1, length=1)  # UP from (1, 1)


def test_a_terminal_start_ends_at_once():
    got = _calm(np.zeros((S, 4)), 9, first=15, gamma=0.5)
    _one(got, end=15, length=0, ret=0, outcome=1, word=0)
    assert got['discounted'][0] == 0.0
    lava = dict(OPEN, lava=[5])
    _one(_calm(np.zeros((S, 4)), 9, first=5, g=lava), length=0, outcome=2)


def test_a_loop_runs_to_L_and_sums_in_the_rules_order():
    got = _calm(np.zeros((S, 4)), 7, gamma=0.9)  # UP from cell 0 for ever
    _one(got, end=0, length=7, ret=-7, outcome=0)
    disc, w = 0.0, 1.0
    for _ in range(7):
        disc, w = disc + w * -1.0, w * 0.9
    assert got['discounted'][0] == disc


def test_lava_is_outcome_2_and_a_goal_outcome_1():
    g = dict(OPEN, lava=[1], goals=[4])
    _one(_calm(_best(S, [(0, RIGHT)]), 5, g=g), end=1, length=1, ret=-10, outcome=2)
    _one(_calm(_best(S, [(0, DOWN)]), 5, g=g), end=4, length=1, ret=10, outcome=1)


def test_every_test_episode_of_one_start_without_gusts_is_the_same_walk():
    got = _calm(_best(S, [(0, RIGHT), (1, DOWN)]), 4, K=3)
    for k in EO.KEYS:
        assert (got[k] == got[k][0]).all()


def test_a_fruit_eaten_on_a_bump_changes_the_row():
    plane = fruit_plane(W, H, [2], ['apple'])
    o = FO.FruitOracle(BO.grid_of(OPEN), 0, 1, plane, (7, 0, 0), q0=None)
    q = _best(S << 1, [(2, UP), (S + 2, RIGHT)])  # on the fruit, uneaten: UP, a bump that eats it; eaten: RIGHT
    log = EO.new_log()
    got = EO.evaluate_with(o, 'fruit', q[None], 1, 2, first_state=[[2]], log=log)
    _one({k: v[:, 0] for k, v in got.items()}, end=3, length=2, ret=(-1 + 7) - 1, word=1, outcome=0)
    assert log['bumps_that_changed_row'] == 1


def test_a_shut_door_refuses_and_its_key_opens_it():
    plane = door_plane(W, H, {0: 1}, keys={0: 4})
    grid = BO.grid_of(OPEN)
    shut = EO.evaluate_with(DO.DoorsOracle(grid, 0, 1, plane, q0=None), 'doors', _best(S << 1, [(0, RIGHT)])[None], 1, 3)
    _one({k: v[:, 0] for k, v in shut.items()}, end=0, length=3, ret=-3, word=0, outcome=0)
    q = _best(S << 1, [(0, DOWN), (S + 4, UP), (S + 0, RIGHT)])
    through = EO.evaluate_with(DO.DoorsOracle(grid, 0, 1, plane, q0=None), 'doors', q[None], 1, 3)
    _one({k: v[:, 0] for k, v in through.items()}, end=1, length=3, word=1, outcome=0)


def test_a_solved_box_level_is_outcome_3():
    g = dict(OPEN, starts=[4])
    plane = box_plane(W, H, [5], [6])
    o = BO.BoxesOracle(BO.grid_of(g), 0, 1, plane, 5, q0=None)
    q = _best(S << 4, [(5 * S + 4, RIGHT)])  # the word of a box on cell 5 is 5
    got = EO.evaluate_with(o, 'boxes', q[None], 1, 9)
    _one({k: v[:, 0] for k, v in got.items()}, end=5, length=1, ret=BO.SOLVED_REWARD, word=6, outcome=3)


def test_a_completed_errand_is_outcome_3_and_leaves_its_absorbing_word():
    g = dict(OPEN, starts=[4])
    plane = ER.plane_of(S, [5], ['apple'])
    o = ER.ErrandsOracle(BO.grid_of(g), 0, 1, plane, [['apple']], (5, -8, 10), q0=None)
    assert (o.F, o.pb, o.ib) == (1, 1, 0)
    q = _best(S << 2, [(4, RIGHT)])
    got = EO.evaluate_with(o, 'errands', q[None], 1, 9)
    _one({k: v[:, 0] for k, v in got.items()}, end=5, length=1, ret=10, outcome=3, word=1 | (1 << 1))  # eaten, and p = the list's length
    assert o.log['completed'] == 1 and (o.p == o.length[o.j]).all()  # the word every further move would be absorbed by


# ---- the facade ----
class _Double(Scripted):
    td_rows = 48

    def td_evaluate(self, K, L, gamma, first):
        self.calls.append(('td_evaluate', (K, L, gamma, first)))
        return dict(ret=0, len=1, outcome=2, end=3, word=4, disc=5)


def _vec(n=4):
    vec = gua.VecGridUniverse(n, template=GridSpec(4, 4, [0], [15], [], []), engine_factory=_Double)
    vec.engine.held = dict(PRESENT)
    return vec


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    vec = _vec()
    ok = np.zeros((2, 4), np.int32)
    for kw in (dict(episodes=0), dict(episodes=1.5), dict(episodes=True), dict(episodes=65536), dict(episodes=2, max_steps=0), dict(max_steps=-3),
               dict(max_steps=2.0), dict(episodes=3, max_steps=33333334), dict(discount_factor=float('nan')), dict(discount_factor=float('inf')),
               dict(episodes=2, first_state=ok[:1]), dict(episodes=2, first_state=ok + 16), dict(episodes=2, first_state=ok - 1),
               dict(episodes=2, first_state=ok.astype(float)), dict(episodes=2, first_state=ok.astype(bool))):
        with pytest.raises(ValueError):
            vec.evaluate(**kw)
    assert vec.engine.calls == []
    big = gua.VecGridUniverse(1 << 20, template=GridSpec(4, 4, [0], [15], [], []), engine_factory=_Double)
    with pytest.raises(ValueError):
        big.evaluate(episodes=17)  # 17 x 2^20 test episodes: more than 2^24
    assert big.engine.calls == []
    for bad in (np.zeros(4), np.zeros((16, 3)), np.zeros((2, 2, 16, 4)), np.zeros((0, 16, 4))):
        with pytest.raises(ValueError):
            evaluation.evaluate(None, bad)
    for kw in (dict(episodes=0), dict(gust=2.0), dict(fruit=([1], 'apple')), dict(wind=np.zeros(4, int), doors=dict(doors={0: 1}))):
        with pytest.raises(ValueError):  # (before a batch is made: there is no env to make it from)
            evaluation.evaluate(None, np.zeros((16, 4)), **kw)
    for kw in (dict(total_steps=0, every=5), dict(total_steps=5, every=0)):
        with pytest.raises(ValueError):
            evaluation.learning_curve(vec, lambda v, T: None, **kw)
    assert vec.engine.calls == []


def test_evaluate_sends_one_call_and_renames_the_results():
    vec = _vec()
    first = np.arange(8).reshape(2, 4)
    got = vec.evaluate(2, 9, 0.5, first)
    assert got == dict(ret=0, length=1, outcome=2, end=3, word=4, discounted=5)
    calls = [c for c in vec.engine.calls if c[0] != 'stores']
    assert len(calls) == 1 and calls[0][0] == 'td_evaluate' and calls[0][1][:3] == (2, 9, 0.5)
    assert calls[0][1][3].dtype == np.int32 and np.array_equal(calls[0][1][3], first)


def test_max_steps_defaults_to_the_rows_of_a_table_clipped_to_the_budget():
    vec = _vec()
    vec.evaluate(3)
    assert vec.engine.calls[-1] == ('td_evaluate', (3, 48, 1.0, None))
    vec.engine.td_rows = 10 ** 8
    vec.evaluate(3)
    assert vec.engine.calls[-1] == ('td_evaluate', (3, 33333333, 1.0, None))


def test_evaluate_gives_every_env_a_table_first_when_the_library_holds_none():
    vec = _vec()
    vec.engine.held['td_rows'] = 0
    vec.evaluate()
    assert [c[0] for c in vec.engine.calls if c[0] != 'stores'] == ['td_init', 'td_evaluate']


def test_success_counts_goals_and_overlay_endings():
    r = dict(outcome=np.array([[0, 1, 3, 2], [1, 1, 0, 2]]))
    assert evaluation.success(r).tolist() == [0.5, 1.0, 0.5, 0.0]


def test_learning_curve_trains_and_measures_in_turn():
    class Vec(object):
        def __init__(self):
            self.log = []

        def evaluate(self, **kw):
            self.log.append(('evaluate', kw))
            n = len(self.log)
            return {k: np.full((2, 3), n, EO.DTYPES[k]) for k in EO.KEYS}

    vec = Vec()
    got = evaluation.learning_curve(vec, lambda v, T: v.log.append(('launch', T)), 25, 10, episodes=2, max_steps=7)
    kw = dict(episodes=2, max_steps=7)
    assert vec.log == [('launch', 10), ('evaluate', kw), ('launch', 10), ('evaluate', kw), ('launch', 5), ('evaluate', kw)]
    assert got['steps'].tolist() == [10, 20, 25] and got['outcome'].shape == (3, 2, 3) and got['length'][:, 0, 0].tolist() == [2, 4, 6]


# ---- the device cases compare something ----
@pytest.mark.parametrize('env_id0', EC.IDS)
@pytest.mark.parametrize('kind,grid', EC.CASES)
def test_the_device_cases_are_not_vacuous(kind, grid, env_id0):
    log = EO.new_log()
    lengths = EC.restate(kind, grid, env_id0, None, log)['length']
    first = EC.first_states(kind, grid)
    if first is not None:
        lengths = np.concatenate([lengths, EC.restate(kind, grid, env_id0, first, log)['length']])
    EC.not_vacuous(kind, grid, log)
    assert (lengths == EC.L).any() and ((lengths > 0) & (lengths < EC.L)).any()  # some walks loop, others end
    assert first is None or (lengths == 0).any()  # ... and some of the given cells are terminal


def test_the_learning_claims_step_count_is_twice_the_largest_measured():
    assert sorted(EO.CLAIM_MEASURED) == [0, 1, 2] and EO.CLAIM_STEPS == 2 * max(EO.CLAIM_MEASURED.values())
