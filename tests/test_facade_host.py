"""The Python facade without a device: what VecGridUniverse sends to its engine, in which order, and what it and
griduniverse_amd.algorithms refuse before they send anything.

The engine is a scripted fake: `stores()` answers with a dict the test sets (as Engine.stores() would), every other call is
recorded with its positional arguments.  The tables below were written from the facade's code BEFORE it asked the library what it
holds (it kept flags of its own then); with the `stores` entries left out of the comparison they hold for that code too, which was
checked once on a checkout of it, the fake's `held` being copied into those flags.
"""
import subprocess
import sys

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms.search import uct_tables
from griduniverse_amd.envs.griduniverse_env import GridUniverseEnv
from griduniverse_amd.grid import GridSpec

from ._fake_engine import ABSENT, PRESENT, Scripted

T = 5
Q16 = {0: 0, 0.1: 6554, 1 / 3: 21845, 1: 65536}  # epsilon -> the library's 1/65536 units


def _vec(held=None):
    vec = gua.VecGridUniverse(4, template=GridSpec(4, 4, [0], [15], [], []), engine_factory=Scripted)
    vec.engine.held = dict(ABSENT if held is None else held)
    return vec


def _sent(vec):
    """The recorded calls without the queries; arrays as lists, so that == compares them."""
    return [(name, tuple(a.tolist() if isinstance(a, np.ndarray) else a for a in args)) for name, args in vec.engine.calls if name != 'stores']


UCT = ('set_tree_tables', tuple(t.tolist() for t in uct_tables()))

# name -> (the call, given the batch, epsilon and the two keywords; what it allocates on an engine that holds nothing; the engine's run
# and its arguments between T and the two flags, Q standing for epsilon in 1/65536; stores it needs to get as far as allocating)
LAUNCHES = {
    'td_run': (lambda v, e, **kw: v.td_run(T, 'sarsa', 0.2, 0.9, e, **kw), [('td_init', (0.0,))], ('td_run', ('sarsa', 0.2, 0.9, 'Q')), {}),
    'expected_sarsa_run': (lambda v, e, **kw: v.expected_sarsa_run(T, 0.2, 0.9, e, **kw), [('td_init', (0.0,))], ('esarsa_run', (0.2, 0.9, 'Q')), {}),
    'double_q_run': (lambda v, e, **kw: v.double_q_run(T, 0.2, 0.9, e, **kw), [('double_init', (0.0,))], ('double_run', (0.2, 0.9, 'Q')), {}),
    'dyna_run': (lambda v, e, **kw: v.dyna_run(T, 3, 0.2, 0.9, e, **kw), [('td_init', (0.0,)), ('dyna_init', ())], ('dyna_run', (3, 0.2, 0.9, 'Q')), {}),
    'sweep_run': (lambda v, e, **kw: v.sweep_run(T, 3, 1e-3, 0.2, 0.9, e, **kw), [('td_init', (0.0,)), ('sweep_init', ())],
                  ('sweep_run', (3, 1e-3, 0.2, 0.9, 'Q')), {}),
    'search_run': (lambda v, e, **kw: v.search_run(T, 2, 7, 0.2, 0.9, e, 0.1, **kw), [('td_init', (0.0,))], ('search_run', (2, 7, 0.2, 0.9, 'Q', 6554)), {}),
    'tree_search_run': (lambda v, e, **kw: v.tree_search_run(T, 6, 3, 2, 0.2, 0.9, e, 1 / 3, **kw), [('td_init', (0.0,)), ('mcts_init', (6,)), UCT],
                        ('mcts_run', (6, 3, 2, 0.2, 0.9, 'Q', 21845)), {}),
    'explore_run': (lambda v, e, **kw: v.explore_run(T, 'thompson', 0.2, 0.9, e, **kw), [('td_init', (0.0,)), ('explore_init', ())],
                    ('explore_run', ('thompson', 0.2, 0.9, 'Q')), dict(explore_c=16)),
    'nstep_run': (lambda v, e, **kw: v.nstep_run(T, 3, 'q_learning', 0.2, 0.9, e, **kw), [('td_init', (0.0,))], ('nstep_run', ('q_learning', 3, 0.2, 0.9, 'Q')), {}),
    'lambda_run': (lambda v, e, **kw: v.lambda_run(T, 0.8, 16, 'q_learning', 0.2, 0.9, e, **kw), [('td_init', (0.0,))],
                   ('lambda_run', ('q_learning', 16, 0.8, 0.2, 0.9, 'Q')), {}),
    'fa_run': (lambda v, e, **kw: v.fa_run(T, 'q_learning', 0.2, 0.9, e, **kw), [], ('fa_run', ('q_learning', 0.2, 0.9, 'Q')), dict(fa_f=16, fa_k=1)),
    'actor_critic_run': (lambda v, e, **kw: v.actor_critic_run(T, 0.3, 0.4, 0.9, **kw), [('ac_init', (0.0, 0.0))], ('ac_run', (0.3, 0.4, 0.9)), {}),
    'reinforce_run': (lambda v, e, **kw: v.reinforce_run(T, 32, 0.3, 0.4, 0.9, **kw), [('ac_init', (0.0, 0.0))], ('reinforce_run', (32, 0.3, 0.4, 0.9)), {}),
    'off_policy_mc_run': (lambda v, e, **kw: v.off_policy_mc_run(T, 32, 0.9, e, 4.0, **kw), [('td_init', (0.0,)), ('is_init', ())],
                          ('is_run', (32, 0.9, 'Q', 4.0)), {}),
}


@pytest.mark.parametrize('trajectory,stats', [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize('present', [False, True])
@pytest.mark.parametrize('name', sorted(LAUNCHES))
def test_every_launch_sends_exactly_these_calls(name, present, trajectory, stats):
    call, allocates, (run, args), needs = LAUNCHES[name]
    for eps, q in Q16.items():
        vec = _vec(PRESENT if present else dict(ABSENT, **needs))
        out = call(vec, eps, trajectory=trajectory, stats=stats)
        want = [] if present else list(allocates)
        if trajectory:
            want.append(('reserve_trajectory', (T,)))
        want.append((run, (T,) + tuple(q if a == 'Q' else a for a in args) + (trajectory, stats)))
        if trajectory:
            want.append(('read_trajectory', (0, T)))
        if stats:
            want.append(('read_stats', ()))
        assert _sent(vec) == want, eps
        assert sorted(out) == (['episodes', 'ret'] if stats else [])
        assert sum(1 for c in vec.engine.calls if c[0] == 'stores') <= 1  # one question per launch at the most


# helper call -> (what it sends to an engine that holds nothing, what to one that holds everything)
ENSURES = [
    (lambda v: v._ensure_q(), [('td_init', (0.0,))], []),
    (lambda v: v._ensure_q(2.5), [('td_init', (2.5,))], [('td_init', (2.5,))]),
    (lambda v: v._ensure_model(), [('dyna_init', ())], []),
    (lambda v: v._ensure_model(True), [('dyna_init', ())], [('dyna_init', ())]),
    (lambda v: v._ensure_model(clear=True), [('dyna_init', ())], [('dyna_init', ())]),
    (lambda v: v._ensure_pairs(), [('double_init', (0.0,))], []),
    (lambda v: v._ensure_pairs(1.5), [('double_init', (1.5,))], [('double_init', (1.5,))]),
    (lambda v: v._ensure_queue(), [('sweep_init', ())], []),
    (lambda v: v._ensure_tree(), [('td_init', (0.0,)), ('mcts_init', (1,))], []),
    (lambda v: v._ensure_counts(), [('td_init', (0.0,)), ('explore_init', ())], []),
    (lambda v: v._ensure_ac(), [('ac_init', (0.0, 0.0))], []),
    (lambda v: v._ensure_ac(1.0), [('ac_init', (1.0, 0.0))], [('ac_init', (1.0, 0.0))]),
    (lambda v: v._ensure_ac(None, 2.0), [('ac_init', (0.0, 2.0))], [('ac_init', (0.0, 2.0))]),
    (lambda v: v._ensure_ac(h0=0.0, v0=0.0), [('ac_init', (0.0, 0.0))], [('ac_init', (0.0, 0.0))]),
    (lambda v: v._ensure_is(), [('td_init', (0.0,)), ('is_init', ())], []),
]


@pytest.mark.parametrize('k', range(len(ENSURES)))
def test_every_ensure_helper_allocates_what_is_missing_and_nothing_else(k):
    call, absent, present = ENSURES[k]
    for held, want in ((ABSENT, absent), (PRESENT, present)):
        vec = _vec(held)
        call(vec)
        assert _sent(vec) == want


def test_helpers_that_need_two_stores_allocate_the_one_that_is_missing():
    for call, init in ((lambda v: v._ensure_counts(), 'explore_init'), (lambda v: v._ensure_is(), 'is_init')):
        vec = _vec(dict(ABSENT, td_rows=16))
        call(vec)
        assert _sent(vec) == [(init, ())]
    vec = _vec(dict(ABSENT, td_rows=16))
    vec._ensure_tree()
    assert _sent(vec) == [('mcts_init', (1,))]
    vec = _vec(dict(PRESENT, mcts_nodes=7))  # a pool of 6 simulations: 6 fit, 7 need a new one; the schedule stays
    vec.tree_search_run(T, 6)
    vec.tree_search_run(T, 7)
    assert [c[0] for c in _sent(vec)] == ['mcts_run', 'mcts_init', 'mcts_run'] and _sent(vec)[1] == ('mcts_init', (7,))
    vec = _vec(dict(PRESENT, mcts_nodes=0))  # no pool: even a launch without simulations gets one, of one simulation
    vec.tree_search_run(T, 0)
    assert _sent(vec)[0] == ('mcts_init', (1,))
    vec = _vec(dict(PRESENT, mcts_nodes=0, overlay=2, overlay_bits=2, td_rows=64))  # ... but not under an overlay: the library refuses the launch itself
    vec.tree_search_run(T, 3)
    assert [c[0] for c in _sent(vec)] == ['mcts_run']


def test_masks_take_their_width_from_the_library():
    vec = _vec(dict(ABSENT, overlay=2, overlay_bits=3))
    vec.set_fruit_eaten([7, 0], env0=1)
    with pytest.raises(ValueError, match='masks of the 3 fruits set'):
        vec.set_fruit_eaten([8])
    with pytest.raises(ValueError, match='masks of the 0 door slots set'):  # fruit is set, not doors
        vec.set_doors_open([2])
    vec = _vec(dict(ABSENT, overlay=3, overlay_bits=2))
    vec.set_doors_open(3)
    with pytest.raises(ValueError, match='masks of the 2 door slots set'):
        vec.set_doors_open([4])
    assert [c[0] for c in _sent(vec)] == ['set_doors_state']


def test_set_fruit_and_set_doors_leave_the_tables_to_the_library():
    """The facade keeps no flag: after an overlay it asks.  The library's half -- tables of another row count are dropped -- is
    tests/test_gpu_stores.py's."""
    for put in (lambda v: v.set_fruit([1, 2]), lambda v: v.set_doors({0: 1}, keys={0: 2})):
        vec = _vec(PRESENT)
        put(vec)
        vec.engine.held = dict(PRESENT, td_rows=0)  # the library says: the tables went
        vec._ensure_q()
        assert _sent(vec)[1:] == [('td_init', (0.0,))]
        vec.engine.held = dict(PRESENT, td_rows=16 << 2)  # ... and now: they are there
        vec._ensure_q()
        assert _sent(vec)[1:] == [('td_init', (0.0,))]


# ---- what is refused, with which words, before anything is sent ----
BAD = float('nan')
FACADE_REFUSALS = [
    (lambda v: v.set_wind(np.ones(4, int), gust=1.5), ValueError, 'gust must lie in [0, 1]'),
    (lambda v: v.set_wind(None, gust=BAD), ValueError, 'gust must lie in [0, 1]'),
    (lambda v: v.expected_sarsa_run(T, epsilon=1.5), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.double_q_run(T, epsilon=-0.1), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.search_run(T, epsilon=BAD), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.search_run(T, rollout_epsilon=2), ValueError, 'rollout_epsilon must lie in [0, 1]'),
    (lambda v: v.search_run(T, epsilon=2, rollout_epsilon=2), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.tree_search_run(T, epsilon=2), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.tree_search_run(T, rollout_epsilon=-1), ValueError, 'rollout_epsilon must lie in [0, 1]'),
    (lambda v: v.tree_search_run(T, simulations=256), ValueError, 'simulations must lie in 0 .. 255'),
    (lambda v: v.tree_search_run(T, simulations=-1, epsilon=2, rollout_epsilon=2), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.tree_search_run(T, simulations=-1, rollout_epsilon=2), ValueError, 'rollout_epsilon must lie in [0, 1]'),
    (lambda v: v.explore_run(T, rule='greedy'), ValueError, "rule must be 'ucb' or 'thompson'"),
    (lambda v: v.explore_run(T, epsilon=2), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.explore_run(T, rule='greedy', epsilon=2), ValueError, "rule must be 'ucb' or 'thompson'"),
    (lambda v: v.explore_run(T), ValueError, 'no exploration schedule: call set_exploration(U, B) first'),
    (lambda v: v.off_policy_mc_run(T, max_episode_len=0), ValueError, 'max_episode_len must lie in 1 .. 1024'),
    (lambda v: v.off_policy_mc_run(T, epsilon=2), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.off_policy_mc_run(T, w_cap=0.5), ValueError, 'w_cap must lie in [1, 2**256]'),
    (lambda v: v.off_policy_mc_run(T, max_episode_len=1025, epsilon=2, w_cap=BAD), ValueError, 'max_episode_len must lie in 1 .. 1024'),
    (lambda v: v.off_policy_mc_run(T, epsilon=2, w_cap=BAD), ValueError, 'epsilon must lie in [0, 1]'),
    (lambda v: v.fa_run(T), RuntimeError, 'no features: call set_features first'),
    (lambda v: v.weights(), RuntimeError, 'no features: call set_features first'),
    (lambda v: v.set_weights(np.zeros((16, 4))), RuntimeError, 'no features: call set_features first'),
    (lambda v: v.fa_q_table(), RuntimeError, 'no features: call set_features first'),
    (lambda v: v.set_fruit([1], values=(17, 0, 0)), ValueError, 'values must be three integers in -16 .. 16 (apple, lemon, melon)'),
    (lambda v: v.set_fruit([15]), ValueError, 'fruit on cell 15, which is a wall or a goal or lava cell'),
    (lambda v: v.set_doors(None, keys={0: 1}), ValueError, 'set_doors(None) takes the doors away: keys and levers must be None too'),
    (lambda v: v.set_doors({0: 15}, keys={0: 1}), ValueError, 'a door, key or lever on cell 15, which is a wall or a goal or lava cell'),
]


@pytest.mark.parametrize('k', range(len(FACADE_REFUSALS)))
def test_the_facade_refuses_before_it_sends_anything(k):
    call, kind, message = FACADE_REFUSALS[k]
    vec = _vec()
    with pytest.raises(kind) as err:
        call(vec)
    assert str(err.value) == message
    assert _sent(vec) == []


def test_epsilon_out_of_range_is_left_to_the_library_where_it_always_was():
    for name in ('td_run', 'dyna_run', 'sweep_run', 'nstep_run', 'lambda_run', 'fa_run'):
        vec = _vec(PRESENT)
        LAUNCHES[name][0](vec, 1.5)
        assert _sent(vec)[-1][0] == LAUNCHES[name][2][0] and 98304 in _sent(vec)[-1][1]


def test_engine_weights_before_fa_init_are_a_runtime_error():
    from griduniverse_amd.engine import Engine
    eng = Engine.__new__(Engine)  # no library: the refusal comes before any call into it
    eng.N, eng._h, eng.stores = 4, None, lambda: dict(ABSENT)
    for call in (lambda: eng.fa_get_w(), lambda: eng.fa_set_w(np.zeros((16, 4)))):
        with pytest.raises(RuntimeError) as err:
            call()
        assert type(err.value) is RuntimeError and str(err.value) == 'no features: call fa_init first'


def _algorithms():
    from griduniverse_amd.algorithms import dyna, exploration, function_approximation as fa, off_policy, policy_gradient as pg, search
    from griduniverse_amd.algorithms import temporal_difference as td
    L, EPS, STEPS = 'num_learners must be at least 1', 'epsilon must lie in [0, 1]', 'num_steps must not be negative'
    REPS, LEN = 'rollout_epsilon must lie in [0, 1]', 'max_episode_len must lie in 1 .. 1024'
    P, SIZE = 'planning_steps must lie in 0 .. 256', 'size must lie in 2 .. 4096'
    cases = []
    for f in (td.q_learning, td.sarsa):
        cases += [(f, dict(num_learners=0), L), (f, dict(epsilon=1.5), EPS), (f, dict(gust=2), 'gust must lie in [0, 1]'),
                  (f, dict(num_learners=0, epsilon=2, gust=2), L), (f, dict(epsilon=2, gust=2), EPS),
                  (f, dict(wind=np.zeros(4, int), fruit=([1], 'apple', (1, 5, -5))), 'wind and fruit exclude each other'),
                  (f, dict(fruit=([1], 'apple')), 'fruit must be (cells, kinds, values)'),
                  (f, dict(wind=np.zeros(4, int), doors=dict(doors={0: 1}, keys={0: 2})), 'doors exclude wind and fruit'),
                  (f, dict(doors=dict(keys={0: 2})), 'doors must be dict(doors=, keys=, levers=)'), (f, dict(gust=2, fruit=7), 'gust must lie in [0, 1]')]
    for f in (td.expected_sarsa, td.double_q_learning, fa.semi_gradient_sarsa, fa.semi_gradient_q_learning):
        cases += [(f, dict(num_learners=0), L), (f, dict(epsilon=-1), EPS), (f, dict(num_learners=0, epsilon=-1), L)]
    for f in (td.n_step_sarsa, td.n_step_q_learning):
        cases += [(f, dict(n=0), 'n must lie in 1 .. 16'), (f, dict(n=17, num_learners=0), 'n must lie in 1 .. 16'), (f, dict(num_learners=0, epsilon=2), L),
                  (f, dict(epsilon=2), EPS)]
    for f in (td.sarsa_lambda, td.watkins_q_lambda):
        cases += [(f, dict(trace_len=0, lam=2), 'trace_len must lie in 1 .. 64'), (f, dict(trace_len=65), 'trace_len must lie in 1 .. 64'),
                  (f, dict(lam=2, num_learners=0), 'lam must lie in [0, 1]'), (f, dict(num_learners=0, epsilon=2), L), (f, dict(epsilon=2), EPS)]
    for f in (dyna.dyna_q, dyna.prioritized_sweeping):
        cases += [(f, dict(num_learners=0, planning_steps=-1), L), (f, dict(planning_steps=257, epsilon=2), P), (f, dict(epsilon=2, steps=-1), EPS),
                  (f, dict(steps=-1), STEPS)]
    cases += [(dyna.prioritized_sweeping, dict(epsilon=2, theta=-1.0), EPS), (dyna.prioritized_sweeping, dict(theta=BAD, steps=-1), 'theta must be finite and not negative')]
    f = search.rollout_search
    cases += [(f, dict(num_learners=0, simulations=65), L), (f, dict(simulations=65, depth=257), 'simulations must lie in 0 .. 64'),
              (f, dict(depth=257, epsilon=2), 'depth must lie in 0 .. 256'), (f, dict(epsilon=2, rollout_epsilon=2), EPS), (f, dict(rollout_epsilon=2, steps=-1), REPS),
              (f, dict(steps=-1), STEPS)]
    f = search.tree_search
    cases += [(f, dict(num_learners=0, simulations=256), L), (f, dict(simulations=256, tree_depth=0), 'simulations must lie in 0 .. 255'),
              (f, dict(tree_depth=65, depth=-1), 'tree_depth must lie in 1 .. 64'), (f, dict(depth=257, epsilon=2), 'depth must lie in 0 .. 256'),
              (f, dict(epsilon=2, rollout_epsilon=2), EPS), (f, dict(rollout_epsilon=2, steps=-1), REPS), (f, dict(steps=-1, c=-1.0), STEPS),
              (f, dict(c=-1.0), 'c must be finite and not negative')]
    cases += [(search.uct_tables, dict(no_env=True, size=1, c=-1), SIZE), (search.uct_tables, dict(no_env=True, c=BAD), 'c must be finite and not negative')]
    for f, scale, word in ((exploration.ucb_q_learning, 'c', 'c'), (exploration.thompson_q_learning, 'sigma', 'sigma')):
        cases += [(f, dict(table_size=1, num_learners=0, **{scale: -1}), SIZE), (f, dict(num_learners=0, **{scale: -1}), word + ' must be finite and not negative'),
                  (f, dict(num_learners=0, epsilon=2), L), (f, dict(epsilon=2, steps=-1), EPS), (f, dict(steps=-1), STEPS)]
    f = pg.actor_critic
    cases += [(f, dict(num_learners=0, steps=-1), L), (f, dict(steps=-1, actor_lr=BAD), STEPS), (f, dict(actor_lr=BAD, critic_lr=BAD), 'actor_lr must be finite'),
              (f, dict(critic_lr=float('inf'), discount_factor=BAD), 'critic_lr must be finite'), (f, dict(discount_factor=BAD), 'discount_factor must be finite')]
    f = pg.reinforce
    cases += [(f, dict(num_learners=0, steps=-1), L), (f, dict(steps=-1, max_episode_len=0), STEPS), (f, dict(max_episode_len=1025, actor_lr=BAD), LEN),
              (f, dict(actor_lr=BAD, baseline_lr=BAD), 'actor_lr must be finite'), (f, dict(baseline_lr=BAD, discount_factor=BAD), 'baseline_lr must be finite'),
              (f, dict(discount_factor=BAD), 'discount_factor must be finite')]
    f = off_policy.off_policy_mc_control
    cases += [(f, dict(num_learners=0, steps=-1), L), (f, dict(steps=-1, max_episode_len=0), STEPS), (f, dict(max_episode_len=0, epsilon=2), LEN),
              (f, dict(epsilon=2, w_cap=0.5), EPS), (f, dict(w_cap=0.5, discount_factor=BAD), 'w_cap must lie in [1, 2**256]'),
              (f, dict(discount_factor=BAD, q0=BAD), 'discount_factor must be finite'), (f, dict(q0=BAD), 'q0 must be finite')]
    cases += [(off_policy.ratio_table, dict(no_env=True, epsilon=2), EPS)]
    return cases


def test_the_algorithms_refuse_before_they_open_a_batch(monkeypatch):
    from griduniverse_amd.algorithms import _batch

    def no_device(*a, **kw):
        raise AssertionError('a batch was opened before the arguments were checked')

    monkeypatch.setattr(_batch, 'VecGridUniverse', no_device)
    env = GridUniverseEnv((4, 4))
    for f, kw, message in _algorithms():
        kw = dict(kw)
        steps = kw.pop('steps', 10)
        with pytest.raises(ValueError) as err:
            f(**kw) if kw.pop('no_env', False) else f(env, steps, **kw)
        assert str(err.value) == message, (f.__name__, kw)


def test_every_algorithm_runs_its_batch_through_the_one_loop(monkeypatch):
    """prepare, reset, launches of at most a chunk, read, close -- on a batch that records, for a learner of each kind."""
    from griduniverse_amd.algorithms import _batch, dyna, off_policy, policy_gradient as pg
    from griduniverse_amd.algorithms import temporal_difference as td
    made = []
    makes = dict(td_init=dict(td_rows=16), double_init=dict(double=16), dyna_init=dict(dyna=16), ac_init=dict(ac=16), is_init={'is': 16})

    class Keeping(Scripted):
        """... and holds what it was told to allocate, as the library does."""

        def __getattr__(self, name):
            self.held.update(makes.get(name, {}))
            return Scripted.__getattr__(self, name)

    class Batch(gua.VecGridUniverse):
        def __init__(self, L, template=None, seed=0):
            super().__init__(L, template=template, seed=seed, engine_factory=Keeping)
            made.append(self)

        def q_table(self, env0=0, n=None):
            return np.zeros((self.num_envs, 16, 4))

        def double_q_tables(self, env0=0, n=None):
            return np.zeros((self.num_envs, 16, 2, 4))

        def softmax_policy(self, env0=0, n=None):
            return np.full((self.num_envs, 16, 4), 0.25)

        def state_values(self, env0=0, n=None):
            return np.zeros((self.num_envs, 16))

    monkeypatch.setattr(_batch, 'VecGridUniverse', Batch)
    monkeypatch.setattr(_batch, '_CHUNK', 4)
    monkeypatch.setattr(td, '_CHUNK', 4)
    monkeypatch.setattr(pg, '_CHUNK', 4)
    monkeypatch.setattr(off_policy, '_CHUNK', 4)
    env = GridUniverseEnv((4, 4))

    def names():
        return [c[0] for c in _sent(made[-1])]

    assert td.q_learning(env, 10, q0=1.0).shape == (16, 4)
    assert _sent(made[-1])[:2] == [('td_init', (1.0,)), ('reset', (None, None))]
    assert [c[1][0] for c in _sent(made[-1]) if c[0] == 'td_run'] == [4, 4, 2] and names()[-1] == 'close'
    assert td.sarsa(env, 3, num_learners=2, wind=np.ones(4, int), gust=0.5).shape == (2, 16, 4)
    assert names() == ['set_wind', 'td_init', 'reset', 'td_run', 'close']
    assert td.double_q_learning(env, 5, num_learners=3, q0=2.0).shape == (3, 16, 4)
    assert names() == ['double_init', 'reset', 'double_run', 'double_run', 'close'] and _sent(made[-1])[0] == ('double_init', (2.0,))
    assert td.sarsa_lambda(env, 5, trace_len=8).shape == (16, 4)  # long traces, shorter launches: chunk * 4 // trace_len steps
    assert [c[1][0] for c in _sent(made[-1]) if c[0] == 'lambda_run'] == [2, 2, 1]
    assert dyna.dyna_q(env, 2, q0=0.5).shape == (16, 4)
    assert names() == ['td_init', 'dyna_init', 'reset', 'dyna_run', 'close']
    policy, v = pg.actor_critic(env, 6)
    assert policy.shape == (16, 4) and v.shape == (16,) and not policy[15].any() and policy[0].tolist() == [0.25] * 4
    assert names() == ['ac_init', 'reset', 'ac_run', 'ac_run', 'close']
    policy, v = pg.reinforce(env, 1, num_learners=2)
    assert policy.shape == (2, 16, 4) and v.shape == (2, 16)
    assert off_policy.off_policy_mc_control(env, 0, q0=3.0).shape == (16, 4)
    assert names() == ['td_init', 'reset', 'close']
    with pytest.raises(ValueError):  # a batch that fails on the way is closed all the same
        td.q_learning(env, 10, fruit=([15], 'apple', (1, 5, -5)))
    assert names() == ['close']


def test_importing_the_algorithms_package_loads_no_learner_module_and_no_library():
    code = ("import sys, griduniverse_amd.algorithms, griduniverse_amd._lib as L\n"
            "assert L._lib is None\n"
            "print(' '.join(sorted(m for m in sys.modules if m.startswith('griduniverse_amd'))))")
    out = subprocess.run([sys.executable, '-c', code], check=True, capture_output=True, text=True).stdout.split()
    # (the list the package had before the batch loop moved into algorithms/_batch.py)
    assert out == ['griduniverse_amd', 'griduniverse_amd._lib', 'griduniverse_amd.algorithms', 'griduniverse_amd.envs',
                   'griduniverse_amd.envs.griduniverse_env', 'griduniverse_amd.envs.maze_generation', 'griduniverse_amd.envs.spaces',
                   'griduniverse_amd.grid']
