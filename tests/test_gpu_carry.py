"""What a learner carries from one launch to the next (the n-step and lambda windows, the episode buffers of REINFORCE and of
off-policy Monte-Carlo control) is dropped by ANY other call that touches the envs or the learner's tables, and by nothing else.
The learners' own files test this pair by pair against their oracles; this file pins the rule itself: every carrier against every
intervener, observed through the carrier's getter.

One engine per carrier (a default 4x4 grid, one wave of envs), with every learner's stores allocated up front: a first use would
allocate them through an init call that drops the carry by itself and would hide a launch that does not."""
import numpy as np
import pytest

import griduniverse_amd as gua

pytestmark = pytest.mark.gpu

N, T, S = 64, 6, 16

# carrier -> (launch(vec, steps, key), the key of its own launches, another key, its getter as a dict of arrays)
CARRIERS = {
    'nstep': (lambda v, t, k: v.nstep_run(t, k, 'sarsa', stats=True), 4, 5, lambda v: v.nstep_window()),
    'lambda': (lambda v, t, k: v.lambda_run(t, trace_len=k, stats=True), 8, 9, lambda v: {'sa': v.lambda_window()}),
    'reinforce': (lambda v, t, k: v.reinforce_run(t, max_episode_len=k, stats=True), 16, 17, lambda v: v.episode_buffer()),
    'off_policy_mc': (lambda v, t, k: v.off_policy_mc_run(t, max_episode_len=k, stats=True), 16, 17,
                      lambda v: v.off_policy_episode_buffer()),
}

# a one-step launch of every learner
LEARNERS = {
    'td_run': lambda v: v.td_run(1),
    'expected_sarsa_run': lambda v: v.expected_sarsa_run(1),
    'double_q_run': lambda v: v.double_q_run(1),
    'dyna_run': lambda v: v.dyna_run(1),
    'sweep_run': lambda v: v.sweep_run(1),
    'search_run': lambda v: v.search_run(1),
    'explore_run': lambda v: v.explore_run(1),
    'tree_search_run': lambda v: v.tree_search_run(1, simulations=4),
    'actor_critic_run': lambda v: v.actor_critic_run(1),
    'fa_run': lambda v: v.fa_run(1),
}
for _name, (_launch, _key, _, _) in CARRIERS.items():
    LEARNERS[_name + '_run'] = lambda v, launch=_launch, key=_key: launch(v, 1, key)


def _identity_features():
    return np.arange(S, dtype=np.int32)[:, None]


def _vi_sweep_step(v):
    v.engine.vi_set(np.zeros(S), np.full((S, 4), 0.25))
    v.engine.vi_sweep_step()


def _reset_one(v):
    mask = np.zeros(N, bool)
    mask[3] = True
    v.reset(mask)


INTERVENERS = {
    'reset': lambda v: v.reset(),
    'reset_one_env': _reset_one,
    'step': lambda v: v.step(np.zeros(N, np.int32)),
    'rollout': lambda v: v.rollout(1, trajectory=False, stats=True),
    'set_state': lambda v: v.engine.set_state(pos=v.get_state()['pos']),
    'seed': lambda v: v.seed(0),
    'set_q_table': lambda v: v.set_q_table(v.q_table()),
    'set_actor_critic': lambda v: v.set_actor_critic(h=v.preferences()),
    'set_importance_weights': lambda v: v.set_importance_weights(v.importance_weights()),
    'set_features': lambda v: v.set_features(_identity_features()),
    'set_weights': lambda v: v.set_weights(v.weights()),
    'vi_sweep_step': _vi_sweep_step,
}
INTERVENERS.update(LEARNERS)

CONTROLS = {
    'q_table': lambda v: v.q_table(),
    'sense': lambda v: v.sense(),
    'sync': lambda v: v.engine.sync(),
    'read_stats': lambda v: v.engine.read_stats(),
    'td_run_of_zero_steps': lambda v: v.td_run(0),
}


@pytest.fixture(scope='module')
def engines():
    """carrier -> its engine, made on first use and kept for the module"""
    made = {}

    def get(name):
        if name not in made:
            vec = made[name] = gua.VecGridUniverse(N, seed=0, auto_reset=True)
            vec.reset()
            vec.set_features(_identity_features())
            vec.set_exploration(np.zeros(2), np.zeros(2))
            for launch in LEARNERS.values():
                launch(vec)
            vec.importance_weights(), vec.preferences(), vec.weights()
        return made[name]

    yield get
    for vec in made.values():
        vec.close()


def _entries(left):
    """entries per env of what a getter returned"""
    return left['count'] if 'count' in left else (left['sa'] != -1).sum(axis=1)


def _left_something(name, vec):
    """The carrier's own launch, and what it left: asserted not to be empty, so that no case passes vacuously."""
    launch, key, _, getter = CARRIERS[name]
    launch(vec, T, key)
    left = getter(vec)
    assert _entries(left).any()
    return left


@pytest.mark.parametrize('name,intervener', [(c, i) for c in sorted(CARRIERS) for i in sorted(INTERVENERS) if i != c + '_run'])
def test_any_other_call_leaves_the_carrier_empty(engines, name, intervener):
    vec = engines(name)
    _left_something(name, vec)
    INTERVENERS[intervener](vec)
    left = CARRIERS[name][3](vec)
    assert not _entries(left).any()
    assert (left['sa'] == -1).all()


@pytest.mark.parametrize('name', sorted(CARRIERS))
def test_the_same_carrier_with_another_key_starts_empty(engines, name):
    """A launch of zero steps returns before it looks at the key, and a launch of one step leaves its own entry behind: what shows
    that the other key dropped the carry is that no env holds more than that one entry afterwards, where some held more before."""
    vec = engines(name)
    launch, _, other_key, getter = CARRIERS[name]
    assert _entries(_left_something(name, vec)).max() >= 2
    launch(vec, 1, other_key)
    assert _entries(getter(vec)).max() <= 1


@pytest.mark.parametrize('control', sorted(CONTROLS))
@pytest.mark.parametrize('name', sorted(CARRIERS))
def test_a_call_that_touches_nothing_leaves_the_carrier_as_it_was(engines, name, control):
    vec = engines(name)
    before = _left_something(name, vec)
    CONTROLS[control](vec)
    after = CARRIERS[name][3](vec)
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
