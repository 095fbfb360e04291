"""Tabular temporal-difference control: Q-learning (off-policy) and SARSA (on-policy), the next algorithms on the reference's
roadmap (README.md "Temporal Difference (TD) Learning"; it ships no code for them, so the semantics are this build's:
include/gu.h, gu_td_run).

`q_learning` / `sarsa` run `num_learners` independent epsilon-greedy learners on the grid of a facade `GridUniverseEnv`, learner e
in env e of a batch, each with its own float64 Q table, all advanced on the MI355X by one kernel (csrc/gu_td.hip).  The facade's
own state is left alone.  `greedy_policy` turns a learned table into the reference's policy-matrix format, so it feeds
`get_policy_map`, `engine.vi_set` and `rollout(policy='greedy')` like a policy from dynamic programming.

`n_step_sarsa` / `n_step_q_learning` are the n-step variations (Sutton & Barto ch. 7; include/gu.h, gu_nstep_run), on the same
tables, by csrc/gu_nstep.hip.  `sarsa_lambda` / `watkins_q_lambda` are the eligibility-trace variations (Sutton & Barto ch. 12;
include/gu.h, gu_lambda_run), on the same tables, by csrc/gu_lambda.hip.  `expected_sarsa` (Sutton & Barto 6.6; gu_esarsa_run) is a
third rule of csrc/gu_td.hip on the same tables; `double_q_learning` (6.7; gu_double_run) keeps two tables per learner, by
csrc/gu_double.hip.
"""
import numpy as np

from .. import _lib
from ._batch import _CHUNK, learn, need_learners, unit


def overlay_installer(wind=None, gust=0.0, fruit=None, doors=None, boxes=None, errands=None):
    """The checks of the overlay arguments that q_learning and sarsa take (ValueError), and the function that puts the overlay they
    name on a batch (algorithms.evaluation walks under it too)."""
    unit('gust', gust)
    if fruit is not None:
        if wind is not None:
            raise ValueError('wind and fruit exclude each other')
        if not isinstance(fruit, (tuple, list)) or len(fruit) != 3:
            raise ValueError('fruit must be (cells, kinds, values)')
    if doors is not None:
        if wind is not None or fruit is not None:
            raise ValueError('doors exclude wind and fruit')
        if not isinstance(doors, dict) or 'doors' not in doors or set(doors) - {'doors', 'keys', 'levers'}:
            raise ValueError('doors must be dict(doors=, keys=, levers=)')
    if boxes is not None:
        if wind is not None or fruit is not None or doors is not None:
            raise ValueError('boxes exclude wind, fruit and doors')
        if not isinstance(boxes, dict) or not {'boxes', 'targets'} <= set(boxes) or set(boxes) - {'boxes', 'targets', 'on_target'}:
            raise ValueError('boxes must be dict(boxes=, targets=, on_target=)')
    if errands is not None:
        if wind is not None or fruit is not None or doors is not None or boxes is not None:
            raise ValueError('errands exclude wind, fruit, doors and boxes')
        if not isinstance(errands, dict) or not {'cells', 'instructions'} <= set(errands) or set(errands) - {'cells', 'kinds', 'instructions', 'right', 'wrong', 'finish'}:
            raise ValueError('errands must be dict(cells=, kinds=, instructions=, right=, wrong=, finish=)')

    def install(vec):
        if wind is not None:
            strength, direction = wind if isinstance(wind, tuple) else (wind, 'up')
            vec.set_wind(strength, direction, gust)
        if fruit is not None:
            vec.set_fruit(*fruit)
        if doors is not None:
            vec.set_doors(doors['doors'], doors.get('keys'), doors.get('levers'))
        if boxes is not None:
            vec.set_boxes(boxes['boxes'], boxes['targets'], boxes.get('on_target', 5))
        if errands is not None:
            vec.set_errands(**errands)

    return install


def _td(method, env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0, wind=None, gust=0.0, fruit=None, doors=None, boxes=None, errands=None):
    need_learners(num_learners)
    unit('epsilon', epsilon)
    install = overlay_installer(wind, gust, fruit, doors, boxes, errands)

    def prepare(vec):  # (the tables have S << F rows under fruit and S << D under doors: the overlay goes on before them)
        install(vec)
        vec._ensure_q(q0)

    return learn(env, num_learners, seed, num_steps, _CHUNK, prepare, lambda vec, T: vec.td_run(T, method, alpha, discount_factor, epsilon))


def q_learning(env, num_steps, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0, wind=None, gust=0.0, fruit=None, doors=None, boxes=None,
               errands=None):
    """Epsilon-greedy Q-learning, `num_steps` env steps per learner (episodes restart at a start cell when they end).  Returns
    Q float64[S][4], or [L][S][4] for L = num_learners > 1.  `wind`: a strength array ([H, W], or [W] per column; blowing up) or a
    (strength, direction) pair as VecGridUniverse.set_wind takes them, gusting with probability `gust`; None: the calm grid.  `fruit`: (cells, kinds, values)
    as VecGridUniverse.set_fruit takes them -- the result then has S << F rows, row eaten * S + s for cell s with the mask `eaten` of
    eaten fruit; not together with `wind`.  `doors`: dict(doors=, keys=, levers=) as VecGridUniverse.set_doors takes them -- the result
    then has S << D rows, row open * S + s for cell s under the mask `open` of open slots; not together with `wind` or `fruit`.  `boxes`: dict(boxes=, targets=, on_target=)
    as VecGridUniverse.set_boxes takes them -- the result then has S << (b * B) rows, row word * S + s for cell s under the word
    grid.pack_boxes(S, cells) of the boxes' cells; not together with `wind`, `fruit` or `doors`.  `errands`: dict(cells=, kinds=,
    instructions=, right=, wrong=, finish=) as VecGridUniverse.set_errands takes them -- the result then has S << bits rows, row word * S + s
    for cell s under the word eaten | progress << F | instruction << (F + pb) (grid.errand_fields); not together with the other four."""
    return _td('q_learning', env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0, wind, gust, fruit, doors, boxes, errands)


def sarsa(env, num_steps, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0, wind=None, gust=0.0, fruit=None, doors=None, boxes=None, errands=None):
    """Epsilon-greedy SARSA; arguments and result as `q_learning`."""
    return _td('sarsa', env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0, wind, gust, fruit, doors, boxes, errands)


def expected_sarsa(env, num_steps, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy Expected SARSA (Sutton & Barto 6.6): acts as `q_learning` does and bootstraps on the mean of Q[s'] under the
    epsilon-greedy policy itself, so the target has no sampling noise from the next action.  `num_steps` env steps per learner.
    Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1.  With epsilon = 0 it is `q_learning`.  The calm grid only."""
    need_learners(num_learners)
    unit('epsilon', epsilon)
    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.expected_sarsa_run(T, alpha, discount_factor, epsilon))


def double_q_learning(env, num_steps, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy Double Q-learning (Sutton & Barto 6.7): two tables A and B per learner, both filled with q0; the learner acts
    on A + B, and a coin per step picks the table that learns from the other's estimate of its own greedy action.  `num_steps` env
    steps per learner.  Returns the MEAN of the two tables, (A + B) * 0.5, float64[S][4], or [L][S][4] for L = num_learners > 1
    (VecGridUniverse.double_q_tables gives the two apart).  The calm grid only."""
    need_learners(num_learners)
    unit('epsilon', epsilon)
    q = learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec._ensure_pairs(q0),
              lambda vec, T: vec.double_q_run(T, alpha, discount_factor, epsilon), lambda vec: vec.double_q_tables())
    return (q[..., 0, :] + q[..., 1, :]) * 0.5


def _nstep(method, env, num_steps, n, alpha, discount_factor, epsilon, num_learners, seed, q0):
    if not 1 <= int(n) <= _lib.NSTEP_MAX:
        raise ValueError('n must lie in 1 .. {}'.format(_lib.NSTEP_MAX))
    need_learners(num_learners)
    unit('epsilon', epsilon)
    # consecutive launches of one method and n carry the window, so chunking changes nothing
    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.nstep_run(T, n, method, alpha, discount_factor, epsilon))


def n_step_sarsa(env, num_steps, n=4, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy n-step SARSA (Sutton & Barto 7.2), 1 <= n <= 16, `num_steps` env steps per learner.  Returns Q
    float64[S][4], or [L][S][4] for L = num_learners > 1.  With n = 1 it is `sarsa`."""
    return _nstep('sarsa', env, num_steps, n, alpha, discount_factor, epsilon, num_learners, seed, q0)


def n_step_q_learning(env, num_steps, n=4, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy n-step Q-learning, uncorrected (it bootstraps on max Q[S_{t+n}], as asynchronous n-step Q-learning does);
    arguments and result as `n_step_sarsa`.  With n = 1 it is `q_learning`."""
    return _nstep('q_learning', env, num_steps, n, alpha, discount_factor, epsilon, num_learners, seed, q0)


def _lambda(method, env, num_steps, lam, trace_len, alpha, discount_factor, epsilon, num_learners, seed, q0):
    if not 1 <= int(trace_len) <= _lib.LAMBDA_MAX:
        raise ValueError('trace_len must lie in 1 .. {}'.format(_lib.LAMBDA_MAX))
    unit('lam', lam)
    need_learners(num_learners)
    unit('epsilon', epsilon)
    # a step costs up to trace_len entry updates, so launches get shorter as traces get longer; consecutive launches of one method
    # and trace_len carry the window, so chunking changes nothing
    chunk = min(_CHUNK, _CHUNK * 4 // int(trace_len))
    return learn(env, num_learners, seed, num_steps, chunk, lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.lambda_run(T, lam, trace_len, method, alpha, discount_factor, epsilon))


def sarsa_lambda(env, num_steps, lam=0.9, trace_len=32, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy SARSA(lambda) with replacing eligibility traces (Sutton & Barto ch. 12), each trace truncated after
    `trace_len` (1 .. 64) steps, `num_steps` env steps per learner.  Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1.
    With lam = 0 or trace_len = 1 it is `sarsa`."""
    return _lambda('sarsa', env, num_steps, lam, trace_len, alpha, discount_factor, epsilon, num_learners, seed, q0)


def watkins_q_lambda(env, num_steps, lam=0.9, trace_len=32, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0,
                     q0=0.0):
    """Epsilon-greedy Watkins's Q(lambda): as `sarsa_lambda`, bootstrapping on max Q[s'], and a non-greedy action cuts the traces
    of the pairs before it.  With lam = 0 or trace_len = 1 it is `q_learning`."""
    return _lambda('q_learning', env, num_steps, lam, trace_len, alpha, discount_factor, epsilon, num_learners, seed, q0)


def greedy_policy(q, env):
    """Policy matrix [S][4] of the greedy actions of Q [S][4], in the format of the reference's
    greedy_policy_from_value_function (core/algorithms/utils.py:55-72): the actions whose value equals the row maximum after
    rounding to 8 decimals share the probability equally; rows of terminal states are all zero."""
    q = np.asarray(q, np.float64)
    S = env.world.size
    if q.shape != (S, 4):
        raise ValueError('q must have shape ({}, 4), got {}'.format(S, q.shape))
    rounded = np.around(q, 8)
    best = rounded == np.around(np.amax(q, axis=1), 8)[:, None]
    policy = best / best.sum(axis=1, keepdims=True)
    terminal = np.array([bool(env.is_terminal(s)) for s in range(S)])
    policy[terminal] = 0.0
    return policy
