"""Tabular Dyna-Q (Sutton & Barto 8.2): Q-learning plus a learned model of the env, replayed for `planning_steps` updates after
every real step -- "Integrating learning and planning (Dyna, ...)" on the reference's roadmap (README.md "GridUniverse features
and plans"; it ships no code for it, so the semantics are this build's: include/gu.h, gu_dyna_run).

`dyna_q` runs `num_learners` independent learners on the grid of a facade `GridUniverseEnv`, learner e in env e of a batch, each
with its own float64 Q table and its own model, all advanced on the MI355X by one kernel (csrc/gu_dyna.hip).  Its result has the
shape of `q_learning`'s and feeds `greedy_policy` the same way.

`prioritized_sweeping` (Sutton & Barto 8.4; include/gu.h, gu_sweep_run; csrc/gu_sweep.hip) keeps the same model and spends its
planning updates where they change something: every learner has a priority queue of observed pairs, ordered by the size of the
update waiting for them, takes its planning updates from the top and queues the predecessors of what it updated.
"""
import math

from ._batch import learn, need_learners, need_steps, unit

MAX_PLANNING_STEPS = 256
MAX_SWEEP_STATES = 16384  # the queue's keys hold the pair index s*4+a in 16 bits
_UPDATES = 1000000  # real steps x (planning steps + 1) per launch (the launch limit is 1e8; shorter launches keep the device responsive)


def dyna_q(env, num_steps, planning_steps=10, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy Dyna-Q, `num_steps` real env steps per learner (episodes restart at a start cell when they end), each
    followed by `planning_steps` model updates (0 .. 256; 0 is Q-learning).  Returns Q float64[S][4], or [L][S][4] for
    L = num_learners > 1."""
    L, P = need_learners(num_learners), int(planning_steps)
    if not 0 <= P <= MAX_PLANNING_STEPS:
        raise ValueError('planning_steps must lie in 0 .. {}'.format(MAX_PLANNING_STEPS))
    unit('epsilon', epsilon)
    need_steps(num_steps)
    return learn(env, L, seed, num_steps, max(1, _UPDATES // (P + 1)), lambda vec: (vec._ensure_q(q0), vec._ensure_model()),
                 lambda vec, T: vec.dyna_run(T, P, alpha, discount_factor, epsilon))


def prioritized_sweeping(env, num_steps, planning_steps=10, theta=1e-4, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0,
                         q0=0.0):
    """Epsilon-greedy prioritized sweeping, `num_steps` real env steps per learner (episodes restart at a start cell when they end).
    A real step queues its pair when its |TD error| exceeds `theta` (finite, not negative) and is followed by up to `planning_steps`
    (0 .. 256) updates from the top of the learner's priority queue, each of which queues the predecessors of its pair; a real step
    updates nothing by itself.  Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1."""
    L, P, theta = need_learners(num_learners), int(planning_steps), float(theta)
    if not 0 <= P <= MAX_PLANNING_STEPS:
        raise ValueError('planning_steps must lie in 0 .. {}'.format(MAX_PLANNING_STEPS))
    unit('epsilon', epsilon)
    if not (math.isfinite(theta) and theta >= 0.0):
        raise ValueError('theta must be finite and not negative')
    need_steps(num_steps)
    if int(env.world.size) > MAX_SWEEP_STATES:
        raise ValueError('prioritized sweeping takes grids of at most {} states'.format(MAX_SWEEP_STATES))
    return learn(env, L, seed, num_steps, max(1, _UPDATES // (P + 1)), lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.sweep_run(T, P, theta, alpha, discount_factor, epsilon))
