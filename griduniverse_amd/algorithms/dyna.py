"""Tabular Dyna-Q (Sutton & Barto 8.2): Q-learning plus a learned model of the env, replayed for `planning_steps` updates after
every real step -- "Integrating learning and planning (Dyna, ...)" on the reference's roadmap (README.md "GridUniverse features
and plans"; it ships no code for it, so the semantics are this build's: include/gu.h, gu_dyna_run).

`dyna_q` runs `num_learners` independent learners on the grid of a facade `GridUniverseEnv`, learner e in env e of a batch, each
with its own float64 Q table and its own model, all advanced on the MI355X by one kernel (csrc/gu_dyna.hip).  Its result has the
shape of `q_learning`'s and feeds `greedy_policy` the same way.
"""
from .temporal_difference import _learn

MAX_PLANNING_STEPS = 256
_UPDATES = 1000000  # real steps x (planning steps + 1) per launch (the launch limit is 1e8; shorter launches keep the device responsive)


def dyna_q(env, num_steps, planning_steps=10, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy Dyna-Q, `num_steps` real env steps per learner (episodes restart at a start cell when they end), each
    followed by `planning_steps` model updates (0 .. 256; 0 is Q-learning).  Returns Q float64[S][4], or [L][S][4] for
    L = num_learners > 1."""
    L, P = int(num_learners), int(planning_steps)
    if L < 1:
        raise ValueError('num_learners must be at least 1')
    if not 0 <= P <= MAX_PLANNING_STEPS:
        raise ValueError('planning_steps must lie in 0 .. {}'.format(MAX_PLANNING_STEPS))
    if not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError('epsilon must lie in [0, 1]')
    if int(num_steps) < 0:
        raise ValueError('num_steps must not be negative')
    return _learn(env, L, seed, q0, num_steps, max(1, _UPDATES // (P + 1)),
                  lambda vec, T: vec.dyna_run(T, P, alpha, discount_factor, epsilon), model=True)
