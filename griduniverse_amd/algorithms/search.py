"""Simulation-based search: Monte-Carlo rollouts at decision time (Sutton & Barto 8.10, "rollout algorithms"; "simple Monte-Carlo
search" in Silver's lecture 8) -- the second half of "Integrating learning and planning (Dyna, MC/TD Tree search, Forward and
Simulation-based search)" on the reference's roadmap (README.md "GridUniverse features and plans"; it ships no code for it, so the
semantics are this build's: include/gu.h, gu_search_run).

`dyna.dyna_q` plans in the background from a learned model.  `rollout_search` plans before every real move, from the state the
learner stands in, with the true model: `simulations` rollouts of `depth` moves per action, scored by their summed discounted
returns (a truncated rollout bootstraps on max Q at its leaf).  It runs `num_learners` independent learners on the grid of a facade
`GridUniverseEnv`, learner e in env e of a batch, each with its own float64 Q table, all advanced on the MI355X by one kernel
(csrc/gu_search.hip).  Its result has the shape of `q_learning`'s and feeds `greedy_policy` the same way.
"""
from .. import _lib
from .temporal_difference import _learn

_MOVES = 1000000  # real steps x (1 + 4 x simulations x depth) moves per launch (the launch limit is 1e8; shorter launches keep the device responsive)


def rollout_search(env, num_steps, simulations=4, depth=16, alpha=0.1, discount_factor=0.99, epsilon=0.1, rollout_epsilon=1.0,
                   num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy learners that choose every non-exploring action by rollout search and learn by Q-learning, `num_steps` real
    env steps per learner (episodes restart at a start cell when they end).  `simulations` (0 .. 64; 0 is `q_learning`) rollouts
    per action, `depth` (0 .. 256) simulated moves each, under an epsilon-greedy rollout policy on the learner's table
    (`rollout_epsilon`; 1.0 = uniformly random).  Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1."""
    L, M, D = int(num_learners), int(simulations), int(depth)
    if L < 1:
        raise ValueError('num_learners must be at least 1')
    if not 0 <= M <= _lib.SEARCH_MAX_M:
        raise ValueError('simulations must lie in 0 .. {}'.format(_lib.SEARCH_MAX_M))
    if not 0 <= D <= _lib.SEARCH_MAX_D:
        raise ValueError('depth must lie in 0 .. {}'.format(_lib.SEARCH_MAX_D))
    if not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError('epsilon must lie in [0, 1]')
    if not 0.0 <= float(rollout_epsilon) <= 1.0:
        raise ValueError('rollout_epsilon must lie in [0, 1]')
    if int(num_steps) < 0:
        raise ValueError('num_steps must not be negative')
    return _learn(env, L, seed, q0, num_steps, max(1, _MOVES // (1 + 4 * M * D)),
                  lambda vec, T: vec.search_run(T, M, D, alpha, discount_factor, epsilon, rollout_epsilon))
