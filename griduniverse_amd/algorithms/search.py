"""Simulation-based search: Monte-Carlo rollouts at decision time (Sutton & Barto 8.10, "rollout algorithms"; "simple Monte-Carlo
search" in Silver's lecture 8) -- the second half of "Integrating learning and planning (Dyna, MC/TD Tree search, Forward and
Simulation-based search)" on the reference's roadmap (README.md "GridUniverse features and plans"; it ships no code for it, so the
semantics are this build's: include/gu.h, gu_search_run).

`dyna.dyna_q` plans in the background from a learned model.  `rollout_search` plans before every real move, from the state the
learner stands in, with the true model: `simulations` rollouts of `depth` moves per action, scored by their summed discounted
returns (a truncated rollout bootstraps on max Q at its leaf).  It runs `num_learners` independent learners on the grid of a facade
`GridUniverseEnv`, learner e in env e of a batch, each with its own float64 Q table, all advanced on the MI355X by one kernel
(csrc/gu_search.hip).  Its result has the shape of `q_learning`'s and feeds `greedy_policy` the same way.

`tree_search` is the "MC/TD Tree search" of the same roadmap entry (include/gu.h, gu_mcts_run; csrc/gu_mcts.hip): instead of a
fixed budget per action, every learner grows a UCT tree at the state it stands in -- UCB1 selection on the tree's own statistics, one
new node per simulation, the same rollout behind it (`depth` = 0: bootstrap on max Q at once, TD tree search), a backup -- and takes
the root action with the largest mean return.  `uct_tables` builds the UCB1 schedule it selects by.
"""
import numpy as np

from .. import _lib
from ._batch import learn, need_learners, need_steps, unit

_MOVES = 1000000  # real steps x (1 + 4 x simulations x depth) moves per launch (the launch limit is 1e8; shorter launches keep the device responsive)


def rollout_search(env, num_steps, simulations=4, depth=16, alpha=0.1, discount_factor=0.99, epsilon=0.1, rollout_epsilon=1.0,
                   num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy learners that choose every non-exploring action by rollout search and learn by Q-learning, `num_steps` real
    env steps per learner (episodes restart at a start cell when they end).  `simulations` (0 .. 64; 0 is `q_learning`) rollouts
    per action, `depth` (0 .. 256) simulated moves each, under an epsilon-greedy rollout policy on the learner's table
    (`rollout_epsilon`; 1.0 = uniformly random).  Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1."""
    L, M, D = need_learners(num_learners), int(simulations), int(depth)
    if not 0 <= M <= _lib.SEARCH_MAX_M:
        raise ValueError('simulations must lie in 0 .. {}'.format(_lib.SEARCH_MAX_M))
    if not 0 <= D <= _lib.SEARCH_MAX_D:
        raise ValueError('depth must lie in 0 .. {}'.format(_lib.SEARCH_MAX_D))
    unit('epsilon', epsilon)
    unit('rollout_epsilon', rollout_epsilon)
    need_steps(num_steps)
    return learn(env, L, seed, num_steps, max(1, _MOVES // (1 + 4 * M * D)), lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.search_run(T, M, D, alpha, discount_factor, epsilon, rollout_epsilon))


def uct_tables(c=3.0, size=256):
    """(U, B, I) of UCB1 in a tree (Kocsis & Szepesvari 2006): an action tried n_b times, with summed returns w_b, at a node visited
    n_s times scores w_b * I[n_b] + U[n_s] * B[n_b] = its mean return + c * sqrt(ln(n_s + 1) / n_b).  U[n] = c * sqrt(ln(n + 1)),
    B[n] = 1 / sqrt(n), I[n] = 1 / n, B[0] = I[0] = 0 (an untried action is taken first, whatever the tables say).  Counts beyond
    size - 1 use the last entry: `size` above the simulations per decision keeps every mean exact.  The rewards are not scaled to
    [0, 1] -- a step costs 1, lava 10, the goal pays 10 --, hence c of their order."""
    size, c = int(size), float(c)
    if not 2 <= size <= _lib.EXPLORE_MAX_C:
        raise ValueError('size must lie in 2 .. {}'.format(_lib.EXPLORE_MAX_C))
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError('c must be finite and not negative')
    n = np.arange(size, dtype=np.float64)
    U = c * np.sqrt(np.log(n + 1.0))
    B, I = np.zeros(size, np.float64), np.zeros(size, np.float64)
    B[1:] = 1.0 / np.sqrt(n[1:])
    I[1:] = 1.0 / n[1:]
    return U, B, I


def tree_search(env, num_steps, simulations=64, tree_depth=8, depth=4, c=3.0, alpha=0.1, discount_factor=0.99, epsilon=0.1,
                rollout_epsilon=1.0, num_learners=1, seed=0, q0=0.0):
    """Epsilon-greedy learners that choose every non-exploring action by a UCT tree and learn by Q-learning, `num_steps` real env
    steps per learner (episodes restart at a start cell when they end).  `simulations` (0 .. 255; 0 is `q_learning`) per decision,
    selection down to `tree_depth` (1 .. 64) levels, rollouts of `depth` (0 .. 256) moves under an epsilon-greedy policy on the
    learner's table (`rollout_epsilon`; 1.0 = uniformly random), UCB1 with constant `c`.  Returns Q float64[S][4], or [L][S][4]
    for L = num_learners > 1."""
    L, M, H, D = need_learners(num_learners), int(simulations), int(tree_depth), int(depth)
    if not 0 <= M <= _lib.MCTS_MAX_SIMS:
        raise ValueError('simulations must lie in 0 .. {}'.format(_lib.MCTS_MAX_SIMS))
    if not 1 <= H <= _lib.MCTS_MAX_DEPTH:
        raise ValueError('tree_depth must lie in 1 .. {}'.format(_lib.MCTS_MAX_DEPTH))
    if not 0 <= D <= _lib.SEARCH_MAX_D:
        raise ValueError('depth must lie in 0 .. {}'.format(_lib.SEARCH_MAX_D))
    unit('epsilon', epsilon)
    unit('rollout_epsilon', rollout_epsilon)
    need_steps(num_steps)
    tables = uct_tables(c, max(256, M + 1))
    return learn(env, L, seed, num_steps, max(1, _MOVES // (1 + M * (H + D))), lambda vec: (vec._ensure_q(q0), vec.set_tree_search(*tables)),
                 lambda vec, T: vec.tree_search_run(T, M, H, D, alpha, discount_factor, epsilon, rollout_epsilon))
