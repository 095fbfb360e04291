"""Exploration against exploitation: UCB and Thompson-style action selection on visit counts -- the last entry of the reference's
roadmap, "Exploration vs Exploitation (Optimistic policy, optimistic policy with uncertainty, Thompson sampling, UCB)" (README.md
"GridUniverse features and plans"; it ships no code for it, so the semantics are this build's: include/gu.h, gu_explore_run).
"Optimistic policy" is the `q0` of every learner here.

`ucb_q_learning` / `thompson_q_learning` run `num_learners` independent Q-learners on the grid of a facade `GridUniverseEnv`,
learner e in env e of a batch, each with its own float64 Q table and its own uint32 visit counts, all advanced on the MI355X by one
kernel (csrc/gu_explore.hip).  A learner takes the action that maximises Q[s][b] + bonus_b (UCB) or Q[s][b] + bonus_b * z_b with
z_b an approximate standard normal (Thompson); the bonus is U[n_s] * B[n_b] for the visits n_s of the state and n_b of the pair.
The schedule is data: `ucb_tables` and `thompson_tables` build the two usual ones on the host, and any pair of non-negative
vectors can be installed with `VecGridUniverse.set_exploration`.  The results have the shape of `q_learning`'s and feed
`greedy_policy` the same way.
"""
import numpy as np

from .. import _lib
from ._batch import _CHUNK, learn, need_learners, need_steps, unit

IRWIN_HALL_VARIANCE = 21845.0  # of the sum of four uniform bytes, 4 * (256 ** 2 - 1) / 12: the kernel's z_b before scaling


def _size(size):
    size = int(size)
    if not 2 <= size <= _lib.EXPLORE_MAX_C:
        raise ValueError('size must lie in 2 .. {}'.format(_lib.EXPLORE_MAX_C))
    return size


def ucb_tables(c=1.0, size=1024):
    """(U, B) of UCB1 (Sutton & Barto 2.7): bonus = c * sqrt(ln n_s / n_b).  U[k] = c * sqrt(ln max(k, 2)); B[0] = 1e6 (an untried
    action goes first), B[n] = 1 / sqrt(n).  Counts beyond size - 1 use the last entry."""
    size, c = _size(size), float(c)
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError('c must be finite and not negative')
    k = np.arange(size, dtype=np.float64)
    U = c * np.sqrt(np.log(np.maximum(k, 2.0)))
    B = np.empty(size, np.float64)
    B[0] = 1e6
    B[1:] = 1.0 / np.sqrt(k[1:])
    return U, B


def thompson_tables(sigma=1.0, size=1024):
    """(U, B) of Gaussian Thompson sampling: score_b = Q[s][b] + sigma / sqrt(n_b + 1) * z_b, z_b approximately standard normal.
    U = 1; B[n] = sigma / sqrt(21845) / sqrt(n + 1): the kernel's variate has variance 21845."""
    size, sigma = _size(size), float(sigma)
    if not (np.isfinite(sigma) and sigma >= 0.0):
        raise ValueError('sigma must be finite and not negative')
    n = np.arange(size, dtype=np.float64)
    return np.ones(size, np.float64), sigma / np.sqrt(IRWIN_HALL_VARIANCE) / np.sqrt(n + 1.0)


def _explore(rule, tables, env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0):
    need_learners(num_learners)
    unit('epsilon', epsilon)
    need_steps(num_steps)
    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: (vec._ensure_q(q0), vec.set_exploration(*tables)),
                 lambda vec, T: vec.explore_run(T, rule, alpha, discount_factor, epsilon))


def ucb_q_learning(env, num_steps, c=1.0, table_size=1024, alpha=0.1, discount_factor=0.99, epsilon=0.0, num_learners=1, seed=0, q0=0.0):
    """Q-learning that takes the action maximising Q[s][b] + c * sqrt(ln n_s / n_b) (untried actions first), `num_steps` env steps
    per learner (episodes restart at a start cell when they end); `epsilon` adds uniform exploration on top.  Returns Q
    float64[S][4], or [L][S][4] for L = num_learners > 1.  With c = 0 it is `q_learning`."""
    return _explore('ucb', ucb_tables(c, table_size), env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0)


def thompson_q_learning(env, num_steps, sigma=1.0, table_size=1024, alpha=0.1, discount_factor=0.99, epsilon=0.0, num_learners=1, seed=0,
                        q0=0.0):
    """Q-learning that takes the action maximising a draw Q[s][b] + sigma / sqrt(n_b + 1) * z_b, z_b approximately standard
    normal; arguments and result as `ucb_q_learning`.  With sigma = 0 it is `q_learning`."""
    return _explore('thompson', thompson_tables(sigma, table_size), env, num_steps, alpha, discount_factor, epsilon, num_learners, seed, q0)
