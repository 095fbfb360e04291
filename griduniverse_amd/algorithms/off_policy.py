"""Off-policy Monte-Carlo control with weighted importance sampling (Sutton & Barto 5.7), the second half of the reference's roadmap
entry "Off-policy control (Q-Learning, Importance Sampling)" (README.md; it ships no code for it, so the semantics are this
build's: include/gu.h, gu_is_run).  `temporal_difference.q_learning` is the first half.

`off_policy_mc_control` runs `num_learners` independent learners on the grid of a facade `GridUniverseEnv`, learner e in env e of a
batch, all advanced on the MI355X by one kernel (csrc/gu_is.hip).  A learner behaves epsilon-greedily on its own Q table and
learns the values of the GREEDY policy: when an episode ends it walks the episode backwards, weighting each return by the product
of the ratios pi / b of the actions behind it, and stops at the first action the greedy policy would not have taken.  The result
has `q_learning`'s format, so `temporal_difference.greedy_policy` turns it into a policy matrix.

The method learns from the tails of episodes only.  Where greedy runs are short compared with the episodes -- large open grids,
long `max_episode_len` -- it is slower than Q-learning; that is the textbook weakness, not a defect of this build.
"""
import numpy as np

from ..vec_env import _q16, check_off_policy_args
from ._batch import _CHUNK, learn, need_finite, need_learners, need_steps, unit


def ratio_table(epsilon):
    """float64[5, 5]: R[m][c] = pi(a|s) / b(a|s) of gu_is_run for an action that is one of m (1 .. 4) maxima of its row now and was
    one of c maxima when the epsilon-greedy behaviour took it (c = 0: none of them); row 0 is unused and zero.  The bytes are the
    ones the library computes from eps_q16 = round(epsilon * 65536) (include/gu.h)."""
    unit('epsilon', epsilon)
    eps = _q16(epsilon) / 65536.0
    R = np.zeros((5, 5), np.float64)
    for c in range(5):
        b = eps * 0.25 if c == 0 else (1.0 - eps) / c + eps * 0.25
        for m in range(1, 5):
            R[m][c] = 0.0 if b == 0 else (1.0 / m) / b
    return R


def off_policy_mc_control(env, num_steps, max_episode_len=64, discount_factor=0.99, epsilon=0.1, w_cap=2.0 ** 64, num_learners=1, seed=0,
                          q0=0.0):
    """Off-policy every-visit Monte-Carlo control with weighted importance sampling, `num_steps` env steps per learner (episodes
    restart at a start cell when they end; one still running after `max_episode_len` (1 .. 1024) steps is learned from there,
    bootstrapping on max Q, and goes on), tables of q0 and zeroed cumulative weights at the start.  A backward pass ends where
    its weight reaches `w_cap` (1 .. 2**256; small values give truncated importance sampling).  Transitions still in a learner's
    buffer after the last step are not learned from.  Returns Q float64[S][4], or [L][S][4] for L = num_learners > 1, as
    `q_learning` does."""
    need_learners(num_learners)
    need_steps(num_steps)
    check_off_policy_args(max_episode_len, epsilon, w_cap)
    need_finite(discount_factor=discount_factor, q0=q0)
    # (consecutive launches carry the episode buffer, so chunking changes nothing)
    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec._ensure_q(q0),
                 lambda vec, T: vec.off_policy_mc_run(T, max_episode_len, discount_factor, epsilon, w_cap))
