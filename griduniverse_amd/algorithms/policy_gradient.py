"""Tabular policy gradients with a softmax policy: one-step actor-critic (Sutton & Barto 13.5) and REINFORCE with baseline, the
Monte-Carlo policy gradient (13.3/13.4) -- "Policy Gradients (MC Policy Gradients and Actor-critic)" on the reference's roadmap
(README.md "GridUniverse features and plans"; it ships no code for either, so the semantics are this build's: include/gu.h,
gu_ac_run and gu_reinforce_run).

`actor_critic` runs `num_learners` independent learners on the grid of a facade `GridUniverseEnv`, learner e in env e of a
batch, each with its own float64 preferences H[S][4] (the actor) and state values V[S] (the critic), all advanced on the MI355X by
one kernel (csrc/gu_ac.hip).  The facade's own state is left alone.  The returned policy is the softmax of the learned
preferences in the reference's policy-matrix format, so it feeds `get_policy_map`, and `engine.vi_set` with
`rollout(policy='sample')`, like a policy from dynamic programming.

`reinforce` does the same with whole-episode returns (csrc/gu_reinforce.hip): a learner updates its tables in a backward pass
when its episode ends, or after `max_episode_len` steps, where the return bootstraps on the baseline V.
"""
import numpy as np

from ..vec_env import VecGridUniverse

_CHUNK = 100000  # steps per launch (the launch limit is 1e8; shorter launches keep the device responsive)
_REINFORCE_MAX = 1024  # GU_REINFORCE_MAX


def actor_critic(env, num_steps, actor_lr=0.1, critic_lr=0.1, discount_factor=0.99, num_learners=1, seed=0):
    """One-step actor-critic, `num_steps` env steps per learner (episodes restart at a start cell when they end), tables of
    zeros at the start.  Returns (policy, V): the softmax policy float64[S][4] with the rows of terminal states zero, and the
    critic's values float64[S]; [L][S][4] and [L][S] for L = num_learners > 1."""
    L = int(num_learners)
    if L < 1:
        raise ValueError('num_learners must be at least 1')
    if int(num_steps) < 0:
        raise ValueError('num_steps must not be negative')
    for name, x in (('actor_lr', actor_lr), ('critic_lr', critic_lr), ('discount_factor', discount_factor)):
        if not np.isfinite(float(x)):
            raise ValueError('{} must be finite'.format(name))
    vec = VecGridUniverse(L, template=env, seed=seed)
    try:
        vec._ensure_ac(0.0, 0.0)
        vec.reset()
        left = int(num_steps)
        while left > 0:  # (the learner carries nothing from one launch to the next, so chunking changes nothing)
            T = min(left, _CHUNK)
            vec.actor_critic_run(T, actor_lr, critic_lr, discount_factor)
            left -= T
        policy, v = vec.softmax_policy(), vec.state_values()
    finally:
        vec.close()
    terminal = np.array([bool(env.is_terminal(s)) for s in range(env.world.size)])
    policy[:, terminal] = 0.0
    return (policy[0], v[0]) if L == 1 else (policy, v)


def reinforce(env, num_steps, max_episode_len=256, actor_lr=0.003, baseline_lr=0.1, discount_factor=0.99, num_learners=1, seed=0):
    """REINFORCE with baseline, `num_steps` env steps per learner (episodes restart at a start cell when they end; one still
    running after `max_episode_len` steps is learned from there and goes on), tables of zeros at the start.  Transitions still
    in a learner's buffer after the last step are not learned from.  Returns (policy, V) in `actor_critic`'s format, V being the
    baseline.  The default rates are small on purpose: an update is scaled by a whole-episode return, not by a one-step error."""
    L = int(num_learners)
    if L < 1:
        raise ValueError('num_learners must be at least 1')
    if int(num_steps) < 0:
        raise ValueError('num_steps must not be negative')
    if not 1 <= int(max_episode_len) <= _REINFORCE_MAX:
        raise ValueError('max_episode_len must lie in 1 .. {}'.format(_REINFORCE_MAX))
    for name, x in (('actor_lr', actor_lr), ('baseline_lr', baseline_lr), ('discount_factor', discount_factor)):
        if not np.isfinite(float(x)):
            raise ValueError('{} must be finite'.format(name))
    vec = VecGridUniverse(L, template=env, seed=seed)
    try:
        vec._ensure_ac(0.0, 0.0)
        vec.reset()
        left = int(num_steps)
        while left > 0:  # (consecutive launches carry the episode buffer, so chunking changes nothing)
            T = min(left, _CHUNK)
            vec.reinforce_run(T, max_episode_len, actor_lr, baseline_lr, discount_factor)
            left -= T
        policy, v = vec.softmax_policy(), vec.state_values()
    finally:
        vec.close()
    terminal = np.array([bool(env.is_terminal(s)) for s in range(env.world.size)])
    policy[:, terminal] = 0.0
    return (policy[0], v[0]) if L == 1 else (policy, v)
