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

from .. import _lib
from ._batch import _CHUNK, learn, need_finite, need_learners, need_steps


def _softmax_learner(env, num_learners, seed, num_steps, launch):
    """What actor_critic and reinforce share: tables of zeros, `launch` in chunks (the learners carry nothing, or their episode buffer,
    from one launch to the next, so chunking changes nothing), and the result (policy, V) with the rows of terminal states zero."""
    terminal = np.array([bool(env.is_terminal(s)) for s in range(env.world.size)])

    def read(vec):
        policy = vec.softmax_policy()
        policy[:, terminal] = 0.0
        return policy, vec.state_values()

    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec._ensure_ac(0.0, 0.0), launch, read)


def actor_critic(env, num_steps, actor_lr=0.1, critic_lr=0.1, discount_factor=0.99, num_learners=1, seed=0):
    """One-step actor-critic, `num_steps` env steps per learner (episodes restart at a start cell when they end), tables of
    zeros at the start.  Returns (policy, V): the softmax policy float64[S][4] with the rows of terminal states zero, and the
    critic's values float64[S]; [L][S][4] and [L][S] for L = num_learners > 1."""
    need_learners(num_learners)
    need_steps(num_steps)
    need_finite(actor_lr=actor_lr, critic_lr=critic_lr, discount_factor=discount_factor)
    return _softmax_learner(env, num_learners, seed, num_steps, lambda vec, T: vec.actor_critic_run(T, actor_lr, critic_lr, discount_factor))


def reinforce(env, num_steps, max_episode_len=256, actor_lr=0.003, baseline_lr=0.1, discount_factor=0.99, num_learners=1, seed=0):
    """REINFORCE with baseline, `num_steps` env steps per learner (episodes restart at a start cell when they end; one still
    running after `max_episode_len` steps is learned from there and goes on), tables of zeros at the start.  Transitions still
    in a learner's buffer after the last step are not learned from.  Returns (policy, V) in `actor_critic`'s format, V being the
    baseline.  The default rates are small on purpose: an update is scaled by a whole-episode return, not by a one-step error."""
    need_learners(num_learners)
    need_steps(num_steps)
    if not 1 <= int(max_episode_len) <= _lib.REINFORCE_MAX:
        raise ValueError('max_episode_len must lie in 1 .. {}'.format(_lib.REINFORCE_MAX))
    need_finite(actor_lr=actor_lr, baseline_lr=baseline_lr, discount_factor=discount_factor)
    return _softmax_learner(env, num_learners, seed, num_steps,
                            lambda vec, T: vec.reinforce_run(T, max_episode_len, actor_lr, baseline_lr, discount_factor))
