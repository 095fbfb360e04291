"""Tabular REINFORCE with baseline (Monte-Carlo policy gradient) on the MI355X engine, headless: 4096 independent learners on an
11x11 maze, one learner per env, each with its own softmax preferences and its own baseline, all advanced by one kernel per
launch.  A learner updates its tables in a backward pass over its episode when the episode ends, or after `max_episode_len`
steps.  After a fixed number of steps: how many of the 4096 learners' argmax walks reach the goal, and for the first
learner whose walk does, its length, the most probable action per state and the baseline's value of the start state.

    python examples/griduniverse_reinforce_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.policy_gradient import reinforce  # noqa: E402


def argmax_walk(env, pi):
    """Steps of the walk that takes the most probable action from the start to the goal, or None when it does not get there."""
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(pi[s])))
        n += 1
    return n if env.is_terminal_goal(s) else None


def main():
    random.seed(0)  # the maze generator draws from the global streams, like the reference's
    np.random.seed(0)
    world_shape = (11, 11)
    env = GridUniverseEnv(grid_shape=world_shape, random_maze=True)
    steps, L = 40000, 4096
    pi, v = reinforce(env, steps, max_episode_len=256, actor_lr=0.003, baseline_lr=0.1, discount_factor=0.99, num_learners=L, seed=1)
    walks = [argmax_walk(env, pi[e]) for e in range(L)]
    reached = sum(w is not None for w in walks)
    best = next((e for e, w in enumerate(walks) if w is not None), 0)  # the first learner whose walk arrives
    print('REINFORCE with baseline after %d steps: %d of %d learners reach the goal; learner %d walks %s' %
          (steps, reached, L, best, 'to the goal in %d steps' % walks[best] if walks[best] is not None else 'nowhere'))
    print('V(start) of learner %d: %.3f' % (best, v[best][env.starting_states[0]]))
    print('most probable action per state of learner %d (a softmax gives every action a probability above 0):' % best)
    top = np.zeros_like(pi[best])
    live = pi[best].sum(axis=1) > 0  # (the rows of terminal states are zero)
    top[np.flatnonzero(live), pi[best][live].argmax(axis=1)] = 1.0
    utils.get_policy_map(top, world_shape)
    env.close()


if __name__ == '__main__':
    main()
