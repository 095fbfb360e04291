"""Tabular one-step actor-critic on the MI355X engine, headless: 4096 independent learners on an 11x11 maze, one learner per env,
each with its own softmax preferences and state values, all advanced by one kernel per launch.  After a fixed number of steps:
the argmax walk of learner 0 from the start, how many of the 4096 learners' argmax walks reach the goal, the arrows of learner 0's
softmax policy and its critic's value of the start state.

    python examples/griduniverse_actor_critic_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.policy_gradient import actor_critic  # noqa: E402


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
    steps, L = 10000, 4096
    pi, v = actor_critic(env, steps, actor_lr=0.1, critic_lr=0.1, discount_factor=0.99, num_learners=L, seed=1)
    walks = [argmax_walk(env, pi[e]) for e in range(L)]
    reached = sum(w is not None for w in walks)
    print('actor-critic after %d steps: learner 0 walks %s; %d of %d learners reach the goal' %
          (steps, 'to the goal in %d steps' % walks[0] if walks[0] is not None else 'nowhere', reached, L))
    print('V(start) of learner 0: %.3f' % v[0][env.starting_states[0]])
    print('softmax policy of learner 0 (actions with probability above 0):')
    utils.get_policy_map(pi[0], world_shape)
    env.close()


if __name__ == '__main__':
    main()
