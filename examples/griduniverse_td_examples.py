"""Tabular Q-learning on the MI355X engine, headless: 4096 independent learners on an 11x11 maze, one learner per env, all
advanced by one kernel per launch.  Prints the greedy policy of learner 0 as arrows and how long its greedy walk to the goal is.

    python examples/griduniverse_td_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy, q_learning  # noqa: E402


def main():
    random.seed(0)  # the maze generator draws from the stdlib's global stream, like the reference's
    world_shape = (11, 11)
    env = GridUniverseEnv(grid_shape=world_shape, random_maze=True)
    q = q_learning(env, 20000, alpha=0.2, discount_factor=0.99, epsilon=0.1, num_learners=4096, seed=1)
    policy = greedy_policy(q[0], env)
    print('greedy policy of learner 0 after 20 000 steps:')
    utils.get_policy_map(policy, world_shape)
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(policy[s])))
        n += 1
    print('greedy walk from the start: %d steps, %s' % (n, 'goal reached' if env.is_terminal_goal(s) else 'goal NOT reached'))
    env.close()


if __name__ == '__main__':
    main()
