"""Tabular n-step SARSA on the MI355X engine, headless: 4096 independent learners on an 11x11 maze, one learner per env, each with
its own Q table, all advanced by one kernel per launch.  After the same small number of steps, n-step SARSA with n = 8 is set
against one-step SARSA (n = 1): the greedy walk of learner 0 from the start, and how many of the 4096 learners already walk to
the goal.  n-step returns carry the reward back n states per update instead of one.

    python examples/griduniverse_nstep_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy, n_step_sarsa  # noqa: E402


def greedy_walk(env, q):
    """Steps of the greedy walk from the start to the goal, or None when it does not get there."""
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(q[s])))
        n += 1
    return n if env.is_terminal_goal(s) else None


def main():
    random.seed(0)  # the maze generator draws from the global streams, like the reference's
    np.random.seed(0)
    world_shape = (11, 11)
    env = GridUniverseEnv(grid_shape=world_shape, random_maze=True)
    steps, L = 3000, 4096
    results = {n: n_step_sarsa(env, steps, n=n, alpha=0.1, discount_factor=0.9, epsilon=0.1, num_learners=L, seed=1) for n in (8, 1)}
    for n, q in results.items():
        walks = [greedy_walk(env, q[e]) for e in range(L)]
        reached = sum(w is not None for w in walks)
        print('%d-step SARSA after %d steps: learner 0 walks %s; %d of %d learners reach the goal' %
              (n, steps, 'to the goal in %d steps' % walks[0] if walks[0] is not None else 'nowhere', reached, L))
    print('greedy policy of 8-step SARSA learner 0:')
    utils.get_policy_map(greedy_policy(results[8][0], env), world_shape)
    env.close()


if __name__ == '__main__':
    main()
