"""Tabular SARSA(lambda) on the MI355X engine, headless: 4096 independent learners on an 11x11 maze, one learner per env, each with
its own Q table and its own trace window, all advanced by one kernel per launch.  After the same small number of steps,
SARSA(lambda) with lambda = 0.9 and traces of 32 steps is set against one-step SARSA: the greedy walk of learner 0 from the start,
and how many of the 4096 learners already walk to the goal.  Eligibility traces carry each TD error back along the recent path
instead of one state.

    python examples/griduniverse_lambda_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy, sarsa, sarsa_lambda  # noqa: E402


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
    kw = dict(alpha=0.1, discount_factor=0.9, epsilon=0.1, num_learners=L, seed=1)
    results = {'SARSA(lambda = 0.9, 32 steps)': sarsa_lambda(env, steps, lam=0.9, trace_len=32, **kw), 'one-step SARSA': sarsa(env, steps, **kw)}
    for name, q in results.items():
        walks = [greedy_walk(env, q[e]) for e in range(L)]
        reached = sum(w is not None for w in walks)
        print('%s after %d steps: learner 0 walks %s; %d of %d learners reach the goal' %
              (name, steps, 'to the goal in %d steps' % walks[0] if walks[0] is not None else 'nowhere', reached, L))
    print('greedy policy of SARSA(lambda) learner 0:')
    utils.get_policy_map(greedy_policy(results['SARSA(lambda = 0.9, 32 steps)'][0], env), world_shape)
    env.close()


if __name__ == '__main__':
    main()
