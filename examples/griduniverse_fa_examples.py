"""Semi-gradient SARSA with tile coding on the MI355X engine, headless: 4096 independent learners on the open 8x8 grid, one
learner per env, all advanced by one kernel per launch.  Each learner holds 36 weight rows (4 tilings of 4x4-cell tiles) instead of
a 64-row table.  Prints the greedy policy of learner 0 as arrows and how long its greedy walk to the goal is.

    python examples/griduniverse_fa_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.function_approximation import semi_gradient_sarsa, tile_coding  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy  # noqa: E402


def main():
    world_shape = (8, 8)
    env = GridUniverseEnv(grid_shape=world_shape)
    phi, n_features = tile_coding(8, 8, tilings=4, tile=4)
    print('%d states, %d active features per state, %d features' % (phi.shape[0], phi.shape[1], n_features))
    q = semi_gradient_sarsa(env, 6000, features=(phi, n_features), alpha=0.2, discount_factor=0.9, epsilon=0.2, num_learners=4096,
                            seed=5)
    policy = greedy_policy(q[0], env)
    print('greedy policy of learner 0 after 6000 steps:')
    utils.get_policy_map(policy, world_shape)
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(policy[s])))
        n += 1
    print('greedy walk from the start: %d steps, %s' % (n, 'goal reached' if env.is_terminal_goal(s) else 'goal NOT reached'))
    env.close()


if __name__ == '__main__':
    main()
