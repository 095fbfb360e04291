"""Simulation-based search on the MI355X engine, headless: 4096 independent learners on the open 8x8 grid, one learner per env, all
advanced by one kernel per launch.  Before every non-exploring move a learner simulates 4 random rollouts of 16 moves per action
with the true model and takes the action whose rollouts returned the most; it learns from its real moves by Q-learning.  Prints
how many episodes the learners finished in 300 steps against plain Q-learning on the same seeds, the score row behind learner 0's
last searched move, and its greedy policy.

    python examples/griduniverse_search_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy  # noqa: E402


def main():
    world_shape, learners, steps = (8, 8), 4096, 300
    env = GridUniverseEnv(grid_shape=world_shape)
    kw = dict(alpha=0.1, discount_factor=0.99, epsilon=0.1, stats=True)
    for name, run in (('plain Q-learning', lambda vec: vec.td_run(steps, 'q_learning', **kw)),
                      ('rollout search, 4 x 16', lambda vec: vec.search_run(steps, simulations=4, depth=16, **kw))):
        vec = VecGridUniverse(learners, template=env, seed=7)
        try:
            vec.reset()
            out = run(vec)
            print('%-24s %d steps x %d learners: %d episodes finished, mean reward per step %.3f'
                  % (name, steps, learners, int(out['episodes'].sum()), out['ret'].sum() / float(steps * learners)))
            if name.startswith('rollout'):
                s = vec.search_scores(0, 1)
                print('learner 0: %d simulated moves; summed returns of its last searched move (up, right, down, left): %s'
                      % (int(s['sim_steps'][0]), np.array2string(s['score'][0], precision=2)))
                print('greedy policy of learner 0:')
                utils.get_policy_map(greedy_policy(vec.q_table(0, 1)[0], env), world_shape)
        finally:
            vec.close()
    env.close()


if __name__ == '__main__':
    main()
