"""Exploration against exploitation on the MI355X engine, headless: 4096 independent Q-learners on the open 8x8 grid, one learner
per env, all advanced by one kernel per launch.  Each learner keeps visit counts beside its Q table and chooses its actions by
UCB (Q + c * sqrt(ln n_s / n_b), untried actions first) or by Thompson-style sampling (Q + sigma / sqrt(n_b + 1) * a normal draw),
without any epsilon.  Prints how many of the 252 state-action pairs the learners have tried after 500 steps against plain
epsilon-greedy Q-learning on the same seeds, and the greedy policy that learner 0 has after 20 000 steps of UCB.

    python examples/griduniverse_exploration_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.exploration import thompson_tables, ucb_q_learning, ucb_tables  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy  # noqa: E402


def main():
    world_shape, learners, steps = (8, 8), 4096, 500
    env = GridUniverseEnv(grid_shape=world_shape)
    kw = dict(alpha=0.1, discount_factor=0.99, stats=True)
    zero = (np.zeros(2), np.zeros(2))  # tables of zeros: explore_run is plain Q-learning that also counts its visits
    for name, rule, tables, epsilon in (('epsilon-greedy, 0.1', 'ucb', zero, 0.1), ('UCB, c = 1', 'ucb', ucb_tables(1.0), 0.0),
                                        ('Thompson, sigma = 1', 'thompson', thompson_tables(1.0), 0.0)):
        vec = VecGridUniverse(learners, template=env, seed=7)
        try:
            vec.set_exploration(*tables)
            vec.reset()
            out = vec.explore_run(steps, rule, epsilon=epsilon, **kw)
            tried = (vec.visit_counts() != 0).sum(axis=(1, 2))
            print('%-22s %d steps x %d learners: pairs tried mean %.1f, least %d of %d; %d episodes finished'
                  % (name, steps, learners, tried.mean(), tried.min(), 4 * (env.world.size - 1), int(out['episodes'].sum())))
        finally:
            vec.close()
    q = ucb_q_learning(env, 20000, c=1.0, seed=7)
    print('greedy policy of one UCB learner after 20000 steps:')
    utils.get_policy_map(greedy_policy(q, env), world_shape)
    env.close()


if __name__ == '__main__':
    main()
