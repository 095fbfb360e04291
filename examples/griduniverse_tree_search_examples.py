"""Monte-Carlo tree search (UCT) on the MI355X engine, headless: 4096 independent learners on the default 4x4 grid, one learner per
env, all advanced by one kernel per launch.  Before every non-exploring move a learner grows a tree of 64 simulations at the cell it
stands in -- UCB1 selection down to 8 levels, one new node, a random rollout of 4 moves that bootstraps on its Q table -- and takes
the root action with the largest mean return; it learns from its real moves by Q-learning.  Prints how many episodes the learners
finished in 300 steps against plain Q-learning and against the flat rollout search on the same seeds, the root of learner 0's last
tree, and its greedy policy.

    python examples/griduniverse_tree_search_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.search import uct_tables  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy  # noqa: E402


def main():
    world_shape, learners, steps = (4, 4), 4096, 300
    env = GridUniverseEnv(grid_shape=world_shape)
    kw = dict(alpha=0.1, discount_factor=0.99, epsilon=0.1, stats=True)
    for name, run in (('plain Q-learning', lambda vec: vec.td_run(steps, 'q_learning', **kw)),
                      ('rollout search, 4 x 16', lambda vec: vec.search_run(steps, simulations=4, depth=16, **kw)),
                      ('tree search, 64 (8 + 4)', lambda vec: vec.tree_search_run(steps, simulations=64, tree_depth=8, depth=4, **kw))):
        vec = VecGridUniverse(learners, template=env, seed=7)
        try:
            vec.reset()
            vec.set_tree_search(*uct_tables(3.0))
            out = run(vec)
            print('%-24s %d steps x %d learners: %d episodes finished, mean reward per step %.3f'
                  % (name, steps, learners, int(out['episodes'].sum()), out['ret'].sum() / float(steps * learners)))
            if name.startswith('tree'):
                r, t = vec.tree_search_roots(0, 1), vec.tree_search_tree(0, 1)
                n = int(t['count'][0])
                depth = np.zeros(n, np.int64)
                for v in range(1, n):
                    depth[v] = depth[t['parent'][0, v] >> 2] + 1
                print('learner 0: %d simulated moves; its last tree has %d nodes, the deepest at level %d' % (int(r['sim_steps'][0]), n, depth.max()))
                print('visits of the root actions (up, right, down, left): %s, their mean returns: %s'
                      % (r['visits'][0], np.array2string(r['w'][0] / np.maximum(r['visits'][0], 1), precision=2)))
                print('greedy policy of learner 0:')
                utils.get_policy_map(greedy_policy(vec.q_table(0, 1)[0], env), world_shape)
        finally:
            vec.close()
    env.close()


if __name__ == '__main__':
    main()
