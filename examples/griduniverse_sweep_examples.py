"""Prioritized sweeping on the MI355X engine, headless: 4096 independent learners on the 11x11 maze level, one learner per env, each
with its own Q table, its own learned model of the maze and its own priority queue, all advanced by one kernel per launch.  At the
same small planning budget (5 updates per real step) prioritized sweeping is set against Dyna-Q, which replays uniformly drawn
pairs: after 250 to 2000 real steps, where the greedy walk of learner 0 leads and how many of the first 256 learners walk to the
goal, and how fast.  Then a look into learner 0's queue.

    python examples/griduniverse_sweep_examples.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.dyna import dyna_q, prioritized_sweeping  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy  # noqa: E402


def maze_11x11():
    with open(os.path.join(ROOT, 'tests', 'golden', 'levels.json')) as f:
        level = json.load(f)['maze_11x11.txt']
    return GridUniverseEnv(grid_shape=(level['W'], level['H']), initial_state=level['starts'][0], goal_states=level['goals'],
                           lava_states=level['lava'], walls=level['walls'])


def greedy_walk(env, q):
    """Steps of the greedy walk from the start to the goal, or None when it does not get there."""
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(q[s])))
        n += 1
    return n if env.is_terminal_goal(s) else None


def main():
    env = maze_11x11()
    L, P = 4096, 5
    kw = dict(planning_steps=P, alpha=0.5, discount_factor=0.95, epsilon=0.1, num_learners=L, seed=1)
    learners = {'prioritized sweeping': lambda steps: prioritized_sweeping(env, steps, theta=1e-4, **kw),
                'Dyna-Q': lambda steps: dyna_q(env, steps, **kw)}
    look = 256  # learners whose greedy walks are taken
    for steps in (250, 500, 1000, 2000):
        for name, learn in learners.items():
            q = learn(steps)
            walks = [greedy_walk(env, q[e]) for e in range(look)]
            found = [w for w in walks if w is not None]
            print('%s, %d updates per step, after %d real steps: learner 0 walks %s; %d of the first %d learners reach the goal%s' %
                  (name, P, steps, 'to the goal in %d steps' % walks[0] if walks[0] is not None else 'nowhere', len(found), look,
                   ', %d of them in %d steps, the fewest' % (found.count(min(found)), min(found)) if found else ''))
    print('greedy policy of prioritized-sweeping learner 0:')
    utils.get_policy_map(greedy_policy(learners['prioritized sweeping'](2000)[0], env), (11, 11))
    # the queue itself: 64 learners, a few hundred real steps in
    vec = VecGridUniverse(64, template=env, seed=1)
    try:
        vec.reset()
        for _ in range(4):
            vec.sweep_run(100, P, theta=1e-4, alpha=0.5, discount_factor=0.95, epsilon=0.1)
            queue = vec.priority_queue()
            pr = queue['priority'][0].reshape(-1)
            top = np.argsort(-pr)[:3]
            print('learner 0 holds %3d pairs (the 64 learners: %d .. %d); its top three (state, action, priority): %s' %
                  (queue['size'][0], queue['size'].min(), queue['size'].max(),
                   ', '.join('(%d, %d, %.3g)' % (p >> 2, p & 3, pr[p]) for p in top if pr[p] > 0) or 'none'))
    finally:
        vec.close()
    env.close()


if __name__ == '__main__':
    main()
