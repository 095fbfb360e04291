"""Off-policy Monte-Carlo control with weighted importance sampling (Sutton & Barto 5.7) on the MI355X engine, headless: 4096
independent learners on the default 4x4 grid and on an 11x11 maze, one learner per env, each behaving epsilon-greedily on its own Q
table and learning the greedy policy's values from whole-episode returns weighted by the importance ratio, all advanced by one
kernel per launch.  Q-learning runs beside it with the same seeds.  After a fixed number of steps: how many learners' greedy
walks reach the goal, and the greedy policy of the first that does.  On the maze, where a greedy run is short compared with an
episode, the method learns from the tails of its episodes only and Q-learning is ahead: the textbook weakness.

    python examples/griduniverse_offpolicy_examples.py
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv  # noqa: E402
from griduniverse_amd.algorithms import utils  # noqa: E402
from griduniverse_amd.algorithms.off_policy import off_policy_mc_control, ratio_table  # noqa: E402
from griduniverse_amd.algorithms.temporal_difference import greedy_policy, q_learning  # noqa: E402


def greedy_walk(env, q):
    """Steps of the walk that takes the first greedy action from the start to the goal, or None when it does not get there."""
    s, n = env.starting_states[0], 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(q[s])))
        n += 1
    return n if env.is_terminal_goal(s) else None


def report(name, env, q, steps):
    walks = [greedy_walk(env, q[e]) for e in range(len(q))]
    reached = sum(w is not None for w in walks)
    best = next((e for e, w in enumerate(walks) if w is not None), 0)
    print('%s after %d steps: %d of %d learners reach the goal; learner %d walks %s' %
          (name, steps, reached, len(q), best, 'to the goal in %d steps' % walks[best] if walks[best] is not None else 'nowhere'))
    return best


def main():
    random.seed(0)  # the maze generator draws from the global streams, like the reference's
    np.random.seed(0)
    print('importance ratios pi/b at epsilon 0.1, rows m = 1..4 (maxima now), columns c = 0..4 (maxima at action time):')
    print(np.array2string(ratio_table(0.1)[1:], precision=4))
    L = 4096
    for title, env, shape, steps in (('default 4x4 grid', GridUniverseEnv(grid_shape=(4, 4)), (4, 4), 500),
                                     ('11x11 maze', GridUniverseEnv(grid_shape=(11, 11), random_maze=True), (11, 11), 20000)):
        print('--- ' + title)
        q_mc = off_policy_mc_control(env, steps, max_episode_len=64, discount_factor=0.9, epsilon=0.1, num_learners=L, seed=1)
        q_td = q_learning(env, steps, alpha=0.1, discount_factor=0.9, epsilon=0.1, num_learners=L, seed=1)
        best = report('off-policy Monte-Carlo control', env, q_mc, steps)
        report('Q-learning', env, q_td, steps)
        print('greedy policy of off-policy Monte-Carlo learner %d:' % best)
        utils.get_policy_map(greedy_policy(q_mc[best], env), shape)
        env.close()


if __name__ == '__main__':
    main()
