"""SARSA against Q-learning on Sutton & Barto's windy gridworld (Example 6.5, and Exercise 6.10's stochastic wind), headless: 256
independent learners of each method on the 10x7 grid, calm gusts and gusts of 2/3, all advanced by one kernel per launch.  Prints,
per method and wind, the mean reward per step of the last launch (exploration included) and how long the greedy walks to the goal
are without gusts.

Under this engine's rule the agent is pushed cell by cell and a terminal cell stops it, so the shortest path has 10 moves (15 under
the book's vector-sum rule, which can blow an agent across the goal).

    python examples/griduniverse_wind_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402

W, H = 10, 7
STRENGTH = np.array([0, 0, 0, 1, 1, 1, 2, 2, 1, 0])  # per column, blowing up
START, GOAL = 3 * W + 0, 3 * W + 7
DELTA = (-W, 1, W, -1)  # UP, RIGHT, DOWN, LEFT


def move(s, a):
    """The engine's move on this open grid: the border stops it, the goal absorbs."""
    if s == GOAL:
        return s
    x, y = s % W, s // W
    if (a == 0 and y == 0) or (a == 1 and x == W - 1) or (a == 2 and y == H - 1) or (a == 3 and x == 0):
        return s
    return s + DELTA[a]


def greedy_walk(q, limit=100):
    """Moves of the greedy policy of q from the start to the goal without gusts (None: not within `limit`)."""
    s = START
    for n in range(1, limit + 1):
        k = int(STRENGTH[s % W])
        s = move(s, int(np.argmax(q[s])))
        for _ in range(k):
            s = move(s, 0)
        if s == GOAL:
            return n
    return None


def main():
    env = GridUniverseEnv(grid_shape=(W, H), initial_state=START, goal_states=[GOAL])
    L, launches, T = 256, 8, 2000
    for gust in (0.0, 2.0 / 3.0):
        for method in ('sarsa', 'q_learning'):
            vec = VecGridUniverse(L, template=env, seed=1)
            vec.set_wind(STRENGTH, 'up', gust)
            vec.reset()
            for _ in range(launches):
                out = vec.td_run(T, method, alpha=0.5, discount_factor=0.99, epsilon=0.1, stats=True)
            q = vec.q_table()
            vec.close()
            walks = [greedy_walk(q[e]) for e in range(L)]
            found = [n for n in walks if n is not None]
            print('%-10s gust %.2f: reward per step %.3f in the last %d steps; greedy walks reach the goal for %d of %d learners, '
                  'median %s moves (shortest: 10)' % (method, gust, out['ret'].sum() / (L * T), T, len(found), L,
                                                      int(np.median(found)) if found else '-'))
    env.close()


if __name__ == '__main__':
    main()
