"""Fruit, headless: a melon worth +8 off the straight path and a lemon worth -8 on it, on a 5x3 open grid with the start at (0, 1) and
the goal at (4, 1).  The optimal walk leaves the middle row, eats the melon, avoids the lemon and returns 13 in six moves; the
straight walk returns -1.  256 independent Q-learners, all advanced by one kernel per launch, learn on the rows of (cell, eaten):
their tables have S << F = 60 rows.  Prints how many learners walk greedily to the optimal return after each launch, and what a
uniformly random batch eats.

    python examples/griduniverse_fruit_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402

W, H = 5, 3
S = W * H
START, GOAL = 1 * W + 0, 1 * W + 4
CELLS, KINDS, VALUES = [2, 7], ['melon', 'lemon'], (0, -8, 8)  # (2, 0) and (2, 1); values of apple, lemon, melon
FRUIT = {2: (0, 8), 7: (1, -8)}  # cell: (slot, value) -- slots go by ascending cell index
DELTA = ((0, -1), (1, 0), (0, 1), (-1, 0))  # UP, RIGHT, DOWN, LEFT


def step(s, eaten, a):
    """The engine's rule on this grid: (s', eaten', r, done)."""
    x, y = s % W + DELTA[a][0], s // W + DELTA[a][1]
    s2 = y * W + x if 0 <= x < W and 0 <= y < H else s
    r = 10 if s2 == GOAL else -1
    if s2 in FRUIT and not (eaten >> FRUIT[s2][0]) & 1:
        r += FRUIT[s2][1]
        eaten |= 1 << FRUIT[s2][0]
    return s2, eaten, r, s2 == GOAL


def greedy_return(q, limit=50):
    """The undiscounted return of the greedy walk of one table q [S << 2][4] (None: no goal within `limit` moves)."""
    s, eaten, total = START, 0, 0
    for _ in range(limit):
        s, eaten, r, done = step(s, eaten, int(np.argmax(q[eaten * S + s])))
        total += r
        if done:
            return total
    return None


def main():
    env = GridUniverseEnv(grid_shape=(W, H), initial_state=START, goal_states=[GOAL])
    L, T = 256, 100
    vec = VecGridUniverse(L, template=env, seed=1)
    vec.set_fruit(CELLS, KINDS, VALUES)
    print('fruit:', vec.fruit())
    vec.reset()
    for launch in range(1, 9):
        out = vec.td_run(T, 'q_learning', alpha=0.5, discount_factor=0.95, epsilon=0.1, stats=True)
        q = vec.q_table()  # [L, 60, 4]
        best = sum(greedy_return(q[e]) == 13 for e in range(L))
        print('after %4d steps: %3d of %d learners walk greedily to the optimal return 13; reward per step %.3f' % (launch * T, best, L, out['ret'].sum() / (L * T)))
    vec.reset()
    out = vec.rollout(20, 'uniform', auto_reset=False)
    eaten = vec.fruit_eaten()
    print('20 uniformly random steps: %d of %d envs ate the melon, %d the lemon; rewards seen: %s' % (
        int((eaten & 1).sum()), L, int((eaten >> 1 & 1).sum()), sorted(set(out['reward'].ravel().tolist()))))
    vec.close()
    env.close()


if __name__ == '__main__':
    main()
