"""Doors and keys, headless: a 7x3 grid cut in two by the column x = 4 -- walls above and below, a door in the middle --, the key of the
door at (2, 0), off the straight line from the start (0, 1) to the goal (6, 1).  The shortest walk fetches the key first: three
moves to the key, three to the door, two to the goal, return 3.  64 independent Q-learners, all advanced by one kernel per launch,
learn on the rows of (cell, mask of open slots): their tables have S << D = 42 rows.  Prints how many learners walk greedily along a
shortest walk after each launch, and the greedy walk of the first learner with the mask along it.

    python examples/griduniverse_doors_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402

W, H = 7, 3
S = W * H
START, GOAL, WALLS = 7, 13, [4, 18]
DOOR, KEY = 11, 2  # slot 0
DELTA = ((0, -1), (1, 0), (0, 1), (-1, 0))  # UP, RIGHT, DOWN, LEFT
NAMES = ('UP', 'RIGHT', 'DOWN', 'LEFT')


def step(s, mask, a):
    """The engine's rule on this grid: (s', mask', r, done)."""
    x, y = s % W + DELTA[a][0], s // W + DELTA[a][1]
    c = y * W + x if 0 <= x < W and 0 <= y < H else s
    if c in WALLS or (c == DOOR and not mask & 1):
        c = s
    if c != s and c == KEY:
        mask |= 1
    return c, mask, 10 if c == GOAL else -1, c == GOAL


def greedy_walk(q, limit=50):
    """[(cell, mask, action)] of the greedy walk of one table q [S << 1][4], and its return (None: no goal within `limit` moves)."""
    s, mask, total, walk = START, 0, 0, []
    for _ in range(limit):
        a = int(np.argmax(q[mask * S + s]))
        walk.append((s, mask, NAMES[a]))
        s, mask, r, done = step(s, mask, a)
        total += r
        if done:
            return walk, total
    return walk, None


def main():
    env = GridUniverseEnv(grid_shape=(W, H), initial_state=START, goal_states=[GOAL], walls=WALLS)
    L, T = 64, 200
    vec = VecGridUniverse(L, template=env, seed=1)
    vec.set_doors({0: DOOR}, keys={0: KEY})
    print('doors:', vec.doors())
    vec.reset()
    for launch in range(1, 8):
        out = vec.td_run(T, 'q_learning', alpha=0.5, discount_factor=0.95, epsilon=0.1, stats=True)
        q = vec.q_table()  # [L, 42, 4]
        walks = [greedy_walk(q[e]) for e in range(L)]
        best = sum(total == 3 and len(walk) == 8 for walk, total in walks)
        print('after %4d steps: %2d of %d learners walk greedily along a shortest walk (8 moves, return 3); reward per step %.3f' % (
            launch * T, best, L, out['ret'].sum() / (L * T)))
    walk, total = greedy_walk(vec.q_table(0, 1)[0])
    print('learner 0, greedy: ' + ' '.join('%d/%d:%s' % w for w in walk) + ' -> return %s   (cell/mask:action)' % total)
    print('masks of the learners now:', np.bincount(vec.doors_open(), minlength=2).tolist(), '(closed, open)')
    vec.close()
    env.close()


if __name__ == '__main__':
    main()
