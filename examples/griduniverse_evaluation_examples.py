"""Learning curves over thousands of levels, measured on the device, headless.

4096 random mazes of 8x8 cells are carved on the GPU, one per env, and one Q-learner learns on each.  Training and measuring take
turns: `td_run` advances all learners by one kernel launch, `evaluate` lets every learner walk its own table greedily from its
level's start (one more launch; nothing learns, and the envs stay where training left them).  `shortest_paths` gives the optimum of
every level by breadth-first search -- generated mazes have no lava, so the first terminal cell it reaches is the goal.

Prints, after every 500 steps of training, the share of levels whose greedy walk reaches the goal and the share whose walk is as short
as the level's shortest path.

    python examples/griduniverse_evaluation_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms.evaluation import learning_curve, success  # noqa: E402

LEVELS, EVERY, TOTAL = 4096, 500, 6000


def main():
    vec = VecGridUniverse(LEVELS, grid_shape=(8, 8), device_mazes=LEVELS, maze_seed=3, seed=0)
    paths, _ = vec.engine.shortest_paths()
    best = np.array([len(p) for p in paths])
    vec.reset()
    curve = learning_curve(vec, lambda v, T: v.td_run(T, 'q_learning', alpha=0.5, discount_factor=0.95, epsilon=0.1), TOTAL, EVERY)
    vec.close()
    print('%d levels, shortest paths of %d .. %d moves (mean %.1f)' % (LEVELS, best.min(), best.max(), best.mean()))
    print('%8s %16s %16s %12s' % ('steps', 'reach the goal', 'on a shortest', 'mean return'))
    for p, steps in enumerate(curve['steps']):
        point = {k: curve[k][p] for k in ('outcome', 'length', 'ret')}
        reached = point['outcome'][0] == 1
        shortest = reached & (point['length'][0] == best)
        assert success(point).mean() == reached.mean()
        print('%8d %15.1f%% %15.1f%% %12.2f' % (steps, 100.0 * reached.mean(), 100.0 * shortest.mean(), point['ret'][0].mean()))


if __name__ == '__main__':
    main()
