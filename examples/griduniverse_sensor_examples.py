"""Agent sensors on the MI355X engine, headless: what an agent on the 11x11 maze sees at radius 1 and 2, and what seeing costs a
learner.  256 independent semi-gradient Q-learners run on the maze with the view as their ONLY feature: at radius 1 many cells
look alike (27 distinct views over 49 free cells) and share one weight row, at radius 3 every free cell looks different, and
`one_hot` is the tabular learner.  Prints the episodes each kind finished in the same number of steps.

    python examples/griduniverse_sensor_examples.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402
from griduniverse_amd.algorithms import view_features  # noqa: E402
from griduniverse_amd.algorithms.function_approximation import one_hot  # noqa: E402

GLYPHS = np.array(list('.#LG '))  # ground, wall, lava, goal, outside the grid


def maze_11x11():
    with open(os.path.join(ROOT, 'tests', 'golden', 'levels.json')) as f:
        level = json.load(f)['maze_11x11.txt']
    return GridUniverseEnv(grid_shape=(level['W'], level['H']), initial_state=level['starts'][0], goal_states=level['goals'],
                           lava_states=level['lava'], walls=level['walls'])


def show(view):
    for row in GLYPHS[view]:
        print('    ' + ' '.join(row))


def main():
    env = maze_11x11()
    vec = VecGridUniverse(4, template=env, seed=2)
    vec.reset()
    vec.rollout(25, trajectory=False)
    print('env 0 stands on cell %d and sees, at radius 1 and 2 (itself at the centre):' % vec.get_state()['pos'][0])
    for r in (1, 2):
        show(vec.sense(radius=r)[0])
        print()
    print('the whole grid as env 0 sees it (the agent: x):')
    whole = vec.sense(mode='grid')[0]
    for row in np.where(whole >= 8, 'x', GLYPHS[whole & 7]):
        print('    ' + ' '.join(row))
    vec.close()

    N, T = 256, 20000
    S = env.world.size
    kinds = (('view, radius 1', view_features(env, 1)), ('view, radius 3', view_features(env, 3)), ('one_hot', one_hot(S)))
    print('\n%d learners x %d steps of semi-gradient Q-learning on what they see:' % (N, T))
    print('    %-16s %9s %22s' % ('features', 'F', 'episodes finished/env'))
    for name, (phi, F) in kinds:
        vec = VecGridUniverse(N, template=env, seed=7)
        vec.set_features(phi, F)
        vec.reset()
        episodes = np.zeros(N, np.int64)
        for _ in range(T // 1000):
            episodes += vec.fa_run(1000, 'q_learning', alpha=0.2, discount_factor=0.95, epsilon=0.1, stats=True)['episodes']
        vec.close()
        print('    %-16s %9d %22.1f' % (name, F, episodes.mean()))
    env.close()


if __name__ == '__main__':
    main()
