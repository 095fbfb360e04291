"""Pushable boxes (Sokoban), headless.

1. A random agent on an XSB level: 4096 envs roll out 200 uniform steps in one kernel launch; prints how many envs solved the level
   at least once and where the boxes of the first envs stand.
2. The learning claim: a 4x4 grid, start 4, one box on 5, its target on 10, a lava cell on 12 as the way out of a deadlock (a box
   pushed into a corner ends no episode: only a goal or lava cell brings an auto-resetting env back).  The shortest solution has 4
   moves and return 7: push right, walk up and around, push down.  64 independent Q-learners, all advanced by one kernel per launch,
   learn on the rows of (cell, word of box cells): their tables have S << 4 = 256 rows.

    python examples/griduniverse_sokoban_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import VecGridUniverse  # noqa: E402
from griduniverse_amd.grid import GridSpec, sokoban_level  # noqa: E402

LEVEL = '''
#######
#.    #
# $ $ #
#  @ .#
#######
'''
NAMES = ('UP', 'RIGHT', 'DOWN', 'LEFT')


def random_agent():
    spec, boxes, targets = sokoban_level(LEVEL)
    vec = VecGridUniverse(4096, template=spec, seed=0)
    vec.set_boxes(boxes, targets, on_target=5)
    print('level %dx%d: start %d, boxes %s, targets %s' % (spec.W, spec.H, spec.starts[0], boxes, targets))
    vec.reset()
    out = vec.rollout(200, 'uniform', auto_reset=True, trajectory=False, stats=True)
    print('200 uniform steps: %d of %d envs solved the level at least once; mean return %.1f' % (
        (out['episodes'] > 0).sum(), vec.num_envs, out['ret'].mean()))
    print('box cells of envs 0 .. 3 now:', vec.box_cells(0, 4).tolist())
    vec.close()


def claim():
    S, START, BOX, TARGET, LAVA = 16, 4, 5, 10, 12
    spec = GridSpec(4, 4, [START], [], [LAVA], [])
    L, T = 64, 1000
    vec = VecGridUniverse(L, template=spec, seed=1)
    vec.set_boxes([BOX], [TARGET], on_target=5)
    vec.reset()
    probe = VecGridUniverse(1, template=spec, seed=0)  # one env that walks a table greedily, on the engine's own rule
    probe.set_boxes([BOX], [TARGET], on_target=5)

    def greedy_walk(q, limit=30):
        probe.reset()
        s, walk, total = START, [], 0
        for _ in range(limit):
            w = int(probe.engine.get_boxes_state()[0])
            a = int(np.argmax(q[w * S + s]))
            walk.append('%d/%d:%s' % (s, w, NAMES[a]))
            obs, r, d, _ = probe.step(np.array([a], np.int32))
            s, total = int(obs[0]), total + int(r[0])
            if d[0]:
                return walk, total, int(probe.box_cells()[0, 0]) == TARGET
        return walk, None, False

    for launch in range(1, 7):
        out = vec.td_run(T, 'q_learning', alpha=0.5, discount_factor=0.95, epsilon=0.1, stats=True)
        q = vec.q_table()  # [L, 256, 4]
        walks = [greedy_walk(q[e]) for e in range(L)]
        best = sum(solved and total == 7 and len(walk) == 4 for walk, total, solved in walks)
        print('after %4d steps: %2d of %d learners solve the level greedily in 4 moves (return 7); reward per step %.3f' % (
            launch * T, best, L, out['ret'].sum() / (L * T)))
    walk, total, solved = greedy_walk(vec.q_table(0, 1)[0])
    print('learner 0, greedy: ' + ' '.join(walk) + ' -> return %s, solved %s   (cell/word:action)' % (total, solved))
    vec.close()
    probe.close()


if __name__ == '__main__':
    random_agent()
    claim()
