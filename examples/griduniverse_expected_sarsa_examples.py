"""Q-learning, SARSA, Expected SARSA and Double Q-learning on a cliff grid, headless on the MI355X engine: 64 independent learners of
each kind on a 12x4 grid whose bottom row is the start, ten lava cells and the goal (Sutton & Barto, Example 6.6, with this
project's rewards: -1 a step, +10 the goal, -10 and the end of the episode in the lava).  Prints, for each learner kind, the mean
return per finished episode over the last third of the run (while still exploring), how many of the 64 greedy policies reach the
goal and how long their walks are.

    python examples/griduniverse_expected_sarsa_examples.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from griduniverse_amd import GridUniverseEnv, VecGridUniverse  # noqa: E402

W, H = 12, 4
START, GOAL = (H - 1) * W, H * W - 1
STEPS, LEARNERS = 12000, 64
ALPHA, GAMMA, EPSILON = 0.5, 0.99, 0.1


def learn(env, kind):
    """(mean return per finished episode over the last third, tables [L][S][4]) of 64 learners of one kind."""
    vec = VecGridUniverse(LEARNERS, template=env, seed=7)
    try:
        vec.reset()
        kw = dict(alpha=ALPHA, discount_factor=GAMMA, epsilon=EPSILON)
        run = {'q_learning': lambda T, **k: vec.td_run(T, 'q_learning', **k), 'sarsa': lambda T, **k: vec.td_run(T, 'sarsa', **k),
               'expected_sarsa': vec.expected_sarsa_run, 'double_q': vec.double_q_run}[kind]
        run(STEPS - STEPS // 3, **kw)
        out = run(STEPS // 3, stats=True, **kw)
        if kind == 'double_q':
            pair = vec.double_q_tables()
            q = (pair[:, :, 0] + pair[:, :, 1]) * 0.5
        else:
            q = vec.q_table()
    finally:
        vec.close()
    return float(np.sum(out['ret'])) / max(int(np.sum(out['episodes'])), 1), q


def greedy_walk(env, q):
    s, n = START, 0
    while not env.is_terminal(s) and n < env.world.size:
        s, _, _ = env.look_step_ahead(s, int(np.argmax(q[s])))
        n += 1
    return n if env.is_terminal_goal(s) else -1


def main():
    env = GridUniverseEnv(grid_shape=(W, H), initial_state=START, goal_states=[GOAL], lava_states=list(range(START + 1, GOAL)))
    print('cliff %d x %d, %d learners each, %d steps, alpha %.1f, gamma %.2f, epsilon %.1f' % (W, H, LEARNERS, STEPS, ALPHA, GAMMA, EPSILON))
    for kind in ('q_learning', 'sarsa', 'expected_sarsa', 'double_q'):
        ret, q = learn(env, kind)
        walks = np.array([greedy_walk(env, q[e]) for e in range(LEARNERS)])
        reached = walks[walks >= 0]
        print('%-15s mean return %7.3f   greedy walks reaching the goal: %2d of %d%s' % (
            kind, ret, len(reached), LEARNERS, ', %d .. %d steps' % (reached.min(), reached.max()) if len(reached) else ''))
    env.close()


if __name__ == '__main__':
    main()
