"""Env steps per second of the batched count-based exploration (gu_explore_run, csrc/gu_explore.hip) on one MI355X.

65 536 learners on the open 8x8 grid and on a 32x32 maze of the generator.  Per grid, five learners alternate in one process,
each on a batch of its own: td_run('q_learning') -- the yardstick --, explore_run with tables of zeros (which it equals byte for
byte: the ratio of the two rates is what the count row costs), and UCB and Thompson with the builders' tables of 1024 entries
(16 KiB, staged in LDS beside the map) and of 4096 entries (64 KiB, read through L2).  A timed block is `--launches` launches of
`--steps` steps, timed with HIP events, after two warm-up launches; `--repeats` blocks per learner, the median is reported.  The
learners go on learning from block to block.

Prints ONE JSON line.

    python tools/explore_rate.py > profiles/explore_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
KW = dict(alpha=0.1, discount_factor=0.99)


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def point(spec, grid, n, launches, steps, repeats):
    import numpy as np

    import griduniverse_amd as gua
    from griduniverse_amd.algorithms.exploration import thompson_tables, ucb_tables
    learners = [('td_run', None, None, 0.1),
                ('explore_run zero tables', 'ucb', (np.zeros(1024), np.zeros(1024)), 0.1),
                ('ucb 1024', 'ucb', ucb_tables(1.0, 1024), 0.0),
                ('thompson 1024', 'thompson', thompson_tables(1.0, 1024), 0.0),
                ('ucb 4096', 'ucb', ucb_tables(1.0, 4096), 0.0),
                ('thompson 4096', 'thompson', thompson_tables(1.0, 4096), 0.0)]
    runs = []
    try:
        for name, rule, tables, eps in learners:
            vec = gua.VecGridUniverse(n, template=spec, seed=1)
            runs.append((name, vec, rule, eps))
            vec._ensure_q(0.0)
            if rule:
                vec.set_exploration(*tables)
            vec.reset()

        def launch(vec, rule, eps):
            if rule:
                vec.explore_run(steps, rule, epsilon=eps, **KW)
            else:
                vec.td_run(steps, 'q_learning', epsilon=eps, **KW)

        times = {name: [] for name, _, _, _ in runs}
        for _, vec, rule, eps in runs:
            for _ in range(2):
                launch(vec, rule, eps)
        for _ in range(repeats):  # alternating
            for name, vec, rule, eps in runs:
                vec.engine.timer_begin()
                for _ in range(launches):
                    launch(vec, rule, eps)
                times[name].append(round(vec.engine.timer_end(), 3))
        rate = {k: n * steps * launches / (_median(v) * 1e-3) for k, v in times.items()}
        return dict(grid=grid, S=spec.S, N=n, launches=launches, steps=steps, ms=times,
                    env_steps_per_s={k: float('%.4g' % v) for k, v in rate.items()},
                    ratio_to_td_run={k: round(v / rate['td_run'], 3) for k, v in rate.items() if k != 'td_run'})
    finally:
        for _, vec, _, _ in runs:
            vec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--learners', type=int, default=N)
    ap.add_argument('--launches', type=int, default=10, help='launches per timed block')
    ap.add_argument('--steps', type=int, default=1000, help='steps per launch')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    line = dict(tool='explore_rate', points=[])
    for grid, spec in grids().items():
        line['points'].append(point(spec, grid, args.learners, args.launches, args.steps, args.repeats))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
