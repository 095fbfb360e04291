"""Walked steps per second of the batched greedy evaluation (gu_td_evaluate, csrc/gu_eval.hip) on one MI355X.

65 536 learners on the open 8x8 grid and on a 32x32 maze of the generator.  Per grid two batches are trained `--train` steps of
td_run('q_learning') each; then, taking turns in one process, the first goes on with td_run launches -- the yardstick -- and the
second is evaluated with K = 1 and with K = 4 test episodes of at most S steps.  A timed block of td_run is `--launches` launches of
`--steps` steps between HIP events; a timed block of evaluate() is `--launches` calls on the wall clock, because the call is
synchronous and its time includes the copy of the six [K, N] arrays to the host.  `--repeats` blocks each, the median is reported.
The evaluation's rate is walked steps per second: the sum of `length` over the block's time (walks that end early walk less).

Prints ONE JSON line.

    python tools/eval_rate.py > profiles/eval_rate.json
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
KW = dict(alpha=0.1, discount_factor=0.99, epsilon=0.1)


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def point(spec, grid, n, train, launches, steps, repeats):
    import griduniverse_amd as gua
    learner = gua.VecGridUniverse(n, template=spec, seed=1)
    walker = gua.VecGridUniverse(n, template=spec, seed=1)
    try:
        for vec in (learner, walker):
            vec.reset()
            vec.td_run(train, 'q_learning', **KW)
        walked = {K: int(walker.evaluate(K, spec.S)['length'].sum()) for K in (1, 4)}  # (also the warm-up; the tables do not change)
        learner.td_run(steps, 'q_learning', **KW)
        ms = {'td_run': [], 'evaluate K=1': [], 'evaluate K=4': []}
        for _ in range(repeats):  # taking turns
            learner.engine.timer_begin()
            for _ in range(launches):
                learner.td_run(steps, 'q_learning', **KW)
            ms['td_run'].append(round(learner.engine.timer_end(), 3))
            for K in (1, 4):
                t0 = time.perf_counter()
                for _ in range(launches):
                    walker.evaluate(K, spec.S)
                ms['evaluate K=%d' % K].append(round((time.perf_counter() - t0) * 1e3, 3))
        rate = {'td_run': n * steps * launches / (_median(ms['td_run']) * 1e-3)}
        for K in (1, 4):
            rate['evaluate K=%d' % K] = walked[K] * launches / (_median(ms['evaluate K=%d' % K]) * 1e-3)
        return dict(grid=grid, S=spec.S, N=n, trained_steps=train, launches=launches, steps=steps, max_steps=spec.S, ms=ms,
                    walked_steps_per_call={str(K): v for K, v in walked.items()}, mean_length={str(K): round(v / (K * n), 2) for K, v in walked.items()},
                    steps_per_s={k: float('%.4g' % v) for k, v in rate.items()})
    finally:
        learner.close()
        walker.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--learners', type=int, default=N)
    ap.add_argument('--train', type=int, default=20000, help='steps both batches are trained before the timed blocks')
    ap.add_argument('--launches', type=int, default=10, help='launches or calls per timed block')
    ap.add_argument('--steps', type=int, default=1000, help='steps per td_run launch')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    line = dict(tool='eval_rate', clock='td_run: HIP events; evaluate: wall clock of the synchronous call, host copies included', points=[])
    for grid, spec in grids().items():
        line['points'].append(point(spec, grid, args.learners, args.train, args.launches, args.steps, args.repeats))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
