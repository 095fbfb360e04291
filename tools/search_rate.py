"""Simulated moves and real steps per second of the batched rollout search (gu_search_run, csrc/gu_search.hip) on one MI355X.

65 536 learners on the open 8x8 grid and on a 32x32 maze of the generator; (simulations, depth) = (4, 16) and (16, 64); uniform
rollouts (rollout_epsilon 1.0: the instantiation that reads no row until the leaf) and epsilon-greedy ones (0.1).  A point is
one launch of `--moves` / (1 + 4 M D) real steps per learner, timed with HIP events, after one warm-up launch of the same shape;
it is repeated `--repeats` times on the same learners (they go on learning, so the work of a repeat differs: every repeat's time
and counted moves are kept).  simulated moves = the sum of gu_search_get's sim_steps, so moves that a terminal cell cut off, and
the steps that explored, are not counted.

Then simulations = 0 against td_run('q_learning'), which it equals byte for byte, alternating in one process: the ratio of the
two rates is what the search kernel's loop structure costs a learner that never searches.

Prints ONE JSON line.

    python tools/search_rate.py > profiles/search_rate.json
"""
import argparse
import json
import os
import random
import sys

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


def search_points(spec, grid, moves, repeats):
    import griduniverse_amd as gua
    out = []
    for M, D in ((4, 16), (16, 64)):
        T = max(1, moves // (1 + 4 * M * D))
        for rollout_epsilon in (1.0, 0.1):
            vec = gua.VecGridUniverse(N, template=spec, seed=1)
            try:
                vec._ensure_q(0.0)
                vec.reset()
                run = lambda: vec.search_run(T, M, D, rollout_epsilon=rollout_epsilon, **KW)  # noqa: E731
                run()  # warm-up: the same shape
                ms, sims = [], []
                for _ in range(repeats):
                    vec.engine.timer_begin()
                    run()
                    ms.append(round(vec.engine.timer_end(), 3))
                    sims.append(int(vec.search_scores()['sim_steps'].sum()))
                out.append(dict(grid=grid, S=spec.S, N=N, simulations=M, depth=D, rollout_epsilon=rollout_epsilon, real_steps_per_launch=T,
                                ms=ms, simulated_moves=sims,
                                simulated_moves_per_s=float('%.4g' % _median([s / (m * 1e-3) for s, m in zip(sims, ms)])),
                                real_steps_per_s=float('%.4g' % _median([N * T / (m * 1e-3) for m in ms]))))
            finally:
                vec.close()
    return out


def no_search_point(spec, grid, launches, steps, repeats):
    import griduniverse_amd as gua
    a = gua.VecGridUniverse(N, template=spec, seed=1)
    b = gua.VecGridUniverse(N, template=spec, seed=1)
    try:
        runs = (('search_run simulations=0', a, lambda: a.search_run(steps, 0, 16, **KW)),
                ('td_run', b, lambda: b.td_run(steps, 'q_learning', **KW)))
        times = {k: [] for k, _, _ in runs}
        for _, vec, run in runs:
            vec._ensure_q(0.0)
            vec.reset()
            for _ in range(2):
                run()
        for _ in range(repeats):  # alternating
            for k, vec, run in runs:
                vec.engine.timer_begin()
                for _ in range(launches):
                    run()
                times[k].append(round(vec.engine.timer_end(), 3))
        rate = {k: N * steps * launches / (_median(v) * 1e-3) for k, v in times.items()}
        return dict(grid=grid, S=spec.S, N=N, launches=launches, steps=steps, ms=times,
                    env_steps_per_s={k: float('%.4g' % v) for k, v in rate.items()},
                    ratio_to_td_run=round(rate['search_run simulations=0'] / rate['td_run'], 3))
    finally:
        a.close()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moves', type=int, default=2000000, help='real + simulated moves per learner and launch, at the most')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20, help='the simulations = 0 point: launches per timed block')
    ap.add_argument('--steps', type=int, default=1000, help='... and steps per launch')
    args = ap.parse_args()
    specs = grids()
    line = dict(tool='search_rate', search=[], no_search=[])
    for grid, spec in specs.items():
        line['search'] += search_points(spec, grid, args.moves, args.repeats)
        line['no_search'].append(no_search_point(spec, grid, args.launches, args.steps, args.repeats))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
