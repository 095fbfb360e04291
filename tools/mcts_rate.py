"""Simulated moves and real steps per second of the batched Monte-Carlo tree search (gu_mcts_run, csrc/gu_mcts.hip) on one MI355X.

65 536 learners on the open 8x8 grid and on a 32x32 maze of the generator; (simulations, tree depth, rollout depth) = (64, 8, 4)
and (255, 32, 16); uniform rollouts (rollout_epsilon 1.0: the instantiation that reads no Q row until the leaf) and epsilon-greedy
ones (0.1); UCB1 tables with c = 3.  A point is one launch of `--moves` / (1 + M (H + D)) real steps per learner, timed with HIP
events, after one warm-up launch of the same shape; it is repeated `--repeats` times on the same learners (they go on learning, so
the work of a repeat differs: every repeat's time and counted moves are kept).  simulated moves = the sum of gu_mcts_get's
sim_steps, selection and rollout moves alike; backup turns, moves that a terminal cell cut off and the steps that explored are not
counted.  The flat rollout search (tools/search_rate.py's points, (4, 16) and (16, 64)) is timed in the same process on the same
grids, so that the two can be read side by side.

Then simulations = 0 against td_run('q_learning'), which it equals byte for byte, alternating in one process: the ratio of the
two rates is what the kernel's loop structure costs a learner that never searches.

Prints ONE JSON line.

    python tools/mcts_rate.py > profiles/mcts_rate.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.search_rate import KW, N, _median, grids, search_points  # noqa: E402


def tree_points(spec, grid, moves, repeats):
    import griduniverse_amd as gua
    from griduniverse_amd.algorithms.search import uct_tables
    out = []
    for M, H, D in ((64, 8, 4), (255, 32, 16)):
        T = max(1, moves // (1 + M * (H + D)))
        for rollout_epsilon in (1.0, 0.1):
            vec = gua.VecGridUniverse(N, template=spec, seed=1)
            try:
                vec._ensure_q(0.0)
                vec.reset()
                vec.set_tree_search(*uct_tables(3.0, 256))
                run = lambda: vec.tree_search_run(T, M, H, D, rollout_epsilon=rollout_epsilon, **KW)  # noqa: E731
                run()  # warm-up: the same shape
                ms, sims = [], []
                for _ in range(repeats):
                    vec.engine.timer_begin()
                    run()
                    ms.append(round(vec.engine.timer_end(), 3))
                    sims.append(int(vec.tree_search_roots()['sim_steps'].sum()))
                out.append(dict(grid=grid, S=spec.S, N=N, simulations=M, tree_depth=H, depth=D, rollout_epsilon=rollout_epsilon,
                                real_steps_per_launch=T, ms=ms, simulated_moves=sims,
                                mean_nodes=round(float(vec.tree_search_roots()['nodes'].mean()), 2),
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
        runs = (('tree_search_run simulations=0', a, lambda: a.tree_search_run(steps, 0, 8, 4, **KW)),
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
                    ratio_to_td_run=round(rate['tree_search_run simulations=0'] / rate['td_run'], 3))
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
    line = dict(tool='mcts_rate', tree_search=[], rollout_search=[], no_search=[])
    for grid, spec in grids().items():
        line['tree_search'] += tree_points(spec, grid, args.moves, args.repeats)
        line['rollout_search'] += search_points(spec, grid, args.moves, args.repeats)
        line['no_search'].append(no_search_point(spec, grid, args.launches, args.steps, args.repeats))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
