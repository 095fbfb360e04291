"""Env-steps per second of batched Expected SARSA (gu_esarsa_run, csrc/gu_td.hip) and Double Q-learning (gu_double_run,
csrc/gu_double.hip) against Q-learning (gu_td_run) at the same shapes IN THE SAME RUN, on one MI355X.

For each grid (8x8 open grid; a 32x32 maze of the generator), 65 536 learners on one engine that holds both the Q tables and the
pairs: a few warm-up launches of each learner, then `--rounds` rounds, each timing `--launches` launches of `--steps` steps of
q_learning, expected_sarsa and double_q one after the other with HIP events around each block -- the three alternate, so a drift of
the machine falls on all of them.  Every block starts from tables of zeros and reset envs: a learner's rate changes as it learns
(in a run whose blocks continued each other, Q-learning on the maze fell from 4.6e10 env-steps/s in its first block to 3.0e10 in
its fifth, as the learners spread over the grid), so blocks that continue each other compare different stretches of that curve.  Reported per learner: every round's rate, the median, the spread (max / min - 1) and the ratio of the median to
q_learning's.  Prints ONE JSON line.

    python tools/double_rate.py > profiles/double_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
LEARNERS = ('q_learning', 'expected_sarsa', 'double_q')


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def launch(vec, learner, steps):
    kw = dict(alpha=0.1, discount_factor=0.99, epsilon=0.1)
    if learner == 'q_learning':
        vec.td_run(steps, 'q_learning', **kw)
    elif learner == 'expected_sarsa':
        vec.expected_sarsa_run(steps, **kw)
    else:
        vec.double_q_run(steps, **kw)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(rounds, launches, steps, warmup, n=N):
    import griduniverse_amd as gua
    out = []
    for name, spec in grids().items():
        vec = gua.VecGridUniverse(n, template=spec, seed=1)
        try:
            vec._ensure_q(0.0)
            vec._ensure_pairs(0.0)
            vec.reset()
            for learner in LEARNERS:
                for _ in range(warmup):
                    launch(vec, learner, steps)
            rates = dict((learner, []) for learner in LEARNERS)
            for _ in range(rounds):
                for learner in LEARNERS:
                    vec._ensure_q(0.0)  # the same work in every block: learning from scratch
                    vec._ensure_pairs(0.0)
                    vec.reset()
                    vec.engine.timer_begin()
                    for _ in range(launches):
                        launch(vec, learner, steps)
                    ms = vec.engine.timer_end()
                    rates[learner].append(n * steps * launches / (ms * 1e-3))
            base = median(rates['q_learning'])
            for learner in LEARNERS:
                r = rates[learner]
                out.append(dict(grid=name, S=spec.S, N=n, learner=learner, rounds=rounds, launches=launches, steps=steps,
                                env_steps_per_s=[float('%.4g' % x) for x in r], median=float('%.4g' % median(r)),
                                spread=round(max(r) / min(r) - 1.0, 4), of_q_learning=round(median(r) / base, 4)))
        finally:
            vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--envs', type=int, default=N)
    args = ap.parse_args()
    print(json.dumps(dict(tool='double_rate', results=measure(args.rounds, args.launches, args.steps, args.warmup, args.envs))))


if __name__ == '__main__':
    main()
