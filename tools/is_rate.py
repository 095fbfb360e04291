"""Env-steps per second of batched off-policy Monte-Carlo control with weighted importance sampling (gu_is_run, csrc/gu_is.hip) on
one MI355X, with gu_td_run (Q-learning) and gu_reinforce_run measured in the same run on the same engine for comparison.

For each grid (8x8 open grid; a 32x32 maze of the generator), batch size N in {4096, 65536} and segment length L in {1, 16, 256}:
a few warm-up launches, then `--launches` (>= 100) launches of `--steps` (1000) steps timed with HIP events around the whole
block.  Every learner starts from tables of zeros and freshly reset envs.  Each gu_is_run point carries `frac_of_td`, its rate
over gu_td_run's on the same engine, and `frac_of_reinforce`, its rate over gu_reinforce_run's at the same L; each
gu_reinforce_run point carries `frac_of_td` too.  Prints ONE JSON line.

    python tools/is_rate.py > profiles/is_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 65536)
LENGTHS = (1, 16, 256)


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def measure(launches, steps, warmup, sizes):
    import griduniverse_amd as gua
    out = []
    for name, spec in grids().items():
        for N in sizes:
            vec = gua.VecGridUniverse(N, template=spec, seed=1)
            try:
                rates = {}
                for learner in [('td', 0)] + [('reinforce', L) for L in LENGTHS] + [('off_policy_mc', L) for L in LENGTHS]:
                    kind, L = learner
                    vec._ensure_q(0.0)
                    vec._ensure_ac(0.0, 0.0)
                    vec._ensure_is()
                    vec.engine.is_init()  # (zeroes the weights on the device)
                    vec.reset()
                    if kind == 'td':
                        run = lambda: vec.td_run(steps, 'q_learning', 0.1, 0.99, 0.1)  # noqa: E731
                    elif kind == 'reinforce':
                        run = lambda L=L: vec.reinforce_run(steps, L, 0.003, 0.1, 0.99)  # noqa: E731
                    else:
                        run = lambda L=L: vec.off_policy_mc_run(steps, L, 0.99, 0.1)  # noqa: E731
                    for _ in range(warmup):
                        run()
                    vec.engine.timer_begin()
                    for _ in range(launches):
                        run()
                    ms = vec.engine.timer_end()
                    rates[learner] = N * steps * launches / (ms * 1e-3)
                    row = dict(grid=name, S=spec.S, N=N, learner=kind, launches=launches, steps=steps, ms=round(ms, 3),
                               env_steps_per_s=float('%.4g' % rates[learner]))
                    if kind != 'td':
                        row['L'] = L
                        row['frac_of_td'] = round(rates[learner] / rates[('td', 0)], 3)
                    if kind == 'off_policy_mc':
                        row['frac_of_reinforce'] = round(rates[learner] / rates[('reinforce', L)], 3)
                    out.append(row)
            finally:
                vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=list(SIZES))
    args = ap.parse_args()
    from griduniverse_amd import _lib
    line = dict(tool='is_rate', library=os.path.basename(_lib.LIB_PATH), results=measure(args.launches, args.steps, args.warmup, args.sizes))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
