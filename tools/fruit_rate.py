"""Env-steps per second of the fruit kernels (gu_set_fruit; csrc/gu_fruit.hip, csrc/gu_td.hip) on one MI355X, beside the engine
without fruit.

On `--envs` (65 536) envs on a 32x32 maze of the generator and on the open 8x8 grid: uniform rollouts with int32 rows and with
statistics only -- the fruit kernel (six fruits) beside the calm engine's general rollout kernel (the transition-row and K-step
kernels switched off) --, and td_run (Q-learning) with two and with six fruits (tables of S << F rows) beside the calm td_run.
The two engines of a pair live in ONE process and take turns: after a few warm-up launches each, `--rounds` rounds of `--launches`
launches of `--steps` steps on the one, then on the other, each block timed with HIP events.  Prints ONE JSON line; every fruit result
carries its ratio to the calm result of its pair.

    python tools/fruit_rate.py > profiles/fruit_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALUES = (1, 5, -5)


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    return [('maze32', GridSpec.from_env(gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True))),
            ('open8x8', GridSpec(8, 8, [0], [63], [], []))]


def fruit_cells(spec, F):
    """F cells that may bear fruit, spread evenly over the grid."""
    import numpy as np
    free = np.flatnonzero(~(spec.wall | spec.goal | spec.lava))
    return free[np.linspace(0, len(free) - 1, F + 2).astype(int)[1:-1]]


def timed(vec, launch, launches):
    vec.engine.timer_begin()
    for _ in range(launches):
        launch(vec)
    return vec.engine.timer_end()


def pair(spec, N, F, launch, prepare, rounds, launches, warmup):
    """ms of rounds x launches launches on the calm engine and on the one with F fruits, taking turns."""
    import griduniverse_amd as gua
    calm = gua.VecGridUniverse(N, template=spec, seed=1)
    fruit = gua.VecGridUniverse(N, template=spec, seed=1)
    try:
        for opt in ('rollout_rows', 'rollout_multi'):
            calm.engine.set_option(opt, 0)
        fruit.set_fruit(fruit_cells(spec, F), ['apple', 'lemon', 'melon'] * (F // 3) + ['apple'] * (F % 3), VALUES)
        ms = [0.0, 0.0]
        for vec in (calm, fruit):
            prepare(vec)
            vec.reset()
            for _ in range(warmup):
                launch(vec)
            vec.engine.sync()
        for _ in range(rounds):
            for k, vec in enumerate((calm, fruit)):
                ms[k] += timed(vec, launch, launches)
        return ms
    finally:
        calm.close()
        fruit.close()


def measure(N, rounds, launches, steps, warmup):
    import griduniverse_amd as gua
    kinds = [('rollout_rows', 6, lambda v: v.engine.rollout(steps, 'uniform', True, True), lambda v: v.engine.reserve_trajectory(steps)),
             ('rollout_stats', 6, lambda v: v.engine.rollout(steps, 'uniform', True, False, stats=True), lambda v: None),
             ('td_q_learning', 2, lambda v: v.engine.td_run(steps, 'q_learning'), lambda v: v._ensure_q(0.0)),
             ('td_q_learning', 6, lambda v: v.engine.td_run(steps, 'q_learning'), lambda v: v._ensure_q(0.0))]
    out = []
    for name, spec in grids():
        for kind, F, launch, prepare in kinds:
            try:
                ms = pair(spec, N, F, launch, prepare, rounds, launches, warmup)
            except gua.GuError as err:  # (tables of S << F rows that the device cannot hold: said, not hidden)
                out.append(dict(grid=name, kind=kind, mode='fruit', fruits=F, N=N, S=spec.S, error=str(err)))
                continue
            rates = [N * steps * launches * rounds / (m * 1e-3) for m in ms]
            for mode, m, rate in (('calm', ms[0], rates[0]), ('fruit', ms[1], rates[1])):
                out.append(dict(grid=name, kind=kind, mode=mode, fruits=F if mode == 'fruit' else 0, N=N, S=spec.S, rounds=rounds, launches=launches,
                                steps=steps, ms=round(m, 3), env_steps_per_s=float('%.4g' % rate), ratio_to_calm=round(rate / rates[0], 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(dict(tool='fruit_rate', results=measure(args.envs, args.rounds, args.launches, args.steps, args.warmup))))


if __name__ == '__main__':
    main()
