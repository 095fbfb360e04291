"""Env-steps per second of the door kernels (gu_set_doors; csrc/gu_doors.hip, csrc/gu_td.hip) on one MI355X, beside the engine
without doors and the engine with fruit.

On `--envs` (65 536) envs on a 32x32 maze of the generator and on the open 8x8 grid, with two door slots (a key and a lever): uniform
rollouts with int32 rows and with statistics only, and td_run (Q-learning; tables of S << 2 rows).  In the same run, at the same
shapes: the calm engine's general rollout kernel (the transition-row and K-step kernels switched off) and calm td_run, and the
fruit kernels with two fruits (tables of S << 2 rows as well).  The three engines of a shape live in ONE process and take turns: after
a few warm-up launches each, `--rounds` rounds of `--launches` launches of `--steps` steps on the one, then on the next, each block
timed with HIP events.  Prints ONE JSON line; every row carries its ratio to the calm row and to the fruit row of its shape, and the
time of its first and of its last round (a learner's rate moves with what it has learnt).

    python tools/doors_rate.py > profiles/doors_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('calm', 'fruit', 'doors')


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    return [('maze32', GridSpec.from_env(gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True))),
            ('open8x8', GridSpec(8, 8, [0], [63], [], []))]


def spread(spec, n):
    """n free cells spread evenly over the grid."""
    import numpy as np
    free = np.flatnonzero(~(spec.wall | spec.goal | spec.lava))
    return [int(c) for c in free[np.linspace(0, len(free) - 1, n + 2).astype(int)[1:-1]]]


def timed(vec, launch, launches):
    vec.engine.timer_begin()
    for _ in range(launches):
        launch(vec)
    return vec.engine.timer_end()


def trio(spec, N, launch, prepare, rounds, launches, warmup):
    """ms of each round of `launches` launches on the calm engine, the one with two fruits and the one with two door slots, taking turns."""
    import griduniverse_amd as gua
    vecs = [gua.VecGridUniverse(N, template=spec, seed=1) for _ in MODES]
    try:
        for opt in ('rollout_rows', 'rollout_multi'):
            vecs[0].engine.set_option(opt, 0)
        key, door0, lever, door1 = spread(spec, 4)  # the key in front of its door, the lever in front of its door, in cell order
        vecs[1].set_fruit([key, lever], ['apple', 'lemon'], (1, 5, -5))
        vecs[2].set_doors({0: door0, 1: door1}, keys={0: key}, levers={1: lever})
        ms = [[] for _ in vecs]
        for vec in vecs:
            prepare(vec)
            vec.reset()
            for _ in range(warmup):
                launch(vec)
            vec.engine.sync()
        for _ in range(rounds):
            for k, vec in enumerate(vecs):
                ms[k].append(timed(vec, launch, launches))
        forms = [vec.engine.rollout_last_form()['family'] for vec in vecs]
        return ms, forms
    finally:
        for vec in vecs:
            vec.close()


def measure(N, rounds, launches, steps, warmup):
    kinds = [('rollout_rows', lambda v: v.engine.rollout(steps, 'uniform', True, True), lambda v: v.engine.reserve_trajectory(steps)),
             ('rollout_stats', lambda v: v.engine.rollout(steps, 'uniform', True, False, stats=True), lambda v: None),
             ('td_q_learning', lambda v: v.engine.td_run(steps, 'q_learning'), lambda v: v._ensure_q(0.0))]
    out = []
    for name, spec in grids():
        for kind, launch, prepare in kinds:
            per_round, forms = trio(spec, N, launch, prepare, rounds, launches, warmup)
            ms = [sum(r) for r in per_round]
            rates = [N * steps * launches * rounds / (m * 1e-3) for m in ms]
            for mode, m, rate, form, rs in zip(MODES, ms, rates, forms, per_round):
                out.append(dict(grid=name, kind=kind, mode=mode, slots=2 if mode != 'calm' else 0, N=N, S=spec.S, rounds=rounds, launches=launches,
                                steps=steps, ms=round(m, 3), env_steps_per_s=float('%.4g' % rate), ratio_to_calm=round(rate / rates[0], 3),
                                ratio_to_fruit=round(rate / rates[1], 3), rollout_family=form if kind.startswith('rollout') else None,
                                first_round_ms=round(rs[0], 3), last_round_ms=round(rs[-1], 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(dict(tool='doors_rate', results=measure(args.envs, args.rounds, args.launches, args.steps, args.warmup))))


if __name__ == '__main__':
    main()
