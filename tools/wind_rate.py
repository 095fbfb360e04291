"""Env-steps per second of the windy kernels (gu_set_wind; csrc/gu_wind.hip, csrc/gu_td.hip) on one MI355X, against the calm engine.

On `--envs` (65 536) envs on a 32x32 maze of the generator: uniform rollouts, statistics only and with int32 rows, and td_run (both
methods), each under
    calm          the calm engine as it dispatches by default
    calm_general  the calm engine's general rollout kernel (the transition-row and K-step kernels switched off)
    wind0         wind of strength 0 everywhere (the windy kernels, no push ever taken)
    wind1         strength 1 upward everywhere, no gusts
    wind1_gust    the same with gust 43691 / 65536 (one third each for k - 1, k, k + 1)
A few warm-up launches, then `--launches` launches of `--steps` steps timed with HIP events around the whole block.  Prints ONE
JSON line; every result carries its ratio to the calm launch of the same kind (rollouts: to calm_general).

    python tools/wind_rate.py > profiles/wind_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUST_THIRDS = 43691
MODES = ('calm', 'calm_general', 'wind0', 'wind1', 'wind1_gust')


def maze():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    return GridSpec.from_env(gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True))


def set_mode(vec, mode):
    import numpy as np
    from griduniverse_amd.grid import wind_plane
    general = mode == 'calm_general'
    vec.engine.set_option('rollout_rows', 0 if general else None)
    vec.engine.set_option('rollout_multi', 0 if general else None)
    if mode.startswith('calm'):
        vec.engine.set_wind(None)
    else:
        strength = np.full(vec.spec.W, 0 if mode == 'wind0' else 1)
        vec.engine.set_wind(wind_plane(vec.spec.W, vec.spec.H, strength), GUST_THIRDS if mode == 'wind1_gust' else 0)


def timed(vec, launch, launches, warmup):
    for _ in range(warmup):
        launch()
    vec.engine.timer_begin()
    for _ in range(launches):
        launch()
    return vec.engine.timer_end()


def measure(N, launches, steps, warmup):
    import griduniverse_amd as gua
    spec = maze()
    out = []
    vec = gua.VecGridUniverse(N, template=spec, seed=1)
    try:
        vec.engine.reserve_trajectory(steps)
        vec._ensure_q(0.0)
        kinds = [('rollout_stats', lambda: vec.engine.rollout(steps, 'uniform', True, False, stats=True)),
                 ('rollout_rows', lambda: vec.engine.rollout(steps, 'uniform', True, True)),
                 ('td_q_learning', lambda: vec.engine.td_run(steps, 'q_learning')),
                 ('td_sarsa', lambda: vec.engine.td_run(steps, 'sarsa'))]
        for kind, launch in kinds:
            base = None
            for mode in MODES:
                if kind.startswith('td') and mode == 'calm_general':
                    continue  # (the learners have one calm form)
                set_mode(vec, mode)
                vec.reset()
                ms = timed(vec, launch, launches, warmup)
                rate = N * steps * launches / (ms * 1e-3)
                if mode == ('calm' if kind.startswith('td') else 'calm_general'):
                    base = rate
                out.append(dict(kind=kind, mode=mode, N=N, S=spec.S, launches=launches, steps=steps, ms=round(ms, 3),
                                env_steps_per_s=float('%.4g' % rate)))
            for r in out:
                if r['kind'] == kind:
                    r['ratio_to_calm'] = round(r['env_steps_per_s'] / base, 3)
    finally:
        vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(dict(tool='wind_rate', results=measure(args.envs, args.launches, args.steps, args.warmup))))


if __name__ == '__main__':
    main()
