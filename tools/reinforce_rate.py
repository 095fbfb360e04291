"""Env-steps per second of batched tabular REINFORCE with baseline (gu_reinforce_run, csrc/gu_reinforce.hip) on one MI355X, with
gu_ac_run measured in the same run on the same engine for comparison (`learner: "actor_critic"`).

For each grid (8x8 open grid; a 32x32 maze of the generator), batch size N in {4096, 65536, 262144} and segment length L in
{1, 16, 256}: a few warm-up launches, then `--launches` (>= 100) launches of `--steps` (1000) steps timed with HIP events around
the whole block.  Each REINFORCE point carries `frac_of_ac`, its rate over gu_ac_run's on the same engine, and the points with
L > 1 carry `frac_of_L1`, their rate over the L = 1 point of the same grid and N (at L = 1 every lane alternates one real step
and one backward update in step with its neighbours; at L = 256 on the open grid episodes end at scattered steps in every wave).
Prints ONE JSON line.  With --rocprof the same measurement is repeated once in a child process under
`rocprofv3 --kernel-trace --stats` (a short form: 20 launches per point) and the kernels' average duration per instantiation is
added to the line.

    python tools/reinforce_rate.py [--rocprof DIR] > profiles/reinforce_rate.json
"""
import argparse
import csv
import glob
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 65536, 262144)
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
                for learner in ('actor_critic',) + LENGTHS:
                    vec._ensure_ac(0.0, 0.0)  # every learner starts from tables of zeros and freshly reset envs
                    vec.reset()
                    if learner == 'actor_critic':
                        run = lambda: vec.actor_critic_run(steps, 0.1, 0.1, 0.99)  # noqa: E731
                    else:
                        run = lambda L=learner: vec.reinforce_run(steps, L, 0.003, 0.1, 0.99)  # noqa: E731
                    for _ in range(warmup):
                        run()
                    vec.engine.timer_begin()
                    for _ in range(launches):
                        run()
                    ms = vec.engine.timer_end()
                    rates[learner] = N * steps * launches / (ms * 1e-3)
                    row = dict(grid=name, S=spec.S, N=N, learner=learner if learner == 'actor_critic' else 'reinforce',
                               launches=launches, steps=steps, ms=round(ms, 3), env_steps_per_s=float('%.4g' % rates[learner]))
                    if learner != 'actor_critic':
                        row['L'] = learner
                        row['frac_of_ac'] = round(rates[learner] / rates['actor_critic'], 3)
                        if learner != 1:
                            row['frac_of_L1'] = round(rates[learner] / rates[1], 3)
                    out.append(row)
            finally:
                vec.close()
    return out


def rocprof_stats(out_dir, steps):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
           sys.executable, os.path.abspath(__file__), '--launches', '20', '--warmup', '1', '--steps', str(steps)]
    with open(os.path.join(out_dir, 'rocprofv3.log'), 'w') as log:
        subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, check=True, timeout=1500)
    stats = {}
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if 'gu_reinforce_kernel' in row['Name'] or 'gu_ac_kernel' in row['Name']:
                    stats[row['Name']] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=list(SIZES))
    ap.add_argument('--rocprof', default=None, help='directory for a rocprofv3 kernel-trace run of the short form')
    args = ap.parse_args()
    from griduniverse_amd import _lib
    line = dict(tool='reinforce_rate', library=os.path.basename(_lib.LIB_PATH),
                results=measure(args.launches, args.steps, args.warmup, args.sizes))
    if args.rocprof:
        line['rocprofv3_kernel_stats'] = rocprof_stats(args.rocprof, args.steps)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
