"""Env-steps per second of batched tabular n-step Q-learning and n-step SARSA (gu_nstep_run, csrc/gu_nstep.hip) on one MI355X,
with one-step gu_td_run measured in the same run on the same engine for comparison (`n: null`).

For each grid (8x8 open grid; a 32x32 maze of the generator), batch size N in {4096, 65536, 262144}, method and n in {1, 4, 16}
(and gu_td_run): a few warm-up launches, then `--launches` (>= 100) launches of `--steps` (1000) steps timed with HIP events
around the whole block.  Prints ONE JSON line.  With --rocprof the same measurement is repeated once in a child process under
`rocprofv3 --kernel-trace --stats` (a short form: 20 launches per point) and the kernels' average duration per instantiation is
added to the line.

    python tools/nstep_rate.py [--rocprof DIR] > profiles/nstep_rate.json
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
NS = (1, 4, 16)


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def measure(launches, steps, warmup):
    import griduniverse_amd as gua
    out = []
    for name, spec in grids().items():
        for N in SIZES:
            vec = gua.VecGridUniverse(N, template=spec, seed=1)
            try:
                vec.reset()
                for method in ('q_learning', 'sarsa'):
                    for n in (None,) + NS:
                        if n is None:
                            run = lambda: vec.td_run(steps, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                        else:
                            run = lambda: vec.nstep_run(steps, n, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                        vec._ensure_q(0.0)
                        for _ in range(warmup):
                            run()
                        vec.engine.timer_begin()
                        for _ in range(launches):
                            run()
                        ms = vec.engine.timer_end()
                        out.append(dict(grid=name, S=spec.S, N=N, method=method, n=n, launches=launches, steps=steps, ms=round(ms, 3),
                                        env_steps_per_s=float('%.4g' % (N * steps * launches / (ms * 1e-3)))))
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
                if 'gu_td_kernel' in row['Name'] or 'gu_nstep_kernel' in row['Name']:
                    stats[row['Name']] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rocprof', default=None, help='directory for a rocprofv3 kernel-trace run of the short form')
    args = ap.parse_args()
    line = dict(tool='nstep_rate', results=measure(args.launches, args.steps, args.warmup))
    if args.rocprof:
        line['rocprofv3_kernel_stats'] = rocprof_stats(args.rocprof, args.steps)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
