"""Env-steps per second of batched tabular SARSA(lambda) and Watkins's Q(lambda) (gu_lambda_run, csrc/gu_lambda.hip) on one MI355X,
with one-step gu_td_run (`learner: "td"`) and n-step gu_nstep_run with n = 16 (`learner: "nstep16"`) measured in the same run on
the same engine for comparison.

For each grid (8x8 open grid; a 32x32 maze of the generator), batch size N in {4096, 65536, 262144}, method and trace length K in
{1, 8, 32, 64} at lambda = 0.9 (and the two references): a few warm-up launches, then `--launches` (>= 100) launches of `--steps`
(1000) steps timed with HIP events around the whole block.  Each lambda point carries `frac_of_td`, its rate over gu_td_run's of
the same method on the same engine.  Prints ONE JSON line (progress goes to stderr).  With --rocprof the same measurement is
repeated once in a child process under `rocprofv3 --kernel-trace --stats` (a short form: 20 launches per point) and the kernels'
average duration per instantiation is added to the line.

    python tools/lambda_rate.py [--rocprof DIR] > profiles/lambda_rate.json
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
KS = (1, 8, 32, 64)
LAM = 0.9


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
                    td = None
                    for learner, K in (('td', None), ('nstep16', None)) + tuple(('lambda', K) for K in KS):
                        if learner == 'td':
                            run = lambda: vec.td_run(steps, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                        elif learner == 'nstep16':
                            run = lambda: vec.nstep_run(steps, 16, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                        else:
                            run = lambda: vec.lambda_run(steps, LAM, K, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                        vec._ensure_q(0.0)
                        for _ in range(warmup):
                            run()
                        vec.engine.timer_begin()
                        for _ in range(launches):
                            run()
                        ms = vec.engine.timer_end()
                        rate = N * steps * launches / (ms * 1e-3)
                        td = rate if learner == 'td' else td
                        row = dict(grid=name, S=spec.S, N=N, method=method, learner=learner, K=K, lam=LAM if K else None,
                                   launches=launches, steps=steps, ms=round(ms, 3), env_steps_per_s=float('%.4g' % rate),
                                   frac_of_td=round(rate / td, 3))
                        out.append(row)
                        print(json.dumps(row), file=sys.stderr, flush=True)
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
                if any(k in row['Name'] for k in ('gu_td_kernel', 'gu_nstep_kernel', 'gu_lambda_kernel')):
                    stats[row['Name']] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rocprof', default=None, help='directory for a rocprofv3 kernel-trace run of the short form')
    ap.add_argument('--rocprof-only', action='store_true', help='skip the timed run: only the kernel-trace run of the short form')
    args = ap.parse_args()
    line = dict(tool='lambda_rate')
    if not args.rocprof_only:
        line['results'] = measure(args.launches, args.steps, args.warmup)
    if args.rocprof:
        line['rocprofv3_kernel_stats'] = rocprof_stats(args.rocprof, args.steps)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
