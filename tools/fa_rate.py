"""Env-steps per second of batched semi-gradient SARSA / Q-learning on binary features (gu_fa_run, csrc/gu_fa.hip) on one MI355X,
with tabular gu_td_run measured in the same run as the yardstick (`learner: "td"`).

65 536 learners on the open 8x8 grid and on a 32x32 maze of the generator: td_run, fa_run with identity features (what the
phi lookup and the K-generic code cost), and -- on the maze -- fa_run with tile_coding(32, 32, K, 4) for K = 1, 2, 4, 8 and
tile_coding(32, 32, 8, 8), each with the bytes of weights a learner holds.  Then td_run against tile_coding(32, 32, 4, 4) once
more at 16 384 learners, where the weights are a third of the tabular tables.  Both methods everywhere.

Per point: a few warm-up launches, then `--launches` launches of `--steps` steps timed with HIP events around the whole block;
the block is timed `--repeats` times and every time is kept (the spread is in the file).  Prints ONE JSON line.  With --rocprof
the identity-feature and td points are repeated once in a child process under `rocprofv3 --kernel-trace --stats` (a short form)
and the kernels' average duration per instantiation is added to the line.

    python tools/fa_rate.py [--rocprof DIR] > profiles/fa_rate.json
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


def grids():
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    maze = gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True)
    return {'open8x8': GridSpec(8, 8, [0], [63], [], []), 'maze32': GridSpec.from_env(maze)}


def points(short):
    """(grid, N, label, features): features None = td_run."""
    from griduniverse_amd.algorithms.function_approximation import one_hot, tile_coding
    out = []
    for grid, S in (('open8x8', 64), ('maze32', 1024)):
        out.append((grid, 65536, 'td', None))
        out.append((grid, 65536, 'fa identity', one_hot(S)))
    if short:
        return out
    for K in (1, 2, 4, 8):
        out.append(('maze32', 65536, 'fa tile_coding(32, 32, %d, 4)' % K, tile_coding(32, 32, K, 4)))
    out.append(('maze32', 65536, 'fa tile_coding(32, 32, 8, 8)', tile_coding(32, 32, 8, 8)))
    out.append(('maze32', 16384, 'td', None))
    out.append(('maze32', 16384, 'fa tile_coding(32, 32, 4, 4)', tile_coding(32, 32, 4, 4)))
    return out


def measure(launches, steps, warmup, repeats, short=False):
    import griduniverse_amd as gua
    specs = grids()
    out = []
    for grid, N, label, feats in points(short):
        spec = specs[grid]
        vec = gua.VecGridUniverse(N, template=spec, seed=1)
        try:
            for method in ('q_learning', 'sarsa'):
                if feats is None:
                    K, per_learner = None, spec.S * 32
                    vec._ensure_q(0.0)
                    run = lambda: vec.td_run(steps, method, alpha=0.1, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                else:
                    K, per_learner = feats[0].shape[1], feats[1] * 32
                    vec.set_features(feats[0], feats[1], 0.0)
                    run = lambda: vec.fa_run(steps, method, alpha=0.1 / K, discount_factor=0.99, epsilon=0.1)  # noqa: E731
                vec.reset()
                for _ in range(warmup):
                    run()
                times = []
                for _ in range(repeats):
                    vec.engine.timer_begin()
                    for _ in range(launches):
                        run()
                    times.append(round(vec.engine.timer_end(), 3))
                ms = sorted(times)[len(times) // 2]
                out.append(dict(grid=grid, S=spec.S, N=N, learner=label, K=K, method=method, table_bytes_per_learner=per_learner,
                                launches=launches, steps=steps, ms=times, env_steps_per_s=float('%.4g' % (N * steps * launches / (ms * 1e-3)))))
        finally:
            vec.close()
    return out


def rocprof_stats(out_dir, steps):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
           sys.executable, os.path.abspath(__file__), '--short', '--launches', '20', '--warmup', '1', '--repeats', '1', '--steps', str(steps)]
    with open(os.path.join(out_dir, 'rocprofv3.log'), 'w') as log:
        subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, check=True, timeout=600)
    stats = {}
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if 'gu_td_kernel' in row['Name'] or 'gu_fa_kernel' in row['Name']:
                    stats[row['Name']] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--short', action='store_true', help='td_run and identity features only (the form --rocprof traces)')
    ap.add_argument('--rocprof', default=None, help='directory for a rocprofv3 kernel-trace run of the short form')
    args = ap.parse_args()
    line = dict(tool='fa_rate', results=measure(args.launches, args.steps, args.warmup, args.repeats, args.short))
    if args.rocprof:
        line['rocprofv3_kernel_stats'] = rocprof_stats(args.rocprof, args.steps)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
