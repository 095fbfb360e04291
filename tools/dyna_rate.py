"""Real env-steps and planning updates per second of batched tabular Dyna-Q (gu_dyna_run, csrc/gu_dyna.hip) on one MI355X.

For each grid (8x8 open grid; a 32x32 maze of the generator), batch size N in {4096, 65536} and planning steps P in {0, 5, 50}: a
few warm-up launches, then `--launches` launches of `--steps` real steps (P = 50: a tenth of them, so that a launch does a similar
amount of work) timed with HIP events around the whole block.  The same engine's gu_td_run Q-learning is timed alongside as the
reference for P = 0 (the rows with P = null).  Prints ONE JSON line.  With --rocprof the same measurement is repeated once in a
child process under `rocprofv3 --kernel-trace --stats` (a short form: 20 launches per point) and the kernels' average duration per
instantiation is added to the line.

    python tools/dyna_rate.py [--rocprof DIR] > profiles/dyna_rate.json
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

SIZES = (4096, 65536)
PLANNING = (None, 0, 5, 50)  # None: gu_td_run Q-learning on the same engine


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
                for P in PLANNING:
                    T = steps if P is None or P < 50 else max(1, steps // 10)
                    vec._ensure_q(0.0)
                    vec._ensure_model(clear=True)

                    def launch():
                        if P is None:
                            vec.td_run(T, 'q_learning', alpha=0.1, discount_factor=0.99, epsilon=0.1)
                        else:
                            vec.dyna_run(T, P, alpha=0.1, discount_factor=0.99, epsilon=0.1)
                    for _ in range(warmup):
                        launch()
                    vec.engine.timer_begin()
                    for _ in range(launches):
                        launch()
                    ms = vec.engine.timer_end()
                    real = N * T * launches / (ms * 1e-3)
                    out.append(dict(grid=name, S=spec.S, N=N, P=P, kernel='gu_td_run' if P is None else 'gu_dyna_run', launches=launches,
                                    steps=T, ms=round(ms, 3), env_steps_per_s=float('%.4g' % real),
                                    planning_updates_per_s=float('%.4g' % (real * (P or 0)))))
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
                if 'gu_dyna_kernel' in row['Name'] or 'gu_td_kernel' in row['Name']:
                    stats[row['Name']] = dict(calls=int(row['Calls']), average_us=round(float(row['AverageNs']) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rocprof', default=None, help='directory for a rocprofv3 kernel-trace run of the short form')
    args = ap.parse_args()
    line = dict(tool='dyna_rate', results=measure(args.launches, args.steps, args.warmup))
    if args.rocprof:
        line['rocprofv3_kernel_stats'] = rocprof_stats(args.rocprof, args.steps)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
