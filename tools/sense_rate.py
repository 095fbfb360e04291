"""Env-views per second and bytes written per second of the sensor kernel (gu_sense_trajectory, csrc/gu_sense.hip) on one MI355X,
with the rollout that wrote the rows measured in the same run on the same engine as the yardstick for the store rate.

65 536 envs on a 32x32 maze of the generator, T = 1000 rows from a uniform rollout with auto-reset.  For the egocentric view at
r = 1, 2, 3, 7 and the whole-grid view: one warm-up pass over the rows, then at least `--passes` passes and `--min-gib` GiB of
views timed with HIP events around the whole block, the views staying in the engine's scratch memory (view = NULL: device time,
no copy).  A pass is cut into calls of at most `--call-mib` of views (the library takes at most 4 GiB per call).  Prints ONE
JSON line.

    python tools/sense_rate.py > profiles/sense_rate.json
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ((1, 'ego'), (2, 'ego'), (3, 'ego'), (7, 'ego'), (0, 'grid'))


def measure(N, T, min_passes, min_bytes, call_bytes, launches):
    import griduniverse_amd as gua
    from griduniverse_amd.grid import GridSpec
    random.seed(0)
    spec = GridSpec.from_env(gua.GridUniverseEnv(grid_shape=(32, 32), random_maze=True))
    vec = gua.VecGridUniverse(N, template=spec, seed=1, auto_reset=True)
    eng = vec.engine
    out = []
    try:
        vec.reset()
        eng.reserve_trajectory(T)
        for _ in range(3):
            eng.rollout(T, 'uniform', True, True, False)
        eng.timer_begin()
        for _ in range(launches):
            eng.rollout(T, 'uniform', True, True, False)
        ms = eng.timer_end()
        out.append(dict(kernel='rollout', N=N, T=T, launches=launches, ms=round(ms, 3), bytes_per_env_step=12,
                        env_steps_per_s=float('%.4g' % (N * T * launches / (ms * 1e-3))),
                        bytes_written_per_s=float('%.4g' % (12.0 * N * T * launches / (ms * 1e-3)))))
        for r, mode in MODES:
            V = spec.S if mode == 'grid' else (2 * r + 1) ** 2
            rows = max(1, min(T, call_bytes // (N * V)))
            passes = max(min_passes, -(-min_bytes // (N * T * V)))  # a timed window of at least min_bytes of views

            def one_pass():
                for t0 in range(0, T, rows):
                    eng.sense_device(min(rows, T - t0), t0, r, mode)

            one_pass()
            eng.timer_begin()
            for _ in range(passes):
                one_pass()
            ms = eng.timer_end()
            views = N * T * passes
            out.append(dict(kernel='sense', mode=mode, radius=None if mode == 'grid' else r, bytes_per_view=V, N=N, T=T, passes=passes,
                            rows_per_call=rows, ms=round(ms, 3), env_views_per_s=float('%.4g' % (views / (ms * 1e-3))),
                            bytes_written_per_s=float('%.4g' % (float(V) * views / (ms * 1e-3)))))
    finally:
        vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=1000)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--min-gib', type=int, default=64)
    ap.add_argument('--call-mib', type=int, default=1024)
    ap.add_argument('--rollout-launches', type=int, default=100)
    args = ap.parse_args()
    from griduniverse_amd import _lib
    line = dict(tool='sense_rate', library=os.path.basename(_lib.LIB_PATH), grid='maze32', S=1024,
                results=measure(args.envs, args.rows, args.passes, args.min_gib << 30, args.call_mib << 20, args.rollout_launches))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
