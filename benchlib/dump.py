"""bench.py --dump-outputs DIR: what the timed path computed in its last launch, as a caller of that path receives it, so that two
builds of the project can be compared output for output on identical inputs.

The timed path is `gu_rollout` with trajectory rows: a caller reads obs / reward / done as int32[T, N] (Engine.read_trajectory).
They are written as float32 (exact: every value is far below 2**24), together with the env ids and step indices they hold, one
.npy file per array.  At the headline size the rows are 786 MB, so a fixed sample of env columns (drawn with a fixed seed) and,
for very long launches, of rows keeps the files under MAX_BYTES in all."""
import os

import numpy as np

MAX_BYTES = 64 << 20
MAX_ENVS = 4096  # env columns kept at most (4096 x 1000 steps x 3 arrays x 4 bytes = 49 MB)
SAMPLE_SEED = 20240601
READ_BYTES = 32 << 20  # rows read from the device per call


def sample(n_rows, n_envs, seed=SAMPLE_SEED):
    """(row indices, env column indices), both sorted: every row and env if they fit, else a seeded sample that does."""
    rng = np.random.default_rng(seed)
    budget = MAX_BYTES - (1 << 20)  # (room for the index arrays and the .npy headers)
    per_cell = 3 * 4
    rows = np.arange(n_rows)
    if n_rows * per_cell > budget:
        rows = np.sort(rng.choice(n_rows, budget // per_cell, replace=False))
    n_cols = min(n_envs, MAX_ENVS, max(1, budget // (len(rows) * per_cell)))
    cols = np.arange(n_envs) if n_cols == n_envs else np.sort(rng.choice(n_envs, n_cols, replace=False))
    return rows, cols


def dump_trajectory(eng, N, T, out_dir, env_id0=0, prefix=''):
    """Write the sampled trajectory rows of the engine's last launch to out_dir/<prefix><name>.npy; returns the paths."""
    rows, cols = sample(T, N)
    out = {k: np.empty((len(rows), len(cols)), np.float32) for k in ('obs', 'reward', 'done')}
    chunk = max(1, READ_BYTES // (3 * 4 * N))
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        lo, hi = np.searchsorted(rows, [t0, t1])
        if lo == hi:
            continue
        got = eng.read_trajectory(t0, t1 - t0)
        for k in out:
            out[k][lo:hi] = got[k][rows[lo:hi] - t0][:, cols]
    out['env_id'] = (env_id0 + cols).astype(np.float64)
    out['step'] = rows.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, arr in out.items():
        path = os.path.join(out_dir, prefix + name + '.npy')
        np.save(path, arr)
        paths.append(path)
    return paths
