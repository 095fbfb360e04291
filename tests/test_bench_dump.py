"""bench.py --dump-outputs on CPU, through the oracle-backed stub engine: the files hold the trajectory rows of the LAST timed
launch (checked against the C oracle advanced by the same launches), every run writes the same bytes, --steps is the number of
timed launches, and the files stay float32 / float64 and under 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from benchlib import dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_ON_STUB = os.path.join(ROOT, 'tests', '_bench_stub.py')
NAMES = {'obs', 'reward', 'done', 'env_id', 'step'}


def _bench(out_dir, steps, *extra, full=True):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, BENCH_ON_STUB, '--gpus', '1', '--envs', '512', '--T', '40', '--steps', str(steps), '--warmup', '1',
           '--no-cpu-baseline', '--no-strong-c4', '--no-configs', '--no-other-modes', '--detail', '', '--dump-outputs', str(out_dir)]
    proc = subprocess.run(cmd + (['--full'] if full else []) + list(extra), env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    files = {n: np.load(os.path.join(str(out_dir), n + '.npy')) for n in NAMES}
    assert set(f[:-4] for f in os.listdir(str(out_dir))) == NAMES
    return json.loads(lines[0]), files


def _oracle_rows(launches, N, T):
    """Trajectory rows of launch number `launches` of the bench workload, by the C oracle from reset."""
    import griduniverse_amd as gua
    from benchlib.workloads import WORKLOAD_SEED, build_workload
    from oracle import c_oracle as C
    template, _ = build_workload('c3')
    spec, seed = gua.GridSpec.from_env(template), WORKLOAD_SEED['c3']
    grid = C.Grid(spec.W, spec.H, spec.wall, spec.lava, spec.goal, spec.reward, spec.starts)
    st = C.State(N, 0)
    st.pos[:] = spec.starts[0]
    C.reset(grid, seed, st)
    for _ in range(launches):
        out = C.rollout(grid, seed, st, T, True)
    return out


def test_dump_is_the_last_timed_launch_and_the_same_on_every_run(tmp_path):
    line, a = _bench(tmp_path / 'a', 2)
    _, b = _bench(tmp_path / 'b', 2)
    for n in NAMES:
        assert a[n].dtype in (np.float32, np.float64), n
        assert a[n].tobytes() == b[n].tobytes(), n
    assert sum(os.path.getsize(str(tmp_path / 'a' / (n + '.npy'))) for n in NAMES) <= dump.MAX_BYTES
    assert a['obs'].shape == (40, 512) and np.array_equal(a['env_id'], np.arange(512)) and np.array_equal(a['step'], np.arange(40))
    # launches_total counts the K instrumented launches behind the timed block too: the last timed launch is K before the end
    assert line['steps'] == 2 and line['timing']['blocks'] == 1
    want = _oracle_rows(line['timing']['launches_total'] - 2, 512, 40)
    for k in ('obs', 'reward', 'done'):
        assert np.array_equal(a[k], want[k].astype(np.float32)), k
    # one more timed launch: two more launches in all (timed + instrumented), and other rows
    line3, c = _bench(tmp_path / 'c', 3)
    assert line3['steps'] == 3 and line3['timing']['launches_total'] == line['timing']['launches_total'] + 2
    assert not np.array_equal(a['obs'], c['obs'])


@pytest.mark.parametrize('form', ['ranks', 'single-process'])
def test_a_plain_run_ends_with_its_timed_launches_and_dumps_what_a_full_run_dumps(tmp_path, form):
    """Without --full: no checks, no launch behind the timed block (the dump is the run's last launch), and the same rows as a
    --full run, whose instrumented block adds K launches behind them (the single-process form has none)."""
    extra = ['--single-process'] if form == 'single-process' else []
    line, a = _bench(tmp_path / 'a', 2, *extra, full=False)
    full, b = _bench(tmp_path / 'b', 2, *extra)
    for key in ('bit_exact_vs_oracle', 'bit_exact_vs_reference_digest', 'final_state_vs_oracle', 'cpu_baseline', 'strong_c4', 'other_modes',
                'configs', 'rccl'):
        assert key not in line, key
    assert full['bit_exact_vs_oracle'] is True and full['final_state_vs_oracle']['equal'] is True
    assert line['steps'] == 2 and line['timing']['launches_total'] + (2 if form == 'ranks' else 0) == full['timing']['launches_total']
    for n in NAMES:
        assert a[n].tobytes() == b[n].tobytes(), n
    want = _oracle_rows(line['timing']['launches_total'], 512, 40)
    for k in ('obs', 'reward', 'done'):
        assert np.array_equal(a[k], want[k].astype(np.float32)), k


def test_dump_sample_stays_under_the_budget():
    rows, cols = dump.sample(1000, 65536)  # the headline launch: every step, a seeded sample of 4096 envs
    assert np.array_equal(rows, np.arange(1000)) and len(cols) == dump.MAX_ENVS and len(np.unique(cols)) == len(cols)
    assert np.array_equal(cols, dump.sample(1000, 65536)[1]) and cols.max() < 65536
    assert len(rows) * len(cols) * 12 <= dump.MAX_BYTES
    rows, cols = dump.sample(10 ** 7, 8)  # a launch too long for every row
    assert len(rows) * len(cols) * 12 <= dump.MAX_BYTES and rows.max() < 10 ** 7 and np.all(np.diff(rows) > 0)
