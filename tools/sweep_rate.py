"""Pops per second of batched prioritized sweeping (gu_sweep_run, csrc/gu_sweep.hip) on one MI355X, next to the planning updates
per second of Dyna-Q (gu_dyna_run) at the same shapes, in the same process on the same device.

For each grid (8x8 open grid; a 32x32 maze of the generator) and planning steps P in {5, 50}, with 65 536 learners: fresh tables, model
and queue, a few warm-up launches, then `--launches` launches of `--steps` real steps (P = 50: a tenth of them) timed with HIP events
around the whole block.  A planning slot is used only while the learner's queue holds a pair, so the tool also reports how the slots
were spent, from the two counters the kernel keeps per learner (include/gu.h: gu_diag_sweep_heap, slot 0 of the raw heap; read for the
first `--sample` learners) and the queue sizes of all learners after every timed launch:

    pops_per_s        pops of all learners per second (sample's pops per slot x slots per second)
    inserts_per_pop   inserts that changed a queue (a new pair, or a larger key for a queued one) per pop
    mean_queue_size   mean over learners and timed launches of the size after the launch
    unused_share      planning slots that found the queue empty / all planning slots

The learners learn while they are measured: a launch late in a run sees emptier queues than an early one, which is what
unused_share shows.  Prints ONE JSON line.

    python tools/sweep_rate.py > profiles/sweep_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dyna_rate import grids  # noqa: E402  (the same two grids)

PLANNING = (5, 50)


def _counters(vec, sample):
    word = vec.engine.diag_sweep_heap(0, sample)['heap'][:, 0]
    return (word & np.uint64(0xFFFFFFFF)).astype(np.int64), (word >> np.uint64(32)).astype(np.int64)


def measure(N, launches, steps, warmup, sample, theta):
    import griduniverse_amd as gua
    out = []
    sample = min(sample, N)
    np.random.seed(0)  # (the maze generator draws from numpy's global stream as well as from random's)
    for name, spec in grids().items():
        vec = gua.VecGridUniverse(N, template=spec, seed=1)
        try:
            for P in PLANNING:
                T = steps if P < 50 else max(1, steps // 10)
                row = dict(grid=name, S=spec.S, N=N, P=P, theta=theta, launches=launches, steps=T)
                for kernel in ('gu_sweep_run', 'gu_dyna_run'):
                    vec.reset()
                    vec._ensure_q(0.0)
                    vec._ensure_queue()
                    vec.engine.sweep_init()  # empty model, empty queue, counters at zero

                    def launch():
                        if kernel == 'gu_sweep_run':
                            vec.sweep_run(T, P, theta=theta, alpha=0.1, discount_factor=0.99, epsilon=0.1)
                        else:
                            vec.dyna_run(T, P, alpha=0.1, discount_factor=0.99, epsilon=0.1)
                    for _ in range(warmup):
                        launch()
                    if kernel == 'gu_dyna_run':
                        vec.engine.timer_begin()
                        for _ in range(launches):
                            launch()
                        ms = vec.engine.timer_end()
                        row['dyna_ms'] = round(ms, 3)
                        row['dyna_planning_updates_per_s'] = float('%.4g' % (N * T * launches * P / (ms * 1e-3)))
                        continue
                    pops0, ins0 = _counters(vec, sample)
                    sizes, ms = [], 0.0
                    for _ in range(launches):  # (timed one by one: the sizes are read between the launches)
                        vec.engine.timer_begin()
                        launch()
                        ms += vec.engine.timer_end()
                        sizes.append(float(_sizes(vec).mean()))
                    pops1, ins1 = _counters(vec, sample)
                    pops, ins = int((pops1 - pops0).sum()), int((ins1 - ins0).sum())  # (far below 2^32 per learner and run)
                    slots = sample * T * launches * P
                    per_slot = pops / slots
                    row.update(ms=round(ms, 3), env_steps_per_s=float('%.4g' % (N * T * launches / (ms * 1e-3))),
                               pops_per_s=float('%.4g' % (per_slot * N * T * launches * P / (ms * 1e-3))),
                               inserts_per_pop=round(ins / max(pops, 1), 3), mean_queue_size=round(float(np.mean(sizes)), 2),
                               unused_share=round(1.0 - per_slot, 4), sample=sample)
                row['pops_per_dyna_update'] = round(row['pops_per_s'] / row['dyna_planning_updates_per_s'], 4)
                out.append(row)
        finally:
            vec.close()
    return out


def _sizes(vec):
    """int32[N] queue sizes without the keys (the key planes of 65 536 learners on 1024 states are 2 GiB)."""
    from griduniverse_amd import _lib
    eng = vec.engine
    size = np.empty(eng.N, np.int32)
    _lib.check(eng.lib.gu_sweep_get_queue(eng._h, 0, eng.N, None, _lib.ptr(size)))
    return size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--learners', type=int, default=65536)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=1024, help='learners whose counters are read')
    ap.add_argument('--theta', type=float, default=1e-4)
    args = ap.parse_args()
    print(json.dumps(dict(tool='sweep_rate', results=measure(args.learners, args.launches, args.steps, args.warmup, args.sample, args.theta))))


if __name__ == '__main__':
    main()
