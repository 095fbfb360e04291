"""Env-steps per second of the box kernels (gu_set_boxes; csrc/gu_boxes.hip, csrc/gu_td.hip) on one MI355X, beside the door kernels of
the same shape in the same run: the door kernel is the same loop with a gate and no second round of reads, so it is the yardstick.

On `--envs` (65 536) envs on a 32x32 maze of the generator and on the open 8x8 grid, with 1 and with 3 boxes: uniform rollouts with
int32 rows and with statistics only.  td_run (Q-learning) with 1 box on the 8x8 grid only: a table has S << b rows, 4096 there and
2^20 on the maze, which 65 536 learners cannot hold.  The door engine of a pair has two slots (a key and a lever; tables of S << 2
rows).  The two engines of a pair live in ONE process and take turns: after a few warm-up launches each, `--rounds` rounds of
`--launches` launches of `--steps` steps on the one, then on the other, each block timed with HIP events.  Prints ONE JSON line; every
box row carries its ratio to the door row of its pair, and the time of its first and of its last round.

    python tools/boxes_rate.py > profiles/boxes_rate.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.doors_rate import grids, spread, timed  # noqa: E402

MODES = ('doors', 'boxes')


def pair(spec, N, n_boxes, launch, prepare, rounds, launches, warmup):
    """ms of each round of `launches` launches on the engine with two door slots and the one with `n_boxes` boxes, taking turns."""
    import griduniverse_amd as gua
    vecs = [gua.VecGridUniverse(N, template=spec, seed=1) for _ in MODES]
    try:
        key, door0, lever, door1 = spread(spec, 4)
        vecs[0].set_doors({0: door0, 1: door1}, keys={0: key}, levers={1: lever})
        cells = [c for c in spread(spec, 2 * n_boxes + 2) if c not in spec.starts][:2 * n_boxes]
        vecs[1].set_boxes(cells[0::2], cells[1::2])
        ms = [[] for _ in vecs]
        for vec in vecs:
            prepare(vec)
            vec.reset()
            for _ in range(warmup):
                launch(vec)
            vec.engine.sync()
        for _ in range(rounds):
            for k, vec in enumerate(vecs):
                ms[k].append(timed(vec, launch, launches))
        return ms, [vec.engine.rollout_last_form()['family'] for vec in vecs]
    finally:
        for vec in vecs:
            vec.close()


def measure(N, rounds, launches, steps, warmup):
    rows = ('rollout_rows', lambda v: v.engine.rollout(steps, 'uniform', True, True), lambda v: v.engine.reserve_trajectory(steps))
    stats = ('rollout_stats', lambda v: v.engine.rollout(steps, 'uniform', True, False, stats=True), lambda v: None)
    td = ('td_q_learning', lambda v: v.engine.td_run(steps, 'q_learning'), lambda v: v._ensure_q(0.0))
    out = []
    for name, spec in grids():
        for n_boxes, kinds in ((1, (rows, stats) + ((td,) if spec.S <= 64 else ())), (3, (rows, stats))):
            for kind, launch, prepare in kinds:
                per_round, forms = pair(spec, N, n_boxes, launch, prepare, rounds, launches, warmup)
                ms = [sum(r) for r in per_round]
                rates = [N * steps * launches * rounds / (m * 1e-3) for m in ms]
                for mode, m, rate, form, rs in zip(MODES, ms, rates, forms, per_round):
                    out.append(dict(grid=name, kind=kind, mode=mode, boxes=n_boxes if mode == 'boxes' else 0, slots=2 if mode == 'doors' else 0, N=N, S=spec.S,
                                    rounds=rounds, launches=launches, steps=steps, ms=round(m, 3), env_steps_per_s=float('%.4g' % rate),
                                    ratio_to_doors=round(rate / rates[0], 3), rollout_family=form if kind.startswith('rollout') else None,
                                    first_round_ms=round(rs[0], 3), last_round_ms=round(rs[-1], 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(dict(tool='boxes_rate', results=measure(args.envs, args.rounds, args.launches, args.steps, args.warmup))))


if __name__ == '__main__':
    main()
