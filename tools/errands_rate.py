"""Env-steps per second of the errand kernels (gu_set_errands; csrc/gu_errands.hip, csrc/gu_td.hip) on one MI355X, beside the fruit
kernels of the same shape with the same number of fruit in the same run: the fruit kernel is the same loop without the instruction, so
it is the yardstick.

On `--envs` (65 536) envs on a 32x32 maze of the generator and on the open 8x8 grid: uniform rollouts with int32 rows and with
statistics only, five fruit (two kinds doubled) and three instructions (one of four kinds), and td_run (Q-learning) with two fruit and
two instructions of one kind each -- the errand tables have S << (2 + 1 + 1) rows, the fruit tables S << 2.  The two engines of a
pair live in ONE process and take turns: after a few warm-up launches each, `--rounds` rounds of `--launches` launches of `--steps`
steps on the one, then on the other, each block timed with HIP events.  Prints ONE JSON line; every errands row carries its ratio to the
fruit row of its pair, and the time of its first and of its last round.

    python tools/errands_rate.py > profiles/errands_rate.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fruit_rate import fruit_cells, grids, timed  # noqa: E402

MODES = ('fruit', 'errands')
CASES = {5: (['apple', 'lemon', 'melon', 'apple', 'lemon'], [['lemon', 'apple'], ['apple', 'apple', 'melon', 'lemon'], ['melon']]),
         2: (['apple', 'lemon'], [['apple'], ['lemon']])}


def pair(spec, N, F, launch, prepare, rounds, launches, warmup):
    """ms of each round of `launches` launches on the engine with F fruit and on the one with errands on the same F fruit, taking turns."""
    import griduniverse_amd as gua
    vecs = [gua.VecGridUniverse(N, template=spec, seed=1) for _ in MODES]
    try:
        kinds, instructions = CASES[F]
        cells = fruit_cells(spec, F)
        vecs[0].set_fruit(cells, kinds, (5, 5, 5))
        vecs[1].set_errands(cells, kinds, instructions)
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
        return ms, [vec.engine.rollout_last_form()['family'] for vec in vecs], [vec.engine.td_rows for vec in vecs]
    finally:
        for vec in vecs:
            vec.close()


def measure(N, rounds, launches, steps, warmup):
    import griduniverse_amd as gua
    kinds = [('rollout_rows', 5, lambda v: v.engine.rollout(steps, 'uniform', True, True), lambda v: v.engine.reserve_trajectory(steps)),
             ('rollout_stats', 5, lambda v: v.engine.rollout(steps, 'uniform', True, False, stats=True), lambda v: None),
             ('td_q_learning', 2, lambda v: v.engine.td_run(steps, 'q_learning'), lambda v: v._ensure_q(0.0))]
    out = []
    for name, spec in grids():
        for kind, F, launch, prepare in kinds:
            try:
                per_round, forms, rows = pair(spec, N, F, launch, prepare, rounds, launches, warmup)
            except gua.GuError as err:  # (tables that the device cannot hold: said, not hidden)
                out.append(dict(grid=name, kind=kind, mode='errands', fruits=F, N=N, S=spec.S, error=str(err)))
                continue
            ms = [sum(r) for r in per_round]
            rates = [N * steps * launches * rounds / (m * 1e-3) for m in ms]
            for mode, m, rate, form, rs, tr in zip(MODES, ms, rates, forms, per_round, rows):
                out.append(dict(grid=name, kind=kind, mode=mode, fruits=F, instructions=len(CASES[F][1]) if mode == 'errands' else 0, N=N, S=spec.S,
                                table_rows=tr if kind.startswith('td') else None, rounds=rounds, launches=launches, steps=steps, ms=round(m, 3),
                                env_steps_per_s=float('%.4g' % rate), ratio_to_fruit=round(rate / rates[0], 3),
                                rollout_family=form if kind.startswith('rollout') else None, first_round_ms=round(rs[0], 3), last_round_ms=round(rs[-1], 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    print(json.dumps(dict(tool='errands_rate', results=measure(args.envs, args.rounds, args.launches, args.steps, args.warmup))))


if __name__ == '__main__':
    main()
