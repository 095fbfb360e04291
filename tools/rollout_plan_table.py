"""The rollout dispatch as a table of cases: which kernel, layout and launch shape every kind of gu_rollout call runs on.

    python tools/rollout_plan_table.py --record     writes tests/golden/rollout_plan.json (on an MI355X)
    python tools/rollout_plan_table.py --check      replays every row on the device and compares

Every row is one launch: the inputs the launcher decides by (batch, grid, policy, flags, length, wind / trail / straddle / entry
state; the launch-shape options in force are kept once per section) followed by the twelve words of Engine.rollout_last_form().  The rows are grouped in
sections named after the threshold of csrc/gu_rollout_plan.hpp that their cases bracket.  tests/test_rollout_plan.py checks the
planner against the file without a device, tests/test_gpu_rollout_plan.py replays a few rows on one.  The file in the tree was
recorded on the dispatch ladder as it stood BEFORE the planner existed: it is what the planner is measured against.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rollout_plan.json')
OPTS = ('rollout_block', 'rollout_rows', 'rows_copies', 'rollout_multi', 'rollout_multi_k', 'rollout_multi_copies', 'rollout_xcd',
        'traj_layout', 'rollout_half_waves', 'rollout_pace', 'rollout_entry', 'pace_record')
INPUTS = ('N', 'W', 'H', 'grids', 'multi_start', 'policy', 'flags', 'T', 'wind', 'gust', 'trail', 'straddle', 'entry') + OPTS
FORM = ('family', 'layout', 'map', 'block', 'workgroups', 'lds_bytes', 'flags', 'K', 'row_shift', 'stream_words', 'pace_slot', 'pace_mode')
POLICIES = ('uniform', 'stream', 'greedy', 'sample')
F_AUTO, F_TRAJ, F_STATS, F_PACKED = 1, 2, 4, 16


def case(N, W, H, policy=0, flags=F_AUTO | F_STATS, T=64, grids=1, multi_start=0, wind=0, gust=0, trail=0, straddle=0, entry=0, **opts):
    assert set(opts) <= set(OPTS), opts
    return dict(N=N, W=W, H=H, grids=grids, multi_start=multi_start, policy=policy, flags=flags, T=T, wind=wind, gust=gust, trail=trail,
                straddle=straddle, entry=entry, opts=opts)


def kinds(policies=(0, 1, 2, 3), autos=(F_AUTO, 0), rows=(0, F_TRAJ, F_PACKED), stats=(F_STATS, 0)):
    return [(p, a | r | s) for p in policies for a in autos for r in rows for s in stats if r or s]


def sections():
    """[(name, [case, ...])]: each axis at the values on either side of every threshold of the plan; all cases of a section run under
    the same options.  (No decision asks whether statistics are kept: they are, everywhere.)"""
    out = []
    every = kinds(autos=(F_AUTO,), stats=(F_STATS,))  # four policies x no rows / int32 / packed, with auto-reset
    # workgroups of 256 against the CU count (256): n_cu / 8, / 4, / 2, one per CU; triples and half waves, the int32 and packed limits
    for lo, hi, what in ((8192, 8448, 'blocks * 8 > n_cu: half waves begin'), (16384, 16640, 'blocks * 4 <= n_cu: triples with pair tables, half waves end')):
        out.append(('N %d / %d -- %s' % (lo, hi, what), [case(n, 32, 32, p, f) for n in (lo, hi) for p, f in kinds(policies=(0,), stats=(F_STATS,)) + kinds(policies=(1,), autos=(F_AUTO,), stats=(F_STATS,))]))
    for lo, hi, what in ((32768, 33024, 'blocks <= n_cu / 2: int32 rows on the row kernel'), (65536, 65792, 'blocks <= n_cu: packed rows, pairs, sampled int32 rows')):
        out.append(('N %d / %d -- %s' % (lo, hi, what), [case(n, 32, 32, p, f) for n in (lo, hi) for p, f in kinds(policies=(0, 1), autos=(F_AUTO,), stats=(F_STATS,)) + kinds(policies=(2, 3), stats=(F_STATS,))]))
    out.append(('N 1 / 65 / 1000 -- ragged batches', [case(n, 32, 32, p, f) for n in (1, 65, 1000) for p, f in every]))
    out.append(('N 262144 / 262400 -- pace eligibility: more than four waves per SIMD',
                [case(n, 32, 32, 0, f) for n in (262144, 262400) for f in (F_AUTO | F_STATS, F_AUTO | F_TRAJ, F_AUTO | F_PACKED)]))
    grids = (((8, 8),), 'small grid'), (((12, 12), (13, 13)), 'K = 4 tables fit'), (((32, 32),), 'pair tables fit'), (((34, 33), (34, 34)), 'pair tables'), \
        (((44, 45), (45, 45)), 'K = 2 tables fit'), (((60, 60), (61, 61)), 'pi_lds: thresholds behind the planes'), (((100, 100), (101, 101)), 'row table fits'), \
        (((147, 148), (148, 148)), 'three planes for greedy'), (((181, 181), (182, 181)), 'MAP 1 -> 3'), (((404, 404), (405, 404)), 'MAP 3 -> 0')
    for shapes, what in grids:
        out.append(('grid %s -- %s' % (' / '.join('%dx%d' % s for s in shapes), what), [case(256, w, h, p, f) for w, h in shapes for p, f in kinds(policies=(0, 2, 3), autos=(F_AUTO,), stats=(F_STATS,))
                                                                                        if not (f & F_PACKED and w * h > 65536)]))  # (packed rows hold 16-bit states)
    out.append(('T 16 / 63 / 64 -- K-step kernel and pacing want 64 steps; staged stream words',
                [case(n, 32, 32, p, F_AUTO | F_STATS | r, T=t) for t in (16, 63, 64) for n in (256, 8192) for p in (0, 1) for r in (0, F_TRAJ, F_PACKED)]))
    out.append(('several start cells -- auto mode 2', [case(n, 32, 32, p, f, multi_start=1) for n in (256, 8192) for p, f in every]))
    # (value / policy tables need a single-grid engine: the uniform and stream policies only)
    multi = [case(768, w, w, p, f, grids=768 // g) for g in (1, 64, 128, 192, 256) for w in (8, 32) for p, f in kinds(policies=(0, 1), autos=(F_AUTO,), stats=(F_STATS,))]
    multi += [case(256, w, w, p, f, grids=256) for w in (45, 61, 101) for p, f in kinds(policies=(0, 1), autos=(F_AUTO,), stats=(F_STATS,))]
    multi += [case(768, 8, 8, p, f, grids=g, multi_start=1) for g in (768, 6) for p, f in kinds(policies=(0, 1), autos=(F_AUTO,), stats=(F_STATS,))]
    out.append(('multi-grid engines, group 1 / 64 / 128 / 192 / 256 -- per-wave staging, MAP 5 and its workgroup size', multi))
    out.append(('wind', [case(n, w, w, p, f, wind=1, gust=g) for n, w, gusts in ((256, 32, (0, 1)), (8192, 32, (0,)), (256, 148, (0,))) for g in gusts
                         for p, f in kinds(autos=(F_AUTO,), rows=(0, F_TRAJ), stats=(F_STATS,))]))
    out.append(('trail', [case(n, 32, 32, p, f, trail=1) for n in (256, 4096) for p, f in kinds(autos=(F_AUTO,), rows=(F_TRAJ, F_PACKED), stats=(F_STATS,))]))
    out.append(('straddle -- a launch across a multiple of 2^32 steps goes to the general kernel', [case(n, 32, 32, p, f, straddle=1) for n in (256, 4096) for p, f in every]))
    out.append(('entry -- the launch follows a rollout', [case(n, 32, 32, p, f, entry=1) for n in (256, 33024) for p, f in every]))
    out.append(('entry, option rollout_entry = 0', [case(256, 32, 32, p, f, entry=1, rollout_entry=0) for p, f in every]))
    settings = [{'rollout_rows': v} for v in (0, 1, 2, 3)] + [{'rollout_multi': v} for v in (0, 1)] + [{'rollout_multi_k': v} for v in (2, 4)] + \
        [{'traj_layout': v} for v in (0, 1)] + [{'rollout_half_waves': v} for v in (0, 1)] + [{'rollout_block': v} for v in (64, 1024)] + \
        [{'rollout_pace': v} for v in (0, 200)] + [{'rollout_pace': 200, 'pace_record': 0}, {'rollout_xcd': 1}, {'rollout_multi_copies': 2},
                                                  {'rows_copies': 1}, {'rows_copies': 32}, {'rollout_rows': 3, 'traj_layout': 1}, {'rollout_rows': 1, 'rollout_multi': 0}]
    for o in settings:
        name = 'option ' + ', '.join('%s = %d' % kv for kv in sorted(o.items()))
        rows = [case(n, 32, 32, p, F_AUTO | F_STATS | r, **o) for n, p in ((4096, 0), (16640, 0), (4096, 2)) for r in (0, F_TRAJ, F_PACKED)]
        rows += [case(256, w, w, 0, F_AUTO | F_STATS, **o) for w in (12, 13)] + [case(768, 8, 8, 0, F_AUTO | F_STATS | F_TRAJ, grids=g, **o) for g in (768, 6)]
        out.append((name, rows))
    out.append(('the benchmark shape: 65536 x 1000, int32 rows -- the paced launch', [case(65536, 32, 32, 0, F_AUTO | F_TRAJ, T=1000), case(65536, 32, 32, 0, F_AUTO | F_PACKED, T=1000),
                                                                                    case(65536, 32, 32, 3, F_AUTO | F_TRAJ, T=1000)]))
    out.append(('the benchmark shape, option rollout_pace = 200', [case(65536, 32, 32, 0, F_AUTO | F_TRAJ, T=1000, rollout_pace=200)]))
    out.append(('the benchmark shape, option pace_record = 0, rollout_pace = 200', [case(65536, 32, 32, 0, F_AUTO | F_TRAJ, T=1000, rollout_pace=200, pace_record=0)]))
    return out


class Runner(object):
    """Launches cases, keeping one engine per (batch, grid) so that the whole table stays a matter of a minute: every case starts
    from a fresh reset with every option of the plan set as the case says."""

    def __init__(self):
        self.key, self.eng, self.cap, self.windy = None, None, 0, False

    def close(self):
        if self.eng is not None:
            self.eng.close()
        self.key = self.eng = None

    def engine(self, c):
        import numpy as np
        from griduniverse_amd import Engine, GridSpec
        key = (c['N'], c['W'], c['H'], c['grids'], c['multi_start'])
        if key != self.key:
            self.close()
            S = c['W'] * c['H']
            spec = GridSpec(c['W'], c['H'], [0, S // 2] if c['multi_start'] else [0], [S - 1], [], [])
            self.eng = Engine(c['N'], spec, seed=3)
            if c['grids'] > 1:
                self.eng.set_grids([spec] * c['grids'])
            else:
                self.eng.vi_set(np.zeros(S), np.full((S, 4), 0.25))
            self.key, self.cap, self.acts, self.windy = key, 0, 0, False
        return self.eng

    def run(self, c):
        """The form words of case `c`, and the option values that were in force."""
        import numpy as np
        eng = self.engine(c)
        S = c['W'] * c['H']
        for name in OPTS:
            eng.set_option(name, c['opts'].get(name))
        if not c['trail']:
            eng.trail_enable(0)
        if c['wind'] or self.windy:  # (wind and trail exclude each other; a multi-grid engine knows no wind)
            eng.set_wind(np.full(S, 4, np.uint8) if c['wind'] else None, 43691 if c['gust'] else 0)
            self.windy = bool(c['wind'])
        if c['trail']:
            eng.trail_enable(8)
        if c['flags'] & (F_TRAJ | F_PACKED) and self.cap < c['T']:
            eng.reserve_trajectory(c['T'])
            self.cap = c['T']
        if c['policy'] == 1 and self.acts < c['T']:
            eng.upload_actions(np.zeros((c['T'], c['N']), np.int32))
            self.acts = c['T']
        eng.reset()
        eng.set_state(tcount=np.full(c['N'], 2 ** 32 - 8 if c['straddle'] else 0, np.uint64))
        f = c['flags']
        if c['entry']:
            eng.rollout(1, 'uniform', bool(f & F_AUTO), False, stats=True)
        eng.rollout(c['T'], POLICIES[c['policy']], bool(f & F_AUTO), 'packed' if f & F_PACKED else bool(f & F_TRAJ), stats=bool(f & F_STATS))
        return eng.rollout_last_form()['words'], [eng.get_option(name) for name in OPTS]


def row_case(row):
    c = dict(zip(INPUTS, row))
    c['opts'] = {name: c.pop(name) for name in OPTS}
    return c


def load():
    """The table with every row in full: the inputs (the section's options among them), then the form words."""
    with open(GOLDEN) as f:
        table = json.load(f)
    k = len(INPUTS) - len(OPTS)
    for sec in table['sections']:
        sec['rows'] = [row[:k] + sec['options'] + row[k:] for row in sec['rows']]
    return table


def record():
    from griduniverse_amd import Engine
    info = Engine.device_info(0)
    runner, out = Runner(), []
    for name, cases in sections():
        rows, options = [], None
        for c in cases:
            form, opts = runner.run(c)
            assert options in (None, opts), (name, options, opts)
            options = opts
            rows.append([c[k] for k in INPUTS[:len(INPUTS) - len(OPTS)]] + form)
        out.append((name, options, rows))
        sys.stderr.write('%4d  %s\n' % (len(rows), name))
    runner.close()
    with open(GOLDEN, 'w') as f:
        f.write('{"n_cu": %d, "lds_per_cu": %d,\n "inputs": %s,\n "form": %s,\n "sections": [\n' % (int(info['cus']), int(info['lds_per_cu']), json.dumps(INPUTS), json.dumps(FORM)))
        f.write(',\n'.join('  {"name": %s, "options": %s, "rows": [\n%s]}' % (json.dumps(name), json.dumps(options), ',\n'.join('   ' + json.dumps(r, separators=(',', ':')) for r in rows))
                            for name, options, rows in out))
        f.write('\n ]}\n')
    print('%d rows in %d sections -> %s' % (sum(len(r) for _, _, r in out), len(out), GOLDEN))


def check():
    runner, bad, n = Runner(), 0, 0
    for sec in load()['sections']:
        for row in sec['rows']:
            form, _ = runner.run(row_case(row))
            n += 1
            if form != row[len(INPUTS):]:
                bad += 1
                print('%s\n  inputs %s\n  golden %s\n  device %s' % (sec['name'], row[:len(INPUTS)], row[len(INPUTS):], form))
    runner.close()
    print('%d of %d rows differ' % (bad, n))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--record', action='store_true')
    ap.add_argument('--check', action='store_true')
    args = ap.parse_args()
    if args.record:
        record()
    elif args.check:
        sys.exit(check())
    else:
        n = [len(c) for _, c in sections()]
        print('%d cases in %d sections' % (sum(n), len(n)))
