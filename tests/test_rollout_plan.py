"""The rollout planner (csrc/gu_rollout_plan.hpp) against the table of launches recorded on an MI355X BEFORE the planner existed
(tests/golden/rollout_plan.json, tools/rollout_plan_table.py): a stand-alone host program builds a gu_engine from every row's inputs,
plans, and prints the form words -- no device, no libgu.so."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_the_plan_equals_every_recorded_launch(tmp_path):
    with open(os.path.join(ROOT, 'tests', 'golden', 'rollout_plan.json')) as f:
        table = json.load(f)
    n_in = len(table['inputs'])
    assert len(table['form']) == 12 and n_in == 25
    # (a row in full: the thirteen inputs of the case, the twelve options its section ran under, the form words)
    rows = [(sec['name'], row[:13] + sec['options'] + row[13:]) for sec in table['sections'] for row in sec['rows']]
    assert len(rows) > 800 and all(len(row) == n_in + 12 for _, row in rows)
    exe = str(tmp_path / 'rollout_plan_host')
    csrc = os.path.join(ROOT, 'griduniverse_amd', 'csrc')
    subprocess.check_call([HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-Wall', '-Wno-unused-function', '-o', exe,
                           os.path.join(ROOT, 'tests', 'rollout_plan_host.cpp'), os.path.join(csrc, 'gu_options.hip')])
    text = '%d %d\n' % (table['n_cu'], table['lds_per_cu']) + ''.join(' '.join(str(x) for x in row[:n_in]) + '\n' for _, row in rows)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    bad = [(name, dict(zip(table['inputs'], row[:n_in])), dict(zip(table['form'], row[n_in:])), dict(zip(table['form'], (int(x) for x in line.split()))))
           for (name, row), line in zip(rows, out) if [int(x) for x in line.split()] != row[n_in:]]
    assert not bad, '%d of %d rows differ; the first: %s\n inputs %s\n golden %s\n plan   %s' % ((len(bad), len(rows)) + bad[0])
