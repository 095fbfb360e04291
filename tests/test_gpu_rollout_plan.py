"""The launcher runs what the planner planned: rows of tests/golden/rollout_plan.json (recorded on the dispatch ladder as it stood
before csrc/gu_rollout_plan.hpp existed) replayed on the device -- one small launch per kernel family x row layout x MAP x pair /
half waves / per-wave grids / thresholds in LDS / straddle / entry table / XCD order x K, wind included -- and what
Engine.rollout_last_form() reports compared with the recorded words."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('rollout_plan_table', os.path.join(ROOT, 'tools', 'rollout_plan_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_launcher_runs_what_the_golden_table_says():
    from griduniverse_amd import Engine
    tool = _tool()
    table = tool.load()
    info = Engine.device_info(0)
    if (int(info['cus']), int(info['lds_per_cu'])) != (table['n_cu'], table['lds_per_cu']):
        pytest.skip('the table was recorded on a device of %d CUs with %d bytes of LDS each' % (table['n_cu'], table['lds_per_cu']))
    n_in, F = len(tool.INPUTS), tool.FORM
    picked = {}
    for sec in table['sections']:
        for row in sec['rows']:
            c, form = dict(zip(tool.INPUTS, row)), dict(zip(F, row[n_in:]))
            if c['N'] <= 16640 and c['T'] <= 64:  # small launches: the first row of every form
                picked.setdefault((form['family'], form['layout'], form['map'], form['flags'], form['K']), (sec['name'], row))
    assert len(picked) >= 40 and {k[0] for k in picked} == {1, 2, 3, 4} and {k[2] for k in picked} == {-1, 0, 1, 3, 5}
    runner = tool.Runner()
    try:
        assert Engine(64, runner_spec()).rollout_last_form()['words'] == [0] * len(F)  # (before the first rollout)
        for name, row in picked.values():
            got, _ = runner.run(tool.row_case(row))
            assert got == row[n_in:], (name, dict(zip(tool.INPUTS, row)), dict(zip(F, row[n_in:])), dict(zip(F, got)))
    finally:
        runner.close()


def runner_spec():
    from griduniverse_amd import GridSpec
    return GridSpec(4, 4, [0], [15], [], [])
