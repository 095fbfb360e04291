"""The device tests' own scaffold, checked without a device: the adapter registry of tests/_learners.py reaches every learner entry
point of the engine, and the shared comparisons of tests/_tabular_cases.py and tests/_learners.py fail when one element differs."""
import copy

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.engine import Engine
from griduniverse_amd.grid import GridSpec

from . import _td_oracle as TD
from ._fake_engine import PRESENT, Scripted
from ._learners import LEARNERS, _same_stores
from ._tabular_cases import GRIDS, SideBySide, _eps, _grid, _same, same_env_state


# ---------------------------------------------------------------------------------------------------------------- (a) completeness
def _runs_reached(learner):
    """The engine's *_run methods that one launch of the adapter reaches on an engine that holds every store."""
    vec = gua.VecGridUniverse(4, template=GridSpec(4, 4, [0], [15], [], []), engine_factory=Scripted)
    vec.engine.held = dict(PRESENT)
    learner.device(vec, 5)
    return [name for name, _ in vec.engine.calls if name.endswith('_run')]


def test_the_adapters_reach_every_learner_entry_point_of_the_engine():
    """A learner added to the engine without an adapter, or an adapter that drives another call than its own, fails here."""
    reached = dict((name, _runs_reached(learner)) for name, learner in LEARNERS.items())
    for name, runs in reached.items():
        assert len(runs) == 1, (name, runs)
    learners = set(n for n in dir(Engine) if n.endswith('_run') and not n.startswith('vi_'))
    assert len(learners) >= 14, sorted(learners)
    assert set(runs[0] for runs in reached.values()) == learners


# ---------------------------------------------------------------------------------------------------------------- (b) the helpers bite
GROUPS, PER_GROUP, T = 2, 3, 12


def _side():
    """Two groups of three Q-learners on the 4 x 4 grid, side by side, reset."""
    grid = _grid(GRIDS['default4x4']())
    side = SideBySide(TD.TdOracle(grid, 5, PER_GROUP, k * PER_GROUP, 0.5) for k in range(GROUPS))
    side.reset()
    return side


def _launch(o):
    return o.run(T, TD.Q_LEARNING, 0.25, 0.9, _eps(0.3))


class _Vec(object):
    """Stands in for a batch: get_state() answers what the restatements hold, as copies that a test may spoil."""

    def __init__(self, side):
        self.state = dict((k, side.cat(lambda o: getattr(o.state, k)).copy()) for k in ('pos', 'done', 'episode', 'tcount'))

    def get_state(self):
        return self.state


@pytest.fixture
def ran():
    """(the restatements after one launch, that launch's rows and statistics, the stand-in batch that agrees with them)."""
    side = _side()
    rows = side.run(_launch)
    assert (side.cat(lambda o: o.q) != 0.5).any() and rows['obs'].shape == (T, GROUPS * PER_GROUP)
    return side, rows, _Vec(side)


def _spoil(a, index):
    a[index] = (not a[index]) if a.dtype == np.bool_ else a[index] + 1


def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_equal_sides_pass_every_comparison(ran):
    side, rows, vec = ran
    _same(copy.deepcopy(rows), rows)
    _same_stores(dict(q=side.cat(lambda o: o.q).copy()), dict(q=side.cat(lambda o: o.q)), 'equal')
    same_env_state(vec, side)
    same_env_state(vec, side.oracles)
    one = side.oracles[0]
    same_env_state(_Vec(SideBySide([one])), one)


def test_one_table_entry_of_the_last_env_of_the_last_group(ran):
    side = ran[0]
    got = side.cat(lambda o: o.q).copy()
    got[-1, -1, -1] = np.nextafter(got[-1, -1, -1], 1e9)
    _fails(_same_stores, dict(q=got), dict(q=side.cat(lambda o: o.q)), 'one entry')


def test_one_step_count_of_the_first_env(ran):
    side, _, vec = ran
    _spoil(vec.state['tcount'], 0)
    _fails(same_env_state, vec, side)
    _fails(same_env_state, vec, side.oracles)


@pytest.mark.parametrize('key', ['pos', 'done', 'episode'])
def test_one_other_field_of_the_last_env(ran, key):
    side, _, vec = ran
    _spoil(vec.state[key], -1)
    _fails(same_env_state, vec, side)


@pytest.mark.parametrize('key', ['obs', 'reward', 'done'])
def test_one_trajectory_cell_of_the_last_step(ran, key):
    rows = ran[1]
    got = copy.deepcopy(rows)
    _spoil(got[key], (-1, -1))
    _fails(_same, got, rows)


def test_the_groups_swapped(ran):
    """The order of the concatenation is part of what is compared: rows, tables and env state of the groups the other way round."""
    side, rows, vec = ran
    swapped = SideBySide(reversed(_side().oracles))
    other = swapped.run(_launch)
    assert all(np.array_equal(other[k][..., :PER_GROUP], rows[k][..., PER_GROUP:]) for k in rows)  # (the same groups, the other order)
    assert not np.array_equal(rows['obs'][:, :PER_GROUP], rows['obs'][:, PER_GROUP:])  # (... and the groups do differ)
    _fails(_same, other, rows)
    _fails(_same_stores, dict(q=swapped.cat(lambda o: o.q)), dict(q=side.cat(lambda o: o.q)), 'swapped')
    _fails(same_env_state, vec, swapped)


def test_a_store_on_one_side_only(ran):
    q = ran[0].cat(lambda o: o.q)
    _fails(_same_stores, dict(q=q), dict(q=q, counts=np.zeros(3)), 'one more wanted')
    _fails(_same_stores, dict(q=q, counts=np.zeros(3)), dict(q=q), 'one more got')
