"""The conditions under which tests/test_gpu_env_ids.py and tests/test_gpu_overlay_starts.py compare something, evaluated with the CPU
restatements alone: a later change to a grid, a plane, a seed or a learner's parameters cannot hollow out the device tests unnoticed.

(a) every learner of tests/_learners.py::LEARNERS at every env id of _learners.env_ids on GRIDS['test_env'], N = 130, with the
    launches of the device test: an episode ended, every table left its fill, the first reset put envs on both start cells, and the
    rows differ from those of the same restatement at env_id0 = 0.
(b) every overlay kind on 'starts8' (and the boxes' learners on 'learn4') at both ids of tests/_overlay_starts.py, every run of the
    device test at its full length (none of the restatements is slow at these sizes): the lazy resets drew every one of the three
    start cells, and some step reset two envs to different cells.  The epoch cases: resets behind the crossing.
(c) the log those conditions rest on (tests/_start_log.py) counts what it is given."""
import functools

import numpy as np
import pytest

from . import _overlay_starts as S
from ._learners import LEARNERS, _a_shard_worth_comparing, _restated, env_ids
from ._start_log import StartLog
from ._tabular_cases import GRIDS, _eps
from ._td_oracle import Q_LEARNING, SARSA

N, SEED = 130, 3  # (those of tests/test_gpu_env_ids.py)


# ---------------------------------------------------------------------------------------------------------------- (a)
@functools.lru_cache(maxsize=None)
def _learner_at(name, env_id0):
    return _restated(LEARNERS[name], GRIDS['test_env'](), N, SEED, env_id0)


@pytest.mark.parametrize('name', sorted(LEARNERS))
def test_every_learner_has_something_to_compare_at_every_env_id(name):
    g = GRIDS['test_env']()
    assert len(g['starts']) == 2 and len(g['lava']) == 3
    for env_id0 in env_ids(N):
        assert 0 < env_id0 and env_id0 + N <= 0xFFFFFFFF
        _a_shard_worth_comparing(LEARNERS[name], g, _learner_at(name, env_id0), _learner_at(name, 0))


def test_the_env_ids_are_the_three_kinds_of_shard():
    a, b, c = env_ids(N)
    assert a % 16 != 0 and a % 64 != 0  # lane index and env id disagree in their low bits
    assert b < 2 ** 31 < b + N  # the batch straddles bit 31
    assert c + N == 0xFFFFFFFF  # the highest gu_create admits


# ---------------------------------------------------------------------------------------------------------------- (b)
def _fresh(kind, grid, env_id0, q0=None):
    o = S.oracle(kind, grid, env_id0, q0=q0)
    o.reset()
    S.place(kind, grid, o)
    return o


@pytest.mark.parametrize('env_id0', S.IDS)
@pytest.mark.parametrize('kind', S.KINDS)
def test_every_overlay_run_draws_all_three_starts(kind, env_id0):
    grid = 'starts8'
    assert len(S.grid_dict(grid)['starts']) == 3
    o = _fresh(kind, grid, env_id0)  # step
    acts = S.step_actions()
    for i in range(S.T):
        assert not o.step(acts[i], True)[3].any()
    S.drew_every_start(o)
    for policy in S.POLICIES:  # rollout
        o = _fresh(kind, grid, env_id0)
        S.rollout_of(o, grid, policy)
        S.drew_every_start(o)
    td_grid = S.td_grid(kind, grid)
    for method in (Q_LEARNING, SARSA):  # td_run
        o = _fresh(kind, td_grid, env_id0, q0=S.Q0)
        o.td_run(300, method, 0.25, 0.9, _eps(0.3))
        S.drew_every_start(o)
        assert (o.q != S.Q0).any()
    o = _fresh(kind, grid, env_id0)  # the reset paths halfway
    S.rollout_of(o, grid, 'uniform', 16, auto=False)
    done = o.state.done != 0
    assert done.any() and not done.all()
    d = o.reset_done()
    assert len(set(o.state.pos[d].tolist())) > 1
    mask = (np.arange(S.N) % 3 == 0).astype(np.uint8)
    o.reset(mask)
    assert len(set(o.state.pos[mask != 0].tolist())) == 3
    S.rollout_of(o, grid, 'uniform', 17)
    S.drew_every_start(o)


@pytest.mark.parametrize('env_id0', S.IDS)
@pytest.mark.parametrize('kind,grid', [('fruit', 'starts8'), ('doors', 'starts8'), ('boxes', 'one_box8'), ('errands', 'starts8')])
def test_the_epoch_cases_reset_behind_the_crossing(kind, grid, env_id0):
    tc = np.full(S.N, 2 ** 32 - 20, np.uint64)
    tc[::3] += 7  # (counts_near_2_32 of tests/_tabular_cases.py)
    for method in (Q_LEARNING, SARSA):
        o = _fresh(kind, grid, env_id0, q0=0.0)
        o.set_state(tcount=tc)
        want = o.td_run(60, method, 0.2, 0.9, _eps(0.5))
        assert (want['done'][40:] != 0).sum() > 10 and (o.state.tcount > 2 ** 32).all()
    for policy in ('uniform', 'sample'):
        o = _fresh(kind, grid, env_id0)
        o.set_state(tcount=tc)
        want = S.rollout_of(o, grid, policy, 40)
        assert (want['done'][28:] != 0).sum() > 10
        S.drew_every_start(o)


def test_the_planes_keep_clear_of_the_start_cells_and_the_ids_differ():
    for grid in ('starts8', 'open150', 'learn4', 'one_box8'):
        g = S.grid_dict(grid)
        assert len(set(g['starts'])) == 3
        for kind in ('fruit', 'doors', 'boxes', 'errands'):
            if grid in ('learn4', 'one_box8') and kind != 'boxes':
                continue
            assert not S.plane(kind, grid)[g['starts']].any(), (grid, kind)
    for grid in ('starts8', 'open150'):
        assert not S.plane('errands', S.td_grid('errands', grid))[S.grid_dict(grid)['starts']].any(), grid
    a, b = (S.oracle('fruit', 'starts8', i) for i in S.IDS)
    assert not np.array_equal(a.reset(), b.reset())  # (a kernel that ignored the id would not pass at the second)
    assert S.IDS[0] == 0 and S.IDS[1] < 2 ** 31 < S.IDS[1] + S.N


# ---------------------------------------------------------------------------------------------------------------- (c)
def test_the_start_log_counts_what_it_is_given():
    log = StartLog([9, 33, 54])
    log.note(np.array([9, 9, 9]))
    assert log.drawn.tolist() == [3, 0, 0] and log.mixed == 0 and not log.every_start_was_drawn_and_some_step_mixed_them()
    log.note(np.array([33]))
    log.note(np.array([54]))
    assert log.drawn.tolist() == [3, 1, 1] and log.mixed == 0 and not log.every_start_was_drawn_and_some_step_mixed_them()
    log.note(np.array([54, 9]))
    assert log.drawn.tolist() == [4, 1, 2] and log.mixed == 1 and log.every_start_was_drawn_and_some_step_mixed_them()
    with pytest.raises(AssertionError):
        log.note(np.array([10]))  # not a start cell
