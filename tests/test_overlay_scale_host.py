"""The cases of tests/test_gpu_overlays_at_scale.py (tests/_overlay_scale.py) on the CPU restatements alone: every run that the
device file compares against met what its case is about -- fruit eaten, a door opened and one found shut, a box pushed and a push
refused, a gust that changed a push, an errand completed and a wrong fruit eaten, every start drawn under auto-reset, an absorbed
step without it -- and the arithmetic of the grids, of the batch and of the crossings is what the device file's docstring says.  A
plane that no env reaches shows here, not on the device."""
import numpy as np
import pytest

from . import _overlay_scale as X
from . import _overlay_starts as S
from ._learners import _crossing
from ._overlays import METHODS
from ._tabular_cases import _eps


# ---------------------------------------------------------------------------------------------------------------- Part A
@pytest.mark.parametrize('grid', sorted(X.GRIDS))
def test_a_the_grids_fall_where_their_rows_say(grid):
    X.arithmetic(grid)
    g = S.grid_dict(grid)
    assert len(set(g['starts'])) == 3 and not set(g['starts']) & set(g['around'] + g['lava'] + g['goals'])
    for kind in ('fruit', 'doors', 'boxes', 'errands'):
        p = S.plane(kind, grid)
        assert p.any() and not p[g['starts'] + g['lava'] + g['goals']].any(), kind
        assert len(set(S.placement(kind, grid).tolist())) >= (3 if g['H'] == 1 else 10)  # (the envs stand on many cells)
        assert not p[S.placement(kind, grid)].any()
    assert np.count_nonzero(S.plane('fruit', grid)) == 3 and X.bits('doors', grid) == 1 and X.bits('errands', grid) == 10
    assert X.bits('boxes', grid) == 2 * (15 if g['W'] * g['H'] <= 32768 else 16)


@pytest.mark.parametrize('policy', S.POLICIES)
@pytest.mark.parametrize('grid', sorted(X.GRIDS))
@pytest.mark.parametrize('kind', X.KINDS)
def test_a_every_rollout_meets_what_it_is_about(kind, grid, policy):
    for auto in (True, False):
        o = X.fresh(kind, grid)
        want = S.rollout_of(o, grid, policy, auto=auto)
        X.met(kind, o, auto)
        if not auto:
            X.absorbed(want)


@pytest.mark.parametrize('grid', sorted(X.GRIDS))
@pytest.mark.parametrize('kind', X.KINDS)
def test_a_every_step_case_meets_what_it_is_about_and_refuses_twice(kind, grid):
    o = X.fresh(kind, grid)
    refused = sum(r for _, _, r, _ in X.steps(o))
    assert refused == 2
    X.met(kind, o)


@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('grid', sorted(X.GRIDS))
@pytest.mark.parametrize('kind', X.KINDS)
def test_a_every_learner_case_learns_and_meets_what_it_is_about(kind, grid, method):
    td, n = X.td_case(kind, grid)
    if kind == 'boxes':
        assert n is None and X.bits(kind, td) > 10  # gu_td_init refuses: that is the boxes' case
        return
    assert n in (6, X.N) and X.bits(kind, td) <= (3 if S.grid_dict(td)['W'] * S.grid_dict(td)['H'] > X.MAX_LDS_CELLS else 6)
    assert (n == 6) == (X.bytes_per_env(td, X.bits(kind, td)) * X.N > X.TD_BYTES)
    o = X.fresh(kind, td, n=n, q0=S.Q0)
    for steps in X.TD_STEPS:
        o.td_run(steps, METHODS[method], X.ALPHA, X.GAMMA, _eps(X.EPS))
    X.learned_on_masked_rows(kind, td, o)
    X.met(kind, o, starts=(n == X.N))


# ---------------------------------------------------------------------------------------------------------------- Part B
def test_b_the_batch_is_257_workgroups_with_a_partial_last_one():
    assert X.BIG_N == 65606 and -(-X.BIG_N // 256) == 257 and X.BIG_N % 256 == 70 == 64 + 6 and X.BIG_N > 256 * 256
    assert X.ID0 < 2 ** 31 < X.ID0 + X.N  # (the ids straddle bit 31 within the first workgroup)


@pytest.mark.parametrize('policy', X.BATCH_POLICIES)
@pytest.mark.parametrize('grid', X.BATCH_GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_b_every_batch_rollout_meets_what_it_is_about(kind, grid, policy):
    for auto in (True, False):
        o = X.fresh(kind, grid, n=X.BIG_N)
        want = S.rollout_of(o, grid, policy, auto=auto)
        X.met(kind, o, auto)
        if not auto:
            X.absorbed(want)
            # (the last workgroup's envs among them: the partial wave ends episodes too)
            assert (want['done'][:, -70:] != 0).any()


@pytest.mark.parametrize('grid', X.BATCH_GRIDS)
@pytest.mark.parametrize('kind', X.KINDS)
def test_b_every_batch_step_case_has_resets_due_in_the_first_and_the_last_workgroup(kind, grid):
    X.batch_step_case(kind, grid, X.fresh(kind, grid, n=X.BIG_N))


# ---------------------------------------------------------------------------------------------------------------- Part C
def _check_crossing(kind, name, b, n, e, width, at):
    per_env = X.bytes_per_env(name, b)
    assert X.bits(kind, name) == b and n % 64 != 0 and 4 <= width <= 16 and width * per_env < 200 << 20
    assert _crossing(per_env, n, at) == e and at % per_env != 0  # inside env e's table, not between two
    starts = X.group_starts(n, e, width)
    assert len(starts) == 3 and starts[1] <= e < starts[1] + width and starts[1] >= width and e + width // 2 <= n
    return per_env, starts


@pytest.mark.parametrize('case', sorted(X.MASKED))
def test_c_the_crossing_lies_inside_a_table_with_a_group_on_each_side(case):
    kind, name, b, n, e, width = X.MASKED[case]
    per_env, _ = _check_crossing(kind, name, b, n, e, width, 2 ** 32)
    assert per_env == {'fruit': 8479744, 'doors': 8479744, 'boxes': 33521664, 'errands': 2359296}[case]
    assert (n, e) == {'fruit': (520, 506), 'doors': (520, 506), 'boxes': (136, 128), 'errands': (1830, 1820)}[case]
    assert per_env * (n - width) < 2 ** 32 + per_env * (width + 2)  # the smallest batch: the last group lies right behind the crossing's
    assert b == 10 or kind in ('fruit', 'doors')  # (boxes and errands at the learners' limit)


def test_c_entry_2_31_lies_inside_a_table():
    kind, name, b, n, e, width = X.ELEMENTS
    per_env, _ = _check_crossing(kind, name, b, n, e, width, 8 * 2 ** 31)
    assert (n, e) == (2040, 2025) and per_env * n > 17.2e9 and (e + 1) * per_env - 2 ** 34 == 2880 * 32


@pytest.mark.parametrize('method', sorted(METHODS))
@pytest.mark.parametrize('case', sorted(X.MASKED) + ['elements'])
def test_c_every_group_learns_on_masked_rows(case, method):
    kind, name, b, n, e, width = X.ELEMENTS if case == 'elements' else X.MASKED[case]
    if case == 'elements' and method != 'q_learning':
        return
    learner, before = X.OverlayTd(kind, name, method), X.put_in_place(kind, name, n)
    for e0 in X.group_starts(n, e, width):
        o = learner.oracle(None, X.C_SEED, width, e0)
        o.reset()
        before(None, e0, o)
        for T in X.C_LAUNCHES:
            learner.restate(o, T)
        X.learned_on_masked_rows(kind, name, o)
