"""Off-policy Monte-Carlo control with weighted importance sampling, the parts that need no GPU: the ratio table, invariants of the
CPU restatement (tests/_is_oracle.py), the weight cap, what the learner buys over plain Q-learning on the small grid, the argument
checks of the Python layer and the library's new symbols."""
import subprocess

import numpy as np
import pytest

import griduniverse_amd.algorithms as algorithms
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.off_policy import off_policy_mc_control, ratio_table

from . import _is_oracle as IO
from ._behaviour import is_behaviour_totals
from ._tabular_cases import GRIDS, _eps, _grid


@pytest.mark.parametrize('epsilon', [0.0, 0.1, 0.3, 0.5, 1.0])
def test_ratio_table(epsilon):
    R = ratio_table(epsilon)
    assert R.shape == (5, 5) and R.dtype == np.float64 and not R[0].any()
    eps = _eps(epsilon) / 65536.0
    for c in range(5):
        b = eps * 0.25 if c == 0 else (1.0 - eps) / c + eps * 0.25
        for m in range(1, 5):
            assert R[m][c] == (0.0 if b == 0 else (1.0 / m) / b), (m, c)
    assert R[4][4] == 1.0
    assert R[1][1] == 1.0 / (1.0 - 0.75 * eps)
    assert R.tobytes() == IO.ratio_table(_eps(epsilon)).tobytes()  # the restatement's own
    if epsilon == 0.0:
        assert not R[:, 0].any() and R[1][1] == 1.0 and R[1][2] == 2.0 and R[2][1] == 0.5
    else:
        assert (R[1:] > 0).all()
        assert R[1][0] == 1.0 / (eps * 0.25)  # a non-greedy action that is greedy by now
    with pytest.raises(ValueError):
        ratio_table(1.5)
    with pytest.raises(ValueError):
        ratio_table(-0.1)


def _run(grid, seed, N, T, L, gamma, epsilon, w_cap=2.0 ** 64, q0=0.0):
    o = IO.IsOracle(_grid(GRIDS[grid]()), seed, N, q0=q0)
    o.reset()
    return o, o.is_run(T, L, gamma, _eps(epsilon), w_cap)


@pytest.mark.parametrize('grid', ['default4x4', 'open8x8'])
@pytest.mark.parametrize('L', [1, 7, 64])
def test_invariants_of_the_restatement(grid, L):
    q0, T = 0.25, 300
    o, _ = _run(grid, 3, 48, T, L, 0.9, 0.2, q0=q0)
    assert (o.c >= 0).all() and np.isfinite(o.c).all() and o.c.any()
    untouched = o.c == 0
    assert untouched.any()
    assert (o.q[untouched].view(np.uint64) == np.float64(q0).view(np.uint64)).all()  # bitwise q0 where nothing was learned
    upd = o.q[~untouched]
    assert (upd >= -10.0).all() and (upd <= 10.0).all()  # a weighted mean of returns, each within the rewards' range / (1 - gamma)
    assert (o.buf_cnt < L).all() and o.passes > 0 and o.walked >= o.passes
    if L == 1:
        assert (o.c == np.rint(o.c)).all()
        assert (o.c.sum(axis=(1, 2)) == T).all()  # every step is a pass of one entry with W = 1
        assert o.walked == o.passes == 48 * T


@pytest.mark.parametrize('grid', ['default4x4', 'open8x8'])
def test_without_discount_and_with_segments_of_one_q_is_the_reward_of_the_move_and_c_the_visit_count(grid):
    T, N = 300, 48
    o, out = _run(grid, 5, N, T, 1, 0.0, 0.3)
    assert np.isin(o.q, [0.0, -1.0, 10.0, -10.0]).all() and (o.q == -1.0).any() and (o.q == 10.0).any()
    assert (o.c == np.rint(o.c)).all() and (o.c.sum(axis=(1, 2)) == T).all()
    # visits of state s = the steps that left from s: the previous row's obs, or the start cell behind a reset
    start = o.grid.starts[0]
    prev = np.vstack([np.full((1, N), start, np.int32), np.where(out['done'][:-1] != 0, start, out['obs'][:-1])])
    visits = np.zeros((N, o.grid.S), np.int64)
    np.add.at(visits, (np.tile(np.arange(N), T), prev.ravel()), 1)
    assert np.array_equal(o.c.sum(axis=2), visits)


def test_the_weight_cap_changes_the_tables():
    """w_cap = 2.0 against w_cap = 2^256 on the 4x4 grid (64 x 500, epsilon 0.1, gamma 0.9, L = 64, seed 7): the small cap ends
    passes earlier (observed mean pass length 4.97 against 5.66 entries) and the tables differ."""
    a, _ = _run('default4x4', 7, 64, 500, 64, 0.9, 0.1, w_cap=2.0)
    b, _ = _run('default4x4', 7, 64, 500, 64, 0.9, 0.1, w_cap=2.0 ** 256)
    la, lb = a.walked / a.passes, b.walked / b.passes
    print('mean pass length: w_cap 2.0 {:.3f}, w_cap 2^256 {:.3f}; largest C {:g} / {:g}'.format(la, lb, a.c.max(), b.c.max()))
    assert a.q.tobytes() != b.q.tobytes() and a.c.tobytes() != b.c.tobytes()
    assert la < lb
    assert np.isfinite(b.q).all() and np.isfinite(b.c).all()


@pytest.mark.parametrize('seed', [7, 1, 2])
def test_finishes_more_episodes_than_plain_q_learning(seed):
    """Bounds: the issue's -- at least 3000 finished episodes and at least 1.25 times plain Q-learning's.  Observed with this
    restatement: 3718 / 3728 / 3679 for seeds 7 / 1 / 2 against 2377 / 2387 / 2389 of plain Q-learning: the prototype's figures."""
    total, plain = is_behaviour_totals(seed)
    print('seed {}: off-policy MC {} finished episodes, plain Q-learning {}'.format(seed, total, plain))
    assert total >= 3000
    assert total >= 1.25 * plain


def test_python_argument_checks():
    env = object()  # (never reached: the checks come first)
    for kw in (dict(max_episode_len=0), dict(max_episode_len=-3), dict(max_episode_len=1025), dict(epsilon=1.5), dict(epsilon=-0.1),
               dict(epsilon=float('nan')), dict(w_cap=0.5), dict(w_cap=2.0 ** 257), dict(w_cap=float('inf')), dict(w_cap=float('nan')),
               dict(w_cap=-2.0), dict(num_learners=0), dict(discount_factor=float('nan')), dict(q0=float('inf'))):
        with pytest.raises(ValueError):
            off_policy_mc_control(env, 10, **kw)
    with pytest.raises(ValueError):
        off_policy_mc_control(env, -1)
    assert algorithms.off_policy_mc_control is off_policy_mc_control and algorithms.ratio_table is ratio_table
    assert algorithms.tree_search is not None


def test_library_exports_the_importance_sampling_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_is_init', 'gu_is_run', 'gu_is_get', 'gu_is_set', 'gu_is_get_episode'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    assert _lib.IS_MAX == 1024 == IO.IS_MAX
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'gu_is_kernel' in blob
