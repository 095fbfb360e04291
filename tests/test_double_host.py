"""Batched Expected SARSA and Double Q-learning, the parts that need no GPU: the CPU restatements (tests/_double_oracle.py) against
Q-learning, exact arithmetic and their own invariants, the library's new symbols, the argument checks of the algorithms, and what the
learners do on a cliff grid."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import double_q_learning, expected_sarsa
from griduniverse_amd.envs.griduniverse_env import GridUniverseEnv
from oracle import c_oracle as C

from . import _double_oracle as O
from . import _td_oracle as TD
from ._tabular_cases import GRIDS, _eps, _grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('gu_esarsa_run', 'gu_double_init', 'gu_double_run', 'gu_double_get_q', 'gu_double_set_q')


@pytest.mark.parametrize('grid', ['maze11', 'lava32'])
def test_restated_expected_sarsa_without_exploration_is_restated_q_learning(grid):
    """eps_q16 = 0: E = 0 * sum + 1 * max, the maximum itself on finite tables without negative zeros."""
    g = _grid(GRIDS[grid]())
    a, b = O.EsarsaOracle(g, 5, 64, q0=0.125), TD.TdOracle(g, 5, 64, q0=0.125)
    assert np.array_equal(a.reset(), b.reset())
    got, want = a.esarsa(300, 0.3, 0.9, 0), b.run(300, TD.Q_LEARNING, 0.3, 0.9, 0)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert a.q.tobytes() == b.q.tobytes() and (a.q != 0.125).any()
    for k in ('pos', 'done', 'episode', 'tcount'):
        assert np.array_equal(getattr(a.state, k), getattr(b.state, k)), k


def test_restated_expectation_is_the_exact_mean_under_the_policy_within_2_ulp():
    """sum_a pi(a) q(a) with pi(a) = eps / 4 + (1 - eps) / m on the m tied maxima, in exact rational arithmetic, against
    pe * sum + pg * max in float64.  Rows of one sign, as the tables of a grid with step costs hold them (a row of mixed signs
    cancels in its sum, and no bound relative to the result holds then); 1, 2, 3 and 4 tied maxima; the eps that have an edge."""
    rs = np.random.RandomState(12)
    worst = Fraction(0)
    for eps_q16 in (0, 1, 6554, 13107, 32768, 43691, 65535, 65536):
        eps = Fraction(eps_q16, 65536)
        for ties in (1, 2, 3, 4):
            for sign in (-1.0, 1.0):
                for _ in range(25):
                    row = sign * rs.uniform(0.01, 20.0, 4)
                    top = rs.permutation(4)[:ties]
                    row[top] = row.max() * (1.5 if sign > 0 else 0.5)  # above every other entry, of the row's sign
                    assert int((row == row.max()).sum()) == ties
                    exact = sum((eps / 4 + ((1 - eps) / ties if v == row.max() else 0)) * Fraction(float(v)) for v in row)
                    got = float(O.expectation(row[None, :], eps_q16)[0])
                    err = abs(Fraction(got) - exact) / Fraction(float(np.spacing(abs(got))))
                    worst = max(worst, err)
                    assert err <= 2, (eps_q16, ties, row.tolist(), got, float(exact), float(err))
    print('largest error: %.3f ulp' % float(worst))


@pytest.mark.parametrize('grid', ['maze11', 'lava32'])
def test_one_restated_double_q_step_changes_at_most_one_entry_in_the_table_the_coin_names(grid):
    g = _grid(GRIDS[grid]())
    n = 48
    o = O.DoubleOracle(g, 9, n, q0=0.0)
    o.reset()
    seen = np.zeros(2, int)
    for _ in range(150):
        before, t = o.q.copy(), o.state.tcount.copy()
        o.run(1, 0.4, 0.9, _eps(0.25))
        coin = O.coins(9, o.env_ids, t)  # drawn here from the count before the step, not taken from the restatement
        changed = (o.q != before).reshape(n, g.S, 2, 4)
        per_env = changed.reshape(n, -1).sum(axis=1)
        assert per_env.max() <= 1
        e = np.flatnonzero(per_env)
        in_b = changed[e].any(axis=(1, 3))[:, 1].astype(np.int64)  # the table that holds the changed entry
        assert np.array_equal(in_b, coin[e])
        s, a = o.last_sa[e] >> 2, o.last_sa[e] & 3
        assert changed[e, s, coin[e], a].all()  # ... and it is the entry of the state left and the action taken
        seen += np.bincount(coin[e], minlength=2)
    assert seen.min() > 1000  # both tables learned


def test_restated_double_q_learns_a_shortest_path_on_the_mean_of_its_tables():
    grid = C.Grid.from_lists(4, 4)
    o = O.DoubleOracle(grid, 5, 16)
    o.reset()
    o.run(6000, 0.1, 0.9, _eps(0.2))
    q = (o.q[:, :, 0] + o.q[:, :, 1]) * 0.5
    for e in range(16):
        s, steps = 0, 0
        while not grid.goal[s] and steps <= grid.S:
            nxt, _, _ = C.look_step_ahead(grid, np.array([s], np.int32), np.array([int(np.argmax(q[e, s]))], np.int32), True)
            s, steps = int(nxt[0]), steps + 1
        assert grid.goal[s] and steps == 6, (e, steps)


def test_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gu.h')).read(), flags=re.S)
    declared = re.findall(r'^\s*int\s+(gu_\w+)\s*\(', text, flags=re.M)
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert ' T ' + name + '\n' in syms, name
    assert _lib.SIGNATURES['gu_esarsa_run'] == _lib.SIGNATURES['gu_double_run']
    assert len(_lib.SIGNATURES['gu_esarsa_run']) == 6 and len(_lib.SIGNATURES['gu_double_get_q']) == 4


@pytest.mark.parametrize('learn', [expected_sarsa, double_q_learning])
def test_algorithms_check_their_arguments_before_they_touch_a_device(learn, monkeypatch):
    from griduniverse_amd.algorithms import _batch as M  # (where every learner function opens its batch)

    def no_device(*a, **kw):
        raise AssertionError('a batch was opened before the arguments were checked')

    monkeypatch.setattr(M, 'VecGridUniverse', no_device)
    env = GridUniverseEnv((4, 4))
    for kw in (dict(num_learners=0), dict(num_learners=-3), dict(epsilon=-0.01), dict(epsilon=1.5)):
        with pytest.raises(ValueError):
            learn(env, 10, **kw)
    for gone in ('wind', 'fruit', 'doors'):
        with pytest.raises(TypeError):
            learn(env, 10, **{gone: None})


# ---- the cliff ----
def cliff_grid():
    """12 x 4; the bottom row is start, ten lava cells, goal.  Rewards as everywhere: -1 a step, +10 the goal, -10 lava."""
    return C.Grid.from_lists(12, 4, goals=[47], lava=list(range(37, 47)), starts=[36])


def mean_return(out, t0):
    """The mean return of the episodes that end at step t0 or later, over all learners."""
    rew, don = out['reward'], out['done']
    acc = np.zeros(rew.shape[1], np.int64)
    total = count = 0
    for i in range(len(rew)):
        acc += rew[i]
        fin = don[i] != 0
        if i >= t0:
            total, count = total + int(acc[fin].sum()), count + int(fin.sum())
        acc[fin] = 0
    return total / count


def cliff_returns(alpha, T=3000, gamma=0.99, L=64, seed=7):
    out = {}
    for name in ('sarsa', 'q_learning', 'expected_sarsa'):
        o = O.EsarsaOracle(cliff_grid(), seed, L)
        o.reset()
        if name == 'expected_sarsa':
            rows = o.esarsa(T, alpha, gamma, _eps(0.1))
        else:
            rows = o.run(T, TD.SARSA if name == 'sarsa' else TD.Q_LEARNING, alpha, gamma, _eps(0.1))
        out[name] = mean_return(rows, T - T // 3)
    return out


@pytest.mark.parametrize('alpha,over_sarsa,under_q', [(0.5, 2.060, 0.811), (0.9, 1.362, 1.928)])
def test_on_the_cliff_expected_sarsa_lies_between_sarsa_and_q_learning(alpha, over_sarsa, under_q):
    """64 learners each, seed 7, epsilon 0.1, gamma 0.99, 3000 steps; the mean return per finished episode over the last 1000 steps,
    as the restatement gave it:

        alpha   SARSA     Expected SARSA   Q-learning
        0.5     -9.625    -7.565           -6.754
        0.9     -10.130   -8.768           -6.840

    (-2 is the best an episode can do: 12 steps at -1 and the goal's +10 on the 13th; -10 is a step from the start into the lava.)  Expected
    SARSA holds up where SARSA's large step size lets one fall poison the path, as the book has it; but on this reward scale -- lava
    costs no more than ten steps -- it does NOT beat Q-learning online over these 3000 steps.  Over 12000 steps the two draw level:
    -6.643 against -6.727 at alpha 0.5, -6.626 against -6.707 at alpha 0.9 (SARSA: -8.943 and -10.119; with gamma = 1 Expected SARSA
    gives -6.658 and -7.455, Q-learning -6.757 and -6.777, SARSA -9.407 and -10.119).  Double Q-learning ends at -10.12 in every one of
    these settings: its estimates of the path sink below the lava's -10 before the goal's reward reaches the start, and from then on it
    steps into the lava.  Asserted: the ordering SARSA < Expected SARSA < Q-learning at 3000 steps, each gap at least half the measured one."""
    r = cliff_returns(alpha)
    print(alpha, r)
    assert r['expected_sarsa'] - r['sarsa'] >= over_sarsa / 2
    assert r['q_learning'] - r['expected_sarsa'] >= under_q / 2
