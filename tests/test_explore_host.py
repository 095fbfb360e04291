"""Count-based exploration (UCB and Thompson Q-learning), the parts that need no GPU: the CPU restatement against the tabular one,
its clamps and its saturation, what directed exploration buys on sparse-reward grids, the table builders, the argument checks of
the Python layer and the library's new symbols."""
import subprocess

import numpy as np
import pytest

import griduniverse_amd.algorithms as algorithms
from griduniverse_amd import _lib
from griduniverse_amd.algorithms import exploration as X
from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _explore_oracle as EO
from . import _td_oracle as O
from ._behaviour import EXPLORE_BEHAVIOUR, coverage
from ._tabular_cases import GRIDS, _grid


def sparse_grid(W, H):
    """The open W x H grid with start 0, the goal in the last cell, reward 10 there and 0 everywhere else (CPU restatement only:
    the engine's reward planes hold -1, +10 and -10)."""
    S = W * H
    reward = np.zeros(S, np.int64)
    reward[S - 1] = 10
    return C.Grid.from_lists(W, H, walls=[], goals=[S - 1], lava=[], starts=[0], reward=reward)


def run_restatement(grid, T, rule, tables, eps_q16):
    b = EXPLORE_BEHAVIOUR
    o = EO.ExploreOracle(grid, b['seed'], b['N'])
    o.set_tables(*tables)
    o.reset()
    out = o.explore(T, EO.THOMPSON if rule == 'thompson' else EO.UCB, b['alpha'], b['gamma'], eps_q16)
    return o, out


def behaviour_coverage(grid, T):
    """(coverage of the UCB learners, of the yardstick: the same restatement with zero tables and epsilon 0.1), per learner."""
    ucb, _ = run_restatement(grid, T, 'ucb', X.ucb_tables(1.0, 1024), 0)
    plain, _ = run_restatement(grid, T, 'ucb', (np.zeros(2), np.zeros(2)), EXPLORE_BEHAVIOUR['plain_eps_q16'])
    return coverage(ucb.counts), coverage(plain.counts)


@pytest.mark.parametrize('mode', [EO.UCB, EO.THOMPSON])
@pytest.mark.parametrize('grid', ['default4x4', 'open8x8', 'maze11', 'lava32'])
def test_with_zero_tables_the_restatement_is_the_q_learning_oracle_byte_for_byte(grid, mode):
    g = _grid(GRIDS[grid]())
    a = O.TdOracle(g, 7, 64, q0=0.25)
    b = EO.ExploreOracle(g, 7, 64, q0=0.25)
    assert np.array_equal(a.reset(), b.reset())
    steps = 0
    for T, U, B in ((200, np.zeros(8), np.arange(8.0)), (100, np.arange(1.0, 4.0), np.zeros(3))):  # U zero, then B zero
        b.set_tables(U, B)
        want = a.run(T, O.Q_LEARNING, 0.1, 0.99, 6554)
        got = b.explore(T, mode, 0.1, 0.99, 6554)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert b.q.tobytes() == a.q.tobytes()
        steps += T
        assert np.array_equal(b.counts.astype(np.int64).sum(axis=(1, 2)), np.full(64, steps))  # the counts: the steps taken
    for k in ('pos', 'done', 'episode', 'tcount'):
        assert np.array_equal(getattr(a.state, k), getattr(b.state, k)), k


def _direct_scores(o, e, s, t, mode):
    """The score row of learner e in state s at step count t, evaluated straight from the rules with scalar arithmetic."""
    C_ = len(o.U)
    n = [int(v) for v in o.counts[e, s]]
    u = float(o.U[min(sum(n), C_ - 1)])
    x = R.word(o.seed, int(o.env_ids[e]), 7, t & 0xFFFFFFFF, epoch=t >> 32)
    row = []
    for b in range(4):
        p = u * float(o.B[min(n[b], C_ - 1)])
        if mode == EO.THOMPSON:
            z = float(sum((x >> (8 * k)) & 0xFF for k in range(4)) - 510)
            p = p * z
            x = R.sample_next(x)
        row.append(float(o.q[e, s, b]) + p)
    return row


@pytest.mark.parametrize('mode', [EO.UCB, EO.THOMPSON])
def test_both_clamps_with_four_entries_match_a_direct_evaluation(mode):
    """C = 4: the state sum passes 3 at a state's fourth visit and a pair's count passes 3 soon after, so 200 steps use both
    clamps; every step's action is checked against the rules evaluated one learner at a time."""
    g = _grid(GRIDS['default4x4']())
    o = EO.ExploreOracle(g, 3, 8)
    o.set_tables([0.0, 0.5, 1.0, 1.5], [4.0, 2.0, 1.0, 0.25])
    o.reset()
    sum_clamped = pair_clamped = 0
    for _ in range(200):
        if (o.state.done != 0).any():
            C.reset(g, o.seed, o.state, (o.state.done != 0).astype(np.uint8))
        s, t = o.state.pos.copy(), o.state.tcount.astype(np.uint64)
        w = O.words(o.seed, o.env_ids, t)
        before = o.counts.copy()
        want = []
        for e in range(8):
            row = _direct_scores(o, e, int(s[e]), int(t[e]), mode)
            assert o.scores(s, t, mode)[e].tolist() == row
            want.append(int(O.choose(np.array([row]), w[e:e + 1], 0)[0]))
            sum_clamped += int(before[e, s[e]].sum() > 3)
            pair_clamped += int(before[e, s[e]].max() > 3)
        out = o.explore(1, mode, 0.2, 0.9, 0)
        assert out['obs'].shape == (1, 8)
        for e in range(8):
            delta = o.counts[e].astype(np.int64) - before[e]
            assert delta.sum() == 1 and delta[s[e], want[e]] == 1, e
    assert sum_clamped > 0 and pair_clamped > 0


def test_counts_at_the_cap_stay_at_the_cap():
    g = _grid(GRIDS['default4x4']())
    o = EO.ExploreOracle(g, 1, 4)
    o.set_tables(*X.ucb_tables(1.0, 16))
    o.set_counts(np.full((4, g.S, 4), EO.COUNT_MAX, np.uint32))
    o.counts[:, :, 2] = EO.COUNT_MAX - 1
    o.reset()
    o.explore(300, EO.UCB, 0.1, 0.9, 65536)  # always exploring: every pair near the start is tried again and again
    assert o.counts.max() == EO.COUNT_MAX and o.counts.min() >= EO.COUNT_MAX - 1
    assert (o.counts[:, 0, 2] == EO.COUNT_MAX).all()  # ... and those one below reached it
    assert EO.COUNT_MAX == _lib.EXPLORE_COUNT_MAX == 0x3FFFFFFF and 4 * EO.COUNT_MAX < 2 ** 32


def test_table_builders():
    U, B = X.ucb_tables(1.0, 1024)
    assert U.shape == B.shape == (1024,) and U.dtype == B.dtype == np.float64
    assert U[0] == U[1] == U[2] == np.sqrt(np.log(2.0)) and U[100] == np.sqrt(np.log(100.0))
    assert B[0] == 1e6 and B[1] == 1.0 and B[4] == 0.5 and B[100] == 0.1
    U2, B2 = X.ucb_tables(2.5, 16)
    assert np.array_equal(U2, 2.5 * U[:16]) and np.array_equal(B2, B[:16])
    U, B = X.thompson_tables(1.0, 1024)
    assert (U == 1.0).all() and B[0] == 1.0 / np.sqrt(21845.0) and B[3] == 1.0 / np.sqrt(21845.0) / 2.0
    assert np.array_equal(X.thompson_tables(3.0, 8)[1], 3.0 / np.sqrt(21845.0) / np.sqrt(np.arange(8.0) + 1.0))
    for U, B in (X.ucb_tables(), X.thompson_tables(), X.ucb_tables(0.0, 2), X.thompson_tables(0.0, 4096)):
        assert np.isfinite(U).all() and np.isfinite(B).all() and (U >= 0).all() and (B >= 0).all()
    # the variate the Thompson tables scale: four uniform bytes, centred -- mean 0, variance 4 * (256^2 - 1) / 12
    byte = np.arange(256.0)
    assert 4 * byte.mean() == 510.0 and 4 * byte.var() == X.IRWIN_HALL_VARIANCE == 21845.0
    z = EO.variates(5, np.arange(4096, dtype=np.uint64), np.full(4096, 17, np.uint64))
    assert z.shape == (4096, 4) and (z == np.round(z)).all() and np.abs(z).max() <= 510
    assert abs(z.mean()) < 5.0 and 0.9 * 21845 < z.var() < 1.1 * 21845
    for bad in (dict(size=1), dict(size=4097), dict(c=-1.0), dict(c=float('nan'))):
        with pytest.raises(ValueError):
            X.ucb_tables(**bad)
    for bad in (dict(size=0), dict(size=5000), dict(sigma=-0.5), dict(sigma=float('inf'))):
        with pytest.raises(ValueError):
            X.thompson_tables(**bad)


def test_python_argument_checks():
    env = object()  # (never reached: the checks come first)
    for fn in (X.ucb_q_learning, X.thompson_q_learning):
        for kw in (dict(num_learners=0), dict(epsilon=1.5), dict(epsilon=-0.1), dict(table_size=1), dict(table_size=4097)):
            with pytest.raises(ValueError):
                fn(env, 10, **kw)
        with pytest.raises(ValueError):
            fn(env, -1)
    with pytest.raises(ValueError):
        X.ucb_q_learning(env, 10, c=-1.0)
    with pytest.raises(ValueError):
        X.thompson_q_learning(env, 10, sigma=-1.0)
    assert algorithms.ucb_q_learning is X.ucb_q_learning and algorithms.thompson_q_learning is X.thompson_q_learning
    with pytest.raises(AttributeError):
        algorithms.no_such_algorithm


def test_library_exports_the_exploration_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_explore_init', 'gu_explore_set_tables', 'gu_explore_run', 'gu_explore_get_counts', 'gu_explore_set_counts'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    assert _lib.EXPLORE_MAX_C == 4096
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'gu_explore_kernel' in blob


def test_ucb_covers_the_sparse_8x8_grid_sooner_than_epsilon_greedy():
    """64 learners, seed 7, alpha 0.1, gamma 0.99, 500 steps on the sparse open 8x8 grid (252 pairs): UCB (ucb_tables(1.0, 1024),
    epsilon 0) against the same restatement with zero tables and epsilon 0.1.  Bounds: the issue's -- UCB's mean coverage at
    least the yardstick's + 27 (half of its prototype's gap of 55.5, as margin for a detail restated differently), UCB's least at
    least the yardstick's least.
    Observed with this restatement (mean / least): UCB 242.5 / 222, epsilon-greedy 187.0 / 141 -- the prototype's numbers."""
    ucb, plain = behaviour_coverage(sparse_grid(8, 8), 500)
    print('sparse 8x8, 500 steps: UCB coverage mean {:.1f} least {}, epsilon-greedy mean {:.1f} least {}'.format(
        ucb.mean(), ucb.min(), plain.mean(), plain.min()))
    assert ucb.mean() >= plain.mean() + 27
    assert ucb.min() >= plain.min()


def test_every_ucb_learner_tries_every_pair_of_the_sparse_8x8_grid_in_2000_steps():
    """As above with 2000 steps: every one of the 64 UCB learners has tried all 252 pairs (the issue's bound).
    Observed with this restatement (mean / least): UCB 252 / 252, epsilon-greedy 241.1 / 222."""
    ucb, plain = behaviour_coverage(sparse_grid(8, 8), 2000)
    print('sparse 8x8, 2000 steps: UCB coverage mean {:.1f} least {}, epsilon-greedy mean {:.1f} least {}'.format(
        ucb.mean(), ucb.min(), plain.mean(), plain.min()))
    assert (ucb == 252).all()


def test_ucb_covers_the_sparse_16x16_grid_sooner_than_epsilon_greedy():
    """As above on the sparse open 16x16 grid (1020 pairs), 2000 steps.  Bound: the issue's -- UCB's mean coverage at least the
    yardstick's + 118 (half of its prototype's gap of 236).
    Observed with this restatement (mean / least): UCB 969.8 / 880, epsilon-greedy 733.8 / 625 -- the prototype's numbers."""
    ucb, plain = behaviour_coverage(sparse_grid(16, 16), 2000)
    print('sparse 16x16, 2000 steps: UCB coverage mean {:.1f} least {}, epsilon-greedy mean {:.1f} least {}'.format(
        ucb.mean(), ucb.min(), plain.mean(), plain.min()))
    assert ucb.mean() >= plain.mean() + 118


def test_thompson_noise_is_used():
    """Thompson with epsilon 0 on the sparse 8x8 grid, 500 steps: its rows differ from those of the greedy learner (zero tables,
    epsilon 0), so the noise decides actions.  No gain is asserted (the issue's prototype had it only marginally ahead of
    epsilon-greedy).  Observed coverage with this restatement (mean / least): Thompson 203.1 / 179, epsilon-greedy 187.0 / 141."""
    grid = sparse_grid(8, 8)
    th, rows = run_restatement(grid, 500, 'thompson', X.thompson_tables(1.0, 1024), 0)
    greedy, rows0 = run_restatement(grid, 500, 'thompson', (np.zeros(2), np.zeros(2)), 0)
    c = coverage(th.counts)
    print('sparse 8x8, 500 steps: Thompson coverage mean {:.1f} least {}; the greedy learner mean {:.1f}'.format(
        c.mean(), c.min(), coverage(greedy.counts).mean()))
    assert not np.array_equal(rows['obs'], rows0['obs'])
    assert (rows['obs'] != rows0['obs']).any(axis=0).all()  # every learner's path leaves the greedy learner's
