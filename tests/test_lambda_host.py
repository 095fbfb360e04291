"""Batched tabular SARSA(lambda) / Watkins's Q(lambda), the parts that need no GPU: the CPU restatement against one-step Q-learning /
SARSA and against an independent dense trace table, hand-worked cases (a repeated pair is replaced, the Watkins cut, coefficients
that underflow), traces learning faster than one-step SARSA, the argument checks and the library's new symbols."""
import os
import subprocess

import numpy as np
import pytest

from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import sarsa_lambda, watkins_q_lambda
from griduniverse_amd.envs.griduniverse_env import GridUniverseEnv
from oracle import c_oracle as C

from . import _golden as G
from . import _lambda_oracle as LO
from . import _td_oracle as O
from . import _walks
from ._lambda_oracle import signed_zero_table
from ._tabular_cases import GRIDS, _grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('signed_zeros', [False, True])
@pytest.mark.parametrize('K,lam', [(1, 0.5), (1, 1.0), (8, 0.0), (64, 0.0)])
@pytest.mark.parametrize('method', [LO.WATKINS, LO.SARSA])
@pytest.mark.parametrize('grid', ['default4x4', 'test_env', 'maze11'])
def test_restatement_with_K_1_or_lambda_0_is_one_step_td(grid, method, K, lam, signed_zeros):
    g = _grid(GRIDS[grid]())
    lo, o = LO.LambdaOracle(g, 9, 40, q0=0.25), O.TdOracle(g, 9, 40, q0=0.25)
    assert np.array_equal(lo.reset(), o.reset())
    alpha = 0.2
    if signed_zeros:
        alpha = -0.0
        lo.set_q(signed_zero_table(40, g.S))
        o.set_q(signed_zero_table(40, g.S))
    for T, eps in ((150, 0.3), (90, 1.0), (70, 0.0)):
        got, want = lo.lam(T, method, K, lam, alpha, 0.9, int(eps * 65536)), o.run(T, method, alpha, 0.9, int(eps * 65536))
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    assert lo.q.tobytes() == o.q.tobytes()
    assert np.array_equal(lo.state.tcount, o.state.tcount)
    if method == LO.SARSA:
        assert np.array_equal(lo.carry, o.carry)


def _dense(grid, seed, n, T, method, lam, alpha, gamma, eps_q16):
    """The textbook backward view, written apart from the restatement: a trace table E[S][4] per learner, set to 1 on a visit
    (replacing), Q += (alpha * delta) * E for the entries with E != 0, then E *= gamma * lambda; zeroed when an episode starts and,
    for Watkins's Q(lambda), when a non-greedy action is taken.  No truncation.  Returns Q and each learner's longest episode."""
    st = C.State(n)
    st.pos[:] = grid.starts[0]
    C.reset(grid, seed, st)
    ids, idx = np.arange(n, dtype=np.uint64), np.arange(n)
    q, E = np.zeros((n, grid.S, 4)), np.zeros((n, grid.S, 4))
    c = gamma * lam
    act = np.full(n, -1, np.int32)
    length, longest = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for _ in range(T):
        d = st.done != 0
        if d.any():
            C.reset(grid, seed, st, d.astype(np.uint8))
            act[d], E[d], length[d] = -1, 0.0, 0
        s = st.pos.copy()
        need = act < 0
        if need.any():
            act = np.where(need, O.choose(q[idx, s], O.words(seed, ids, st.tcount), eps_q16), act).astype(np.int32)
        qsa = q[idx, s, act]
        if method == LO.WATKINS:
            E[qsa != O.row_max(q[idx, s])] = 0.0
        out = C.rollout(grid, seed, st, 1, True, actions=act[None, :])
        s2, r, dn = out['obs'][0], out['reward'][0].astype(np.float64), out['done'][0] != 0
        nxt = q[idx, s2].copy()
        if method == LO.SARSA:
            a2 = O.choose(nxt, O.words(seed, ids, st.tcount), eps_q16)
            m, a2 = nxt[idx, a2], np.where(dn, -1, a2).astype(np.int32)
        else:
            m, a2 = O.row_max(nxt), np.full(n, -1, np.int32)
        g = alpha * (np.where(dn, r, r + gamma * m) - qsa)
        E[idx, s, act] = 1.0
        nz = E != 0.0
        q[nz] = q[nz] + (g[:, None, None] * E)[nz]
        E *= c
        length += 1
        longest = np.maximum(longest, length)
        act = a2
    return q, longest


@pytest.mark.parametrize('method', [LO.WATKINS, LO.SARSA])
@pytest.mark.parametrize('grid', ['default4x4', 'test_env'])
def test_restatement_equals_a_dense_trace_table(grid, method):
    """Learners are independent, so they are compared one by one: those none of whose episodes was longer than K steps never had
    a trace reach age K, and there the truncated window and the dense table must agree byte for byte."""
    g = _grid(GRIDS[grid]())
    n, T, K, lam, alpha, gamma, eps = 400, 300, 64, 0.9, 0.2, 0.95, int(0.2 * 65536)
    o = LO.LambdaOracle(g, 5, n)
    o.reset()
    o.lam(T, method, K, lam, alpha, gamma, eps)
    q, longest = _dense(g, 5, n, T, method, lam, alpha, gamma, eps)
    ok = longest <= K
    assert ok.sum() >= 20, ok.sum()
    assert o.q[ok].tobytes() == q[ok].tobytes()
    assert (o.q[ok] != 0.0).sum() > 10 * ok.sum()  # (the traces did reach back)


def _corridor():
    """1 x 4 corridor, start 0, goal 3: UP and DOWN bump everywhere, LEFT at the start."""
    return C.Grid.from_lists(4, 1, goals=[3], starts=[0], reward=[-1, -1, -1, 10])


def _by_hand(method, steps=300, K=16, lam=0.8, alpha=0.5, gamma=0.9, eps=0.5):
    """One learner in the corridor, one step per launch, against the rules of include/gu.h worked in a plain Python list (the
    window by age, -1 for a hole).  Returns the counts of the cases met: pairs replaced, windows cut, and exploratory greedy
    actions that kept a window."""
    grid = _corridor()
    o = LO.LambdaOracle(grid, 1, 1)
    o.reset()
    st = C.State(1)
    st.pos[:] = grid.starts[0]
    C.reset(grid, 1, st)
    P = LO.coefficients(K, gamma, lam)
    eps_q16 = int(eps * 65536)
    q, win, act = np.zeros((4, 4)), [], -1
    seen = dict(replaced=0, cut=0, kept=0)
    for step in range(steps):
        if st.done[0]:
            C.reset(grid, 1, st, np.ones(1, np.uint8))
            act = -1
        s = int(st.pos[0])
        w = int(O.words(1, np.zeros(1, np.uint64), st.tcount)[0])
        if act < 0:
            act = int(O.choose(q[s][None], np.array([w], np.uint32), eps_q16)[0])
        a = act
        greedy = q[s, a] == O.row_max(q[s][None])[0]
        live = any(p >= 0 for p in win)
        if method == LO.WATKINS and not greedy:
            seen['cut'] += live
            win = []
        elif (w >> 16) < eps_q16 and live:
            seen['kept'] += 1
        out = C.rollout(grid, 1, st, 1, True, actions=np.array([[a]], np.int32))
        s2, r, d = int(out['obs'][0, 0]), int(out['reward'][0, 0]), bool(out['done'][0, 0])
        if method == LO.SARSA:
            a2 = int(O.choose(q[s2][None], O.words(1, np.zeros(1, np.uint64), st.tcount), eps_q16)[0])
            m = q[s2, a2]
        else:
            a2, m = -1, O.row_max(q[s2][None])[0]
        g = alpha * ((r if d else r + gamma * m) - q[s, a])
        if s * 4 + a in win:  # the old entry goes; the others keep their ages
            win[win.index(s * 4 + a)] = -1
            seen['replaced'] += 1
        win.insert(0, s * 4 + a)
        for j, p in enumerate(win):
            if p >= 0 and P[j] != 0.0:
                q[p >> 2, p & 3] = q[p >> 2, p & 3] + g * P[j]
        win = [] if d else win[:K - 1]
        act = -1 if d else a2
        got = o.lam(1, method, K, lam, alpha, gamma, eps_q16)
        assert got['obs'][0, 0] == s2 and got['reward'][0, 0] == r, step
        assert o.q[0].tobytes() == q.tobytes(), step
        assert o.win[0].tolist() == [-1] + win + [-1] * (LO.LAMBDA_MAX - 1 - len(win)), step
    return seen


@pytest.mark.parametrize('method', [LO.WATKINS, LO.SARSA])
def test_a_repeated_pair_is_replaced_not_accumulated(method):
    """A wall bump (UP or DOWN in the corridor) repeats its pair within an episode: the old entry goes, the trace restarts at 1."""
    assert _by_hand(method)['replaced'] > 0


def test_watkins_cut_by_a_non_greedy_action_only():
    """A non-greedy action empties the window; an exploratory action that happens to be greedy does not."""
    seen = _by_hand(LO.WATKINS)
    assert seen['cut'] > 0 and seen['kept'] > 0


def test_coefficients_that_underflow_end_the_updates():
    """From the first P_j that underflows to 0 on, the ages j and beyond are not updated at all -- not updated by zero: an
    infinite entry makes g infinite on the steps that bootstrap on it, and g * 0.0 is NaN.  So K = 8 with P_3 = 0 must leave the
    table exactly as K = 3 does."""
    P = LO.coefficients(8, 0.9, 1e-160)
    assert 0.0 < P[1] < 1e-159 and 0.0 < P[2] < 1e-300 and P[3:] == [0.0] * 5
    g = _grid(GRIDS['default4x4']())
    q = np.zeros((64, g.S, 4))
    q[:, 10, :] = np.inf
    a, b = LO.LambdaOracle(g, 4, 64), LO.LambdaOracle(g, 4, 64)
    a.reset()
    b.reset()
    a.set_q(q)
    b.set_q(q)
    with np.errstate(invalid='ignore'):
        ra, rb = a.lam(300, LO.SARSA, 8, 1e-160, 0.3, 0.9, 6554), b.lam(300, LO.SARSA, 3, 1e-160, 0.3, 0.9, 6554)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert a.q.tobytes() == b.q.tobytes()
    assert (a.win[:, 3:8] >= 0).any()  # pairs of ages 3 .. 7 are in the window, and no longer updated


def _steps_to_shortest(grid, best, lam, K, chunk=100, limit=30000):
    """Real steps until every learner's greedy walk from the start is a shortest path (SARSA(lambda), alpha 0.1, gamma 0.9,
    epsilon 0.1, seed 3, four learners)."""
    o = LO.LambdaOracle(grid, 3, 4)
    o.reset()
    done = 0
    while done < limit:
        o.lam(chunk, LO.SARSA, K, lam, 0.1, 0.9, int(0.1 * 65536))
        done += chunk
        if all(_walks._greedy_walk(grid, o.q[e]) == best for e in range(o.n)):
            return done
    return None


def test_sarsa_lambda_finds_the_shortest_path_in_fewer_real_steps():
    grid = C.Grid.from_env(GridUniverseEnv(custom_world_fp=G.level_path('maze_11x11.txt')))
    best = _walks._shortest_from_start(grid)
    # measured with this restatement (which the device matches byte for byte): 6800 real steps for lambda = 0.9, 21 100 for
    # lambda = 0, which is one-step SARSA
    assert _steps_to_shortest(grid, best, 0.9, 32) == 6800
    assert _steps_to_shortest(grid, best, 0.0, 32) == 21100


def test_lambda_learners_check_their_arguments():
    env = GridUniverseEnv((4, 4))
    for fn in (sarsa_lambda, watkins_q_lambda):
        for kw in (dict(trace_len=0), dict(trace_len=65), dict(lam=-0.1), dict(lam=1.5), dict(lam=float('nan')), dict(num_learners=0),
                   dict(epsilon=1.5), dict(epsilon=-0.1)):
            with pytest.raises(ValueError):
                fn(env, 10, **kw)


def test_library_exports_the_lambda_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    header = open(os.path.join(ROOT, 'include', 'gu.h')).read()
    for name in ('gu_lambda_run', 'gu_lambda_get_window'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
        assert 'int ' + name + '(' in header
    assert '#define GU_LAMBDA_MAX 64' in header and _lib.LAMBDA_MAX == 64
