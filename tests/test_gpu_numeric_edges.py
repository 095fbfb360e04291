"""The float64 building blocks of the softmax and importance-sampling learners on the device, at their edges (csrc/gu_softmax.hpp:
gu_exp, gu_recip14, gu_is_recip, the softmax of one row).  Through the probe of include/gu_diag.h on the vectors of
tests/_numeric_edges.py: reciprocals against the exact rational, exp and the softmax terms against the numpy rule, actions against
the restatement, byte for byte.  Then through gu_is_run, gu_ac_run and gu_reinforce_run themselves on crafted tables, one env per
vector, and through gu_is_run at both ends of its weight window."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.engine import Engine

from . import _ac_oracle as AC
from . import _is_oracle as IO
from . import _numeric_edges as NE
from . import _reinforce_oracle as RO
from . import _td_oracle as TD
from ._tabular_cases import GRIDS, _grid, _same, _spec, same_env_state

pytestmark = pytest.mark.gpu

# 5 x 5, open, start in the centre, goal in a corner: the first two steps are never terminal and never bump
CENTRE = dict(W=5, H=5, starts=[12], goals=[24], lava=[], walls=[])
START = 12


@pytest.fixture(scope='module')
def eng():
    with Engine(8, _spec(GRIDS['default4x4']())) as e:
        yield e


def _bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint64 if got.itemsize == 8 else np.uint32)
                             != want.reshape(-1).view(np.uint64 if got.itemsize == 8 else np.uint32))
        raise AssertionError('{}: {} of {} differ, first at {}: got {!r}, want {!r}'.format(
            what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


# ---- through the probe

def test_probe_recip14_is_the_exact_rational_reciprocal(eng):
    _bytes(eng.probe_recip14(NE.recip_vectors()), NE.recip_reference(), 'gu_recip14')


def test_probe_is_recip_is_the_exact_rational_reciprocal_at_every_exponent(eng):
    v, ref = NE.is_recip_vectors(), NE.is_recip_reference()
    for k in sorted(v):
        _bytes(eng.probe_is_recip(v[k]), ref[k], 'gu_is_recip, ' + k)


def test_probe_exp_equals_the_numpy_rule_and_the_stated_edges(eng):
    x = NE.exp_vectors()
    with np.errstate(all='ignore'):
        want = AC.gu_exp(x)
    got = eng.probe_exp(x)
    _bytes(got, want, 'gu_exp')
    nz, no = len(NE.EXP_ZERO), len(NE.EXP_ONE)
    assert got[:nz].tobytes() == np.zeros(nz).tobytes() and got[nz:nz + no].tobytes() == np.ones(no).tobytes()  # (+0.0 for -inf too)
    assert (got[nz + no:] >= 2.0 ** -1022).all()  # from -700 up the result is normal


def test_probe_softmax_terms_reciprocal_and_action(eng):
    h, w = NE.softmax_vectors()
    with np.errstate(all='ignore'):
        e, Z, _ = AC.softmax(h)
        a = AC.action(e, Z, w)
    got = eng.probe_softmax(h, w)
    _bytes(got['e'], e, 'e')
    _bytes(got['Z'], Z, 'Z')
    _bytes(got['iz'], NE.exact_recip(Z), 'iz against the exact rational')
    _bytes(got['action'], a, 'action')
    assert (got['e'][np.arange(a.size), got['action']] > 0.0).all()


@pytest.mark.parametrize('n', [1, 63, 65])
def test_probe_partial_waves(eng, n):
    z, x = NE.recip_vectors()[-n:], NE.exp_vectors()[:n]
    _bytes(eng.probe_recip14(z), NE.recip_reference()[-n:], 'gu_recip14')
    v = NE.is_recip_vectors()['learner'][-n:]
    _bytes(eng.probe_is_recip(v), NE.is_recip_reference()['learner'][-n:], 'gu_is_recip')
    with np.errstate(all='ignore'):
        _bytes(eng.probe_exp(x), AC.gu_exp(x), 'gu_exp')
        h, w = (t[:n] for t in NE.softmax_vectors())
        e, Z, _ = AC.softmax(h)
        got = eng.probe_softmax(h, w)
        _bytes(got['e'], e, 'e')
        _bytes(got['Z'], Z, 'Z')
        _bytes(got['iz'], 1.0 / Z, 'iz')
        _bytes(got['action'], AC.action(e, Z, w), 'action')


def test_probe_changes_nothing_and_checks_its_arguments():
    g = GRIDS['default4x4']()
    vec = gua.VecGridUniverse(100, template=_spec(g), seed=3)
    o = RO.ReinforceOracle(_grid(g), 3, 100)
    try:
        assert np.array_equal(vec.reset(), o.reset())
        _same(vec.reinforce_run(30, 16, 0.05, 0.3, 0.9, trajectory=True, stats=True), o.reinforce(30, 16, 0.05, 0.3, 0.9))
        assert o.buf_cnt.any()
        eng = vec.engine
        assert eng.probe_exp(np.array([0.0, -1.0]))[0] == 1.0
        eng.probe_softmax(np.zeros((3, 4)), np.zeros(3, np.uint32))
        # the episode buffer is still carried, the tables and the state are untouched
        _same(vec.reinforce_run(30, 16, 0.05, 0.3, 0.9, trajectory=True, stats=True), o.reinforce(30, 16, 0.05, 0.3, 0.9))
        assert vec.preferences().tobytes() == o.h.tobytes() and vec.state_values().tobytes() == o.v.tobytes()
        x, y = np.ones(4), np.empty(4)
        w, a = np.zeros(1, np.uint32), np.zeros(1, np.int32)
        lib, h = eng.lib, eng._h
        p = _lib.ptr
        bad = [lambda: lib.gu_probe_numeric(h, 0, 4, None, p(y)), lambda: lib.gu_probe_numeric(h, 0, 4, p(x), None),
               lambda: lib.gu_probe_numeric(h, 0, -1, p(x), p(y)), lambda: lib.gu_probe_numeric(h, 3, 4, p(x), p(y)),
               lambda: lib.gu_probe_numeric(h, -1, 4, p(x), p(y)), lambda: lib.gu_probe_numeric(h, 0, _lib.PROBE_MAX + 1, p(x), p(y)),
               lambda: lib.gu_probe_numeric_softmax(h, -1, p(x), p(w), p(y), p(y), p(y), p(a))]
        for k in range(6):
            args = [p(x), p(w), p(y), p(y), p(y), p(a)]
            args[k] = None
            bad.append(lambda args=args: lib.gu_probe_numeric_softmax(h, 1, *args))
        for call in bad:
            with pytest.raises(gua.GuError) as err:
                _lib.check(call())
            assert err.value.code == -1
        y[:] = 7.0
        _lib.check(lib.gu_probe_numeric(h, 0, 0, p(x), p(y)))  # n = 0: a no-op
        _lib.check(lib.gu_probe_numeric_softmax(h, 0, p(x), p(w), p(y), p(y), p(y), p(a)))
        assert (y == 7.0).all()
        with pytest.raises(ValueError):
            eng.probe_softmax(np.zeros((3, 4)), np.zeros(2, np.uint32))
    finally:
        vec.close()


# ---- through the real kernels, with crafted tables

IS_N = 8191  # one env per vector; every exponent of NE.IS_EXPONENTS occurs at least six times


def test_is_run_exposes_all_53_bits_of_the_reciprocal_at_every_exponent():
    """T = L = 1, Q = 0, epsilon = 0, gamma = 0: the one entry the pass touches becomes 0 + (1 * RECIP(C + 1)) * (-1 - 0).  C = x - 1
    below 2^53 (C + 1 = x exactly) and C = x from 2^54 up (C + 1 rounds back to x), in every action of the start row."""
    assert IS_N % 64 != 0
    sub = NE.learner_subset(IS_N)
    x, ref = NE.is_recip_vectors()['learner'][sub], NE.is_recip_reference()['learner'][sub]
    assert np.unique(np.frexp(x)[1] - 1).tolist() == list(NE.IS_EXPONENTS)
    c0 = np.where(x < 2.0 ** 53, x - 1.0, x)
    assert ((c0 + 1.0) == x).all()
    vec = gua.VecGridUniverse(IS_N, template=_spec(CENTRE), seed=3)
    o = IO.IsOracle(_grid(CENTRE), 3, IS_N)
    try:
        vec._ensure_q(0.0)
        assert np.array_equal(vec.reset(), o.reset())
        c = np.zeros((IS_N, 25, 4))
        c[:, START, :] = c0[:, None]
        vec.set_importance_weights(c)
        o.set_c(c)
        _same(vec.off_policy_mc_run(1, 1, discount_factor=0.0, epsilon=0.0, trajectory=True, stats=True), o.is_run(1, 1, 0.0, 0, 2.0 ** 64))
        q, cw = vec.q_table(), vec.importance_weights()
        _bytes(q, o.q, 'Q')
        _bytes(cw, o.c, 'C')
        same_env_state(vec, o)
        # without the restatement: one entry of the start row moved, to -1 / x exactly; its weight is x
        moved = q[:, START, :] != 0.0
        assert (moved.sum(axis=1) == 1).all() and not np.delete(q, START, axis=1).any()
        a, idx = moved.argmax(axis=1), np.arange(IS_N)
        assert (np.bincount(a, minlength=4) > IS_N // 8).all()  # (the tie rule spreads the envs over the four actions)
        _bytes(q[idx, START, a], -ref, 'Q[start][a] against the exact rational')
        _bytes(cw[idx, START, a], x, 'C[start][a]')
    finally:
        vec.close()


AC_SEED = 5          # the first seed from 1 on whose words draw, in the restatement, another action than the row's first maximum ...
AC_COVERED = 1010    # ... in more than half of the 1909 rows (seed 1: 1001, seed 5: 1010)


def _crafted_softmax(oracle_cls):
    rows = NE.softmax_rows()
    n = rows.shape[0]
    assert n == 1909 and n % 64 != 0
    vec = gua.VecGridUniverse(n, template=_spec(CENTRE), seed=AC_SEED)
    o = oracle_cls(_grid(CENTRE), AC_SEED, n)
    assert np.array_equal(vec.reset(), o.reset())
    h = np.zeros((n, 25, 4))
    h[:, START, :] = rows
    vec.set_actor_critic(h=h)
    o.set_ac(h=h)
    with np.errstate(all='ignore'):
        e, Z, _ = AC.softmax(rows)
        a = AC.action(e, Z, TD.words(AC_SEED, o.env_ids, o.state.tcount))
    first = NE.first_max(rows)
    covered = a != first
    assert int(covered.sum()) == AC_COVERED and 2 * AC_COVERED > n
    # delta = -1 (reward -1, V = 0, gamma = 0), actor rate 1: H[start][first] = h + (-1) (0 - 1 * iz) = h + iz, and h = 0 on the edge rows
    idx = np.arange(n)
    want = rows[idx, first] + NE.exact_recip(Z)
    assert (rows[idx, first][covered] == 0.0).sum() > 200
    return vec, o, idx, first, covered, want


def _check_softmax_learner(vec, o, idx, first, covered, want):
    h, v = vec.preferences(), vec.state_values()
    _bytes(h, o.h, 'H')
    _bytes(v, o.v, 'V')
    same_env_state(vec, o)
    assert np.isfinite(h).all()
    _bytes(h[idx, START, first][covered], want[covered], 'H[start][first maximum] against the exact rational')


def test_ac_run_on_the_edge_rows():
    vec, o, idx, first, covered, want = _crafted_softmax(AC.AcOracle)
    try:
        with np.errstate(all='ignore'):
            ref = o.ac(1, 1.0, 0.5, 0.0)
        assert (ref['reward'] == -1).all() and not ref['done'].any()
        _same(vec.actor_critic_run(1, 1.0, 0.5, 0.0, trajectory=True, stats=True), ref)
        _check_softmax_learner(vec, o, idx, first, covered, want)
    finally:
        vec.close()


def test_reinforce_run_on_the_edge_rows():
    """T = L = 2: the pass updates the second step's state (a neighbour of the start, a row of zeros) and then the start row."""
    vec, o, idx, first, covered, want = _crafted_softmax(RO.ReinforceOracle)
    try:
        with np.errstate(all='ignore'):
            ref = o.reinforce(2, 2, 1.0, 0.5, 0.0)
        assert (ref['reward'] == -1).all() and not ref['done'].any() and not o.buf_cnt.any()
        _same(vec.reinforce_run(2, 2, 1.0, 0.5, 0.0, trajectory=True, stats=True), ref)
        assert not vec.episode_buffer()['count'].any()
        _check_softmax_learner(vec, o, idx, first, covered, want)
    finally:
        vec.close()


def test_is_run_walks_down_to_the_lower_weight_bound():
    """A corridor of 200 cells, Q rows (-1, -0.5, -1, -1): the walk is forced right; at gamma = 0 every update makes its row all -1
    (four maxima, ratio 1/4), so W = 4^-j and the pass over the 140 entries stops behind the one whose weight is exactly 2^-256."""
    g = dict(W=200, H=1, starts=[0], goals=[199], lava=[], walls=[])
    N, RIGHT = 65, 1
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=5)
    o = IO.IsOracle(_grid(g), 5, N)
    try:
        vec._ensure_q(0.0)
        assert np.array_equal(vec.reset(), o.reset())
        q0 = np.full((N, 200, 4), -1.0)
        q0[:, :, RIGHT] = -0.5
        vec.set_q_table(q0)
        o.set_q(q0)
        _same(vec.off_policy_mc_run(140, 140, discount_factor=0.0, epsilon=0.0, w_cap=2.0 ** 256, trajectory=True, stats=True),
              o.is_run(140, 140, 0.0, 0, 2.0 ** 256))
        assert (o.state.pos == 140).all() and o.walked == 129 * N and o.low == N and o.cap_eq == o.cap_gt == 0
        q, c = vec.q_table(), vec.importance_weights()
        _bytes(q, o.q, 'Q')
        _bytes(c, o.c, 'C')
        same_env_state(vec, o)
        assert not vec.off_policy_episode_buffer()['count'].any()
        # the closed form, without the restatement
        want_c = np.zeros((200, 4))
        want_c[11:140, RIGHT] = 4.0 ** -np.arange(128, -1, -1.0)
        assert want_c[11, RIGHT] == 2.0 ** -256 and want_c[139, RIGHT] == 1.0
        want_q = q0[0].copy()
        want_q[11:140] = -1.0
        for e in range(N):
            assert c[e].tobytes() == want_c.tobytes() and q[e].tobytes() == want_q.tobytes(), e
    finally:
        vec.close()


def test_is_run_ends_passes_at_and_above_the_weight_cap():
    """16 x 16 with the goal walled in, Q = -1000 everywhere, epsilon = 0, gamma = 0, w_cap = 16: a fresh entry becomes the only
    maximum of its row (ratio 4), so W runs 1, 4, 16 and ends ON the cap; entries of rows with two or three maxima carry W past it."""
    g = dict(W=16, H=16, starts=[0], goals=[254], lava=[], walls=[238, 253, 255])
    N, seed = 129, 1
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    o = IO.IsOracle(_grid(g), seed, N, q0=-1000.0)
    try:
        vec._ensure_q(-1000.0)
        assert np.array_equal(vec.reset(), o.reset())
        for T in (128, 64):
            _same(vec.off_policy_mc_run(T, 64, discount_factor=0.0, epsilon=0.0, w_cap=16.0, trajectory=True, stats=True),
                  o.is_run(T, 64, 0.0, 0, 16.0))
        assert o.cap_eq > 0 and o.cap_gt > 0 and o.low == 0 and o.passes == 3 * N
        print('passes ended by W == w_cap: %d, by W > w_cap: %d, of %d' % (o.cap_eq, o.cap_gt, o.passes))
        _bytes(vec.q_table(), o.q, 'Q')
        _bytes(vec.importance_weights(), o.c, 'C')
        same_env_state(vec, o)
        assert (o.c[o.c > 0] < 16.0 * 192).all() and np.isfinite(o.q).all()  # (no single addition to C reached the cap)
    finally:
        vec.close()
