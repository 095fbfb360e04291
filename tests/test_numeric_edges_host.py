"""The exact references behind tests/test_gpu_numeric_edges.py, without a GPU: on the vectors of tests/_numeric_edges.py the
restatements' reciprocal (numpy's 1.0 / x) and a Python emulation of gu_recip14 equal the correctly rounded exact rational; the
exp rule's worst error against the exact exponential (mpmath, 200 bits) is the one DESIGN.md section 13 records; the softmax never
draws an action of probability zero."""
import collections
import os

import numpy as np

from griduniverse_amd import softmax as SM

from . import _ac_oracle as AC
from . import _numeric_edges as NE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured here with the restatement (numpy) on NE.exp_vectors(): 1.0904790... ulp at x = -633.1431925530318.  The arithmetic is
# deterministic, so the bound carries no margin beyond the rounding of the figure itself.  DESIGN.md section 13 quotes it.
EXP_WORST_ULP = 1.0905
# The correction moves of gu_recip14 on NE.recip_vectors(), as the Python emulation counts them.  DESIGN.md section 13 quotes them.
RECIP_MOVES = {0: 86861, 1: 61753, 2: 1400}


def test_reciprocal_vectors_hold_the_named_points_and_the_midpoint_cases():
    z = NE.recip_vectors()
    assert z.size == 13 + 100000 + 50001 and z.min() == 1.0 and z.max() == 4.0
    for v in (1.0, 2.0, 3.0, 4.0, 1.5, 2.5, 3.5, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), np.nextafter(2.0, 3.0), np.nextafter(4.0, 1.0)):
        assert (z == v).any(), v
    hard = z[100013:].reshape(-1, 3)  # (the double nearest to the reciprocal of a midpoint of [0.25, 1), between its two neighbours)
    assert (NE.ulps(hard[:, 0], hard[:, 1]) == 1).all() and (NE.ulps(hard[:, 2], hard[:, 1]) == 1).all()


def test_numpy_division_is_the_exact_rational_reciprocal_on_every_vector():
    """What the restatements write, 1.0 / x, is the correctly rounded quotient: on [1, 4] and at every exponent."""
    assert (1.0 / NE.recip_vectors()).tobytes() == NE.recip_reference().tobytes()
    v, ref = NE.is_recip_vectors(), NE.is_recip_reference()
    assert sorted(v) == ['learner', 'ones', 'pow2', 'small']
    for k in v:
        assert (1.0 / v[k]).tobytes() == ref[k].tobytes(), k
    exps = np.unique(np.frexp(v['learner'])[1] - 1)
    assert exps.tolist() == list(NE.IS_EXPONENTS)
    assert np.unique(np.frexp(v['small'])[1] - 1).tolist() == list(range(-1022, 0))


def test_gu_recip14_as_the_header_states_it_is_correctly_rounded_and_its_newton_part_alone_is_not():
    z, ref = NE.recip_vectors(), NE.recip_reference()
    got = [NE.recip14_emulated(v) for v in z.tolist()]
    assert np.array([g[0] for g in got]).tobytes() == ref.tobytes()
    moves = collections.Counter(g[1] for g in got)
    assert dict(moves) == RECIP_MOVES and max(moves) == 2  # (three rounds are provided)
    newton = NE.recip14_newton_only(z)
    wrong = newton != ref
    assert NE.ulps(newton, ref).max() == 2 and 0.40 < wrong.mean() < 0.44  # the integer correction carries the claim
    assert int(wrong.sum()) == RECIP_MOVES[1] + RECIP_MOVES[2]


def test_gu_exp_edges():
    with np.errstate(all='ignore'):
        for gu_exp in (AC.gu_exp, SM.gu_exp):
            assert gu_exp(np.array(NE.EXP_ZERO)).tobytes() == np.zeros(4).tobytes()  # (+0.0, -inf included)
            assert gu_exp(np.array(NE.EXP_ONE)).tobytes() == np.ones(4).tobytes()
            lowest = gu_exp(np.array([-700.0, np.nextafter(-700.0, 0.0)]))
            assert (lowest >= 2.0 ** -1022).all() and lowest[0] < lowest[1] < 1e-304  # normal, and the cutoff is not early
        x = NE.exp_vectors()
        assert AC.gu_exp(x).tobytes() == SM.gu_exp(x).tobytes()
    header = open(os.path.join(ROOT, 'include', 'gu.h')).read()
    assert 'gu_exp(-inf) = 0.0' in header


def test_gu_exp_worst_error_against_the_exact_exponential_is_the_recorded_one():
    x = NE.exp_vectors()
    x = x[x >= -700.0]
    assert x.size > 84000
    err = NE.exp_error_ulps(x, AC.gu_exp(x))
    worst = int(np.argmax(err))
    print('gu_exp: worst error %.6f ulp at x = %r; %d of %d vectors above 1 ulp' % (err[worst], float(x[worst]), int((err > 1.0).sum()), x.size))
    assert err.max() <= EXP_WORST_ULP
    assert err.max() > 1.0  # (the rule is NOT within 1 ulp of the exact value; it is within 1 ulp of math.exp, test_ac_host.py)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '%.4f ulp' % EXP_WORST_ULP in design


def test_softmax_rows_hold_every_edge_and_the_action_drawn_always_has_a_positive_term():
    rows = NE.softmax_rows()
    assert rows.shape[0] % 64 != 0
    with np.errstate(all='ignore'):
        e, Z, _ = AC.softmax(rows)
        e2, Z2 = SM.softmax_terms(rows)
    assert e.tobytes() == e2.tobytes() and Z.tobytes() == Z2.tobytes()
    assert not np.isnan(e).any() and ((Z >= 1.0) & (Z <= 4.0)).all()
    two = np.full_like(Z, 2.0)
    near = NE.ulps(Z, two) <= 4
    assert (Z == 1.0).sum() >= 100 and (Z == 4.0).sum() >= 6 and (Z == 2.0).sum() >= 100
    assert (near & (Z < 2.0)).sum() >= 16 and (near & (Z > 2.0)).sum() >= 100  # both sides of the `half` branch of gu_recip14
    assert (np.bincount((e == 0.0).sum(axis=1), minlength=4)[1:] >= 20).all()  # rows with one, two and three dead terms
    with np.errstate(over='ignore'):
        assert (rows.max(axis=1) - rows.min(axis=1) == np.inf).any()  # differences that overflow to -inf
    lowest = AC.gu_exp(np.array([-700.0]))[0]
    assert (e == lowest).any()  # a term exactly at the cutoff is alive ...
    h, w = NE.softmax_vectors()
    assert h.shape[0] == w.shape[0] == rows.shape[0] * 16 + 400000
    for word in NE.WORDS_FIXED:
        assert (w[:rows.shape[0] * 16] == word).sum() >= rows.shape[0]
    with np.errstate(all='ignore'):
        e, Z, _ = AC.softmax(h)
        a = AC.action(e, Z, w)
    assert (np.bincount(a, minlength=4) > 10000).all()
    # not a property of the restatement's own text: whatever the word, an action of probability zero is never drawn
    assert (e[np.arange(a.size), a] > 0.0).all()
    dead = (e == 0.0).any(axis=1)
    assert dead.sum() > 10000 and (w[dead] == 0xFFFFFFFF).any() and (w[dead] == 0).any()
