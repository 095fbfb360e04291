"""Vectors and exact references for the float64 building blocks of csrc/gu_softmax.hpp -- gu_exp, gu_recip14, gu_is_recip (RECIP of
gu_is_run) and the softmax of one row -- at the edges learning never reaches.  tests/test_numeric_edges_host.py checks the references
and the restatements on them without a GPU, tests/test_gpu_numeric_edges.py puts the same vectors on the device.  Everything is
seeded and built once per process.  The references for the reciprocals are exact rationals (fractions.Fraction; float() of a
Fraction rounds correctly).  Test infrastructure."""
import functools
import struct
from fractions import Fraction

import numpy as np

from . import _ac_oracle as AC

WORDS_FIXED = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
# the exponents p at which gu_is_run can be handed x = f 2^p through C: x - 1 installs exactly below 2^53 and x itself rounds back
# from x + 1 at 2^54 and above; 2^1021 is the last binade whose reciprocals are all normal
IS_EXPONENTS = tuple(range(1, 53)) + tuple(range(54, 1022))


def bits(x):
    return struct.unpack('<q', struct.pack('<d', x))[0]


def from_bits(b):
    return struct.unpack('<d', struct.pack('<q', b))[0]


def ulps(a, b):
    """Distance in representable doubles (same sign, finite)."""
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def exact_recip(x):
    """float64[n]: the correctly rounded 1 / x, from exact rational arithmetic."""
    return np.array([float(Fraction(1) / Fraction(float(v))) for v in np.asarray(x, np.float64).reshape(-1)], np.float64)


# ---- gu_recip14 as csrc/gu_softmax.hpp states it, in Python floats (one IEEE operation each) and ints

def _fixed(x, shift):
    b = bits(x)
    return ((b & 0xFFFFFFFFFFFFF) | (1 << 52)) << ((b >> 52) - 1023 - 52 + shift)


def recip14_emulated(z):
    """(1 / z as gu_recip14 computes it, the number of one-ulp correction moves it made) for a Python float z in [1, 4]."""
    half = z >= 2.0
    m = z * 0.5 if half else z
    y = 24.0 / 17.0 - (8.0 / 17.0) * m
    for _ in range(4):
        y = y * (2.0 - m * y)
    y = y * 0.5 if half else y
    y = 0.25 if y < 0.25 else 1.0 if y > 1.0 else y
    Z, one_hi, moves = _fixed(z, 52), 1 << 43, 0
    for _ in range(3):
        b = bits(y)
        Y = _fixed(y, 54)
        up = y < 1.0 and ((Z * (Y + _fixed(from_bits(b + 1), 54))) >> 64) < one_hi
        dn = y > 0.25 and ((Z * (Y + _fixed(from_bits(b - 1), 54))) >> 64) >= one_hi
        y = from_bits(b + (1 if up else 0) - (1 if dn else 0))
        moves += (1 if up else 0) + (1 if dn else 0)
    return y, moves


def recip14_newton_only(z):
    """The Newton part alone (no clamp, no correction), vectorised: what the integer test has to repair."""
    z = np.asarray(z, np.float64)
    half = z >= 2.0
    m = np.where(half, z * 0.5, z)
    y = 24.0 / 17.0 - (8.0 / 17.0) * m
    for _ in range(4):
        y = y * (2.0 - m * y)
    return np.where(half, y * 0.5, y)


# ---- the vectors

@functools.lru_cache(None)
def recip_vectors():
    """float64[150 014]: z in [1, 4] -- 1, 2, 3, 4 with their neighbours, 1.5, 2.5, 3.5; 100 000 uniform; 50 001 hard cases: for a random
    double y in [0.25, 1) the double nearest to the reciprocal of the exact midpoint of y and its upper neighbour, and that double's two
    neighbours (1 / z then lies as close to a rounding boundary as this y allows)."""
    rng = np.random.default_rng(20240613)
    special = [1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), 2.0, np.nextafter(2.0, 3.0), np.nextafter(3.0, 2.0), 3.0,
               np.nextafter(3.0, 4.0), np.nextafter(4.0, 3.0), 4.0, 1.5, 2.5, 3.5]
    uniform = rng.uniform(1.0, 4.0, 100000)
    hard = []
    for y in rng.uniform(0.25, 1.0, 16667):
        mid = (Fraction(float(y)) + Fraction(float(np.nextafter(y, 2.0)))) / 2
        z = float(Fraction(1) / mid)
        hard += [float(np.nextafter(z, 0.0)), z, float(np.nextafter(z, 8.0))]
    z = np.concatenate([np.array(special, np.float64), uniform, np.array(hard, np.float64)])
    assert ((z >= 1.0) & (z <= 4.0)).all()
    z.setflags(write=False)
    return z


@functools.lru_cache(None)
def recip_reference():
    ref = exact_recip(recip_vectors())
    ref.setflags(write=False)
    return ref


@functools.lru_cache(None)
def is_recip_vectors():
    """dict of float64 arrays, positive normal x whose reciprocal is normal:
    learner : the mantissas of recip_vectors() (brought into [1, 2)), vector i at exponent IS_EXPONENTS[i % 1020], then 2^p and
              (2 - 2^-52) 2^p for every p of IS_EXPONENTS -- what gu_is_run can be handed through C;
    small   : the same mantissas at exponents -1 .. -1022 (vector i at -1 - i % 1022);
    pow2    : 2^p, p = -1022 .. 1022;   ones : (2 - 2^-52) 2^p, p = -1022 .. 1021."""
    z = recip_vectors()
    f = np.where(z >= 4.0, 1.0, np.where(z >= 2.0, z * 0.5, z))
    i = np.arange(f.size)
    ones = 2.0 - 2.0 ** -52
    p_is = np.array(IS_EXPONENTS)
    out = dict(learner=np.concatenate([np.ldexp(f, p_is[i % p_is.size]), np.ldexp(1.0, p_is), np.ldexp(ones, p_is)]),
               small=np.ldexp(f, -1 - (i % 1022)),
               pow2=np.ldexp(1.0, np.arange(-1022, 1023)),
               ones=np.ldexp(ones, np.arange(-1022, 1022)))
    for x in out.values():
        assert np.isfinite(x).all() and (x >= 2.0 ** -1022).all()
        x.setflags(write=False)
    return out


@functools.lru_cache(None)
def is_recip_reference():
    out = {k: exact_recip(x) for k, x in is_recip_vectors().items()}
    for k, r in out.items():
        assert (r >= 2.0 ** -1022).all(), k  # normal
        r.setflags(write=False)
    return out


def learner_subset(n):
    """Indices of n of is_recip_vectors()['learner'] for the one-env-per-vector test of gu_is_run: the specials, then hard cases and
    uniform mantissas in equal parts, then every 2^p and all-ones vector that fits -- so every exponent of IS_EXPONENTS occurs."""
    total = is_recip_vectors()['learner'].size
    tail = np.arange(total - 2 * len(IS_EXPONENTS), total)
    k = n - 13 - tail.size
    assert k > 2 * len(IS_EXPONENTS)
    idx = np.concatenate([np.arange(13), 13 + np.arange(k // 2), 100013 + np.arange(k - k // 2), tail])
    assert idx.size == n and np.unique(idx).size == n
    return idx


EXP_ZERO = (-700.0000000000001, -745.0, -1e300, -np.inf)  # (the first: the first double below -700)
EXP_ONE = (0.0, -0.0, -2.0 ** -1022, -5e-324)


@functools.lru_cache(None)
def exp_vectors():
    """float64[n], x <= 0: the arguments that give 0.0 (EXP_ZERO), those that give 1.0 (EXP_ONE), -700 and its neighbour above, 60 000
    uniform in [-700, 0], 20 000 in [-1, 0], 3 000 log-uniform tiny ones, and the doubles within 4 ulp of (an estimate good to 2 ulp
    of) every seventh breakpoint -(k + 1/2) ln 2 of the range reduction, k = 0 .. 1009."""
    rng = np.random.default_rng(20240614)
    assert EXP_ZERO[0] == np.nextafter(-700.0, -np.inf)
    edge = list(EXP_ZERO) + list(EXP_ONE) + [-700.0, float(np.nextafter(-700.0, 0.0))]
    near = []
    for k in range(0, 1010, 7):
        b = -(k + 0.5) * 0.6931471805599453  # (within 2 ulp of the breakpoint: two roundings)
        near += [from_bits(bits(b) + d) for d in range(-4, 5)]
    x = np.concatenate([np.array(edge, np.float64), -rng.uniform(0.0, 700.0, 60000), -rng.uniform(0.0, 1.0, 20000),
                        -10.0 ** rng.uniform(-320.0, 0.0, 3000), np.array(near, np.float64)])
    assert (x <= 0.0).all() and (x[len(EXP_ZERO) + len(EXP_ONE):] >= -700.0).all()
    x.setflags(write=False)
    return x


def exp_error_ulps(x, got):
    """float64[n]: |got - exp(x)| in units of the spacing of the doubles at exp(x), exp by mpmath at 200 bits (finite x >= -700)."""
    import mpmath
    out = np.empty(len(x), np.float64)
    with mpmath.workprec(200):
        for i, (xi, gi) in enumerate(zip(x.tolist(), got.tolist())):
            want = mpmath.exp(mpmath.mpf(xi))
            ulp = mpmath.ldexp(mpmath.mpf(1), int(mpmath.floor(mpmath.log(want, 2))) - 52)
            out[i] = float(abs(mpmath.mpf(gi) - want) / ulp)
    return out


def _perms(row):
    """The distinct rotations of a row, so that the maximum visits every position."""
    out = []
    for k in range(4):
        r = tuple(row[k:] + row[:k])
        if r not in out:
            out.append(r)
    return out


@functools.lru_cache(None)
def near_two_rows():
    """Rows whose Z (restatement) lies within 4 doubles of 2.0, found by search: (0, a, D, D) with a a few 2^-53 below 0 (Z = 2 or
    just below) and (0, 0, b, D) with e_b around 2^-52 (Z = 2 or just above); D = -800 contributes 0."""
    D = -800.0
    cand = [[0.0, -j * 2.0 ** -53, D, D] for j in range(0, 48)] + [[0.0, 0.0, b, D] for b in np.linspace(-37.5, -33.5, 129)]
    cand = np.array(cand, np.float64)
    Z = AC.softmax(cand)[1]
    keep = cand[ulps(Z, np.full_like(Z, 2.0)) <= 4]
    return [tuple(r) for r in keep]


@functools.lru_cache(None)
def softmax_rows():
    """float64[n, 4], n odd and no multiple of 64: the edge rows in every rotation -- all tied, two and three maxima, one maximum with
    the rest beyond -700 (Z = 1), gaps straddling -700 by one ulp, differences that overflow to -inf, Z next to 2.0 -- and twice as many
    random rows, seven in eight N(0, 0.5) (every action likely) and the rest N(0, 300) (one action certain)."""
    lo, hi = float(np.nextafter(-700.0, -np.inf)), float(np.nextafter(-700.0, 0.0))
    rows = []
    for c in (0.0, 1e308, -1e308, 5.5, -3.0, -5e-324):  # all tied: Z = 4
        rows.append((c, c, c, c))
    for other in (-800.0, -1.25, -36.7, -1e308, -700.0):  # two and three maxima
        rows += _perms([0.0, 0.0, other, other]) + _perms([0.0, other, 0.0, other]) + _perms([0.0, 0.0, 0.0, other])
        rows += _perms([2.5, 2.5, 2.5 + other, 2.5 + other])
    for far in (-701.0, lo, -1e5, -1e308, -1.7e308):  # one maximum, the others dead: Z = 1 exactly
        rows += _perms([0.0, far, far, far])
    rows += _perms([0.0, -700.0, lo, hi]) + _perms([0.0, lo, lo, -700.0]) + _perms([0.0, hi, -700.0, -700.0])  # straddling -700
    rows += _perms([100.0, -600.0, float(np.nextafter(-600.0, -np.inf)), float(np.nextafter(-600.0, 0.0))])
    rows += _perms([1e308, -1e308, 0.0, -1e308]) + _perms([1.7e308, -1.7e308, 1.7e308, 0.0]) + _perms([0.0, -1.7e308, -1e308, 0.0])
    rows += _perms([1e308, 1e308 - 1e294, -1e308, 0.0])  # (an overflowing difference beside a live one)
    for r in near_two_rows():
        rows += _perms(list(r))
    edge = np.array(rows, np.float64)
    rng = np.random.default_rng(20240615)
    n_random = 2 * edge.shape[0] + (1 - edge.shape[0] % 2)
    n_random += 2 if (edge.shape[0] + n_random) % 64 == 0 else 0
    n_wide = n_random // 8
    h = np.concatenate([edge, rng.normal(0.0, 0.5, (n_random - n_wide, 4)), rng.normal(0.0, 300.0, (n_wide, 4))])
    assert h.shape[0] % 2 == 1 and h.shape[0] % 64 != 0 and np.isfinite(h).all()
    h.setflags(write=False)
    return h


@functools.lru_cache(None)
def softmax_vectors():
    """(h float64[n, 4], w uint32[n]): every row of softmax_rows() with each word of WORDS_FIXED and 11 random words, then 400 000 random
    rows (N(0, 2), N(0, 30), N(0, 300) in turn) with random words."""
    rows = softmax_rows()
    rng = np.random.default_rng(20240616)
    per = len(WORDS_FIXED) + 11
    w = np.concatenate([np.tile(np.array(WORDS_FIXED, np.uint32), (rows.shape[0], 1)),
                        rng.integers(0, 2 ** 32, (rows.shape[0], 11), dtype=np.uint64).astype(np.uint32)], axis=1).reshape(-1)
    h = np.repeat(rows, per, axis=0)
    scale = np.array([2.0, 30.0, 300.0])[np.arange(400000) % 3]
    h = np.concatenate([h, rng.normal(0.0, 1.0, (400000, 4)) * scale[:, None]])
    w = np.concatenate([w, rng.integers(0, 2 ** 32, 400000, dtype=np.uint64).astype(np.uint32)])
    h.setflags(write=False)
    w.setflags(write=False)
    return h, w


def first_max(h):
    """int[n]: the position of the row maximum folded left to right with `>` (the first of equal maxima)."""
    return np.argmax(np.asarray(h, np.float64), axis=1)
