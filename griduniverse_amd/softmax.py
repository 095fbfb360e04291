"""The build's softmax policy on the host: numpy restatements of `gu_exp` and of rule 2 of gu_ac_run (include/gu.h), giving
the same float64 bytes as the device (csrc/gu_softmax.hpp).  Every operation is one IEEE float64 operation, rounded once, in
the order the header states."""
import numpy as np

LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
# 1/13!, 1/12!, ..., 1/2!, 1, 1: the Horner order of gu_exp (each the double nearest to 1/n!; n! is exact in float64)
_COEFFS = [1.0 / float(np.prod(np.arange(1, n + 1, dtype=np.float64))) for n in range(13, -1, -1)]


def gu_exp(x):
    """gu_exp for float64 x <= 0 (an array or a scalar): 0 below -700, else ldexp(p, k) as include/gu.h states it."""
    x = np.asarray(x, np.float64)
    k = np.rint(x * LOG2E)
    r = (x - k * LN2_HI) - k * LN2_LO
    p = np.full_like(x, _COEFFS[0])
    for c in _COEFFS[1:]:
        p = p * r + c
    with np.errstate(invalid='ignore', over='ignore'):
        ki = np.where(x < -700.0, 0, k).astype(np.int64)
    return np.where(x < -700.0, 0.0, np.ldexp(p, ki))


def softmax_terms(h):
    """Rule 2 on preference rows h [..., 4]: (e [..., 4], Z [...]) -- e_b = gu_exp(h_b - m) with m the row maximum folded left
    to right with `>`, Z = ((e_0 + e_1) + e_2) + e_3."""
    h = np.asarray(h, np.float64)
    m = h[..., 0]
    for b in (1, 2, 3):
        m = np.where(h[..., b] > m, h[..., b], m)
    e = gu_exp(h - m[..., None])
    return e, ((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]


def softmax_policy(h):
    """pi [..., 4] of preference rows h [..., 4]: pi_b = e_b * (1 / Z), as the device computes it."""
    e, Z = softmax_terms(h)
    return e * (1.0 / Z)[..., None]
