// gu_softmax.hpp -- the build's float64 softmax pieces for gfx950 (include/gu.h: gu_ac_run rule 2, "the build's exp"):
// gu_exp, a reciprocal for [1, 4] (and, around it, gu_is_run's for any exponent) and the softmax of one preference row.
// gu_probe.hip runs each of them on the caller's arrays (include/gu_diag.h) for the tests of their edges.  Every learner is checked byte for byte against a CPU
// restatement, and neither OCML's exp nor libm's is reproducible on the other side, so both are built here from operations
// that round once and the same way everywhere: float64 multiply and add (__dmul_rn / __dadd_rn, -ffp-contract=off), rint
// (v_rndne_f64), ldexp (v_ldexp_f64) and integer arithmetic.
//
// The division 1 / Z is the one place where the obvious code would not do: a float64 division (x / y, __ddiv_rn) lowers to
// v_div_scale / v_rcp / v_fma_f64 Newton steps / v_div_fmas / v_div_fixup.  Its result is the correctly rounded quotient, but
// its v_fma_f64s would be the only ones in the learner kernels, whose ISA is checked for none (a stray contraction would break
// the byte-for-byte checks).  gu_recip14 gets the same correctly rounded 1 / Z without them: Newton steps with rounded
// multiplies and adds come within 2 ulp, and an exact integer test against the two neighbouring midpoints fixes the last bits.
#pragma once
#include "gu_tabular.hpp"  // (QRow, gu_q_max)

// gu_exp(x) for x <= 0 (include/gu.h): 0 below -700; else k = rint(x * log2(e)) (half to even), r = (x - k * ln2_hi) - k * ln2_lo,
// p = Horner over 1/13!, 1/12!, ..., 1/2!, 1, 1 (p = p * r + c, two roundings per step), result ldexp(p, k).  For x >= -700,
// k >= -1010, so the result is normal and the ldexp exact.  Each 1/n! is the double nearest to it (1.0 / n!, n! exact).
__device__ __forceinline__ double gu_exp(double x)
{
    const double k = __builtin_rint(__dmul_rn(x, 1.4426950408889634));
    const double r = __dsub_rn(__dsub_rn(x, __dmul_rn(k, 6.93147180369123816490e-01)), __dmul_rn(k, 1.90821492927058770002e-10));
    double p = 1.0 / 6227020800.0;  // 1/13!
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 479001600.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 39916800.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 3628800.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 362880.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 40320.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 5040.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 720.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 120.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 24.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 6.0);
    p = __dadd_rn(__dmul_rn(p, r), 0.5);
    p = __dadd_rn(__dmul_rn(p, r), 1.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0);
    return x < -700.0 ? 0.0 : __builtin_ldexp(p, (int)k);
}

// x * 2^shift as an integer, for x whose every bit lies at or above 2^-shift (the callers: z in [1, 4] at 2^52, y in [0.25, 1] at 2^54)
__device__ __forceinline__ uint64_t gu_fixed(double x, int shift)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const uint64_t mant = (b & 0xFFFFFFFFFFFFFull) | (1ull << 52);
    return mant << ((int)(b >> 52) - 1023 - 52 + shift);
}

// 1 / z correctly rounded (round to nearest; the quotient of two doubles is never a midpoint), for z in [1, 4]
__device__ __forceinline__ double gu_recip14(double z)
{
    // seed on m = z or z / 2 in [1, 2]: 24/17 - 8/17 m (relative error <= 1/17), then four Newton steps y = y (2 - m y)
    const bool half = z >= 2.0;
    const double m = half ? __dmul_rn(z, 0.5) : z;
    double y = __dsub_rn(24.0 / 17.0, __dmul_rn(8.0 / 17.0, m));
#pragma unroll
    for (int i = 0; i < 4; ++i) y = __dmul_rn(y, __dsub_rn(2.0, __dmul_rn(m, y)));
    y = half ? __dmul_rn(y, 0.5) : y;
    // within 2 ulp of 1 / z now; the answer lies in [0.25, 1], so clamp, then step towards it while a neighbouring midpoint
    // lies on the far side.  On the 2^-54 grid of [0.25, 1] and the 2^-52 grid of [1, 4]: 1/z > (y + y_up) / 2 iff
    // Z * (Y + Y_up) < 2^107 (Z = z 2^52 < 2^55, Y = y 2^54, sums < 2^56), i.e. iff the high 64 bits of the product are below
    // 2^43; and 1/z < (y + y_down) / 2 iff they are not (the product is never exactly 2^107: 1/z is never a midpoint)
    y = y < 0.25 ? 0.25 : y > 1.0 ? 1.0 : y;
    const uint64_t Z = gu_fixed(z, 52), one_hi = 1ull << 43;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int64_t b = __double_as_longlong(y);
        const uint64_t Y = gu_fixed(y, 54);
        const bool up = y < 1.0 && __umul64hi(Z, Y + gu_fixed(__longlong_as_double(b + 1), 54)) < one_hi;
        const bool dn = y > 0.25 && __umul64hi(Z, Y + gu_fixed(__longlong_as_double(b - 1), 54)) >= one_hi;
        y = __longlong_as_double(b + (up ? 1 : 0) - (dn ? 1 : 0));
    }
    return y;
}

// RECIP of gu_is_run (include/gu.h): 1 / x correctly rounded for a positive normal x whose reciprocal is normal: gu_recip14 on the
// mantissa in [1, 2), the exponent put back by ldexp (exact)
__device__ __forceinline__ double gu_is_recip(double x)
{
    const int64_t b = __double_as_longlong(x);
    const int ex = (int)((b >> 52) & 0x7FF) - 1023;
    const double m = __longlong_as_double((b & 0x000FFFFFFFFFFFFFll) | 0x3FF0000000000000ll);
    return __builtin_ldexp(gu_recip14(m), -ex);
}

// the softmax of one preference row h (include/gu.h, gu_ac_run rule 2): m = the row maximum folded left to right with `>`,
// e_b = gu_exp(h_b - m), Z = ((e_0 + e_1) + e_2) + e_3.  One e_b is gu_exp(0) = 1 and none exceeds 1, so Z lies in [1, 4].
struct SoftRow {
    double e0, e1, e2, e3, Z;
};

__device__ __forceinline__ SoftRow gu_softmax_row(const QRow &h)
{
    const double mx = gu_q_max(h);
    SoftRow s;
    s.e0 = gu_exp(__dsub_rn(h.v0, mx));
    s.e1 = gu_exp(__dsub_rn(h.v1, mx));
    s.e2 = gu_exp(__dsub_rn(h.v2, mx));
    s.e3 = gu_exp(__dsub_rn(h.v3, mx));
    s.Z = __dadd_rn(__dadd_rn(__dadd_rn(s.e0, s.e1), s.e2), s.e3);
    return s;
}

// the action of rule 3: x = (w 2^-32) Z; the first b with x < c_b (c_b = e_0 + .. + e_b, added left to right; c_3 = Z), else 3
// (x < c_3 and no qualifier both give 3)
__device__ __forceinline__ uint32_t gu_softmax_action(const SoftRow &s, uint32_t w)
{
    const double x = __dmul_rn(__dmul_rn((double)w, 2.3283064365386962890625e-10), s.Z);
    const double c0 = s.e0, c1 = __dadd_rn(c0, s.e1), c2 = __dadd_rn(c1, s.e2);
    return x < c0 ? 0u : x < c1 ? 1u : x < c2 ? 2u : 3u;
}
