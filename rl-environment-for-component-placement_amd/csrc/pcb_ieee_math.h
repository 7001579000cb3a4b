// pcb_ieee_math.h -- ln, exp and the square root of a double in IEEE + - * / alone, stated once.  Plain C++17 that compiles
// alone, on the host and on the device.  libm, ocml and torch disagree on these three in the last place, and a result that
// has to be the same bits on the host, on the device and in tensor code (pcbenv/search.py restates every line below as the
// same sequence of operations) cannot call any of them: no library call, no fma (the build passes -ffp-contract=off: one
// IEEE operation per written operator), no run-time table; the exponent and the mantissa are read and written through the
// bits, which is exact.  Deterministic, not correctly rounded.  Relative error against the exact value, measured against
// numpy over the arguments pcb_puct_noise.h can produce (tests/test_puct_noise_model.py asserts the bound REL_ERR):
//   ieee_ln    x a positive normal double.  x = m * 2^e with m in [sqrt(1/2), sqrt(2)); t = (m - 1) / (m + 1), |t| < 0.1716;
//              ln m = 2 t (1 + t^2 / 3 + ... + t^26 / 27), the series cut below 1e-22; + e * ln 2 in two parts.  < 5e-16, and
//              the same of max(|ln x|, 1 ulp of it): a result near 0 has e = 0 and no cancellation.
//   ieee_exp   x <= 0; exactly 0 below -708.  k = round(x / ln 2), r = x - k ln 2 in two parts (Cody-Waite), |r| < 0.3467;
//              14 terms of the Taylor series, cut below 5e-18; * 2^k through the bits, k >= -1021: a normal number.  < 5e-16.
//   ieee_sqrt  x a positive normal double.  x = m * 4^h with m in [1/2, 2); six Heron steps from 1 (relative error 0.41,
//              6e-2, 1.7e-3, 1.4e-6, 1e-12, below 1e-24); * 2^h through the bits.  < 5e-16.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCB_IEEE_HD __host__ __device__
#else
#define PCB_IEEE_HD
#endif

namespace pcb_ieee {

constexpr double REL_ERR = 5e-16;
constexpr double LN2_HI = 6.93147180369123816490e-01;  // 0x3fe62e42fee00000: the low 21 bits are 0, so e * LN2_HI is exact
constexpr double LN2_LO = 1.90821492927058770002e-10;  // ln 2 - LN2_HI
constexpr double LOG2_E = 1.44269504088896338700e+00;
constexpr double SQRT_HALF = 7.07106781186547524401e-01;

PCB_IEEE_HD inline uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
PCB_IEEE_HD inline double double_of(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
// x = mantissa * 2^exponent with the mantissa in [1/2, 1): frexp of a positive normal double
PCB_IEEE_HD inline int exponent_of(double x) { return (int)((bits_of(x) >> 52) & 0x7ffu) - 1022; }
PCB_IEEE_HD inline double mantissa_of(double x) { return double_of((bits_of(x) & 0x000fffffffffffffull) | 0x3fe0000000000000ull); }
// 2^k, -1022 <= k <= 1023
PCB_IEEE_HD inline double pow2(int k) { return double_of((uint64_t)(k + 1023) << 52); }

PCB_IEEE_HD inline double ieee_ln(double x) {
    int e = exponent_of(x);
    double m = mantissa_of(x);
    if (m < SQRT_HALF) { m = 2.0 * m; e = e - 1; }
    const double t = (m - 1.0) / (m + 1.0);
    const double t2 = t * t;
    double p = 1.0 / 27.0;
    p = p * t2 + 1.0 / 25.0;
    p = p * t2 + 1.0 / 23.0;
    p = p * t2 + 1.0 / 21.0;
    p = p * t2 + 1.0 / 19.0;
    p = p * t2 + 1.0 / 17.0;
    p = p * t2 + 1.0 / 15.0;
    p = p * t2 + 1.0 / 13.0;
    p = p * t2 + 1.0 / 11.0;
    p = p * t2 + 1.0 / 9.0;
    p = p * t2 + 1.0 / 7.0;
    p = p * t2 + 1.0 / 5.0;
    p = p * t2 + 1.0 / 3.0;
    p = p * t2 + 1.0;
    const double ef = (double)e;
    return ef * LN2_HI + (ef * LN2_LO + (2.0 * t) * p);
}

PCB_IEEE_HD inline double ieee_exp(double x) {
    if (x < -708.0) return 0.0;
    const double kf = (double)(int)(x * LOG2_E - 0.5);  // x <= 0: the conversion cuts towards 0, which rounds to the nearest
    const double r = (x - kf * LN2_HI) - kf * LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * pow2((int)kf);
}

PCB_IEEE_HD inline double ieee_sqrt(double x) {
    int e = exponent_of(x);
    double m = mantissa_of(x);
    if (e & 1) { m = 2.0 * m; e = e - 1; }  // e is even now and m in [1/2, 2)
    double y = 1.0;
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    return y * pow2(e >> 1);
}

}  // namespace pcb_ieee
