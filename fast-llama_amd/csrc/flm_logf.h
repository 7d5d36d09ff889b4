// flm_logf.h -- the natural logarithm of the entropy-driven samplers (flm_entropy.h; host/sampler.cpp entropy_logits), DEFINED BY ITS OPERATIONS: one function that the
// host (g++) and the device (hipcc, gfx950) both compile, so the two agree bit for bit.  It is not glibc's logf (whose table is not in this tree and which is not correctly
// rounded: "equal to libm" would pin a libm version); it is within 1 ulp of it.
//   x = 2^k m, m in [1, 2) taken as double; m > sqrt(2): m /= 2, k += 1 (m in (sqrt(2) / 2, sqrt(2)]: |s| <= 0.1716)
//   s = (m - 1) / (m + 1), z = s s;  log m = 2 atanh(s) = 2 s (1 + z / 3 + z^2 / 5 + ... + z^9 / 19), Horner with explicit fma, the coefficients IEEE double quotients
//   (the first dropped term, z^10 / 21, is below 2^-55 relative: far under the final rounding to float)
//   result = (float)fma(k, ln2, (2 s) w)
// Every operation is an IEEE double operation in this order, fma where written and nowhere else (no contraction: `#pragma clang fp contract(off)` here, -ffp-contract=off
// in the host's Makefile).  x == 1: m = 1, s = 0, k = 0: exactly +0.  Contract: x positive and normal (the callers pass a softmax sum: >= 1, finite).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLM_LOGF_HD __host__ __device__
#pragma clang fp contract(off)
#else
#define FLM_LOGF_HD
#endif

FLM_LOGF_HD inline float flm_logf(float x) {
    uint32_t ix; memcpy(&ix, &x, 4);
    int k = (int)(ix >> 23) - 127;
    const uint32_t im = (ix & 0x007fffffu) | 0x3f800000u;
    float mf; memcpy(&mf, &im, 4);
    double m = (double)mf;
    if (m > 0x1.6a09e667f3bcdp+0) { m = m * 0.5; k += 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double q = 1.0 / 19.0;
    q = fma(q, z, 1.0 / 17.0);
    q = fma(q, z, 1.0 / 15.0);
    q = fma(q, z, 1.0 / 13.0);
    q = fma(q, z, 1.0 / 11.0);
    q = fma(q, z, 1.0 / 9.0);
    q = fma(q, z, 1.0 / 7.0);
    q = fma(q, z, 1.0 / 5.0);
    q = fma(q, z, 1.0 / 3.0);
    const double w = fma(q, z, 1.0);
    return (float)fma((double)k, 0x1.62e42fefa39efp-1, (2.0 * s) * w);
}
