// round6.h — exact "%.6f" rounding shared by the label-line kernels (K7 boxes, K13 polygons, K17 oriented boxes) with the
// printer of K13 and K17 (a class id's digits, a value's 8 bytes), and its two-decimal sibling for the COCO text (K16).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dyd {

// round-half-even(a * 10^6) for 0 <= a < 4294, exactly: a * 10^6 = t + e with t the rounded product and e the
// error term an FMA returns exactly; t = n + f (n integer, f exact).  f != 1/2 is at least ulp(t) >= 2|e| away
// from one half, so it decides alone; at f == 1/2 the sign of e decides and e == 0 is a true tie.
__device__ __forceinline__ uint32_t round6(double a) {
    const double t = a * 1.0e6;
    const double e = fma(a, 1.0e6, -t);
    const uint32_t n = (uint32_t)t;
    const double f = t - (double)n;
    const bool up = (f > 0.5) || (f == 0.5 && (e > 0.0 || (e == 0.0 && (n & 1u))));
    return n + (up ? 1u : 0u);
}

__device__ __forceinline__ int k13_digits(int32_t cid) {   // cid >= 0
    int n = 1;
    for (uint32_t v = (uint32_t)cid; v >= 10u; v /= 10u) ++n;
    return n;
}

// "%.6f" of n(v) as 8 ASCII bytes, the first in the low byte
__device__ __forceinline__ uint64_t k13_num8(double v) {
    v = (v <= 0.0) ? 0.0 : ((v >= 1.0) ? 1.0 : v);
    uint32_t q = round6(v);
    if (q >= 1000000u) return 0x3030303030302e31ull;   // "1.000000"
    uint64_t r = 0x2e30ull;                             // "0."
#pragma unroll
    for (int k = 7; k >= 2; --k) {
        const uint32_t t = q / 10u;
        r |= (uint64_t)('0' + (q - t * 10u)) << (8 * k);
        q = t;
    }
    return r;
}

// round-half-even(v * 100) for 0 <= v < 2^43, exactly, so "%.2f" of v is this integer with a dot before its last two digits
// (K16).  The same argument: t < 2^50 has ulp(t) <= 2^-3, so f is exact, and f != 1/2 is at least ulp(t) >= 2|e| away from it.
__device__ __forceinline__ uint64_t fix2(double v) {
    const double t = v * 100.0;
    const double e = fma(v, 100.0, -t);
    const uint64_t n = (uint64_t)t;
    const double f = t - (double)n;
    const bool up = (f > 0.5) || (f == 0.5 && (e > 0.0 || (e == 0.0 && (n & 1ull))));
    return n + (up ? 1ull : 0ull);
}

}  // namespace dyd
