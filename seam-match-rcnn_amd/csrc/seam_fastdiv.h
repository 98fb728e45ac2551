// seam_fastdiv.h -- the one rule for the kernels' multiply-high divisions: the host's check and the device's helper.
//
// A kernel divides n by a launch-constant d as q = __umulhi(n, m) with m = ceil(2^32 / d) (d >= 2; every device helper takes n
// itself when d == 1, and m is 0 then).  Write m * d = 2^32 + e with 0 <= e < d and n = q d + r:
//     n m / 2^32 = q + r / d + n e / (d 2^32),
// so the high word is q exactly when r 2^32 + n e < d 2^32.  The worst remainder is r = d - 1, so the division is exact for every
// n < n_max when
//     (n_max - 1) * e < 2^32                                                     (the rule used here)
// -- sufficient, and weaker than the simpler n_max * d <= 2^32 (e < d).  Numerators must fit 32 bits: n_max <= 2^32.
// Example: d = 3906 has e = 3556, and n = 1101491 (r = d - 1) gives 282 instead of 281.
#pragma once

namespace seam_fastdiv {

inline unsigned magic(unsigned long long d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + d - 1) / d); }

// true: __umulhi(n, magic(d)) == n / d for every 0 <= n < n_max (d == 1: the helpers' d == 1 branch; d == 0 never)
inline bool exact(unsigned long long d, unsigned long long n_max) {
    if (d == 0 || d >= (1ull << 32) || n_max > (1ull << 32)) return false;
    if (d == 1 || n_max <= 1) return true;
    const unsigned long long e = (unsigned long long)magic(d) * d - (1ull << 32);
    return e == 0 || (n_max - 1) < ((1ull << 32) + e - 1) / e;         // (n_max - 1) * e < 2^32 without overflow
}

}  // namespace seam_fastdiv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// The device half: a / d with m = magic(d) -- one v_mul_hi_u32 / s_mul_hi_u32 instead of the ~20 VALU instructions of an integer
// division; exact for the numerator bound the launcher's plan checks with exact() for each divisor.
__device__ __forceinline__ int fdivu(int a, int d, unsigned m) { return d == 1 ? a : (int)__umulhi((unsigned)a, m); }
#endif
