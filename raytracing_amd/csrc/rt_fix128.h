// rt_fix128.h -- the two-word (128-bit) fixed-point accumulator of the order-independent sums (sensitivity.hip's A^T in global
// memory, kirchhoff.hip's L in LDS).  A sum is kept as an integer number of quanta 2^e: value = hi 2^64 + lo - 2^63 quanta.  The
// low word starts at the bias 2^63, so that sums of either sign stay clear of the word's ends and the high word is touched only
// on a real carry or borrow.  Integer sums commute: the result has the same bits in every schedule.
//
// Host and device.  A host build (tests/native/fix128_check.cpp) declares a plain atomicAdd of its own before including this.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define RT_FIX_HD __host__ __device__
#else
#define RT_FIX_HD
#endif

namespace rt {

constexpr int kFixBits = 57;                          // a term is below 2^57 quanta: 64 lanes' sum of terms fits an int64
constexpr unsigned long long kFixBias = 1ull << 63;   // what a low word starts from

// The quantum's exponent e from a bound on any term: |term| <= bound = f 2^ex with f in [0.5, 1), so |term| < 2^57 quanta 2^e
RT_FIX_HD inline int fix_exponent(double bound) {
    int ex;
    (void)frexp(bound, &ex);
    return ex - kFixBits;
}

// s quanta added to accumulator q of (lo, hi), sign-extended: the low word's carry, read from the value the add returned, goes
// to the high word; the high word is written only when it changes.  Returns the number of atomics issued.
#if defined(__HIPCC__)
__device__ __forceinline__
#else
inline
#endif
int add128(unsigned long long* lo, unsigned long long* hi, size_t q, long long s) {
    if (s == 0) return 0;
    const unsigned long long a = (unsigned long long)s;
    const unsigned long long old = atomicAdd(lo + q, a);
    const unsigned long long h = (s < 0 ? ~0ull : 0ull) + ((old + a) < old ? 1ull : 0ull);
    if (h == 0) return 1;
    atomicAdd(hi + q, h);
    return 2;
}

// hi 2^64 + lo - 2^63 as the nearest double (ties to even): one rounding.
RT_FIX_HD inline double fix_to_double(unsigned long long lo, unsigned long long hi) {
    if (!(lo >> 63)) hi -= 1ull;                              // the borrow of lo - 2^63
    lo ^= kFixBias;
    const bool neg = (hi >> 63) != 0;
    if (neg) {                                                // two's complement negation of (hi, lo)
        lo = ~lo + 1ull;
        hi = ~hi + (lo == 0 ? 1ull : 0ull);
    }
    double v;
    if (hi == 0) {
        v = (double)lo;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        const int sh = __clzll((long long)hi);                // 0 .. 63; the top 64 bits, the rest folded into a sticky bit
#else
        const int sh = __builtin_clzll(hi);
#endif
        unsigned long long top = sh ? ((hi << sh) | (lo >> (64 - sh))) : hi;
        const unsigned long long rest = sh ? (lo << sh) : lo;
        top |= rest ? 1ull : 0ull;
        v = ldexp((double)top, 64 - sh);
    }
    return neg ? -v : v;
}

}  // namespace rt
