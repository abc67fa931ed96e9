// Test helper (CPU, g++): raytracing_amd/csrc/rt_fix128.h compiled for the host.  The conversion of an accumulator back to
// double beside (double) of the same value as an __int128, and add128 on a plain, non-atomic stand-in for atomicAdd.
// tests/test_fix128_host.py drives it.
#include <cstddef>

static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}

#include "../../raytracing_amd/csrc/rt_fix128.h"

extern "C" int fix_bits() { return rt::kFixBits; }
extern "C" unsigned long long fix_bias() { return rt::kFixBias; }
extern "C" int fix_exponent(double bound) { return rt::fix_exponent(bound); }

// got[i] = rt::fix_to_double(lo[i], hi[i]); want[i] = (double)(hi 2^64 + lo - 2^63) taken as a signed 128-bit integer
extern "C" void fix_convert(long n, const unsigned long long* lo, const unsigned long long* hi, double* got, double* want) {
    for (long i = 0; i < n; i++) {
        got[i] = rt::fix_to_double(lo[i], hi[i]);
        const __int128 q = (__int128)(((unsigned __int128)hi[i] << 64) | lo[i]) - ((__int128)1 << 63);
        want[i] = (double)q;
    }
}

// s[0..n) added in turn to the accumulator acc = {lo, hi}; issued[i] = what add128 returned for s[i], hi_after[i] = the high word
extern "C" void fix_add(unsigned long long* acc, long n, const long long* s, int* issued, unsigned long long* hi_after) {
    for (long i = 0; i < n; i++) {
        issued[i] = rt::add128(acc, acc + 1, 0, s[i]);
        hi_after[i] = acc[1];
    }
}
