// rt_hilbert.h -- the taps of the time-domain Hilbert transform of rtmi_kirchhoff_hilbert (kirchhoff_hilbert.hip; DESIGN.md
// section 23) and the definition of y = H x as a plain host loop.  Plain C++ with no HIP in it: the library takes its taps from
// hilbert_taps (rtmi_hilbert_taps hands them out, the device gets them uploaded), and a host program includes this header
// (tests/native/hilbert_taps.cpp).  Build with -ffp-contract=off, as the library is.
//   H is circular along an axis of n samples, H[cos] = sin; as a matrix, the FFT form with DC and Nyquist zeroed and the positive
//   frequencies doubled.  With K = floor((n - 1) / 2) and a_k = pi k / n:
//     n even:  c_k = (2 / n) cot(a_k) for odd k, c_k = 0 for even k                 k = 1 .. K
//     n odd :  c_k = (cot(a_k) - (-1)^k / sin(a_k)) / n                             k = 1 .. K
//     y[i] = sum over k = 1 .. K ascending with c_k != 0 of fl(c_k fl(x[(i - k) mod n] - x[(i + k) mod n])), from +0.0,
//   every subtract, product and add a separate fp64 operation.  n = 1 and n = 2 have no taps: y = +0.
//   fl(a - b) = -fl(b - a) and a sum of negated terms is the negated sum, so the matrix satisfies H^T = -H in every bit.
// The odd n's taps are evaluated by the half angle, cot(a) - 1 / sin(a) = -tan(a / 2) and cot(a) + 1 / sin(a) = cot(a / 2): the same
// numbers without the cancellation of cos(a) - 1 at small a.
#pragma once
#include <cmath>
#include <cstdint>

namespace rt {

constexpr long double kPiL = 3.14159265358979323846264338327950288L;

inline int64_t hilbert_ntaps(int64_t n) { return (n - 1) / 2; }

// taps[k - 1] = c_k for k = 1 .. hilbert_ntaps(n): long double, rounded once to fp64; exact 0.0 at the even k of an even n
inline void hilbert_taps(int64_t n, double* taps) {
    const int64_t K = hilbert_ntaps(n);
    const long double ln = (long double)n;
    for (int64_t k = 1; k <= K; k++) {
        const long double a = kPiL * (long double)k / ln;
        long double c;
        if (n % 2 == 0) c = (k & 1) ? 2.0L * cosl(a) / (ln * sinl(a)) : 0.0L;
        else c = (k & 1) ? cosl(0.5L * a) / (ln * sinl(0.5L * a)) : -tanl(0.5L * a) / ln;
        taps[k - 1] = (double)c;
    }
}

// y = H x for one trace of n samples, the definition as it is written above; y may not alias x
inline void hilbert_host(const double* taps, int64_t n, const double* x, double* y) {
    const int64_t K = hilbert_ntaps(n);
    for (int64_t i = 0; i < n; i++) {
        double s = 0.0;
        for (int64_t k = 1; k <= K; k++) {
            const double c = taps[k - 1];
            if (c == 0.0) continue;
            const double d = x[(i - k + n) % n] - x[(i + k) % n];
            const double p = c * d;
            s = s + p;
        }
        y[i] = s;
    }
}

}  // namespace rt
