// rt_filter.h -- the trace filter of rtmi_kirchhoff_filter (kirchhoff_filter.hip): the definition of
// y = F x and y = F^T x as a plain host loop, and the library's half-derivative taps.  Plain C++ with no HIP in it: the library
// takes its taps from half_derivative_taps (rtmi_half_derivative_taps hands them out), and a host program includes this header
// (tests/native/filter_taps.cpp).  Build with -ffp-contract=off, as the library is.
//   F is a linear (not circular) convolution along an axis of nt samples with the taps f[0 .. L) and an origin o, 0 <= o < L: tap
//   o is lag zero (a zero-phase wavelet of 2 M + 1 taps has o = M, a causal filter o = 0).
//     F  :  y[i] = sum over k = 0 .. L - 1 ascending with 0 <= i - k + o < nt of fl(f[k] x[i - k + o])
//     F^T:  y[i] = sum over k = 0 .. L - 1 ascending with 0 <= i + k - o < nt of fl(f[k] x[i + k - o])
//   from +0.0, every product and add a separate fp64 operation.  Terms outside the trace do not exist: F is the nt x nt Toeplitz
//   matrix F[i][j] = f[i - j + o], and F^T is its transpose entry for entry -- the same products, each sum over k ascending.
//   A sum that starts at +0.0 never becomes -0.0 (round to nearest), and adding +-0.0 to it changes no bit: with finite taps a
//   trace padded with zeros gives the same bits as the range test, which is how the kernel evaluates it.
// The half-derivative: g_0 = 1, g_k = g_(k-1) (2 k - 3) / (2 k), the coefficients of (1 - z)^(1/2) (the Gruenwald-Letnikov
// half-differentiator), times 1 / sqrt(dt); causal, o = 0.  Its response is (1 - exp(-i w dt))^(1/2) / sqrt(dt), which tends to
// sqrt(i w) for w dt << 1.  The full series sums to zero and every g_k with k >= 1 is negative, so L taps drop a tail whose
// absolute sum is exactly sum over k < L of g_k / sqrt(dt): that is the truncated filter's response at DC (its DC leak), and it
// bounds the distance of its response from the full series' at every frequency.  It falls as 1 / sqrt(pi L dt).
#pragma once
#include <cmath>
#include <cstdint>

namespace rt {

constexpr int64_t kFilterMaxTaps = 2048;
constexpr int64_t kFilterMaxNt = 16384;

// taps[k] = g_k / sqrt(dt) for k = 0 .. L - 1: long double, rounded once to fp64
inline void half_derivative_taps(int64_t L, double dt, double* taps) {
    const long double s = 1.0L / sqrtl((long double)dt);
    long double g = 1.0L;
    for (int64_t k = 0; k < L; k++) {
        if (k > 0) g = g * (long double)(2 * k - 3) / (long double)(2 * k);
        taps[k] = (double)(g * s);
    }
}

// y = F x (transpose: F^T x) for one trace of nt samples, the definition as it is written above; y may not alias x
inline void filter_host(const double* f, int64_t L, int64_t o, bool transpose, int64_t nt, const double* x, double* y) {
    for (int64_t i = 0; i < nt; i++) {
        double s = 0.0;
        for (int64_t k = 0; k < L; k++) {
            const int64_t j = transpose ? i + k - o : i - k + o;
            if (j < 0 || j >= nt) continue;
            const double p = f[k] * x[j];
            s = s + p;
        }
        y[i] = s;
    }
}

}  // namespace rt
