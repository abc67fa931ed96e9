// rt_pchip.h -- scipy.interpolate.PchipInterpolator (scipy 1.15.3) restated in fp64, in one fixed expression order:
// _find_derivatives (Fritsch-Butland weighted harmonic mean, the three-point end rule with its two guards),
// CubicHermiteSpline's power-basis coefficients of one interval, PPoly's interval search and evaluation.  A data set is read
// through two callables t(i), v(i), so that a strided record column and a plain array both fit.
//
// Host and device (tests/native/pchip_check.cpp compiles it with g++).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RT_PCHIP_HD __host__ __device__ __forceinline__
#else
#define RT_PCHIP_HD inline
#endif

namespace rt {
RT_PCHIP_HD double pchip_sgn(double v) { return (v > 0) - (v < 0); }
// the three-point end rule: h0, m0 the end interval's length and slope, h1, m1 its neighbour's
RT_PCHIP_HD double pchip_edge(double h0, double h1, double m0, double m1) {
    double d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
    if (pchip_sgn(d) != pchip_sgn(m0)) d = 0;
    else if (pchip_sgn(m0) != pchip_sgn(m1) && fabs(d) > 3 * fabs(m0)) d = 3 * m0;
    return d;
}
// the derivative estimate at point j of the n-point data set (t, v), n >= 2 (n == 2: the straight line)
template <typename TT, typename VV> RT_PCHIP_HD double pchip_deriv(const TT& t, const VV& v, long j, long n) {
    if (n == 2) return (v(1) - v(0)) / (t(1) - t(0));
    if (j == 0) {
        const double h0 = t(1) - t(0), h1 = t(2) - t(1);
        return pchip_edge(h0, h1, (v(1) - v(0)) / h0, (v(2) - v(1)) / h1);
    }
    if (j == n - 1) {
        const double h0 = t(n - 1) - t(n - 2), h1 = t(n - 2) - t(n - 3);
        return pchip_edge(h0, h1, (v(n - 1) - v(n - 2)) / h0, (v(n - 2) - v(n - 3)) / h1);
    }
    const double ha = t(j) - t(j - 1), hb = t(j + 1) - t(j);
    const double ma = (v(j) - v(j - 1)) / ha, mb = (v(j + 1) - v(j)) / hb;
    if (pchip_sgn(ma) != pchip_sgn(mb) || ma == 0 || mb == 0) return 0;
    const double w1 = 2 * hb + ha, w2 = hb + 2 * ha;
    return 1.0 / ((w1 / ma + w2 / mb) / (w1 + w2));
}

// the interval lo of q in [t(0), t(n-1)]: t(lo) <= q < t(lo + 1), the last one closed on the right
template <typename TT> RT_PCHIP_HD long pchip_interval(const TT& t, long n, double q) {
    long lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (t(mid) <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// CubicHermiteSpline's c[0..3] of one interval, in powers of s = the distance from its left end; pchip_cubic makes them from dx:
// the interval's length, v0: the value at its left end, slope: its secant's, d0 and d1: the derivatives at its ends
struct PchipCubic {
    double c0, c1, c2, c3;
    RT_PCHIP_HD double powers(double s) const { return c3 + c2 * s + c1 * (s * s) + c0 * (s * s * s); }   // as PPoly sums them
    RT_PCHIP_HD double horner(double s) const { return ((c0 * s + c1) * s + c2) * s + c3; }
    RT_PCHIP_HD double deriv(double s) const { return (3 * c0 * s + 2 * c1) * s + c2; }                   // PPoly.derivative()
};
RT_PCHIP_HD PchipCubic pchip_cubic(double dx, double v0, double slope, double d0, double d1) {
    const double tq = (d0 + d1 - 2 * slope) / dx;
    return PchipCubic{tq / dx, (slope - d0) / dx - tq, d0, v0};
}

}  // namespace rt
