// Test helper (CPU, g++): raytracing_amd/csrc/rt_pchip.h compiled for the host, on one data set (t, v) [n] held in plain arrays.
// tests/test_pchip_host.py drives it.
#include "../../raytracing_amd/csrc/rt_pchip.h"

namespace {
struct At {
    const double* p;
    double operator()(long i) const { return p[i]; }
};
}  // namespace

// d[j] = the derivative estimate at every point
extern "C" void pchip_derivs(long n, const double* t, const double* v, double* d) {
    for (long j = 0; j < n; j++) d[j] = rt::pchip_deriv(At{t}, At{v}, j, n);
}

// The interpolant at q[0..m), each within [t[0], t[n-1]]: the interval search, the interval's coefficients from the derivative
// estimates at its two ends, then powers[i] (the sum of powers, as k_isochrone evaluates), horner[i] (as k_fine) and slope[i]
// (the first derivative, as k_nodes takes it at the last breakpoint)
extern "C" void pchip_eval(long n, const double* t, const double* v, long m, const double* q, double* powers, double* horner,
                           double* slope) {
    for (long i = 0; i < m; i++) {
        const long lo = rt::pchip_interval(At{t}, n, q[i]);
        const double dx = t[lo + 1] - t[lo], s = q[i] - t[lo], sec = (v[lo + 1] - v[lo]) / dx;
        const rt::PchipCubic c = rt::pchip_cubic(dx, v[lo], sec, rt::pchip_deriv(At{t}, At{v}, lo, n), rt::pchip_deriv(At{t}, At{v}, lo + 1, n));
        powers[i] = c.powers(s);
        horner[i] = c.horner(s);
        slope[i] = c.deriv(s);
    }
}
