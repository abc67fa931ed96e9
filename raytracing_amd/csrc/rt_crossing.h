// rt_crossing.h -- the crossing rule of a recorded step with a receiver line, shared by rtmi_crossings
// (twopoint.hip) and rtmi_paraxial (paraxial.hip), so that both find the same tau* on the same rows.
//
// Compiled with -ffp-contract=off, sin/cos glibc's own through rt_libm.h: tests/crossing_ref.py, a numpy restatement, gives the
// same bits.  Each translation unit that includes this gets its own copy of the sin/cos table (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "rt_libm.h"

namespace {

__device__ const double kTab[4 * RT_SINCOS_TAB_ENTRIES] = {RT_SINCOS_TAB_VALUES};
__device__ __forceinline__ double sin_g(double x) { return rt::gl::in_range(x) ? rt::gl::sin(kTab, x) : sin(x); }
__device__ __forceinline__ double cos_g(double x) { return rt::gl::in_range(x) ? rt::gl::cos(kTab, x) : cos(x); }

// The normalised line a' x + b' y = c' (host, fp64).  tests/crossing_ref.py normalises the same way.
struct Line { double a, b, c; };
static bool make_line(const double* l, Line* out) {
    const double nrm = std::sqrt(l[0] * l[0] + l[1] * l[1]);
    if (!(nrm > 0) || !std::isfinite(nrm) || !std::isfinite(l[2])) return false;
    *out = Line{l[0] / nrm, l[1] / nrm, l[2] / nrm};
    return true;
}

// The cubic Hermite basis at tau, and its derivative
struct Basis { double h00, h10, h01, h11; };
__device__ __forceinline__ Basis basis(double t) {
    const double t2 = t * t, t3 = t2 * t;
    return Basis{(2.0 * t3 - 3.0 * t2) + 1.0, (t3 - 2.0 * t2) + t, 3.0 * t2 - 2.0 * t3, t3 - t2};
}
__device__ __forceinline__ Basis dbasis(double t) {
    const double t2 = t * t;
    return Basis{6.0 * t2 - 6.0 * t, (3.0 * t2 - 4.0 * t) + 1.0, 6.0 * t - 6.0 * t2, 3.0 * t2 - 2.0 * t};
}
__device__ __forceinline__ double herm(const Basis& h, double p0, double m0, double p1, double m1) {
    return ((p0 * h.h00 + m0 * h.h10) + p1 * h.h01) + m1 * h.h11;
}

// Does the step from signed distance f0 to f1 cross the line?
__device__ __forceinline__ bool crosses(double f0, double f1) { return (f0 < 0.0 && f1 >= 0.0) || (f0 > 0.0 && f1 <= 0.0); }

// tau* of a crossing step: bracketed Newton on g(tau) = a' H_x + b' H_y - c' = herm(f0, d0, f1, d1), from the
// linear-interpolation tau (d0, d1: the end tangents' components along the normal, chord length included)
__device__ __forceinline__ double cross_tau(double f0, double d0, double f1, double d1) {
    double tau = f1 == 0.0 ? 1.0 : f0 / (f0 - f1);
    double lo = 0.0, hi = 1.0;
    for (int it = 0; it < 64 && f1 != 0.0; it++) {
        const double g = herm(basis(tau), f0, d0, f1, d1);
        if (g == 0.0) break;
        if ((g < 0.0) == (f0 < 0.0)) lo = tau; else hi = tau;
        if (hi - lo < 0x1p-52) break;
        const double gd = herm(dbasis(tau), f0, d0, f1, d1);
        const double tn = tau - g / gd;
        tau = (tn > lo && tn < hi) ? tn : 0.5 * (lo + hi);
    }
    return tau;
}

}  // namespace
