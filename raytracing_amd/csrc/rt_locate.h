// rt_locate.h -- the arithmetic of event location by grid search over traveltime tables (locate.hip, rtmi_locate; DESIGN.md
// section 29), with no HIP in it, so that a host program can include it (tests/native/locate_refine.cpp): the two steps of a
// node's objective, which the kernels call once per (event, node, station), and the refinement of the best node on the 3 x 3
// window around it, which the C entry runs on the host.  tests/locate_ref.py restates both in numpy.
//
// Everything is fp64 and every product, sum and quotient below is one rounded operation: build with -ffp-contract=off, as the
// library is.
//
// One node x of one event, r ascending over the valid picks whose T[r][x] is finite, every accumulator from +0.0:
//     pass 1   d = tr - T[r][x]            tr = t[e][r] - ref, computed once per pick
//              n += 1;  sw = sw + w;  sd = sd + w * d       (no weights: sw = sw + 1.0, sd = sd + d)
//     tau = sd / sw
//     pass 2   d as above, the same two operands, hence the same bits
//              u = d - tau;  q = q + (w * u) * u            (no weights: q = q + u * u)
//     obj = q / sw
// Without weights sw is a sum of n ones, exact below 2^53: the kernels take (double)n for it.
//
// Refinement on f = win_obj [3][3], f[j][i] with j the row (y) and i the column (x), both -1, 0, 1 (stored at [j + 1][i + 1]).
// Each sum runs over its index ascending, -1, 0, 1, left to right, and is divided once at the end:
//     gx  = (((f[-1][1] - f[-1][-1]) + (f[0][1] - f[0][-1])) + (f[1][1] - f[1][-1])) / 6          gy: rows and columns swapped
//     hxx = ((c[-1] + c[0]) + c[1]) / 3,   c[j] = (f[j][1] - 2 f[j][0]) + f[j][-1]                hyy: rows and columns swapped
//     hxy = (((f[1][1] - f[1][-1]) - f[-1][1]) + f[-1][-1]) / 4
//     det = hxx hyy - hxy hxy
//     dx  = -((hyy gx - hxy gy) / det),   dy = -((hxx gy - hxy gx) / det)
// accepted iff all nine f are finite, hxx > 0, det > 0, |dx| <= 1 and |dy| <= 1; then
//     x   = gx0 + (ix + dx) gdx,   y = gy0 + (iy + dy) gdy
//     t0  = ((ref + tau_c) + dx ((tau_E - tau_W) / 2)) + dy ((tau_N - tau_S) / 2)      E, W: i = 1, -1 of row 0; N, S: j = 1, -1
//     cov = (2 / sw) H^-1 in grid units, scaled to lengths:  cxx = ((2 / sw) (hyy / det)) (gdx gdx),
//           cxy = ((2 / sw) (-hxy / det)) (gdx gdy),  cyy = ((2 / sw) (hxx / det)) (gdy gdy)
// else dx = dy = 0, x, y and t0 are the node's own, the covariance is NaN and refined = 0.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_LOCATE_HD __host__ __device__ __forceinline__
#else
#define RT_LOCATE_HD inline
#endif

namespace rt {

// the running sums of one node of one event
struct LocateSums {
    int n;
    double sw, sd;
};

template <bool W> RT_LOCATE_HD void locate_pass1(LocateSums& a, double tr, double w, double T) {
    const double d = tr - T;
    a.n += 1;
    if (W) {
        a.sw = a.sw + w;
        a.sd = a.sd + w * d;
    } else {
        a.sd = a.sd + d;
    }
}

template <bool W> RT_LOCATE_HD void locate_pass2(double& q, double tau, double tr, double w, double T) {
    const double d = tr - T;
    const double u = d - tau;
    if (W) q = q + (w * u) * u;
    else q = q + u * u;
}

struct LocateGrid {
    double gx0, gdx, gy0, gdy;
};

struct LocateRefined {
    double x, y, t0, dx, dy, cov[3];        // cov: xx, xy, yy
    int refined;
};

// f, tau: the windows [3][3] around node (ix, iy), row-major; ref + tau[4] is the node's own origin time
inline LocateRefined locate_refine(const double* f, const double* tau, double ref, double sw, int ix, int iy, const LocateGrid& g) {
    const double nan = std::nan("");
    LocateRefined o{};
    o.dx = 0.0;
    o.dy = 0.0;
    o.x = g.gx0 + ((double)ix + 0.0) * g.gdx;
    o.y = g.gy0 + ((double)iy + 0.0) * g.gdy;
    o.t0 = ref + tau[4];
    o.cov[0] = o.cov[1] = o.cov[2] = nan;
    o.refined = 0;
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(f[k])) return o;
    auto F = [&](int j, int i) { return f[(j + 1) * 3 + (i + 1)]; };
    const double gx = (((F(-1, 1) - F(-1, -1)) + (F(0, 1) - F(0, -1))) + (F(1, 1) - F(1, -1))) / 6.0;
    const double gy = (((F(1, -1) - F(-1, -1)) + (F(1, 0) - F(-1, 0))) + (F(1, 1) - F(-1, 1))) / 6.0;
    auto cx = [&](int j) { return (F(j, 1) - 2.0 * F(j, 0)) + F(j, -1); };
    auto cy = [&](int i) { return (F(1, i) - 2.0 * F(0, i)) + F(-1, i); };
    const double hxx = ((cx(-1) + cx(0)) + cx(1)) / 3.0;
    const double hyy = ((cy(-1) + cy(0)) + cy(1)) / 3.0;
    const double hxy = (((F(1, 1) - F(1, -1)) - F(-1, 1)) + F(-1, -1)) / 4.0;
    const double det = hxx * hyy - hxy * hxy;
    if (!(hxx > 0.0 && det > 0.0)) return o;
    const double dx = -((hyy * gx - hxy * gy) / det);
    const double dy = -((hxx * gy - hxy * gx) / det);
    if (!(std::fabs(dx) <= 1.0 && std::fabs(dy) <= 1.0)) return o;
    o.dx = dx;
    o.dy = dy;
    o.x = g.gx0 + ((double)ix + dx) * g.gdx;
    o.y = g.gy0 + ((double)iy + dy) * g.gdy;
    o.t0 = ((ref + tau[4]) + dx * ((tau[5] - tau[3]) / 2.0)) + dy * ((tau[7] - tau[1]) / 2.0);
    const double s = 2.0 / sw;
    o.cov[0] = (s * (hyy / det)) * (g.gdx * g.gdx);
    o.cov[1] = (s * (-hxy / det)) * (g.gdx * g.gdy);
    o.cov[2] = (s * (hxx / det)) * (g.gdy * g.gdy);
    o.refined = 1;
    return o;
}

}  // namespace rt
