// rt_eikonal_attr.h -- the arithmetic that carries launch angle, direction and spreading to the nodes the eikonal fill gave a
// value (eikonal_attr.hip, rtmi_eikonal_attributes), with no HIP in it, so that a host program can include
// it (tests/native/eikonal_attr.cpp): wrap, the gather of the launch angle, the direction from the upwind gradient, the spreading
// from the central difference of the launch angle, and the solve of one source as the serial loops that define it.
// tests/eikonal_attr_ref.py restates all of it in plain Python floats.
//
// Everything is fp64 and every product, sum, quotient and sqrt below is one rounded operation: build with -ffp-contract=off, as
// the library is.  All of it is a function of (grid, ball, n, src, n_src, T, filled), T and filled being what rtmi_eikonal_fill
// returned, and of the input theta0.  Classes, parents, ca and cb are eik_lin_node's (rt_eikonal_lin.h), unchanged.  Only nodes
// of class ball or free are written; dead nodes and seeds keep the bits of every array.
//
// wrap(d), pi and 2 pi the nearest doubles:  d > pi: d - 2 pi;  d <= -pi: d + 2 pi;  else d (a NaN passes through).
// theta0    ball: atan2(dy, dx), dx = X - xs, dy = Y - ys as eik_lin_csrc forms them, by the host's libm (the device reads a table)
//           free: it starts from NaN.  A parent is usable iff its current value is finite.  With a the x-parent, b the y-parent:
//                 both usable: w = cb / (ca + cb);  theta = ta + w wrap(tb - ta), a NaN result being the canonical NaN
//                 one usable: that parent's value;  none: the canonical NaN
//           The result is not wrapped again.  Parents are strictly earlier in T, so the fixed point is unique and its bits depend on
//           no schedule; so that rounds is defined the sweeps are the tangent's (rt_eikonal_lin.h), over the free nodes, a node
//           changing when its bits change; no round runs where no node is free.
// dir       ball: r = sqrt(dx dx + dy dy);  r > 0: (dx / r, dy / r), else (0, 0)
//           free: t the node's T, a, b its parents';  gx = +-(t - a) / gdx where the code names an x-parent (+ west, - east), else
//                 0;  gy likewise (+ south);  m = sqrt(gx gx + gy gy);  m > 0: (gx / m, gy / m), else NaN in both planes
// J, G      after the source's theta0 is final.  ball: J = r.  free: theta0 not finite: NaN.  Else per axis, a neighbour being
//           usable iff it is inside the grid, not dead and its theta0 is finite (seeds count):
//                 both: wrap(tE - tW) / (2 gdx);  east only: wrap(tE - t) / gdx;  west only: wrap(t - tW) / gdx;  neither: 0
//           m = sqrt(ddx ddx + ddy ddy);  J = 1 / m (m == 0: +inf).  G = 1 / sqrt(n J), ttgrid.hip's order: J = +inf gives 0.
#pragma once
#include "rt_eikonal_lin.h"

namespace rt {

constexpr double kEikPi = 0x1.921fb54442d18p+1, kEikTwoPi = 0x1.921fb54442d18p+2;

RT_EIK_HD double eik_attr_wrap(double d) {
    if (d > kEikPi) return d - kEikTwoPi;
    if (d <= -kEikPi) return d + kEikTwoPi;
    return d;
}

// the weight a free node keeps: cb / (ca + cb) where it has both parents, else +0.0 (not read)
RT_EIK_HD double eik_attr_weight(const EikLinNode& c) {
    const uint8_t both = kLinXParent | kLinYParent;
    return (c.code & both) == both ? c.cb / (c.ca + c.cb) : 0.0;
}

// the launch angle from the parents' values ta (x) and tb (y); has_a, has_b: the code names that parent
RT_EIK_HD double eik_attr_combine(bool has_a, double ta, bool has_b, double tb, double w) {
    const bool ua = has_a && eik_finite(ta), ub = has_b && eik_finite(tb);
    if (ua && ub) {
        const double r = ta + w * eik_attr_wrap(tb - ta);
        return r == r ? r : eik_nan();
    }
    if (ua) return ta;
    if (ub) return tb;
    return eik_nan();
}

// The gather of the launch angle at free node x: v [ny][nx] the current values
RT_EIK_HD double eik_attr_gather(long nx, long x, uint8_t code, double w, const double* v) {
    const bool ha = code & kLinXParent, hb = code & kLinYParent;
    const double ta = ha ? v[code & kLinXEast ? x + 1 : x - 1] : 0.0;
    const double tb = hb ? v[code & kLinYNorth ? x + nx : x - nx] : 0.0;
    return eik_attr_combine(ha, ta, hb, tb, w);
}

// dx, dy and r of node (i, j) from the source, as eik_lin_csrc forms them
RT_EIK_HD double eik_attr_radius(const EikGrid& g, long i, long j, double xs, double ys, double* dx, double* dy) {
    const double X = g.gx0 + (double)i * g.gdx, Y = g.gy0 + (double)j * g.gdy;
    *dx = X - xs;
    *dy = Y - ys;
    return std::sqrt(*dx * *dx + *dy * *dy);
}

// the direction of a node of the ball
RT_EIK_HD void eik_attr_ball_dir(double dx, double dy, double r, double* px, double* py) {
    *px = r > 0.0 ? dx / r : 0.0;
    *py = r > 0.0 ? dy / r : 0.0;
}

// The direction of a free node with value t whose code names the parents with values a (x) and b (y)
RT_EIK_HD void eik_attr_free_dir(const EikGrid& g, uint8_t code, double t, double a, double b, double* px, double* py) {
    double gx = 0.0, gy = 0.0;
    if (code & kLinXParent) {
        const double d = t - a;
        gx = (code & kLinXEast ? -d : d) / g.gdx;
    }
    if (code & kLinYParent) {
        const double d = t - b;
        gy = (code & kLinYNorth ? -d : d) / g.gdy;
    }
    const double m = std::sqrt(gx * gx + gy * gy);
    *px = m > 0.0 ? gx / m : eik_nan();
    *py = m > 0.0 ? gy / m : eik_nan();
}

// The difference of the launch angle along one axis of spacing h: lo and hi the neighbours' values, read where usable
RT_EIK_HD double eik_attr_diff(bool use_lo, double lo, double t, bool use_hi, double hi, double h) {
    if (use_lo && use_hi) return eik_attr_wrap(hi - lo) / (2.0 * h);
    if (use_hi) return eik_attr_wrap(hi - t) / h;
    if (use_lo) return eik_attr_wrap(t - lo) / h;
    return 0.0;
}

RT_EIK_HD double eik_attr_spread(double ddx, double ddy) {
    const double m = std::sqrt(ddx * ddx + ddy * ddy);
    return 1.0 / m;
}

RT_EIK_HD double eik_attr_amp(double s, double J) { return 1.0 / std::sqrt(s * J); }

// dir, J and G of node (i, j) of one source, which is of the ball or free (cls); th [ny][nx] the final launch angles.  Any of
// px, py (together), J, G may be NULL
RT_EIK_HD void eik_attr_node(const EikGrid& g, long nx, long ny, long i, long j, const double* n, const double* T, const EikLinNode& c,
                             double xs, double ys, const double* th, double* px, double* py, double* J, double* G) {
    const long x = j * nx + i;
    const double s = n[x];
    double dpx, dpy, Jv;
    if (eik_lin_class(c.code) == kLinBall) {
        double dx, dy;
        const double r = eik_attr_radius(g, i, j, xs, ys, &dx, &dy);
        eik_attr_ball_dir(dx, dy, r, &dpx, &dpy);
        Jv = r;
    } else {
        const double a = c.code & kLinXParent ? T[c.code & kLinXEast ? x + 1 : x - 1] : 0.0;
        const double b = c.code & kLinYParent ? T[c.code & kLinYNorth ? x + nx : x - nx] : 0.0;
        eik_attr_free_dir(g, c.code, T[x], a, b, &dpx, &dpy);
        const double t = th[x];
        Jv = eik_nan();
        if ((J || G) && eik_finite(t)) {
            const bool uw = i > 0 && eik_lin_read(n[x - 1], T[x - 1]) != eik_inf() && eik_finite(th[x - 1]);
            const bool ue = i + 1 < nx && eik_lin_read(n[x + 1], T[x + 1]) != eik_inf() && eik_finite(th[x + 1]);
            const bool us = j > 0 && eik_lin_read(n[x - nx], T[x - nx]) != eik_inf() && eik_finite(th[x - nx]);
            const bool un = j + 1 < ny && eik_lin_read(n[x + nx], T[x + nx]) != eik_inf() && eik_finite(th[x + nx]);
            const double ddx = eik_attr_diff(uw, uw ? th[x - 1] : 0.0, t, ue, ue ? th[x + 1] : 0.0, g.gdx);
            const double ddy = eik_attr_diff(us, us ? th[x - nx] : 0.0, t, un, un ? th[x + nx] : 0.0, g.gdy);
            Jv = eik_attr_spread(ddx, ddy);
        }
    }
    if (px) {
        px[x] = dpx;
        py[x] = dpy;
    }
    if (J) J[x] = Jv;
    if (G) G[x] = Jv == Jv ? eik_attr_amp(s, Jv) : eik_nan();
}

#if !(defined(__HIPCC__) || defined(__HIP__))
// The solve of one source as the serial loops that define it, host only.  theta0 [ny][nx] in place; px, py, J, G [ny][nx] in place
// or NULL; work space: w [ny][nx] doubles and code [ny][nx] bytes.
inline EikLinResult eik_attr_solve(const EikGrid& g, long nx, long ny, const double* n, const double* T, const uint8_t* filled,
                                   double xs, double ys, double n_src, double ball, int max_rounds, double* theta0, double* px,
                                   double* py, double* J, double* G, double* w, uint8_t* code) {
    EikLinResult res{0, 1, 0, 0};
    long nfree = 0;
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const long x = j * nx + i;
            const EikLinNode c = eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
            const uint8_t cls = eik_lin_class(c.code);
            code[x] = c.code;
            w[x] = eik_attr_weight(c);
            if (cls == kLinBall) {
                double dx, dy;
                eik_attr_radius(g, i, j, xs, ys, &dx, &dy);
                theta0[x] = std::atan2(dy, dx);
            } else if (cls == kLinFree) {
                theta0[x] = eik_nan();
                nfree++;
            }
            if (cls >= kLinFree) res.nodes++;
        }
    const int cap = max_rounds > 0 ? max_rounds : kEikDefaultRounds;
    if (nfree > 0) {
        while (res.rounds < cap) {
            res.rounds++;
            int64_t changed = 0;
            for (int s = 0; s < 4; s++) {
                const bool xup = eik_lin_xup(false, s), yup = eik_lin_yup(false, s);
                for (long q = 0; q < ny; q++)
                    for (long p = 0; p < nx; p++) {
                        const long j = yup ? q : ny - 1 - q, i = xup ? p : nx - 1 - p, x = j * nx + i;
                        if (eik_lin_class(code[x]) != kLinFree) continue;
                        const double v = eik_attr_gather(nx, x, code[x], w[x], theta0);
                        if (eik_bits(v) != eik_bits(theta0[x])) {
                            theta0[x] = v;
                            changed++;
                        }
                    }
            }
            res.changes += changed;
            res.clean = changed == 0;
            if (res.clean) break;
        }
    }
    if (px || J || G)
        for (long j = 0; j < ny; j++)
            for (long i = 0; i < nx; i++) {
                if (eik_lin_class(code[j * nx + i]) < kLinFree) continue;
                const EikLinNode c = eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
                eik_attr_node(g, nx, ny, i, j, n, T, c, xs, ys, theta0, px, py, J, G);
            }
    return res;
}
#endif

}  // namespace rt
