// rt_eikonal.h -- the arithmetic of the eikonal continuation of a traveltime table (eikonal.hip, rtmi_eikonal_fill; DESIGN.md
// section 34), with no HIP in it, so that a host program can include it (tests/native/eikonal_update.cpp): the state of a node,
// the value of a node of the source ball, the update of a free node, and the whole solve of one source as the serial loop that
// defines it.  tests/eikonal_ref.py restates all of it in plain Python floats.
//
// Everything is fp64 and every product, sum, quotient and sqrt below is one rounded operation: build with -ffp-contract=off, as
// the library is.  min(x, y) is y < x ? y : x.
//
// Node (i, j) is X = gx0 + i gdx, Y = gy0 + j gdy.  With s = n[j][i]:
//     obstacle   s is not finite or s <= 0: never updated, +inf as a neighbour, its output is its input
//     seeded     not an obstacle and the input T is finite: frozen
//     free       every other node; it starts from +inf
//     ball       a free node with u = (X - xs) / gdx, v = (Y - ys) / gdy, u u + v v <= ball ball, for a source whose n_src is
//                finite and > 0 and a ball >= 0: dx = X - xs, dy = Y - ys, T = (0.5 (n_src + s)) sqrt(dx dx + dy dy), frozen
// The update of a free node, a neighbour outside the grid reading as +inf:
//     a = min(T[j][i-1], T[j][i+1]);  b = min(T[j-1][i], T[j+1][i]);  both +inf: no change
//     ta = a + gdx s;  tb = b + gdy s
//     b == +inf or ta <= b:       t = ta
//     else a == +inf or tb <= a:  t = tb
//     else wx = 1 / (gdx gdx); wy = 1 / (gdy gdy); A = wx + wy; B = a wx + b wy; e = a - b;
//          d = A (s s) - (wx wy) (e e);  t = d < 0 ? min(ta, tb) : (B + sqrt(d)) / A
//     T[j][i] = t iff t < T[j][i], which counts as one change
// A round is four Gauss-Seidel sweeps over the grid in the orders (+x, +y), (-x, +y), (-x, -y), (+x, -y), y the outer loop, each
// update reading its neighbours' current values.  No round runs where no node is free or no node is seeded or of the ball
// (rounds 0, clean); else rounds repeat until one changes nothing (clean) or max_rounds have run.  Free nodes still at +inf are
// unreached.
//
// The source-factored scheme (rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED; DESIGN.md section 39;
// tests/eikonal_factored_ref.py restates it) is additive factoring: T = T0 + u with T0 = n_src r.  Differencing u upwind is the
// update above on shifted neighbour readings -- the parent's value plus the truncation error of differencing T0 across that edge
// -- so the working table stays T, eik_update is untouched and its one-sided branch is T_x = +-s.  For node (i, j) of a source,
// in eik_init's expressions:
//     X = gx0 + (double)i gdx;  dx = X - xs;  Y = gy0 + (double)j gdy;  dy = Y - ys;  rr = sqrt(dx dx + dy dy);  T0 = n_src rr
// States, the ball, the sweep orders, the round rule, filled and unreached -> NaN are unchanged.  Factoring is left out for a
// source whose n_src is not finite or <= 0 and at a node with rr == 0: the plain update.  Otherwise the update of free node x
// reads l = T[j][i-1], r = T[j][i+1], dn = T[j-1][i], up = T[j+1][i] as above and then
//     x-parent east iff r < l;  a_raw = that reading
//       a = a_raw == +inf ? +inf : (a_raw + (T0[x] - T0[parent])) +- px;  px = gdx (n_src (dx / rr));  + for east, - for west
//     y-parent north iff up < dn;  b_raw = that reading
//       b = b_raw == +inf ? +inf : (b_raw + (T0[x] - T0[parent])) +- py;  py = gdy (n_src (dy / rr));  + for north, - for south
//     t = eik_update(a, b, s);  T[j][i] = t iff t < T[j][i]
// The side is chosen on the raw readings.  T0 is a function of the node alone, so evaluating it afresh (as here: three sqrt and
// two quotients per update) and reading it from a table give the same bits.  The corrected scheme is not strictly causal in T:
// the rounds converge geometrically, some ten of them in a smooth medium where the plain scheme needs two.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_EIK_HD __host__ __device__ __forceinline__
#else
#define RT_EIK_HD inline
#endif

namespace rt {

constexpr int kEikDefaultRounds = 64;       // max_rounds 0
enum : uint8_t { kEikFrozen = 0, kEikFree = 1, kEikBall = 2 };      // obstacles and seeded nodes; free nodes; nodes of the ball

// the spacings and what the update derives from them, once per call
struct EikGrid {
    double gx0, gdx, gy0, gdy;
    double wx, wy, A, wxy;
};

RT_EIK_HD double eik_inf() { return __builtin_inf(); }
RT_EIK_HD double eik_nan() { return __builtin_nan(""); }
RT_EIK_HD bool eik_finite(double x) { return __builtin_fabs(x) < eik_inf(); }
RT_EIK_HD double eik_min(double x, double y) { return y < x ? y : x; }
RT_EIK_HD bool eik_obstacle(double s) { return !(eik_finite(s) && s > 0.0); }

RT_EIK_HD EikGrid eik_grid(double gx0, double gdx, double gy0, double gdy) {
    EikGrid g{gx0, gdx, gy0, gdy, 0.0, 0.0, 0.0, 0.0};
    g.wx = 1.0 / (gdx * gdx);
    g.wy = 1.0 / (gdy * gdy);
    g.A = g.wx + g.wy;
    g.wxy = g.wx * g.wy;
    return g;
}

// The state of node (i, j) with slowness s and input tin, and the value it starts from (*w)
RT_EIK_HD uint8_t eik_init(const EikGrid& g, long i, long j, double s, double tin, double xs, double ys, double n_src, double ball,
                           double* w) {
    *w = eik_inf();
    if (eik_obstacle(s)) return kEikFrozen;
    if (eik_finite(tin)) {
        *w = tin;
        return kEikFrozen;
    }
    if (!(ball >= 0.0) || eik_obstacle(n_src)) return kEikFree;
    const double X = g.gx0 + (double)i * g.gdx, Y = g.gy0 + (double)j * g.gdy;
    const double dx = X - xs, dy = Y - ys;
    const double u = dx / g.gdx, v = dy / g.gdy;
    if (!(u * u + v * v <= ball * ball)) return kEikFree;
    *w = (0.5 * (n_src + s)) * std::sqrt(dx * dx + dy * dy);
    return kEikBall;
}

// The candidate value of a free node from a = min of its x neighbours and b = min of its y neighbours; +inf: no change
RT_EIK_HD double eik_update(const EikGrid& g, double a, double b, double s) {
    const double inf = eik_inf();
    if (a == inf && b == inf) return inf;
    const double ta = a + g.gdx * s, tb = b + g.gdy * s;
    if (b == inf || ta <= b) return ta;
    if (a == inf || tb <= a) return tb;
    const double B = a * g.wx + b * g.wy, e = a - b;
    const double d = g.A * (s * s) - g.wxy * (e * e);
    return d < 0.0 ? eik_min(ta, tb) : (B + std::sqrt(d)) / g.A;
}

enum : int32_t { kEikPlain = 0, kEikFactored = 1 };      // rtmi_eikonal_params.scheme

// The distance rr of node (i, j) from the source, in eik_init's expressions, with its dx and dy
RT_EIK_HD double eik_rr(const EikGrid& g, long i, long j, double xs, double ys, double* dx, double* dy) {
    const double X = g.gx0 + (double)i * g.gdx, Y = g.gy0 + (double)j * g.gdy;
    *dx = X - xs;
    *dy = Y - ys;
    return std::sqrt(*dx * *dx + *dy * *dy);
}

// The candidate value of free node (i, j) in the factored scheme from its four neighbour readings (+inf outside the grid): the
// parents are chosen on the raw readings, each is corrected by what differencing T0 = n_src rr across its edge gets wrong, and
// eik_update does the rest.  The plain update where n_src is an obstacle's or rr == 0.
RT_EIK_HD double eik_update_factored(const EikGrid& g, long i, long j, double xs, double ys, double n_src, double l, double r, double dn,
                                     double up, double s) {
    const double inf = eik_inf();
    const bool east = r < l, north = up < dn;
    double a = east ? r : l, b = north ? up : dn;
    if (a == inf && b == inf) return inf;
    double dx, dy, pdx, pdy;                  // the node's; the parent's, not used
    const double rr = eik_rr(g, i, j, xs, ys, &dx, &dy);
    if (!eik_obstacle(n_src) && rr != 0.0) {
        const double T0 = n_src * rr;
        if (a != inf) {
            const double T0p = n_src * eik_rr(g, east ? i + 1 : i - 1, j, xs, ys, &pdx, &pdy);
            const double px = g.gdx * (n_src * (dx / rr));
            a = a + (T0 - T0p);
            a = east ? a + px : a - px;
        }
        if (b != inf) {
            const double T0p = n_src * eik_rr(g, i, north ? j + 1 : j - 1, xs, ys, &pdx, &pdy);
            const double py = g.gdy * (n_src * (dy / rr));
            b = b + (T0 - T0p);
            b = north ? b + py : b - py;
        }
    }
    return eik_update(g, a, b, s);
}

// What eik_update_factored hands to eik_update at free node (i, j), in the same expressions, with the sides the raw readings chose
// (*east, *north): what the linearisation of that update starts from (rt_eikonal_lin.h).  The raw readings where both are +inf,
// where n_src is an obstacle's or where rr == 0.
RT_EIK_HD void eik_factored_readings(const EikGrid& g, long i, long j, double xs, double ys, double n_src, double l, double r, double dn,
                                     double up, double* pa, double* pb, bool* east, bool* north) {
    const double inf = eik_inf();
    *east = r < l;
    *north = up < dn;
    double a = *east ? r : l, b = *north ? up : dn;
    *pa = a;
    *pb = b;
    if (a == inf && b == inf) return;
    double dx, dy, pdx, pdy;                  // the node's; the parent's, not used
    const double rr = eik_rr(g, i, j, xs, ys, &dx, &dy);
    if (!eik_obstacle(n_src) && rr != 0.0) {
        const double T0 = n_src * rr;
        if (a != inf) {
            const double T0p = n_src * eik_rr(g, *east ? i + 1 : i - 1, j, xs, ys, &pdx, &pdy);
            const double px = g.gdx * (n_src * (dx / rr));
            a = a + (T0 - T0p);
            a = *east ? a + px : a - px;
        }
        if (b != inf) {
            const double T0p = n_src * eik_rr(g, i, *north ? j + 1 : j - 1, xs, ys, &pdx, &pdy);
            const double py = g.gdy * (n_src * (dy / rr));
            b = b + (T0 - T0p);
            b = *north ? b + py : b - py;
        }
    }
    *pa = a;
    *pb = b;
}

// what one source's solve reports
struct EikResult {
    int32_t rounds, clean;
    int64_t free_nodes, filled, changes;
};

#if !(defined(__HIPCC__) || defined(__HIP__))
// The solve of one source as the serial loop that defines it, host only.  n [ny][nx]; T [ny][nx] in place (or NULL: all NaN, no
// table returned); w [ny][nx] doubles and st [ny][nx] bytes of work space; filled [ny][nx] or NULL; scheme kEikPlain or
// kEikFactored.
inline EikResult eik_solve(const EikGrid& g, long nx, long ny, const double* n, double xs, double ys, double n_src, double ball,
                           int max_rounds, double* T, double* w, uint8_t* st, uint8_t* filled, int32_t scheme = kEikPlain) {
    EikResult r{0, 1, 0, 0, 0};
    const double inf = eik_inf();
    long seeds = 0, free_now = 0;
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const long x = j * nx + i;
            st[x] = eik_init(g, i, j, n[x], T ? T[x] : eik_nan(), xs, ys, n_src, ball, &w[x]);
            if (st[x] != kEikFrozen) r.free_nodes++;
            if (st[x] == kEikFree) free_now++;
            else if (w[x] < inf) seeds++;
        }
    const int cap = max_rounds > 0 ? max_rounds : kEikDefaultRounds;
    if (free_now > 0 && seeds > 0) {
        while (r.rounds < cap) {
            r.rounds++;
            int64_t changed = 0;
            for (int k = 0; k < 4; k++) {
                const bool xup = k == 0 || k == 3, yup = k < 2;
                for (long q = 0; q < ny; q++) {
                    const long j = yup ? q : ny - 1 - q;
                    for (long p = 0; p < nx; p++) {
                        const long i = xup ? p : nx - 1 - p, x = j * nx + i;
                        if (st[x] != kEikFree) continue;
                        const double l = i > 0 ? w[x - 1] : inf, rr = i + 1 < nx ? w[x + 1] : inf;
                        const double dn = j > 0 ? w[x - nx] : inf, up = j + 1 < ny ? w[x + nx] : inf;
                        const double t = scheme == kEikFactored ? eik_update_factored(g, i, j, xs, ys, n_src, l, rr, dn, up, n[x])
                                                                : eik_update(g, eik_min(l, rr), eik_min(dn, up), n[x]);
                        if (t < w[x]) {
                            w[x] = t;
                            changed++;
                        }
                    }
                }
            }
            r.changes += changed;
            r.clean = changed == 0;
            if (r.clean) break;
        }
    }
    for (long x = 0; x < nx * ny; x++) {
        const bool got = st[x] != kEikFrozen && w[x] < inf;
        if (st[x] != kEikFrozen && T) T[x] = got ? w[x] : eik_nan();
        if (filled) filled[x] = got ? 1 : 0;
        if (got) r.filled++;
    }
    return r;
}
#endif

}  // namespace rt
