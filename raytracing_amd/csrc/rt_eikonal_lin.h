// rt_eikonal_lin.h -- the arithmetic of the linearised eikonal fill (eikonal_lin.hip, rtmi_eikonal_tangent and
// rtmi_eikonal_adjoint), with no HIP in it, so that a host program can include it
// (tests/native/eikonal_lin.cpp): the class of a node, the coefficients of a free node, the gathers of the tangent and of the
// adjoint, and both solves of one source as the serial loops that define them.  tests/eikonal_lin_ref.py restates all of it in
// plain Python floats.
//
// Everything is fp64 and every product, sum, quotient and sqrt below is one rounded operation: build with -ffp-contract=off, as
// the library is.  min(x, y) is y < x ? y : x (rt_eikonal.h).  All of it is a function of (grid, ball, n, src, n_src, T, filled),
// T and filled being what rtmi_eikonal_fill returned.
//
// With s = n[j][i] and t = T[j][i], per source:
//     dead   s is an obstacle (not finite or <= 0), or t is not finite: obstacles and unreached nodes
//     seed   not dead and filled is 0
//     ball   not dead, filled is 1, and eik_init's ball rule holds (rt_eikonal.h, on an input of NaN)
//     free   not dead, filled is 1, not of the ball
// As a neighbour a node reads t unless it is dead, and +inf if it is dead or outside the grid.
// The coefficients of a free node from its neighbours' readings l (west), r (east), dn (south), up (north):
//     a = min(l, r), the x-parent being east iff r < l;  b = min(dn, up), the y-parent being north iff up < dn
//     both +inf: no parent, ca = cb = cs = 0.  Else ta = a + gdx s;  tb = b + gdy s, and
//     b == +inf or ta <= b:       one-sided x:  ca = 1, cb = 0, cs = gdx
//     else a == +inf or tb <= a:  one-sided y:  ca = 0, cb = 1, cs = gdy
//     else B = a wx + b wy; e = a - b; d = A (s s) - (wx wy) (e e); q = d > 0 ? sqrt(d) : 0
//          q > 0:  tt = (B + q) / A;  ca = (wx (tt - a)) / q;  cb = (wy (tt - b)) / q;  cs = s / q
//          else:   one-sided y if tb < ta, else one-sided x
//     A branch that uses an axis names that axis' parent, unless the parent's reading is not strictly less than t: then the
//     node has no parent on that axis and the coefficient is 0.  So every parent is strictly earlier and the network has no cycle.
// A node of the ball has no parent and cs = csrc = 0.5 sqrt(dx dx + dy dy), dx = X - xs, dy = Y - ys.  A seed has neither.
// Tangent (dn [ny][nx], dn_src, dT_seed [ny][nx] or absent: +0.0): dead 0; seed dT_seed; ball (0.0 + cs dn) + csrc dn_src;
//     free   acc = +0.0;  x-parent: acc = acc + ca dT[parent];  y-parent: acc = acc + cb dT[parent];  dT = acc + cs dn
// Adjoint (r [ny][nx]): dead 0; every other node
//     acc = r;  for y in W, E, S, N, where y is free and names this node as its parent on that axis: acc = acc + c lam[y],
//     c being y's ca (W, E) or cb (S, N);  lam = acc
//     g = cs lam at free nodes and nodes of the ball, else +0.0;  g_src = the sum from +0.0 of csrc lam over the ball in node order
// Both are the unique fixed point of their gather, which Gauss-Seidel sweeps find: free nodes start from +0.0 (tangent), nodes
// that are not dead from r (adjoint); a round is four sweeps, y the outer loop, in the orders (+x, +y), (-x, +y), (-x, -y),
// (+x, -y) for the tangent and (-x, -y), (+x, -y), (+x, +y), (-x, +y) for the adjoint; the tangent visits the free nodes, the
// adjoint every node that is not dead; a node changes when the bits of its value change.  No round runs where no node is free
// (rounds 0, clean); else rounds repeat until one changes nothing (clean) or max_rounds have run.  Not clean: the values are
// those of the last sweep, not the fixed point.
//
// The factored update linearised (rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED_LIN; DESIGN.md section 40;
// tests/eikonal_factored_lin_ref.py restates it): the linearisation that is consistent with a table of the factored scheme
// (rt_eikonal.h).  Classes, seeds, nodes of the ball and dead nodes are as above.  A free node x = (i, j) of a source whose n_src
// is no obstacle's, with rr[x] != 0 (eik_rr), chooses its parents on the raw readings, east iff r < l, north iff up < dn, and
//     a, b   eik_factored_readings' corrected readings;  ca, cb, cs, the branch and the strict-parent rule are eik_lin_coef's on a
//            and b, the rule testing the corrected reading (a < t, b < t)
//     ka = (rr[x] - rr[x-parent]) +- gdx (dx / rr[x]), + for east;  kb = (rr[x] - rr[y-parent]) +- gdy (dy / rr[x]), + for north
//     csrc = the sum from +0.0 of ca ka, where the node has an x-parent, and cb kb, where it has a y-parent
// Every other free node has the coefficients above and csrc = 0.
// Tangent: a free node's constant term is (cs dn) + (csrc dn_src); the gather is unchanged.
// Adjoint: the gather is unchanged; g_src = the sum from +0.0 over the rows in ascending j of each row's sum from +0.0, over i
//     ascending, of csrc lam at the row's free nodes and nodes of the ball.
// A corrected parent need not be earlier in T, so the network is not provably acyclic and one pass in the order of T is not its
// fixed point: the bits are those of the sweep orders above from the starting values above, capped by max_rounds, and not clean
// means the last sweep's values.  Some ten rounds in a smooth medium, as the factored fill.
#pragma once
#include "rt_eikonal.h"

namespace rt {

enum : uint8_t { kLinXParent = 1, kLinXEast = 2, kLinYParent = 4, kLinYNorth = 8 };     // the low bits of a node's code
enum : uint8_t { kLinDead = 0, kLinSeed = 1, kLinFree = 2, kLinBall = 3 };               // its class: code >> 4

struct EikLinNode {
    double ca, cb, cs, csrc;
    uint8_t code;
};

RT_EIK_HD uint8_t eik_lin_class(uint8_t code) { return (uint8_t)(code >> 4); }

RT_EIK_HD uint64_t eik_bits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

// what a node with slowness s and value t reads as when it is a neighbour
RT_EIK_HD double eik_lin_read(double s, double t) { return !eik_obstacle(s) && eik_finite(t) ? t : eik_inf(); }

// The coefficients and parents of a free node whose value is t and whose slowness is s; the class bits of code are not set
RT_EIK_HD EikLinNode eik_lin_coef(const EikGrid& g, double l, double r, double dn, double up, double s, double t) {
    EikLinNode c{0.0, 0.0, 0.0, 0.0, 0};
    const double inf = eik_inf();
    const double a = eik_min(l, r), b = eik_min(dn, up);
    if (a == inf && b == inf) return c;
    const double ta = a + g.gdx * s, tb = b + g.gdy * s;
    int branch;                                         // 0: one-sided x, 1: one-sided y, 2: two-sided
    if (b == inf || ta <= b) branch = 0;
    else if (a == inf || tb <= a) branch = 1;
    else {
        const double B = a * g.wx + b * g.wy, e = a - b;
        const double d = g.A * (s * s) - g.wxy * (e * e);
        const double q = d > 0.0 ? std::sqrt(d) : 0.0;
        if (q > 0.0) {
            const double tt = (B + q) / g.A;
            c.ca = (g.wx * (tt - a)) / q;
            c.cb = (g.wy * (tt - b)) / q;
            c.cs = s / q;
            branch = 2;
        } else {
            branch = tb < ta ? 1 : 0;
        }
    }
    if (branch == 0) {
        c.ca = 1.0;
        c.cs = g.gdx;
    } else if (branch == 1) {
        c.cb = 1.0;
        c.cs = g.gdy;
    }
    if (branch != 1) {
        if (a < t) c.code |= (uint8_t)(kLinXParent | (r < l ? kLinXEast : 0));
        else c.ca = 0.0;
    }
    if (branch != 0) {
        if (b < t) c.code |= (uint8_t)(kLinYParent | (up < dn ? kLinYNorth : 0));
        else c.cb = 0.0;
    }
    return c;
}

// cs and csrc of node (i, j) of the ball
RT_EIK_HD double eik_lin_csrc(const EikGrid& g, long i, long j, double xs, double ys) {
    const double X = g.gx0 + (double)i * g.gdx, Y = g.gy0 + (double)j * g.gdy;
    const double dx = X - xs, dy = Y - ys;
    return 0.5 * std::sqrt(dx * dx + dy * dy);
}

// Node (i, j) of one source: its class, parents and coefficients from n, T and filled [ny][nx]
RT_EIK_HD EikLinNode eik_lin_node(const EikGrid& g, long nx, long ny, long i, long j, const double* n, const double* T,
                                  const uint8_t* filled, double xs, double ys, double n_src, double ball) {
    const long x = j * nx + i;
    const double s = n[x], t = T[x], inf = eik_inf();
    EikLinNode c{0.0, 0.0, 0.0, 0.0, 0};
    if (eik_obstacle(s) || !eik_finite(t)) return c;                    // dead
    if (!filled[x]) {
        c.code = (uint8_t)(kLinSeed << 4);
        return c;
    }
    double w;
    if (eik_init(g, i, j, s, eik_nan(), xs, ys, n_src, ball, &w) == kEikBall) {
        c.cs = c.csrc = eik_lin_csrc(g, i, j, xs, ys);
        c.code = (uint8_t)(kLinBall << 4);
        return c;
    }
    const double l = i > 0 ? eik_lin_read(n[x - 1], T[x - 1]) : inf, r = i + 1 < nx ? eik_lin_read(n[x + 1], T[x + 1]) : inf;
    const double dn = j > 0 ? eik_lin_read(n[x - nx], T[x - nx]) : inf, up = j + 1 < ny ? eik_lin_read(n[x + nx], T[x + nx]) : inf;
    c = eik_lin_coef(g, l, r, dn, up, s, t);
    c.code |= (uint8_t)(kLinFree << 4);
    return c;
}

enum : int32_t { kEikFactoredLin = 3 };     // rtmi_eikonal_params.scheme: the factored fill, and this linearisation of it

// csrc of a free node (i, j) in the factored linearisation from its parents and coefficients; 0 where the node is not factored
RT_EIK_HD double eik_flin_csrc(const EikGrid& g, long i, long j, double xs, double ys, double n_src, uint8_t code, double ca, double cb) {
    double dx, dy, pdx, pdy;                  // the node's; a parent's, not used
    const double rr = eik_rr(g, i, j, xs, ys, &dx, &dy);
    double acc = 0.0;
    if (eik_obstacle(n_src) || rr == 0.0) return acc;
    if (code & kLinXParent) {
        const bool east = (code & kLinXEast) != 0;
        const double d = rr - eik_rr(g, east ? i + 1 : i - 1, j, xs, ys, &pdx, &pdy), p = g.gdx * (dx / rr);
        acc = acc + ca * (east ? d + p : d - p);
    }
    if (code & kLinYParent) {
        const bool north = (code & kLinYNorth) != 0;
        const double d = rr - eik_rr(g, i, north ? j + 1 : j - 1, xs, ys, &pdx, &pdy), p = g.gdy * (dy / rr);
        acc = acc + cb * (north ? d + p : d - p);
    }
    return acc;
}

// The coefficients, csrc and parents of free node (i, j) in the factored linearisation from its four raw readings; the class bits
// of code are not set.  eik_lin_coef gets the corrected reading on the side the raw readings chose and +inf on the other, so that
// its min and its side are that reading and that side.
RT_EIK_HD EikLinNode eik_flin_coef(const EikGrid& g, long i, long j, double xs, double ys, double n_src, double l, double r, double dn,
                                   double up, double s, double t) {
    const double inf = eik_inf();
    double a, b;
    bool east, north;
    eik_factored_readings(g, i, j, xs, ys, n_src, l, r, dn, up, &a, &b, &east, &north);
    EikLinNode c = eik_lin_coef(g, east ? inf : a, east ? a : inf, north ? inf : b, north ? b : inf, s, t);
    c.csrc = eik_flin_csrc(g, i, j, xs, ys, n_src, c.code, c.ca, c.cb);
    return c;
}

// eik_lin_node in the factored linearisation: the free nodes differ
RT_EIK_HD EikLinNode eik_flin_node(const EikGrid& g, long nx, long ny, long i, long j, const double* n, const double* T,
                                   const uint8_t* filled, double xs, double ys, double n_src, double ball) {
    const long x = j * nx + i;
    const double s = n[x], t = T[x], inf = eik_inf();
    EikLinNode c{0.0, 0.0, 0.0, 0.0, 0};
    if (eik_obstacle(s) || !eik_finite(t)) return c;                    // dead
    if (!filled[x]) {
        c.code = (uint8_t)(kLinSeed << 4);
        return c;
    }
    double w;
    if (eik_init(g, i, j, s, eik_nan(), xs, ys, n_src, ball, &w) == kEikBall) {
        c.cs = c.csrc = eik_lin_csrc(g, i, j, xs, ys);
        c.code = (uint8_t)(kLinBall << 4);
        return c;
    }
    const double l = i > 0 ? eik_lin_read(n[x - 1], T[x - 1]) : inf, r = i + 1 < nx ? eik_lin_read(n[x + 1], T[x + 1]) : inf;
    const double dn = j > 0 ? eik_lin_read(n[x - nx], T[x - nx]) : inf, up = j + 1 < ny ? eik_lin_read(n[x + nx], T[x + nx]) : inf;
    c = eik_flin_coef(g, i, j, xs, ys, n_src, l, r, dn, up, s, t);
    c.code |= (uint8_t)(kLinFree << 4);
    return c;
}

// the node in either linearisation, for code that carries the choice as a template flag
template <bool FACT> RT_EIK_HD EikLinNode eik_lin_node_of(const EikGrid& g, long nx, long ny, long i, long j, const double* n,
                                                          const double* T, const uint8_t* filled, double xs, double ys, double n_src,
                                                          double ball) {
    if constexpr (FACT) return eik_flin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
    else return eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
}

// One row's share of g_src in the factored linearisation, on C columns at once: acc[c] = the sum from +0.0 over i ascending of
// csrc lam at the free nodes and the nodes of the ball of row j; v is column-minor, [ny nx][C]
template <int C> RT_EIK_HD void eik_flin_g_src_row(const EikGrid& g, long nx, long j, double xs, double ys, double n_src,
                                                   const uint8_t* code, const double* ca, const double* cb, const double* v, double* acc) {
    for (int c = 0; c < C; c++) acc[c] = 0.0;
    for (long i = 0; i < nx; i++) {
        const long x = j * nx + i;
        const uint8_t cls = eik_lin_class(code[x]);
        if (cls < kLinFree) continue;
        const double w = cls == kLinBall ? eik_lin_csrc(g, i, j, xs, ys) : eik_flin_csrc(g, i, j, xs, ys, n_src, code[x], ca[x], cb[x]);
        for (int c = 0; c < C; c++) acc[c] = acc[c] + w * v[x * C + c];
    }
}

// The starting value of the tangent at a node, which is final unless the node is free; *k is the free node's constant term
RT_EIK_HD double eik_lin_tangent_init(const EikLinNode& c, double dn, double dn_src, double seed, double* k) {
    *k = 0.0;
    switch (eik_lin_class(c.code)) {
        case kLinSeed: return seed;
        case kLinBall: return (0.0 + c.cs * dn) + c.csrc * dn_src;
        case kLinFree: *k = c.cs * dn; return 0.0;
        default: return 0.0;
    }
}

// eik_lin_tangent_init in the factored linearisation: a free node's constant term has the source's share
RT_EIK_HD double eik_flin_tangent_init(const EikLinNode& c, double dn, double dn_src, double seed, double* k) {
    if (eik_lin_class(c.code) != kLinFree) return eik_lin_tangent_init(c, dn, dn_src, seed, k);
    *k = c.cs * dn + c.csrc * dn_src;
    return 0.0;
}

// The tangent's gather at free node x: v [ny][nx] the current values, k = cs dn
RT_EIK_HD double eik_lin_tangent_gather(long nx, long x, uint8_t code, double ca, double cb, double k, const double* v) {
    double acc = 0.0;
    if (code & kLinXParent) acc = acc + ca * v[code & kLinXEast ? x + 1 : x - 1];
    if (code & kLinYParent) acc = acc + cb * v[code & kLinYNorth ? x + nx : x - nx];
    return acc + k;
}

// The neighbours of node (i, j) that name it as a parent, as a mask: 1 west, 2 east, 4 south, 8 north.  The adjoint finds it once
// from the codes, so that a sweep's gather reads no neighbour's code
enum : uint8_t { kLinKidWest = 1, kLinKidEast = 2, kLinKidSouth = 4, kLinKidNorth = 8 };
RT_EIK_HD uint8_t eik_lin_kids(long nx, long ny, long i, long j, const uint8_t* code) {
    const long x = j * nx + i;
    uint8_t m = 0;
    if (i > 0 && (code[x - 1] & (kLinXParent | kLinXEast)) == (kLinXParent | kLinXEast)) m |= kLinKidWest;
    if (i + 1 < nx && (code[x + 1] & (kLinXParent | kLinXEast)) == kLinXParent) m |= kLinKidEast;
    if (j > 0 && (code[x - nx] & (kLinYParent | kLinYNorth)) == (kLinYParent | kLinYNorth)) m |= kLinKidSouth;
    if (j + 1 < ny && (code[x + nx] & (kLinYParent | kLinYNorth)) == kLinYParent) m |= kLinKidNorth;
    return m;
}

// The adjoint's gather at node x, which is not dead: r, then the neighbours W, E, S, N of the mask
RT_EIK_HD double eik_lin_adjoint_gather(long nx, long x, uint8_t kids, double r, const double* ca, const double* cb, const double* v) {
    double acc = r;
    if (kids & kLinKidWest) acc = acc + ca[x - 1] * v[x - 1];
    if (kids & kLinKidEast) acc = acc + ca[x + 1] * v[x + 1];
    if (kids & kLinKidSouth) acc = acc + cb[x - nx] * v[x - nx];
    if (kids & kLinKidNorth) acc = acc + cb[x + nx] * v[x + nx];
    return acc;
}

// Both gathers on C columns at once (k_eikonal_lin_multi): v, k and r are column-minor, [ny nx][C], and column c of t gets what the
// gather above gives on column c alone: the same operations in the same order, the node's code and coefficients read once
template <int C> RT_EIK_HD void eik_lin_tangent_gather_cols(long nx, long x, uint8_t code, double ca, double cb, const double* k,
                                                            const double* v, double* t) {
    for (int c = 0; c < C; c++) t[c] = 0.0;
    if (code & kLinXParent) {
        const double* p = v + (code & kLinXEast ? x + 1 : x - 1) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + ca * p[c];
    }
    if (code & kLinYParent) {
        const double* p = v + (code & kLinYNorth ? x + nx : x - nx) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + cb * p[c];
    }
    for (int c = 0; c < C; c++) t[c] = t[c] + k[x * C + c];
}

template <int C> RT_EIK_HD void eik_lin_adjoint_gather_cols(long nx, long x, uint8_t kids, const double* r, const double* ca,
                                                            const double* cb, const double* v, double* t) {
    for (int c = 0; c < C; c++) t[c] = r[x * C + c];
    if (kids & kLinKidWest) {
        const double w = ca[x - 1], *p = v + (x - 1) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + w * p[c];
    }
    if (kids & kLinKidEast) {
        const double w = ca[x + 1], *p = v + (x + 1) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + w * p[c];
    }
    if (kids & kLinKidSouth) {
        const double w = cb[x - nx], *p = v + (x - nx) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + w * p[c];
    }
    if (kids & kLinKidNorth) {
        const double w = cb[x + nx], *p = v + (x + nx) * C;
        for (int c = 0; c < C; c++) t[c] = t[c] + w * p[c];
    }
}

// the directions of sweep k of a round
RT_EIK_HD bool eik_lin_xup(bool adjoint, int k) { return adjoint ? (k == 1 || k == 2) : (k == 0 || k == 3); }
RT_EIK_HD bool eik_lin_yup(bool adjoint, int k) { return adjoint ? k >= 2 : k < 2; }

// A box of nodes [i0, i1] x [j0, j1] that holds the ball with two cells to spare (empty: i1 < i0); the kernel sums g_src over
// it after it has counted that no node of the ball lies outside
RT_EIK_HD void eik_lin_ball_box(const EikGrid& g, long nx, long ny, double xs, double ys, double ball, long* i0, long* i1, long* j0,
                                long* j1) {
    const double u = (xs - g.gx0) / g.gdx, v = (ys - g.gy0) / g.gdy, m = ball + 3.0;
    const double ul = u - m, uh = u + m, vl = v - m, vh = v + m;
    // a NaN anywhere gives the whole grid
    *i0 = ul > 0.0 ? (ul < (double)nx ? (long)ul : nx) : 0;
    *i1 = uh < (double)(nx - 1) ? (uh > -1.0 ? (long)uh : -1) : nx - 1;
    *j0 = vl > 0.0 ? (vl < (double)ny ? (long)vl : ny) : 0;
    *j1 = vh < (double)(ny - 1) ? (vh > -1.0 ? (long)vh : -1) : ny - 1;
}

// what one source's linear solve reports
struct EikLinResult {
    int32_t rounds, clean;
    int64_t nodes, changes;         // free nodes and nodes of the ball; values whose bits changed, all rounds
};

#if !(defined(__HIPCC__) || defined(__HIP__))
// Both solves of one source as the serial loops that define them, host only.  Work space: ca, cb, k [ny][nx] doubles and code,
// kids [ny][nx] bytes.  dn_src is a value; seed, g and g_src may be NULL.  factored: the factored linearisation.
inline EikLinResult eik_lin_tangent(const EikGrid& g, long nx, long ny, const double* n, const double* T, const uint8_t* filled,
                                    double xs, double ys, double n_src, double ball, int max_rounds, const double* dn, double dn_src,
                                    const double* seed, double* dT, double* ca, double* cb, double* k, uint8_t* code,
                                    bool factored = false) {
    EikLinResult res{0, 1, 0, 0};
    long nfree = 0;
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const long x = j * nx + i;
            const EikLinNode c = factored ? eik_flin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball)
                                          : eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
            ca[x] = c.ca;
            cb[x] = c.cb;
            code[x] = c.code;
            dT[x] = factored ? eik_flin_tangent_init(c, dn[x], dn_src, seed ? seed[x] : 0.0, &k[x])
                             : eik_lin_tangent_init(c, dn[x], dn_src, seed ? seed[x] : 0.0, &k[x]);
            if (eik_lin_class(c.code) >= kLinFree) res.nodes++;
            if (eik_lin_class(c.code) == kLinFree) nfree++;
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
                        const double v = eik_lin_tangent_gather(nx, x, code[x], ca[x], cb[x], k[x], dT);
                        if (eik_bits(v) != eik_bits(dT[x])) {
                            dT[x] = v;
                            changed++;
                        }
                    }
            }
            res.changes += changed;
            res.clean = changed == 0;
            if (res.clean) break;
        }
    }
    return res;
}

inline EikLinResult eik_lin_adjoint(const EikGrid& g, long nx, long ny, const double* n, const double* T, const uint8_t* filled,
                                    double xs, double ys, double n_src, double ball, int max_rounds, const double* r, double* lam,
                                    double* gout, double* g_src, double* ca, double* cb, uint8_t* code, uint8_t* kids,
                                    bool factored = false) {
    EikLinResult res{0, 1, 0, 0};
    long nfree = 0;
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const long x = j * nx + i;
            const EikLinNode c = factored ? eik_flin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball)
                                          : eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
            ca[x] = c.ca;
            cb[x] = c.cb;
            code[x] = c.code;
            lam[x] = eik_lin_class(c.code) == kLinDead ? 0.0 : r[x];
            if (eik_lin_class(c.code) >= kLinFree) res.nodes++;
            if (eik_lin_class(c.code) == kLinFree) nfree++;
        }
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) kids[j * nx + i] = eik_lin_kids(nx, ny, i, j, code);
    const int cap = max_rounds > 0 ? max_rounds : kEikDefaultRounds;
    if (nfree > 0) {
        while (res.rounds < cap) {
            res.rounds++;
            int64_t changed = 0;
            for (int s = 0; s < 4; s++) {
                const bool xup = eik_lin_xup(true, s), yup = eik_lin_yup(true, s);
                for (long q = 0; q < ny; q++)
                    for (long p = 0; p < nx; p++) {
                        const long j = yup ? q : ny - 1 - q, i = xup ? p : nx - 1 - p, x = j * nx + i;
                        if (eik_lin_class(code[x]) == kLinDead) continue;
                        const double v = eik_lin_adjoint_gather(nx, x, kids[x], r[x], ca, cb, lam);
                        if (eik_bits(v) != eik_bits(lam[x])) {
                            lam[x] = v;
                            changed++;
                        }
                    }
            }
            res.changes += changed;
            res.clean = changed == 0;
            if (res.clean) break;
        }
    }
    double acc = 0.0;
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const long x = j * nx + i;
            const uint8_t cls = eik_lin_class(code[x]);
            const EikLinNode c = cls < kLinFree ? EikLinNode{}
                                 : factored     ? eik_flin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball)
                                                : eik_lin_node(g, nx, ny, i, j, n, T, filled, xs, ys, n_src, ball);
            if (gout) gout[x] = cls >= kLinFree ? c.cs * lam[x] : 0.0;
            if (cls == kLinBall) acc = acc + c.csrc * lam[x];
        }
    if (factored) {
        acc = 0.0;
        for (long j = 0; j < ny; j++) {
            double row;
            eik_flin_g_src_row<1>(g, nx, j, xs, ys, n_src, code, ca, cb, lam, &row);
            acc = acc + row;
        }
    }
    if (g_src) *g_src = acc;
    return res;
}
#endif

}  // namespace rt
