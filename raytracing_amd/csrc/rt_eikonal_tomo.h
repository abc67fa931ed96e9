// rt_eikonal_tomo.h -- the host arithmetic of first-arrival eikonal tomography (eikonal_tomo.hip, rtmi_eikonal_tomo_*;
// DESIGN.md section 36), with no HIP in it, so that a host program can include it (tests/native/eikonal_tomo.cpp): the bilinear
// cell weights of a point, the sample of a table at a point, the rule for a live row, and the lists the transposed product
// walks.  tests/eikonal_tomo_ref.py restates all of it in plain Python floats.
//
// Everything is fp64 and every product, sum and quotient below is one rounded operation: build with -ffp-contract=off, as the
// library is.
//
// Cell weights of a point (x, y) on the node grid X = gx0 + i gdx, Y = gy0 + j gdy, i < nx, j < ny:
//     u = (x - gx0) / gdx;  i0 = min(max(floor(u), 0), max(nx - 2, 0));  i1 = min(i0 + 1, nx - 1);  fu = i1 > i0 ? u - i0 : 0
//     and the same in y with v, j0, j1, fv.  Corners in the order (i0, j0), (i1, j0), (i0, j1), (i1, j1), node j nx + i, with the
//     weights (1 - fu)(1 - fv), fu (1 - fv), (1 - fu) fv, fu fv.
//     inside: 0 <= u <= nx - 1 and 0 <= v <= ny - 1.  A SOURCE that is not inside has i0 = j0 = 0 and four weights +0.0: it
//     takes no value from the model and gives none back.  A receiver is inside by the handle's argument check on (x, y).
// Sample:    sample(v, p) = ((w0 v0 + w1 v1) + w2 v2) + w3 v3, v_c the value at corner c.
// Live rows: row (s, k) is live iff none of the four corner nodes of receiver k is dead for source s (rt_eikonal_lin.h: an
//     obstacle, or a T that is not finite).
// Lists: the (point, corner) pairs p = 4 k + c of a set of points, sorted by node and then by p; `node` names the touched nodes in
//     increasing order, off[q] .. off[q + 1] is node q's segment of `pair`.  For the receivers every point takes part; for the
//     sources only those inside.
#pragma once
#include "rt_eikonal_lin.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace rt {

struct EtomoCell {
    long idx[4];
    double w[4];
    bool inside;
};

// one axis: i0, i1 and the fraction of coordinate u on an axis of n nodes
RT_EIK_HD void etomo_axis(double u, long n, long* i0, long* i1, double* f) {
    const long top = n - 2 > 0 ? n - 2 : 0;
    const double fl = std::floor(u);
    *i0 = fl > 0.0 ? (fl < (double)top ? (long)fl : top) : 0;      // a NaN gives 0
    *i1 = *i0 + 1 < n - 1 ? *i0 + 1 : n - 1;
    *f = *i1 > *i0 ? u - (double)*i0 : 0.0;
}

// The cell of point (x, y).  source: a point that is not inside gets i0 = j0 = 0 and zero weights
RT_EIK_HD EtomoCell etomo_cell(const EikGrid& g, long nx, long ny, double x, double y, bool source) {
    EtomoCell c;
    double u = (x - g.gx0) / g.gdx, v = (y - g.gy0) / g.gdy;
    c.inside = u >= 0.0 && u <= (double)(nx - 1) && v >= 0.0 && v <= (double)(ny - 1);
    const bool zero = source && !c.inside;
    if (zero) u = v = 0.0;
    long i0, i1, j0, j1;
    double fu, fv;
    etomo_axis(u, nx, &i0, &i1, &fu);
    etomo_axis(v, ny, &j0, &j1, &fv);
    c.idx[0] = j0 * nx + i0;
    c.idx[1] = j0 * nx + i1;
    c.idx[2] = j1 * nx + i0;
    c.idx[3] = j1 * nx + i1;
    const double gu = 1.0 - fu, gv = 1.0 - fv;
    c.w[0] = zero ? 0.0 : gu * gv;
    c.w[1] = zero ? 0.0 : fu * gv;
    c.w[2] = zero ? 0.0 : gu * fv;
    c.w[3] = zero ? 0.0 : fu * fv;
    return c;
}

// a receiver the handle takes: finite and on the grid's rectangle
RT_EIK_HD bool etomo_receiver_ok(const EikGrid& g, long nx, long ny, double x, double y) {
    return eik_finite(x) && eik_finite(y) && x >= g.gx0 && x <= g.gx0 + (double)(nx - 1) * g.gdx && y >= g.gy0 &&
           y <= g.gy0 + (double)(ny - 1) * g.gdy;
}

RT_EIK_HD double etomo_sample(double v0, double v1, double v2, double v3, const double* w) {
    return ((w[0] * v0 + w[1] * v1) + w[2] * v2) + w[3] * v3;
}

RT_EIK_HD bool etomo_dead(double s, double t) { return eik_obstacle(s) || !eik_finite(t); }

// n, T [ny][nx] of one source, i0 .. i3 the corner nodes of a receiver
template <typename I> RT_EIK_HD bool etomo_live(const double* n, const double* T, const I* idx) {
    for (int c = 0; c < 4; c++)
        if (etomo_dead(n[idx[c]], T[idx[c]])) return false;
    return true;
}

// Host only.  The lists of P points with the corner nodes idx [P][4]; take [P] (or NULL: all) names the points that take part
struct EtomoLists {
    std::vector<int32_t> node, off, pair;
};
template <typename I> inline EtomoLists etomo_lists(const I* idx, long P, const uint8_t* take) {
    std::vector<std::pair<long, long>> all;
    for (long k = 0; k < P; k++) {
        if (take && !take[k]) continue;
        for (long c = 0; c < 4; c++) all.emplace_back((long)idx[4 * k + c], 4 * k + c);
    }
    std::sort(all.begin(), all.end());
    EtomoLists L;
    for (size_t p = 0; p < all.size(); p++) {
        if (p == 0 || all[p].first != all[p - 1].first) {
            L.node.push_back((int32_t)all[p].first);
            L.off.push_back((int32_t)p);
        }
        L.pair.push_back((int32_t)all[p].second);
    }
    L.off.push_back((int32_t)all.size());
    return L;
}

}  // namespace rt
