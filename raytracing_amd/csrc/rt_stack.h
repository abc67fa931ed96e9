// rt_stack.h -- the arithmetic of pick-free event detection and location by stacking station traces along the moveout of every
// grid node (stack.hip, rtmi_locate_stack), with no HIP in it, so that a host program can include it
// (tests/native/stack_events.cpp): the step of one (node, origin time, station), which the kernels call, the selection of events
// from the detection series and the two refinements of an event on its 3 x 3 x 3 window, which the C entry runs on the host.
// tests/stack_ref.py restates all of it in numpy.
//
// Everything is fp64 and every product, sum and quotient below is one rounded operation: build with -ffp-contract=off, as the
// library is.
//
// One node x at one scan index m, o = o0 + (double)m * od, r ascending over the valid stations, every sum from +0.0:
//     f = ((o + T[r][x]) - ct0) * inv                         inv = 1.0 / cdt, computed once
//     the station contributes iff f >= 0 and f < nt - 1 (which no NaN or infinite T passes) and, with j = floor(f), c[r][j] and
//     c[r][j + 1] are both finite
//     a = f - j;  v = (1.0 - a) * c[r][j] + a * c[r][j + 1]
//     n += 1;  sw = sw + w[r];  s = s + w[r] * v              (no weights: s = s + v, and sw = (double)n at the end)
//     S = s / sw where n >= max(need, 1), -inf elsewhere
//
// Events from peak [M] and peak_node [M] alone: m is eligible iff peak[m] >= threshold and peak_node[m] >= 0; the eligible m of
// greatest peak that is not masked is taken, ties to the least m, and masks every m' with |m' - m| <= min_sep; until max_events
// are taken or none is left.  Walking the eligible m once in the order (peak descending, m ascending) and taking each one that
// is not masked yet is the same rule.
//
// Refinement of an event on win [3][3][3] = S at (m + dm, iy + j, ix + i), index (dm + 1) * 9 + (j + 1) * 3 + (i + 1):
//     space   rt::locate_refine (rt_locate.h, the function itself) on the negated middle slice -win[9 .. 17], tau all zero,
//             ref 0 and sw 1: only x, y, dx, dy and refined are used
//     time    with S-, S0, S+ = win[4], win[13], win[22]:   dm = ((S- - S+) / 2) / ((S- - 2 S0) + S+)
//             accepted iff the three are finite, the denominator is < 0 and |dm| <= 1; then t0 = o + dm * od, else dm = 0, t0 = o
// The two are independent: each is the vertex of a parabola along its own axes and ignores the cross terms between space and
// time.  The 27 values are returned for callers who want a joint fit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "rt_locate.h"

namespace rt {

// the running sums of one node at one scan index
struct StackSums {
    int n;
    double sw, s;
};

// What a step reads of the traces: their start time, 1 / cdt and (double)(nt - 1)
struct StackAxis {
    double ct0, inv, ntm1;
};

// One (node, scan index, station).  src(j, c0, c1) reads samples j and j + 1 of the station's trace; it is called with j = 0
// where f is out of range, so that the read needs no branch.  Returns whether the station contributed.
template <bool W, typename Src> RT_LOCATE_HD bool stack_step(StackSums& a, double o, double T, double w, const StackAxis& ax, Src&& src) {
    const double f = ((o + T) - ax.ct0) * ax.inv;
    const bool in = f >= 0.0 && f < ax.ntm1;
    const double jf = floor(f);
    const long j = in ? (long)(int)jf : 0;                 // nt <= 2^31: one conversion instruction on the device
    double c0, c1;
    src(j, c0, c1);
    const bool ok = in && fabs(c0) < INFINITY && fabs(c1) < INFINITY;
    const double fr = f - jf;
    const double v = (1.0 - fr) * c0 + fr * c1;
    a.n += ok ? 1 : 0;
    if (W) {
        a.sw = ok ? a.sw + w : a.sw;
        a.s = ok ? a.s + w * v : a.s;
    } else {
        a.s = ok ? a.s + v : a.s;
    }
    return ok;
}

// S of the sums; needv = max(need, 1)
template <bool W> RT_LOCATE_HD double stack_value(const StackSums& a, int needv) {
    return a.n >= needv ? a.s / (W ? a.sw : (double)a.n) : -INFINITY;
}

// The events of a detection series, in the order they are taken.  *remained: eligible samples that are not masked were left
// when max_events stopped the loop.
inline std::vector<int64_t> stack_select(const double* peak, const int32_t* peak_node, int64_t M, double threshold, int64_t min_sep,
                                         int64_t max_events, int* remained) {
    std::vector<int64_t> order, taken;
    for (int64_t m = 0; m < M; m++)
        if (peak[m] >= threshold && peak_node[m] >= 0) order.push_back(m);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return peak[a] > peak[b]; });
    std::vector<char> masked((size_t)M, 0);
    *remained = 0;
    for (int64_t m : order) {
        if (masked[(size_t)m]) continue;
        if ((int64_t)taken.size() >= max_events) {
            *remained = 1;
            break;
        }
        taken.push_back(m);
        const int64_t lo = m - min_sep > 0 ? m - min_sep : 0, hi = min_sep < M - 1 - m ? m + min_sep : M - 1;
        for (int64_t k = lo; k <= hi; k++) masked[(size_t)k] = 1;
    }
    return taken;
}

struct StackRefined {
    double x, y, t0, dx, dy, dm;
    int refined;                  // bit 0: the location is the spatial parabola's, bit 1: the origin time is the temporal one's
};

// win [27] around (m, iy, ix); o the origin time of scan index m
inline StackRefined stack_refine(const double* win, double o, double od, int ix, int iy, const LocateGrid& g) {
    double f[9], tau[9];
    for (int k = 0; k < 9; k++) {
        f[k] = -win[9 + k];
        tau[k] = 0.0;
    }
    const LocateRefined s = locate_refine(f, tau, 0.0, 1.0, ix, iy, g);
    StackRefined r{s.x, s.y, o, s.dx, s.dy, 0.0, s.refined ? 1 : 0};
    const double sm = win[4], s0 = win[13], sp = win[22];
    if (!(std::isfinite(sm) && std::isfinite(s0) && std::isfinite(sp))) return r;
    const double den = (sm - 2.0 * s0) + sp;
    if (!(den < 0.0)) return r;
    const double dm = ((sm - sp) / 2.0) / den;
    if (!(std::fabs(dm) <= 1.0)) return r;
    r.dm = dm;
    r.t0 = o + dm * od;
    r.refined |= 2;
    return r;
}

}  // namespace rt
