// rt_edt.h -- the arithmetic of event location by equal differential time (edt.hip, rtmi_locate_edt; include/rtmi.h, DESIGN.md
// section 31), with no HIP in it, so that a host program can include it (tests/native/edt_node.cpp): the kernel of a station
// pair, which the search calls once per (event, node, pair), and a node's value, station shares and origin time as the window
// kernel walks them.  tests/edt_ref.py restates them in numpy.
//
// Everything is fp64 and every product, sum, quotient and square root below is one rounded operation: build with
// -ffp-contract=off, as the library is.  The only fused operations are those of rt_np_exp.h, which are part of its definition.
//
// Pick variance      v = sigma sigma (no weights),  v_r = 1.0 / w_r + sigma sigma (weights)
// Pair (a, b), a < b g = 1.0 / (v_a + v_b);  with weights h = sqrt(g), without them h is left out
// Node x, event e    a station contributes iff its pick is valid and T[r][x] is finite; n of them; d_r = tr_r - T[r][x]
//     over the contributing pairs, a ascending outside, b > a ascending inside, S and H from +0.0:
//         u = d_a - d_b;  z = -((u u) g);  k = z < -700 ? +0.0 : exp(z)        exp: rt_np_exp.h's main path
//         S = S + h k;  H = H + h                                               (no weights: S = S + k, H = (double)(n (n - 1) / 2))
//     value = S / H where n >= max(need, 2), -inf elsewhere
//     omega_r = sum over the contributing b != r, ascending, of h_rb k_rb, each k with the lower station first in u
//     tau = (sum_r omega_r d_r) / (sum_r omega_r), r ascending, from +0.0
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rt_np_exp.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_EDT_HD __host__ __device__ __forceinline__
#else
#define RT_EDT_HD inline
#endif

namespace rt {

constexpr double kEdtCut = -700.0;      // below it a pair's kernel is +0.0: exp(-700) is 1e-304, and the main path of exp ends at -707.7

// exp on [-700, 0]: numpy's, bit for bit (rtmi_edt_exp hands it out)
RT_EDT_HD double edt_exp(double z, const double* tab) { return np_exp_main(z, tab); }

RT_EDT_HD double edt_sqrt(double g) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(g);
#else
    return std::sqrt(g);
#endif
}

// The kernel of one pair, the lower station first.  Written without a branch -- the exp of a cut pair is taken at -700 and dropped
// -- so that the lanes of a wave stay together; the value is the definition's.
RT_EDT_HD double edt_k(double da, double db, double g, const double* tab) {
    const double u = da - db;
    const double z = -((u * u) * g);
    const bool cut = z < kEdtCut;
    const double k = edt_exp(cut ? kEdtCut : z, tab);
    return cut ? 0.0 : k;
}

RT_EDT_HD double edt_var(double w, double s2) { return 1.0 / w + s2; }
RT_EDT_HD double edt_g(double va, double vb) { return 1.0 / (va + vb); }

// One node of one event as strided memory: station r's staged pick tr[r * trs] (NaN: none), weight wv[r * trs] (W only) and
// table value T[r * Ts]
struct EdtView {
    int P;
    const double* tr;
    const double* wv;
    size_t trs;
    const double* T;
    size_t Ts;
    double s2;          // sigma sigma
    double g0;          // no weights: every pair's g
    const double* tab;  // rt_np_exp.h's tables
};

RT_EDT_HD bool edt_contributes(const EdtView& v, int r, double& d) {
    const double trv = v.tr[(size_t)r * v.trs], Tv = v.T[(size_t)r * v.Ts];
    d = trv - Tv;
    return trv == trv && fabs(Tv) < INFINITY;
}

struct EdtNode {
    int n;
    bool cand;
    double S, H, value;
};

// need2 = max(need, 2)
template <bool W> RT_EDT_HD EdtNode edt_node(const EdtView& v, int need2) {
    EdtNode o{0, false, 0.0, 0.0, 0.0};
    for (int a = 0; a < v.P; a++) {
        double da;
        if (!edt_contributes(v, a, da)) continue;
        o.n += 1;
        const double va = W ? edt_var(v.wv[(size_t)a * v.trs], v.s2) : 0.0;
        for (int b = a + 1; b < v.P; b++) {
            double db;
            if (!edt_contributes(v, b, db)) continue;
            if (W) {
                const double g = edt_g(va, edt_var(v.wv[(size_t)b * v.trs], v.s2)), h = edt_sqrt(g);
                o.S = o.S + h * edt_k(da, db, g, v.tab);
                o.H = o.H + h;
            } else {
                o.S = o.S + edt_k(da, db, v.g0, v.tab);
            }
        }
    }
    if (!W) o.H = (double)((long long)o.n * (o.n - 1) / 2);
    o.cand = o.n >= need2;
    o.value = o.cand ? o.S / o.H : -INFINITY;
    return o;
}

// omega of station r, which contributes with d_r = dr
template <bool W> RT_EDT_HD double edt_share(const EdtView& v, int r, double dr) {
    double om = 0.0;
    const double vr = W ? edt_var(v.wv[(size_t)r * v.trs], v.s2) : 0.0;
    for (int b = 0; b < v.P; b++) {
        double db;
        if (b == r || !edt_contributes(v, b, db)) continue;
        const bool below = b < r;                       // the lower station comes first, in u and in v_a + v_b
        if (W) {
            const double vb = edt_var(v.wv[(size_t)b * v.trs], v.s2);
            const double g = below ? edt_g(vb, vr) : edt_g(vr, vb), h = edt_sqrt(g);
            om = om + h * (below ? edt_k(db, dr, g, v.tab) : edt_k(dr, db, g, v.tab));
        } else {
            om = om + (below ? edt_k(db, dr, v.g0, v.tab) : edt_k(dr, db, v.g0, v.tab));
        }
    }
    return om;
}

// tau of the node and the sum of its shares; share [P] (or null) receives omega, NaN where the station does not contribute
template <bool W> RT_EDT_HD double edt_tau(const EdtView& v, double* den_out, double* share) {
    double num = 0.0, den = 0.0;
    for (int r = 0; r < v.P; r++) {
        double dr;
        const bool c = edt_contributes(v, r, dr);
        const double om = c ? edt_share<W>(v, r, dr) : NAN;
        if (share) share[r] = om;
        if (!c) continue;
        num = num + om * dr;
        den = den + om;
    }
    *den_out = den;
    return num / den;
}

// resid [P] = d_r - tau, NaN where the station does not contribute
RT_EDT_HD void edt_resid(const EdtView& v, double tau, double* resid) {
    for (int r = 0; r < v.P; r++) {
        double dr;
        resid[r] = edt_contributes(v, r, dr) ? dr - tau : NAN;
    }
}

}  // namespace rt
