// rt_sens_walk.h -- the walk along a ray's recorded rows that gives every row its weight in a set of reported traveltimes, cell
// visit by cell visit, shared by sensitivity.hip (rtmi_traveltime_backproject: a visit's partial sums go into the accumulators)
// and tomo.hip (rtmi_tomo_append: a visit's partial sums become one segment of a matrix row).  One piece of device code with two
// sinks: what is computed for a row, and in which order, does not depend on the sink.  Also the field's sample axes as both units
// read them, and the checks both make of a batch and a line.  DESIGN.md sections 12 and 24.  Anonymous namespace, as with
// rt_crossing.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rt_crossing.h"
#include "rt_polytab.h"
#include "rt_rows.h"
#include "rtmi_host.h"

namespace {

constexpr int kMaxLine = 64;      // kmax: at most this many crossings per ray

// The field's map from a point to its cell and (u, v): rt::locate (rt_polytab.h).  The indices are clamped once more so that no
// row, however odd, addresses outside the samples.
struct Axes {
    double ax, bx, inv_hx, ay, by, inv_hy;
    int qx, qy;                   // samples per axis; cells qx - 1, qy - 1
};
typedef rt::PolyPos Cell;
__device__ __forceinline__ Cell locate(const Axes& F, double x, double y) {
    const int ncx = F.qx - 1, ncy = F.qy - 1;
    Cell c = rt::locate(F, ncx, ncy, x, y);
    c.jx = c.jx < 0 ? 0 : (c.jx > ncx - 1 ? ncx - 1 : c.jx);
    c.jy = c.jy < 0 ? 0 : (c.jy > ncy - 1 ? ncy - 1 : c.jy);
    return c;
}
// the sample weights (1-u)(1-v), u(1-v), (1-u)v, uv on Z[j][i], Z[j][i+1], Z[j+1][i], Z[j+1][i+1]
struct Phi { double w00, w01, w10, w11; };
__device__ __forceinline__ Phi phi(const Cell& c) {
    const double u1 = 1.0 - c.u, v1 = 1.0 - c.v;
    return Phi{u1 * v1, c.u * v1, u1 * c.v, c.u * c.v};
}

// anisotropy(theta, gamma) as the step kernels evaluate it (rt_device.h aniso), sin / cos glibc's through rt_libm.h
__device__ __forceinline__ double coef_of(double th, double gamma) {
    const double s = sin_g(th), c = cos_g(th);
    const double gs = gamma * s;
    return sqrt(__builtin_fma(gs, gs, c * c));
}

struct Args {
    const double* dist;           // [R] dist_sim (slot order): the bound of the fixed-point scale
    Axes F;
    Line L;
    int has_line, kmax, aniso;
    double gamma;
};

// The crossings of a ray's rows with the line (rtmi_crossings' rule), counted
template <typename T> __device__ __forceinline__ int count_crossings(const Rows<T>& rec, long k, long last, const Line& L) {
    const long R = rec.R;
    const T* col = rec.row(0, k);
    double f0 = (L.a * (double)col[COL_X * R] + L.b * (double)col[COL_Y * R]) - L.c;
    int n = 0;
    for (long i = 1; i <= last; i++) {
        const T* r = col + (size_t)i * rec.pitch();
        const double f1 = (L.a * (double)r[COL_X * R] + L.b * (double)r[COL_Y * R]) - L.c;
        n += crosses(f0, f1) ? 1 : 0;
        f0 = f1;
    }
    return n;
}

// One lane per ray, the lanes of a wave together.  Step i (rows i-1, i) gives both rows (L_i 0.5) W_i, W_i = we + the weights of
// the crossings after step i; a crossing c < K on step i gives row i-1 wc(c) L_i (0.5 h01 + h10) and row i wc(c) L_i
// (0.5 h01 + h11).  A row's weight times its coef, times phi, goes into the lane's partial sums p[0..3] of its current cell; when
// the cell changes, and after the last row, the sink takes them:
//     sink.flush(go, cx, cy, p)   every lane of the wave calls it together; lanes with `go` hand over p for cell (cx, cy)
//     Sink::kStopAtLast           the walk of a ray whose end carries no weight (we == 0) ends with the step of crossing K - 1,
//                                 the last row that carries any
// last: the ray's last row, -1 for a lane without a ray or a ray without a reported traveltime; K: the crossings that carry a
// weight, the first K (at most the ray's count and kmax); line: whether crossings are looked for at all.
template <typename T, typename WC, typename Sink>
__device__ __forceinline__ void walk_weighted(const Rows<T>& rec, const Args& A, long k, long last, bool line, int K, double we, WC&& wc,
                                              Sink& sink) {
    const long R = rec.R;
    const size_t P = rec.pitch();
    const T* col = rec.row(0, k);
    const Line L = A.L;
    auto weight_after = [&](int c0) {                       // we + the weights of crossings c0 .. K-1
        double w = we;
        for (int c = c0; c < K; c++) w += wc(c);
        return w;
    };
    double W = weight_after(0);
    // the lane's current cell and its partial sums
    int cx = -1, cy = -1;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    // row j's weight a (coef not yet applied) at (x, y): into the partials, after a flush when the cell changes
    auto deposit = [&](bool act, double x, double y, double th, double a) {
        Cell c{0, 0, 0.0, 0.0};
        bool go = false;
        if (act) {
            c = locate(A.F, x, y);
            go = (c.jx != cx || c.jy != cy) && cx >= 0;
        }
        sink.flush(go, cx, cy, p);
        if (act) {
            if (c.jx != cx || c.jy != cy) { cx = c.jx; cy = c.jy; p[0] = p[1] = p[2] = p[3] = 0.0; }
            const double wr = A.aniso ? a * coef_of(th, A.gamma) : a;
            const Phi f = phi(c);
            p[0] += wr * f.w00; p[1] += wr * f.w01; p[2] += wr * f.w10; p[3] += wr * f.w11;
        }
    };
    const bool live = last >= 0 && (we != 0.0 || K > 0);
    double x0 = 0.0, y0 = 0.0, th0 = 0.0, f0 = 0.0, xn = 0.0, yn = 0.0, tn = 0.0;
    if (live) {
        x0 = (double)col[COL_X * R]; y0 = (double)col[COL_Y * R];
        if (A.aniso) th0 = (double)col[COL_TH * R];
        f0 = (L.a * x0 + L.b * y0) - L.c;
        if (last >= 1) { xn = (double)col[P]; yn = (double)col[P + COL_Y * R]; if (A.aniso) tn = (double)col[P + COL_TH * R]; }
    }
    long end = live ? last : 0;
    double aprev = 0.0;                                     // row i-1's weight so far
    int n = 0;
    for (long i = 1;; i++) {
        const bool act = i <= end;
        if (__ballot(act) == 0ull) break;
        double x1 = 0.0, y1 = 0.0, th1 = 0.0, acur = 0.0;
        if (act) {
            x1 = xn; y1 = yn; th1 = tn;
            if (i < end) {
                const T* r = col + (size_t)(i + 1) * P;
                xn = (double)r[COL_X * R]; yn = (double)r[COL_Y * R];
                if (A.aniso) tn = (double)r[COL_TH * R];
            }
            const double dx = x1 - x0, dy = y1 - y0;
            const double len = sqrt(dx * dx + dy * dy);
            if (line) {
                const double f1 = (L.a * x1 + L.b * y1) - L.c;
                if (crosses(f0, f1)) {
                    if (n < K) {
                        const T* r0 = col + (size_t)(i - 1) * P;
                        const T* r1 = col + (size_t)i * P;
                        const double ta = (double)r0[COL_TH * R], tb = (double)r1[COL_TH * R];
                        const double d0 = len * (L.a * cos_g(ta) + L.b * sin_g(ta)), d1 = len * (L.a * cos_g(tb) + L.b * sin_g(tb));
                        const Basis h = basis(cross_tau(f0, d0, f1, d1));
                        const double w = wc(n);
                        aprev += (w * len) * (0.5 * h.h01 + h.h10);
                        acur = (w * len) * (0.5 * h.h01 + h.h11);
                        W = weight_after(n + 1);
                        if (Sink::kStopAtLast && n + 1 == K && we == 0.0) end = i;
                    }
                    n++;
                }
                f0 = f1;
            }
            const double half = (W * len) * 0.5;
            aprev += half;
            acur += half;
        }
        deposit(act, x0, y0, th0, aprev);                   // row i-1 is complete
        if (act) { aprev = acur; x0 = x1; y0 = y1; th0 = th1; }
    }
    deposit(live, x0, y0, th0, aprev);                      // the last row
    sink.flush(cx >= 0, cx, cy, p);
}

// The checks every entry on a batch's rows shares (rtmi_traveltime_perturb, _backproject, rtmi_tomo_append), then the batch's rows
// and the field's axes
int prepare(rtmi_batch* b, const double* line, int32_t kmax, const char* who, Args* A, rtmi_device_view* v) {
    Recorded r;
    RTMI_RC(recorded(who, b, kRecPoly | kRecFromLaunch, 0, &r));
    int qx = 0, qy = 0;
    RTMI_RC(rtmi_field_dims(r.f, &qx, &qy));
    *v = r.v;
    Line L{0.0, 0.0, 0.0};
    if (line) (void)make_line(line, &L);
    *A = Args{v->dist_sim, Axes{r.poly.ax, r.poly.bx, r.poly.inv_hx, r.poly.ay, r.poly.by, r.poly.inv_hy, qx, qy}, L, line ? 1 : 0, line ? kmax : 0,
              r.p.method >= 10 ? 1 : 0, r.p.gamma};
    return RTMI_OK;
}

int check_line(const double* line, int32_t kmax, const char* who) {
    if (!line) return RTMI_OK;
    Line L;
    RTMI_ARG(kmax >= 1 && kmax <= kMaxLine, "kmax must be in 1..64");
    RTMI_ARG(make_line(line, &L), "the line needs (a, b) != (0, 0) and finite coefficients");
    return RTMI_OK;
}

}  // namespace
