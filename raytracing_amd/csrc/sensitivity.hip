// sensitivity.hip -- traveltime sensitivity kernels along recorded rays (rtmi_traveltime_perturb, rtmi_traveltime_backproject):
// the Frechet derivative A of every reported traveltime with respect to the n samples Z[qy][qx] of the field, with the rows
// held fixed, and its transpose.  DESIGN.md section 12.
//
// n is the bilinear spline of the samples (rtmi.h: "bilinear coefficients == n samples"), every recorded T is a trapezoid sum
// of s = coef n over the rows, and rtmi_crossings' T is a cubic Hermite blend of two rows' T and s: each is exactly linear in Z.
//   A   one lane per ray walks its rows, gathers 4 samples of dZ per row and carries dT in fp64 in one fixed order.
//   A^T one lane per ray walks its rows with the weight each row carries, keeps fp64 partial sums for the samples of its current
//       cell and flushes them when the cell changes: each partial is rounded once to a fixed-point integer (a power-of-two
//       quantum chosen from the largest per-ray bound, an order-independent maximum), the lanes of a wave that flush the same
//       cell add their integers with shuffles, and one lane adds the group's sum into a two-word (128-bit) accumulator per
//       sample.  Integer sums do not depend on their order: the result has the same bits under every schedule.
// Batches are read through the public rtmi_batch_view; the field and the batch's parameters through two internal hooks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "rt_crossing.h"
#include "rt_fix128.h"
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

// ------------------------------------------------------------------------------------------------------------ A
// One lane per ray.  dT_i = dT_{i-1} + (L_i (ds_{i-1} + ds_i)) 0.5, ds = coef sum(phi dZ); at a crossing (the rule and tau* of
// rtmi_crossings) dT* = ((dT_{i-1} h00 + (L ds_{i-1}) h10) + dT_i h01) + (L ds_i) h11, rtmi_crossings' herm with dT for T.
template <typename T>
__global__ void k_perturb(Rows<T> rec, Args A, const double* dZ, int32_t* count, double* dT_line, double* dT_end) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rec.R) return;
    const long R = rec.R;
    const long o = rec.caller(k);
    const size_t P = rec.pitch();
    const T* col = rec.row(0, k);
    const long last = rec.last(k);
    const Line L = A.L;
    const int qx = A.F.qx;
    auto ds_at = [&](double x, double y, double th) {
        const Cell c = locate(A.F, x, y);
        const Phi w = phi(c);
        const double* z = dZ + (size_t)c.jy * qx + c.jx;
        const double s = ((w.w00 * z[0] + w.w01 * z[1]) + w.w10 * z[qx]) + w.w11 * z[qx + 1];
        return A.aniso ? coef_of(th, A.gamma) * s : s;
    };
    int n = 0;
    if (last >= rec.rec_rows) {
        n = -1;
        dT_end[o] = NAN;
    } else {
        double x0 = (double)col[COL_X * R], y0 = (double)col[COL_Y * R];
        double th0 = A.aniso ? (double)col[COL_TH * R] : 0.0;
        double s0 = ds_at(x0, y0, th0);
        double f0 = (L.a * x0 + L.b * y0) - L.c;
        double dT = 0.0;
        // the next row's loads go out a step ahead
        double xn = 0.0, yn = 0.0, tn = 0.0;
        if (last >= 1) { xn = (double)col[P]; yn = (double)col[P + COL_Y * R]; if (A.aniso) tn = (double)col[P + COL_TH * R]; }
        for (long i = 1; i <= last; i++) {
            const double x1 = xn, y1 = yn, th1 = tn;
            if (i < last) {
                const T* r = col + (size_t)(i + 1) * P;
                xn = (double)r[COL_X * R]; yn = (double)r[COL_Y * R];
                if (A.aniso) tn = (double)r[COL_TH * R];
            }
            const double s1 = ds_at(x1, y1, th1);
            const double dx = x1 - x0, dy = y1 - y0;
            const double len = sqrt(dx * dx + dy * dy);
            const double dTn = dT + (len * (s0 + s1)) * 0.5;
            if (A.has_line) {
                const double f1 = (L.a * x1 + L.b * y1) - L.c;
                if (crosses(f0, f1)) {
                    if (n < A.kmax) {
                        const T* r0 = col + (size_t)(i - 1) * P;
                        const T* r1 = col + (size_t)i * P;
                        const double ta = (double)r0[COL_TH * R], tb = (double)r1[COL_TH * R];
                        const double d0 = len * (L.a * cos_g(ta) + L.b * sin_g(ta)), d1 = len * (L.a * cos_g(tb) + L.b * sin_g(tb));
                        const Basis h = basis(cross_tau(f0, d0, f1, d1));
                        dT_line[(size_t)n * R + o] = herm(h, dT, len * s0, dTn, len * s1);
                    }
                    n++;
                }
                f0 = f1;
            }
            dT = dTn;
            x0 = x1; y0 = y1; s0 = s1;
        }
        dT_end[o] = dT;
    }
    if (count) count[o] = n;
    if (A.has_line)
        for (int c = n < 0 ? 0 : n; c < A.kmax; c++) dT_line[(size_t)c * R + o] = NAN;
}

// ------------------------------------------------------------------------------------------------------------ A^T
__device__ __forceinline__ double w0(double w) { return w == w ? w : 0.0; }       // NaN weights count as 0

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

// Per ray: a bound on any partial sum its lane can flush, (|w_end| + sum_c |w_c|) 2 len coef_max (a row's weights total at most
// 1.15 len coef_max per unit of weight: DESIGN.md 12), and its maximum over rays (non-negative doubles order as their bits).
template <typename T>
__global__ void k_bound(Rows<T> rec, Args A, const double* w_line, const double* w_end, double coef_max, unsigned long long* maxb) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rec.R) return;
    const long o = rec.caller(k);
    if (rec.last(k) >= rec.rec_rows) return;
    double w = w_end ? fabs(w0(w_end[o])) : 0.0;
    if (w_line)
        for (int c = 0; c < A.kmax; c++) w += fabs(w0(w_line[(size_t)c * rec.R + o]));
    const double b = w * (2.0 * A.dist[k]) * coef_max;
    if (b > 0.0) atomicMax(maxb, (unsigned long long)__double_as_longlong(b));
}

__global__ void k_fill(unsigned long long* p, size_t n, unsigned long long v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// One lane per ray.  Step i (rows i-1, i) gives both rows (L_i 0.5) W_i, W_i = w_end + the weights of the crossings after
// step i; a crossing c < min(count, kmax) on step i gives row i-1 w_c L_i (0.5 h01 + h10) and row i w_c L_i (0.5 h01 + h11).
// A row's weight times its coef, times phi, goes into the lane's partial sums of its cell.
template <typename T>
__global__ void k_backproject(Rows<T> rec, Args A, const double* w_line, const double* w_end, const unsigned long long* maxb,
                              unsigned long long* lo, unsigned long long* hi, unsigned long long* natomics) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < rec.R;
    const long R = rec.R;
    const long o = in ? rec.caller(k) : 0;
    const size_t P = rec.pitch();
    const T* col = rec.row(0, in ? k : 0);
    long last = in ? rec.last(k) : -1;
    if (last >= rec.rec_rows) last = -1;                      // past the record: no reported traveltime, no weight
    const Line L = A.L;
    const int qx = A.F.qx;
    const int e = rt::fix_exponent(__longlong_as_double((long long)*maxb));    // quantum 2^e: every partial is below 2^57 quanta
    // crossings that carry a weight: the first min(count, kmax)
    const bool line = A.has_line && w_line != nullptr;
    const int K = (line && last >= 0) ? min(count_crossings(rec, in ? k : 0, last, L), A.kmax) : 0;
    const double we = (w_end && last >= 0) ? w0(w_end[o]) : 0.0;
    auto wc = [&](int c) { return w0(w_line[(size_t)c * R + o]); };
    auto weight_after = [&](int c0) {                       // w_end + the weights of crossings c0 .. K-1
        double w = we;
        for (int c = c0; c < K; c++) w += wc(c);
        return w;
    };
    double W = weight_after(0);
    // the lane's current cell and its partial sums
    int cx = -1, cy = -1;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    long long nat = 0;
    const int lane = (int)(threadIdx.x & 63);
    // every lane of the wave calls this together; lanes with `go` hand over p for cell (cx, cy)
    auto flush = [&](bool go) {
        unsigned long long todo = __ballot(go);
        long long m[4] = {0, 0, 0, 0};
        if (go) {
#pragma unroll
            for (int q = 0; q < 4; q++) m[q] = (long long)rint(ldexp(p[q], -e));
        }
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lx = __shfl(cx, leader), ly = __shfl(cy, leader);
            const bool mem = go && cx == lx && cy == ly;
            const unsigned long long mm = __ballot(mem);
            long long v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = mem ? m[q] : 0;
            if (__popcll(mm) > 1) {
#pragma unroll
                for (int off = 1; off < 64; off <<= 1)
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q] += __shfl_xor(v[q], off);
            }
            if (lane == leader) {
                const size_t b = (size_t)ly * qx + lx;
                nat += rt::add128(lo, hi, b, v[0]);
                nat += rt::add128(lo, hi, b + 1, v[1]);
                nat += rt::add128(lo, hi, b + qx, v[2]);
                nat += rt::add128(lo, hi, b + qx + 1, v[3]);
            }
            todo &= ~mm;
        }
    };
    // row j's weight a (coef not yet applied) at (x, y): into the partials, after a flush when the cell changes
    auto deposit = [&](bool act, double x, double y, double th, double a) {
        Cell c{0, 0, 0.0, 0.0};
        bool go = false;
        if (act) {
            c = locate(A.F, x, y);
            go = (c.jx != cx || c.jy != cy) && cx >= 0;
        }
        flush(go);
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
    const long end = live ? last : 0;
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
    flush(cx >= 0);
    // one count per wave
    for (int off = 1; off < 64; off <<= 1) nat += __shfl_xor(nat, off);
    if (lane == 0 && nat) atomicAdd(natomics, (unsigned long long)nat);
}

// The checks both entries share, then the batch's rows and the field's axes
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

RTMI_EXPORT int rtmi_traveltime_perturb(rtmi_batch* b, const double line[3], int32_t kmax, const double* dZ, int32_t* count,
                                        double* dT_line, double* dT_end, rtmi_sensitivity_stats* st) {
    const char* who = "rtmi_traveltime_perturb";
    RTMI_RC(check_line(line, kmax, who));
    RTMI_ARG(dZ && dT_end, "null dZ or dT_end");
    RTMI_ARG(!line || (count && dT_line), "a line needs count and dT_line");
    RTMI_ARG(b, "null batch");
    Args A;
    rtmi_device_view v;
    RTMI_RC(prepare(b, line, kmax, who, &A, &v));
    const size_t R = (size_t)v.R, nz = (size_t)A.F.qx * A.F.qy, K = (size_t)A.kmax;
    DevMem mem;
    double *dz = nullptr, *de = nullptr, *dl = nullptr;
    int32_t* dc = nullptr;
    RTMI_HIP(mem.get(&dz, nz * sizeof(double)));
    RTMI_HIP(mem.get(&de, R * sizeof(double)));
    RTMI_HIP(mem.get(&dc, R * sizeof(int32_t)));
    if (K) RTMI_HIP(mem.get(&dl, K * R * sizeof(double)));
    RTMI_HIP(hipMemcpy(dz, dZ, nz * sizeof(double), hipMemcpyHostToDevice));
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const dim3 g = blocks((long)R), blk(256);
    RTMI_HIP(ev.mark(0));
    if (R) {
        by_dtype(v.dtype, [&](auto t) { hipLaunchKernelGGL(k_perturb<decltype(t)>, g, blk, 0, nullptr, rows_of<decltype(t)>(v), A, dz, dc, dl, de); });
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    RTMI_HIP(hipMemcpy(dT_end, de, R * sizeof(double), hipMemcpyDeviceToHost));
    if (count) RTMI_HIP(hipMemcpy(count, dc, R * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (K) RTMI_HIP(hipMemcpy(dT_line, dl, K * R * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        *st = rtmi_sensitivity_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_traveltime_backproject(rtmi_batch* b, const double line[3], int32_t kmax, const double* w_line,
                                            const double* w_end, double* g, rtmi_sensitivity_stats* st) {
    const char* who = "rtmi_traveltime_backproject";
    RTMI_RC(check_line(line, kmax, who));
    RTMI_ARG(g, "null g");
    RTMI_ARG(!w_line || line, "w_line needs a line");
    RTMI_ARG(b, "null batch");
    Args A;
    rtmi_device_view v;
    RTMI_RC(prepare(b, line, kmax, who, &A, &v));
    const size_t R = (size_t)v.R, nz = (size_t)A.F.qx * A.F.qy, K = (size_t)A.kmax;
    DevMem mem;
    double *dwl = nullptr, *dwe = nullptr;
    unsigned long long *acc = nullptr, *misc = nullptr;    // acc: lo [nz], hi [nz]; misc: the bound, the atomics issued
    RTMI_HIP(mem.get(&acc, 2 * nz * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&misc, 2 * sizeof(unsigned long long)));
    if (w_line) {
        RTMI_HIP(mem.get(&dwl, K * R * sizeof(double)));
        RTMI_HIP(hipMemcpy(dwl, w_line, K * R * sizeof(double), hipMemcpyHostToDevice));
    }
    if (w_end) {
        RTMI_HIP(mem.get(&dwe, R * sizeof(double)));
        RTMI_HIP(hipMemcpy(dwe, w_end, R * sizeof(double), hipMemcpyHostToDevice));
    }
    RTMI_HIP(hipMemset(misc, 0, 2 * sizeof(unsigned long long)));
    RTMI_HIP(hipMemset(acc + nz, 0, nz * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_fill, blocks((long)nz), dim3(256), 0, nullptr, acc, nz, rt::kFixBias);   // the low words' bias
    RTMI_HIP(hipGetLastError());
    const double coef_max = A.aniso ? fmax(1.0, fabs(A.gamma)) : 1.0;
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const dim3 gr = blocks((long)R), blk(256);
    RTMI_HIP(ev.mark(0));
    if (R) {
        by_dtype(v.dtype, [&](auto t) {
            hipLaunchKernelGGL(k_bound<decltype(t)>, gr, blk, 0, nullptr, rows_of<decltype(t)>(v), A, dwl, dwe, coef_max, misc);
            hipLaunchKernelGGL(k_backproject<decltype(t)>, gr, blk, 0, nullptr, rows_of<decltype(t)>(v), A, dwl, dwe, misc, acc, acc + nz, misc + 1);
        });
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    std::vector<unsigned long long> h(2 * nz);
    unsigned long long hm[2];
    RTMI_HIP(hipMemcpy(h.data(), acc, 2 * nz * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(hm, misc, sizeof(hm), hipMemcpyDeviceToHost));
    double maxb;
    std::memcpy(&maxb, &hm[0], sizeof(double));
    const int e = rt::fix_exponent(maxb);
    for (size_t i = 0; i < nz; i++) g[i] = std::ldexp(rt::fix_to_double(h[i], h[nz + i]), e);      // one rounding to fp64
    if (st) {
        *st = rtmi_sensitivity_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->atomics = (int64_t)hm[1];
        st->scale_exp = e;
    }
    return RTMI_OK;
}
