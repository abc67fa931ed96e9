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
// A^T's walk is rt_sens_walk.h's, shared with tomo.hip, which compiles the same rows into a matrix.
// Batches are read through the public rtmi_batch_view; the field and the batch's parameters through two internal hooks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "rt_fix128.h"
#include "rt_sens_walk.h"
#include "rtmi_host.h"

namespace {

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

// Every lane of the wave calls this together; lanes with `go` add m[0..3] quanta to the samples base, base + 1, base + qx,
// base + qx + 1 of cell (cx, cy), base = cy qx + cx.  Lanes that name the same cell are summed with shuffles first (64 terms below
// 2^57 fit an int64), and one of them adds the group's sum.  Returns the atomics this lane issued.
__device__ __forceinline__ long long wave_add128(bool go, int cx, int cy, const long long (&m)[4], unsigned long long* lo,
                                                 unsigned long long* hi, int qx, int lane) {
    long long nat = 0;
    unsigned long long todo = __ballot(go);
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
    return nat;
}

// walk_weighted's sink: each partial is rounded once to quanta 2^e, and the lanes of the wave that leave the same cell add as one
struct FlushSink {
    static constexpr bool kStopAtLast = false;
    unsigned long long *lo, *hi;
    int qx, e, lane;
    long long nat;
    __device__ __forceinline__ void flush(bool go, int cx, int cy, const double (&p)[4]) {
        long long m[4] = {0, 0, 0, 0};
        if (go) {
#pragma unroll
            for (int q = 0; q < 4; q++) m[q] = (long long)rint(ldexp(p[q], -e));
        }
        nat += wave_add128(go, cx, cy, m, lo, hi, qx, lane);
    }
};

// One lane per ray: walk_weighted (rt_sens_walk.h) with the caller's weights, into the accumulators.
template <typename T>
__global__ void k_backproject(Rows<T> rec, Args A, const double* w_line, const double* w_end, const unsigned long long* maxb,
                              unsigned long long* lo, unsigned long long* hi, unsigned long long* natomics) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < rec.R;
    const long R = rec.R;
    const long o = in ? rec.caller(k) : 0;
    long last = in ? rec.last(k) : -1;
    if (last >= rec.rec_rows) last = -1;                      // past the record: no reported traveltime, no weight
    const int e = rt::fix_exponent(__longlong_as_double((long long)*maxb));    // quantum 2^e: every partial is below 2^57 quanta
    // crossings that carry a weight: the first min(count, kmax)
    const bool line = A.has_line && w_line != nullptr;
    const int K = (line && last >= 0) ? min(count_crossings(rec, in ? k : 0, last, A.L), A.kmax) : 0;
    const double we = (w_end && last >= 0) ? w0(w_end[o]) : 0.0;
    const int lane = (int)(threadIdx.x & 63);
    FlushSink sink{lo, hi, A.F.qx, e, lane, 0};
    walk_weighted(rec, A, in ? k : 0, last, line, K, we, [&](int c) { return w0(w_line[(size_t)c * R + o]); }, sink);
    // one count per wave
    long long nat = sink.nat;
    for (int off = 1; off < 64; off <<= 1) nat += __shfl_xor(nat, off);
    if (lane == 0 && nat) atomicAdd(natomics, (unsigned long long)nat);
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
