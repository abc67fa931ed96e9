// wavefront.hip -- the reference's wavefront extraction (RT_bench.py:987-1026, 1043-1044) on the device, in two stages.
// Per ray (rtmi_isochrones, :987-1003): scipy's PchipInterpolator(t_ray, v_ray) of x, y and theta over the recorded
// traveltimes, evaluated at fixed traveltimes; one lane per ray.  Across rays (rtmi_wavefronts, :1005-1044): per traveltime,
// the isochrone points of the rays that reach it are sorted by y (np.argsort, :1016), PchipInterpolator x(y) is built through
// them (:1020), and its derivative at the points (:1021-1022), the tangent / normal angles (:1025-1026), |ray angle - normal
// angle| (:1032) and the interpolant on nfine equally spaced y (:1043-1044) are evaluated.  One lane per point; the sort is
// rocPRIM's radix sort through hipCUB (library code: this stage is a consumer of the hot path, not part of it).  Every
// traveltime of a call is handled in one pass -- the reference's animation (:1066-1102) re-does the whole extraction per
// frame, 45 times.  scipy's arithmetic is restated in rt_pchip.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_pchip.h"
#include "rt_rows.h"
#include "rtmi_host.h"

namespace {
// The per-ray stage: x, y, theta (:993) of every ray at the traveltimes `times`, out [ntimes][3][R] in the caller's ray order;
// NaN where the ray's record does not reach the traveltime.
template <typename T> __global__ void k_isochrone(Rows<T> rec, int ntimes, const double* times, double* out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rec.R) return;
    // rows 0..last_i of this ray (:993); a batch created with rec_rows < max_size holds only the first rec_rows of them
    const long n = rec.last_recorded(k) + 1;
    const size_t pitch = rec.pitch();
    const T* col = rec.row(0, k);
    auto tt = [&](long i) { return (double)col[(size_t)COL_T * rec.R + (size_t)i * pitch]; };
    const int qsel[3] = {COL_X, COL_Y, COL_TH};
    for (int it = 0; it < ntimes; it++) {
        const double t = times[it];
        double res[3] = {NAN, NAN, NAN};
        if (n >= 2 && tt(n - 1) >= t && t >= tt(0)) {   // np.max(t_ray) >= travel_time (:997)
            const long lo = rt::pchip_interval(tt, n, t);
            const double dx = tt(lo + 1) - tt(lo), s = t - tt(lo);
            for (int q = 0; q < 3; q++) {
                auto yy = [&](long i) { return (double)col[(size_t)qsel[q] * rec.R + (size_t)i * pitch]; };
                const double y0 = yy(lo), y1 = yy(lo + 1), slope = (y1 - y0) / dx;
                double d0, d1;
                if (n == 2) { d0 = d1 = slope; }
                else { d0 = rt::pchip_deriv(tt, yy, lo, n); d1 = rt::pchip_deriv(tt, yy, lo + 1, n); }
                res[q] = rt::pchip_cubic(dx, y0, slope, d0, d1).powers(s);
            }
        }
        for (int q = 0; q < 3; q++) out[((size_t)it * 3 + q) * rec.R + rec.caller(k)] = res[q];
    }
}

// All the kernels below work on a CHUNK of traveltimes at once (blockIdx.y = traveltime within the chunk): the reference's movie
// path (RT_bench.py:1066-1102) asks for 45 wavefronts of one trajectory set, frame after frame; here they are one pass.
// keys for the sort: y of the rays that reach the traveltime, +inf for the others (they sort last); counts the valid ones.
// vals: the item's index t*R + k.
__global__ void k_keys(const double* iso, long R, double* keys, int* vals, unsigned long long* count) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    bool ok = false;
    if (k < R) {
        const double y = iso[((size_t)t * 3 + 1) * R + k];                 // iso: [nt][3][R] = x, y, theta per traveltime
        ok = y == y;
        keys[(size_t)t * R + k] = ok ? y : HUGE_VAL;
        vals[(size_t)t * R + k] = (int)(t * R + k);
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count + t, (unsigned long long)__popcll(m));
}
// second sort key: the traveltime an item belongs to (a stable sort on it regroups the y-sorted items per traveltime)
__global__ void k_frame_keys(const int* vals, long R, long n, unsigned* fk) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) fk[j] = (unsigned)(vals[j] / R);
}
// sorted order -> ys, xs, angle, ray index rows of `nodes` ([nt][7][R]); NaN beyond the valid count
__global__ void k_gather(const double* iso, long R, const int* order, const unsigned long long* count, double* nodes) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j >= R) return;
    const bool ok = (unsigned long long)j < count[t];
    const long k = (long)order[(size_t)t * R + j] - t * R;
    const double* it = iso + (size_t)t * 3 * R;
    double* nd = nodes + (size_t)t * 7 * R;
    nd[j] = ok ? it[R + k] : NAN;                // y
    nd[R + j] = ok ? it[k] : NAN;                // x
    nd[2 * R + j] = ok ? it[2 * R + k] : NAN;    // ray angle
    nd[6 * R + j] = ok ? (double)k : NAN;        // ray index (caller's order)
}
// tie[t] (zeroed by the caller) = 1 when two neighbours of wavefront t's sorted points have the same y (-0.0 and +0.0 are the
// same): scipy refuses such a data set as a whole, so the whole wavefront gets no interpolant.  Every lane that sees a tie
// stores the same 1.
__global__ void k_ties(long R, const unsigned long long* count, const double* nodes_all, int* tie) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j + 1 >= (long)count[t]) return;               // count <= R
    const double* y = nodes_all + (size_t)t * 7 * R;
    if (y[j + 1] == y[j]) tie[t] = 1;
}
// derivative of the interpolant at its own points, angles (:1021-1026, :1032)
__global__ void k_nodes(long R, const unsigned long long* count, const int* tie, double* nodes_all, double* deriv_all) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    const long n = (long)count[t];
    if (j >= R) return;
    double* nodes = nodes_all + (size_t)t * 7 * R;
    double d = NAN, slope = NAN, normal = NAN, diff = NAN;
    if (j < n && n >= 2 && !tie[t]) {
        auto y = [=](long i) { return nodes[i]; };
        auto x = [=](long i) { return nodes[R + i]; };
        d = rt::pchip_deriv(y, x, j, n);
        slope = d;
        if (j == n - 1) {
            // PPoly.derivative() evaluated at the last breakpoint uses the last interval at its right end
            const double dx = y(n - 1) - y(n - 2), m = (x(n - 1) - x(n - 2)) / dx;
            slope = rt::pchip_cubic(dx, x(n - 2), m, rt::pchip_deriv(y, x, n - 2, n), d).deriv(dx);
        }
        const double tangent = M_PI / 2 - atan(slope);       // (:1025)
        normal = tangent - M_PI / 2;                          // (:1026)
        diff = fabs(nodes[2 * R + j] - normal);               // (:1032) with the ray angle of the SAME sorted point
    }
    deriv_all[(size_t)t * R + j] = d;
    nodes[3 * R + j] = slope;
    nodes[4 * R + j] = normal;
    nodes[5 * R + j] = diff;
}
// the interpolant on nfine equally spaced y between the first and the last point (:1043-1044, :1096-1097)
__global__ void k_fine(long R, const unsigned long long* count, const int* tie, const double* nodes_all, const double* deriv_all, int nfine,
                       double* fine_all) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const long t = blockIdx.y;
    if (q >= nfine) return;
    const long n = (long)count[t];
    const double* nodes = nodes_all + (size_t)t * 7 * R;
    const double* deriv = deriv_all + (size_t)t * R;
    double* fine = fine_all + (size_t)t * 2 * nfine;
    double xf = NAN, yf = NAN;
    if (n >= 2 && !tie[t]) {
        const double *y = nodes, *x = nodes + R;
        const double a = y[0], b = y[n - 1];
        const double step = (b - a) / (double)(nfine - 1);
        yf = q == nfine - 1 ? b : (double)q * step + a;                     // numpy.linspace
        const long lo = rt::pchip_interval([=](long i) { return y[i]; }, n, yf);
        const double dx = y[lo + 1] - y[lo], s = yf - y[lo], m = (x[lo + 1] - x[lo]) / dx;
        xf = rt::pchip_cubic(dx, x[lo], m, deriv[lo], deriv[lo + 1]).horner(s);       // Horner in (y - y_lo); PPoly sums the powers
    }
    fine[q] = xf;
    fine[nfine + q] = yf;
}
// The per-ray stage of a batch with its checks, reported under rtmi_isochrones' name: rec becomes the batch's record, *iso =
// [ntimes][3][R] fp64 on the device, one of mem's allocations, complete when this returns.
int isochrones_device(rtmi_batch* b, int32_t ntimes, const double* times, DevMem& mem, Recorded& rec, double** iso) {
    const char* who = "rtmi_isochrones";
    RTMI_ARG(b && times, "null");
    RTMI_ARG(ntimes > 0 && ntimes <= 4096, "ntimes must be in [1, 4096]");
    RTMI_RC(recorded(who, b, kRecOnDevice, 0, &rec));
    const rtmi_device_view& v = rec.v;
    double* dt = nullptr;
    RTMI_HIP(mem.get(iso, (size_t)ntimes * 3 * (size_t)v.R * sizeof(double)));
    RTMI_HIP(mem.get(&dt, ntimes * sizeof(double)));
    RTMI_HIP(hipMemcpy(dt, times, ntimes * sizeof(double), hipMemcpyHostToDevice));
    by_dtype(v.dtype, [&](auto t) {
        hipLaunchKernelGGL(k_isochrone<decltype(t)>, dim3((unsigned)((v.R + 127) / 128)), dim3(128), 0, nullptr, rows_of<decltype(t)>(v), (int)ntimes, dt, *iso);
    });
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipDeviceSynchronize());
    return RTMI_OK;
}
}  // namespace

RTMI_EXPORT int rtmi_isochrones(rtmi_batch* b, int32_t ntimes, const double* times, double* out) {
    const char* who = "rtmi_isochrones";
    RTMI_ARG(out, "null");
    DevMem mem;
    Recorded rec;
    double* d = nullptr;
    RTMI_RC(isochrones_device(b, ntimes, times, mem, rec, &d));
    RTMI_HIP(hipMemcpy(out, d, (size_t)ntimes * 3 * (size_t)rec.v.R * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_wavefronts(rtmi_batch* b, int32_t ntimes, const double* times, int32_t nfine, int64_t* count, double* nodes,
                                double* fine) {
    const char* who = "rtmi_wavefronts";
    RTMI_ARG(b && times && count && nodes, "null");
    RTMI_ARG(!(nfine < 0 || nfine == 1 || (nfine > 0 && !fine)), "nfine must be 0 or >= 2 (with a fine buffer)");
    RTMI_ARG(ntimes > 0 && ntimes <= 4096, "ntimes must be in [1, 4096]");
    Recorded rec;       // the stage below makes these checks too, under rtmi_isochrones' name
    RTMI_RC(recorded(who, b, 0, 0, &rec));
    DevMem mem;
    double* iso = nullptr;
    RTMI_RC(isochrones_device(b, ntimes, times, mem, rec, &iso));
    const long R = (long)rec.v.R;
    const hipStream_t st = nullptr;     // the batch's stream is idle after recorded(): everything below runs on the null stream
    // Traveltimes are processed in chunks of `tc` (all of them, unless that needs more than ~1 GB of work arrays: 92 bytes per
    // point): per chunk ONE stable radix sort of every point by y, one more by the traveltime it belongs to (which regroups the
    // y-sorted points per wavefront: each has exactly R of them, the rays that do not reach it at the end with y = +inf), the
    // PCHIP stage for all wavefronts at once, one copy to the host.
    const size_t Rz = (size_t)R;
    int tc = (int)std::max<size_t>(1, std::min<size_t>((size_t)ntimes, ((size_t)1 << 30) / (92 * Rz)));
    if (const char* e = getenv("RTMI_WF_CHUNK")) tc = std::max(1, std::min((int)ntimes, atoi(e)));   // tests: force several chunks
    while ((size_t)tc * Rz >= ((size_t)1 << 31)) tc /= 2;              // item indices are 32-bit
    const size_t N = (size_t)tc * Rz;
    double *keys = nullptr, *keys2 = nullptr, *dn = nullptr, *dd = nullptr, *df = nullptr;
    int *vals = nullptr, *vals2 = nullptr;
    unsigned *fk = nullptr, *fk2 = nullptr;
    unsigned long long* dcount = nullptr;
    int* dtie = nullptr;
    std::vector<unsigned long long> hcount;
    void* tmp = nullptr;
    size_t tmp1 = 0, tmp2 = 0;
    const dim3 blk(256);
    int fbits = 1;
    while ((1 << fbits) < tc) fbits++;
    try {
        hcount.resize((size_t)tc);
    } catch (const std::exception&) {
        return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_wavefronts: host allocation failed");
    }
    RTMI_HIP(mem.get(&keys, N * 8)); RTMI_HIP(mem.get(&keys2, N * 8));
    RTMI_HIP(mem.get(&vals, N * 4)); RTMI_HIP(mem.get(&vals2, N * 4));
    RTMI_HIP(mem.get(&fk, N * 4)); RTMI_HIP(mem.get(&fk2, N * 4));
    RTMI_HIP(mem.get(&dn, 7 * N * 8)); RTMI_HIP(mem.get(&dd, N * 8));
    RTMI_HIP(mem.get(&dcount, (size_t)tc * 8));
    RTMI_HIP(mem.get(&dtie, (size_t)tc * 4));
    if (nfine) RTMI_HIP(mem.get(&df, (size_t)tc * 2 * (size_t)nfine * 8));
    RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp1, keys, keys2, vals, vals2, (int)N, 0, 64, st));
    RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp2, fk, fk2, vals2, vals, (int)N, 0, fbits, st));
    RTMI_HIP(mem.get(&tmp, std::max(tmp1, tmp2)));
    for (int t0 = 0; t0 < ntimes; t0 += tc) {
        const int nt = std::min(tc, ntimes - t0);
        const size_t n = (size_t)nt * Rz;
        const double* iso_c = iso + (size_t)t0 * 3 * Rz;
        const dim3 grd(blocks(R).x, (unsigned)nt);
        RTMI_HIP(hipMemsetAsync(dcount, 0, (size_t)nt * 8, st));
        RTMI_HIP(hipMemsetAsync(dtie, 0, (size_t)nt * 4, st));
        hipLaunchKernelGGL(k_keys, grd, blk, 0, st, iso_c, R, keys, vals, dcount);
        RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp1, keys, keys2, vals, vals2, (int)n, 0, 64, st));           // every point by y
        if (nt > 1) {
            hipLaunchKernelGGL(k_frame_keys, blocks((long)n), blk, 0, st, vals2, R, (long)n, fk);
            RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp2, fk, fk2, vals2, vals, (int)n, 0, fbits, st));          // stable: regrouped per traveltime
        }
        const int* order = nt > 1 ? vals : vals2;
        hipLaunchKernelGGL(k_gather, grd, blk, 0, st, iso_c, R, order, dcount, dn);
        hipLaunchKernelGGL(k_ties, grd, blk, 0, st, R, dcount, dn, dtie);
        hipLaunchKernelGGL(k_nodes, grd, blk, 0, st, R, dcount, dtie, dn, dd);
        if (nfine) hipLaunchKernelGGL(k_fine, dim3(blocks(nfine).x, (unsigned)nt), blk, 0, st, R, dcount, dtie, dn, dd, (int)nfine, df);
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(hipMemcpyAsync(hcount.data(), dcount, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        RTMI_HIP(hipMemcpyAsync(nodes + (size_t)t0 * 7 * Rz, dn, 7 * n * 8, hipMemcpyDeviceToHost, st));
        if (nfine) RTMI_HIP(hipMemcpyAsync(fine + (size_t)t0 * 2 * nfine, df, (size_t)nt * 2 * (size_t)nfine * 8, hipMemcpyDeviceToHost, st));
        RTMI_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < nt; i++) count[t0 + i] = (int64_t)hcount[i];
    }
    return RTMI_OK;
}
