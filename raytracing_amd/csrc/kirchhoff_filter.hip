// kirchhoff_filter.hip -- a linear convolution along the traces of a Kirchhoff handle with the caller's taps, and its transpose,
// on the device and defined bit for bit (rtmi_half_derivative_taps, rtmi_kirchhoff_set_filter, rtmi_kirchhoff_filter,
// rtmi_kirchhoff_filter_dev).  include/rtmi.h states the contract, rt_filter.h the definition as a host loop and the
// half-derivative taps, DESIGN.md section 25 the layout, the floors and what was measured.
//   k_trace_filter<false>   y[n][i] = sum over k ascending of fl(f[k] x[n][i - k + o])       F
//   k_trace_filter<true>    y[n][i] = sum over k ascending of fl(f[k] x[n][i + k - o])       F^T
// One workgroup per trace; the trace lives in LDS between the zeros that stand for the samples outside it (L - 1 - o below and o
// above for F, o below and L - 1 - o above for F^T, and one more on the side the window moves to), so that tap k of output i
// reads p[i + L - k] (F) or p[i + k] (F^T) with no range test: the taps are finite, and a sum that starts at +0.0 is changed in
// no bit by adding +-0.0.  A lane owns kR consecutive outputs and keeps the window its taps read in registers: from one tap to the
// next the window moves by one sample (down for F, up for F^T), so a tap costs one 8-byte LDS read and 2 kR fp64 operations for
// kR outputs.  kR is odd: the windows of neighbouring
// lanes sit kR doubles apart, so the 32 lanes of a half-wave read 32 different even banks of the 64 (ds_read_b64: bank (a / 4)
// mod 64) -- no conflict, no padding between lanes.  The sum of one output runs over k ascending and is never reassociated; only
// the blocking over outputs is the kernel's.  Every product and add is a separate fp64 operation: __dmul_rn / __dadd_rn, and the
// unit is built with -ffp-contract=off like the rest of the library.
#include <type_traits>

#include "rt_filter.h"
#include "rt_kirchhoff.h"

namespace {

constexpr int kR = 9;                       // outputs of one lane; odd (the bank rule above)
constexpr int kMaxLanes = 1024;
constexpr int64_t kMaxNt = rt::kFilterMaxNt, kMaxTaps = rt::kFilterMaxTaps;
static_assert(kR % 2 == 1, "an even kR makes the lanes' windows collide on a few banks");

// the doubles of one trace in LDS: the trace, its L - 1 zeros, kR - 1 more above for the window of the last, partial chunk, and
// one for the read behind the last tap (below for F, above for F^T), which no output uses
constexpr size_t lds_doubles(int64_t nt, int64_t L) { return (size_t)(nt + L - 1 + kR); }
static_assert(lds_doubles(kMaxNt, kMaxTaps) * sizeof(double) <= 160 * 1024, "the longest trace and filter fit gfx950's LDS");

__device__ __forceinline__ double lds_at(const double* base, unsigned byte) { return *(const double*)((const char*)base + byte); }

// x [N][nt]; out [N][nt], not x; taps f[0 .. L), L >= 1, origin o in [0, L).  x and taps are written by nobody (__restrict__):
// the taps, at an index every lane shares, come by scalar loads.
template <bool TRANSPOSE>
__global__ void __launch_bounds__(kMaxLanes) k_trace_filter(const double* __restrict__ x, double* __restrict__ out,
                                                           const double* __restrict__ taps, int n, int L, int o) {
    extern __shared__ double p[];           // [below zeros | the trace | above zeros]
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const int below = TRANSPOSE ? o : L - o;
    const int total = n + L - 1 + kR;                         // lds_doubles
    const size_t row = (size_t)blockIdx.x * (size_t)n;
    for (int i = tid; i < total; i += BS) {
        const int j = i - below;
        p[i] = j >= 0 && j < n ? x[row + (size_t)j] : 0.0;
    }
    __syncthreads();
    const int nchunks = (n + kR - 1) / kR;
    for (int c = tid; c < nchunks; c += BS) {
        const int q0 = c * kR;                                // the first output of the chunk; q0 < n
        // W[(r -+ s) mod kR] = the sample tap t0 + s of output q0 + r reads; at: the bytes of the last read
        unsigned at = (unsigned)(TRANSPOSE ? q0 : q0 + L) * 8u;
        double W[kR], acc[kR];
#pragma unroll
        for (int r = 0; r < kR; r++) {
            W[r] = lds_at(p, at + 8u * (unsigned)r);          // tap 0 of output q0 + r; the last index is q0 + L + kR - 1 < total
            acc[r] = 0.0;
        }
        if (TRANSPOSE) at += 8u * (unsigned)(kR - 1);
        // tap t with s = t mod kR: output r reads W[(r - s) mod kR] (F) or W[(r + s) mod kR] (F^T); the sample tap t + 1 needs
        // besides is read first and takes the place of the one that tap t used last.  The read behind the last tap is p[q0] (F)
        // or p[q0 + kR - 1 + L] < total (F^T)
        auto tap = [&](auto sc, double fk) {
            constexpr int s = decltype(sc)::value;
            at = TRANSPOSE ? at + 8u : at - 8u;
            const double nw = lds_at(p, at);
#pragma unroll
            for (int r = 0; r < kR; r++)
                acc[r] = __dadd_rn(acc[r], __dmul_rn(fk, W[TRANSPOSE ? (r + s) % kR : (r - s + kR) % kR]));
            W[TRANSPOSE ? s : (kR - 1 - s) % kR] = nw;
        };
        // taps t0 .. t0 + count - 1, t0 a multiple of kR, count <= kR; a whole group's coefficients are loaded (scalar loads, the
        // index is the block's) before its first tap, so that the group waits for them once
        auto group = [&](int t0, int count) {
            double fk[kR];
#pragma unroll
            for (int s = 0; s < kR; s++) fk[s] = s < count ? taps[t0 + s] : 0.0;
            __builtin_amdgcn_sched_barrier(0);            // the scheduler would sink each load to its tap, and each tap would wait
            if (count > 0) tap(std::integral_constant<int, 0>(), fk[0]);
            if (count > 1) tap(std::integral_constant<int, 1>(), fk[1]);
            if (count > 2) tap(std::integral_constant<int, 2>(), fk[2]);
            if (count > 3) tap(std::integral_constant<int, 3>(), fk[3]);
            if (count > 4) tap(std::integral_constant<int, 4>(), fk[4]);
            if (count > 5) tap(std::integral_constant<int, 5>(), fk[5]);
            if (count > 6) tap(std::integral_constant<int, 6>(), fk[6]);
            if (count > 7) tap(std::integral_constant<int, 7>(), fk[7]);
            if (count > 8) tap(std::integral_constant<int, 8>(), fk[8]);
        };
        static_assert(kR == 9, "group() spells out kR taps");
        int t0 = 0;
        for (; t0 + kR <= L; t0 += kR) group(t0, kR);
        if (t0 < L) group(t0, L - t0);
#pragma unroll
        for (int r = 0; r < kR; r++)
            if (q0 + r < n) out[row + (size_t)(q0 + r)] = acc[r];
    }
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

template <bool TRANSPOSE>
int launch_one(const char* who, int lanes, size_t lds, int64_t N, const double* d_x, double* d_y, const double* d_taps, int nt, int L, int o) {
    if (lds > 65536)
        RTMI_HIP(hipFuncSetAttribute((const void*)k_trace_filter<TRANSPOSE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(lds_doubles(kMaxNt, kMaxTaps) * sizeof(double))));
    hipLaunchKernelGGL(k_trace_filter<TRANSPOSE>, dim3((unsigned)N), dim3(lanes), lds, nullptr, d_x, d_y, d_taps, nt, L, o);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

}  // namespace

// The launch: the handle's N traces of nt samples on the current device's null stream; ms, if not NULL, the kernel's event time
// (waits for it).  The callers have checked that a filter is set, the arguments and the device.
int rtmi_internal_kirchhoff_filter_dev(rtmi_kirchhoff* k, const char* who, const double* d_x, bool transpose, double* d_y, double* ms) {
    const int64_t nt = k->kp.nt;
    const int chunks = (int)((nt + kR - 1) / kR);
    const int lanes = std::min(kMaxLanes, std::max(64, (chunks + 63) / 64 * 64));
    const size_t lds = lds_doubles(nt, k->fL) * sizeof(double);
    EventMarks<2> ev;
    if (ms) {
        RTMI_HIP(ev.create());
        RTMI_HIP(ev.mark(0));
    }
    if (transpose) RTMI_RC(launch_one<true>(who, lanes, lds, k->kp.N, d_x, d_y, k->ftaps, (int)nt, k->fL, k->forigin));
    else RTMI_RC(launch_one<false>(who, lanes, lds, k->kp.N, d_x, d_y, k->ftaps, (int)nt, k->fL, k->forigin));
    if (ms) {
        RTMI_HIP(ev.mark(1));
        RTMI_HIP(ev.wait(1));
        RTMI_HIP(ev.ms(0, 1, ms));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_half_derivative_taps(int64_t L, double dt, double* taps) {
    const char* who = "rtmi_half_derivative_taps";
    RTMI_ARG(taps, "null taps");
    RTMI_ARG(L >= 1, "L must be >= 1");
    RTMI_ARG(std::isfinite(dt) && dt > 0.0, "dt must be finite and > 0");
    rt::half_derivative_taps(L, dt, taps);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_set_filter(rtmi_kirchhoff* k, const double* taps, int64_t L, int64_t origin) {
    const char* who = "rtmi_kirchhoff_set_filter";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(L >= 0 && L <= kMaxTaps, "L must be in 0 .. 2048");
    if (L == 0) {
        RTMI_RC(check_device(k, who));
        if (k->ftaps) RTMI_HIP(hipFree(k->ftaps));
        k->ftaps = nullptr;
        k->fL = k->forigin = 0;
        return RTMI_OK;
    }
    RTMI_ARG(taps, "null taps");
    RTMI_ARG(origin >= 0 && origin < L, "origin must be in [0, L)");
    for (int64_t i = 0; i < L; i++) RTMI_ARG(std::isfinite(taps[i]), "taps has a value that is not finite");
    RTMI_ARG(k->kp.nt <= kMaxNt, "nt must be <= 16384: a trace and the filter's zeros are held in LDS in one piece");
    RTMI_RC(check_device(k, who));
    double* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)L * sizeof(double)) != hipSuccess)
        return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_kirchhoff_set_filter: hipMalloc failed");
    const hipError_t e = hipMemcpy(d, taps, (size_t)L * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        RTMI_HIP(e);
    }
    if (k->ftaps) (void)hipFree(k->ftaps);                // a second call replaces the first
    k->ftaps = d;
    k->fL = (int)L;
    k->forigin = (int)origin;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_filter(rtmi_kirchhoff* k, const double* x, int32_t transpose, double* y) {
    const char* who = "rtmi_kirchhoff_filter";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(x, "null x");
    RTMI_ARG(y, "null y");
    if (!k->ftaps) return rtmi_internal_fail(RTMI_ERR_STATE, "rtmi_kirchhoff_filter: no filter is set (rtmi_kirchhoff_set_filter)");
    RTMI_RC(check_device(k, who));
    const size_t bytes = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    DevMem mem;
    double *dx = nullptr, *dy = nullptr;
    for (double** p : {&dx, &dy})
        if (mem.get(p, bytes) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_kirchhoff_filter: hipMalloc failed");
    RTMI_HIP(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
    RTMI_RC(rtmi_internal_kirchhoff_filter_dev(k, who, dx, transpose != 0, dy, nullptr));
    RTMI_HIP(hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_filter_dev(rtmi_kirchhoff* k, const double* d_x, int32_t transpose, double* d_y) {
    const char* who = "rtmi_kirchhoff_filter_dev";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(d_x, "null d_x");
    RTMI_ARG(d_y, "null d_y");
    if (!k->ftaps) return rtmi_internal_fail(RTMI_ERR_STATE, "rtmi_kirchhoff_filter_dev: no filter is set (rtmi_kirchhoff_set_filter)");
    const size_t bytes = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    RTMI_ARG(!overlap(d_x, d_y, bytes), "d_y may not be d_x or overlap it: every output reads L samples of the trace");
    RTMI_RC(check_device(k, who));
    RTMI_RC(check_device_pointer(k, who, d_x, bytes, "d_x"));
    RTMI_RC(check_device_pointer(k, who, d_y, bytes, "d_y"));
    RTMI_RC(rtmi_internal_kirchhoff_filter_dev(k, who, d_x, transpose != 0, d_y, nullptr));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    return RTMI_OK;
}
