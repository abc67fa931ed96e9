// kirchhoff_hilbert.hip -- the Hilbert transform along the traces of a Kirchhoff handle, on the device and defined bit for bit
// (rtmi_hilbert_taps, rtmi_kirchhoff_hilbert, rtmi_kirchhoff_hilbert_dev, rtmi_debug_hilbert).  include/rtmi.h states the contract,
// rt_hilbert.h the taps and the definition as a host loop, DESIGN.md section 23 the layout, the floors and what was measured.
//   k_hilbert   out[k][i] = (add ? add[k][i] : +0) +- y[k][i],  y = H x[k] in the time domain, the taps ascending.
// One workgroup per trace; the trace lives in LDS (one copy, at most 16 384 samples = 128 KiB), the wrap-around is index arithmetic.
// A lane owns kR consecutive outputs of one source array and keeps the two windows its taps read in registers: from one tap to the
// next the window below the outputs moves down by one sample and the window above them up by one, so a tap costs two 8-byte LDS
// reads for kR outputs.  An even nt has only odd taps, and an output reads only samples of the other parity: the trace is stored
// de-interleaved, the even samples first, and "consecutive" means consecutive of one parity; an odd nt is one array with every tap.
// kR is odd: the windows of neighbouring lanes sit kR doubles apart, so the 32 lanes of a half-wave read 32 different even banks of
// the 64 (ds_read_b64: bank (a / 4) mod 64) -- no conflict, no padding; at an even nt no half-wave holds chunks of both arrays.  The sum of one output is never reassociated.
// Every subtract, product and add is a separate fp64 operation: __dsub_rn / __dmul_rn / __dadd_rn, and the unit is built with
// -ffp-contract=off like the rest of the library.
#include <type_traits>

#include "rt_hilbert.h"
#include "rt_kirchhoff.h"

namespace {

constexpr int kR = 9;                       // outputs of one lane; odd (the bank rule above)
constexpr int kMaxLanes = 1024;
constexpr int64_t kMaxNt = 16384;           // one copy of the trace in LDS: 128 KiB of gfx950's 160
static_assert(kR % 2 == 1, "an even kR makes the lanes' windows collide on a few banks");

__device__ __forceinline__ double lds_at(const double* base, unsigned byte) { return *(const double*)((const char*)base + byte); }

// x [N][nt]; add [N][nt] or NULL, may be out; out [N][nt], not x; taps c_1 .. c_K, K = (nt - 1) / 2 (rt_hilbert.h), not read
// when K = 0.  x and taps are written by nobody (__restrict__): the taps, at an index every lane shares, come by scalar loads.
__global__ void __launch_bounds__(kMaxLanes) k_hilbert(const double* __restrict__ x, const double* add, double* out,
                                                       const double* __restrict__ taps, int n, int negate) {
    extern __shared__ double tr[];          // even nt: [even samples | odd samples]; odd nt: the trace
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const bool even = (n & 1) == 0;
    const int L = even ? n / 2 : n;         // samples of one source array
    const size_t row = (size_t)blockIdx.x * (size_t)n;
    for (int i = tid; i < n; i += BS) tr[even ? (i >> 1) + (i & 1) * L : i] = x[row + i];
    __syncthreads();
    const int ntap = even ? n / 4 : (n - 1) / 2;          // the taps that are not zero: k = 2 t + 1 (even nt), k = t + 1 (odd nt)
    const int cs = even ? 2 : 1;
    const int CH = (L + kR - 1) / kR;                     // chunks of kR outputs per source array
    // even nt: the chunks of the odd outputs start at a lane that is a multiple of 32, so that no half-wave reads both arrays (the
    // two arrays' windows would meet on banks); the lanes between the two runs of chunks idle
    const int CH1 = even ? (CH + 31) / 32 * 32 : CH;      // the first chunk of the second array
    const int nchunks = even ? CH1 + CH : CH;
    for (int c = tid; c < nchunks; c += BS) {
        // even nt: half 0 the even outputs, which read the odd samples from one below (x[i - 1]) and from their own place
        // (x[i + 1]); half 1 the odd outputs, which read the even samples from their own place and from one above
        const int half = c >= CH1 ? 1 : 0;
        if (!half && c >= CH) continue;
        const int q0 = (c - half * CH1) * kR;             // the first output, counted within its array; q0 < L
        const int below = even ? 1 - half : 1, above = even ? half : 1;
        const unsigned start = (even ? (unsigned)(1 - half) * (unsigned)L : 0u) * 8u, end = start + (unsigned)L * 8u;
        // W[r] = the sample tap 0 of output q0 + r reads below it, V[r] the one above it; lo and hi: the bytes of the last read
        unsigned lo = start + (unsigned)(q0 - below < 0 ? L - 1 : q0 - below) * 8u;
        unsigned hi = start + (unsigned)(q0 + above >= L ? q0 + above - L : q0 + above) * 8u;
        const unsigned lo0 = lo;
        double W[kR], V[kR], acc[kR];
#pragma unroll
        for (int r = 0; r < kR; r++) {
            W[r] = lds_at(tr, lo);
            V[r] = lds_at(tr, hi);
            acc[r] = 0.0;
            if (r + 1 < kR) {
                lo += 8u; lo = lo == end ? start : lo;
                hi += 8u; hi = hi == end ? start : hi;
            }
        }
        lo = lo0;
        // tap t with s = t mod kR: output r reads W[(r - s) mod kR] and V[(r + s) mod kR]; the samples tap t + 1 needs besides
        // are read first and take the places of the two that tap t used last
        auto tap = [&](auto sc, double ck) {
            constexpr int s = decltype(sc)::value;
            lo = (lo == start ? end : lo) - 8u;
            hi += 8u; hi = hi == end ? start : hi;
            const double nl = lds_at(tr, lo), nh = lds_at(tr, hi);
#pragma unroll
            for (int r = 0; r < kR; r++)
                acc[r] = __dadd_rn(acc[r], __dmul_rn(ck, __dsub_rn(W[(r - s + kR) % kR], V[(r + s) % kR])));
            W[(kR - 1 - s) % kR] = nl;
            V[s] = nh;
        };
        // taps t0 .. t0 + count - 1, t0 a multiple of kR, count <= kR; a whole group's coefficients are loaded (scalar loads, the
        // index is the block's) before its first tap, so that the group waits for them once
        auto group = [&](int t0, int count) {
            double ck[kR];
#pragma unroll
            for (int s = 0; s < kR; s++) ck[s] = s < count ? taps[(t0 + s) * cs] : 0.0;
            __builtin_amdgcn_sched_barrier(0);            // the scheduler would sink each load to its tap, and each tap would wait
            if (count > 0) tap(std::integral_constant<int, 0>(), ck[0]);
            if (count > 1) tap(std::integral_constant<int, 1>(), ck[1]);
            if (count > 2) tap(std::integral_constant<int, 2>(), ck[2]);
            if (count > 3) tap(std::integral_constant<int, 3>(), ck[3]);
            if (count > 4) tap(std::integral_constant<int, 4>(), ck[4]);
            if (count > 5) tap(std::integral_constant<int, 5>(), ck[5]);
            if (count > 6) tap(std::integral_constant<int, 6>(), ck[6]);
            if (count > 7) tap(std::integral_constant<int, 7>(), ck[7]);
            if (count > 8) tap(std::integral_constant<int, 8>(), ck[8]);
        };
        static_assert(kR == 9, "group() spells out kR taps");
        int t0 = 0;
        for (; t0 + kR <= ntap; t0 += kR) group(t0, kR);
        if (t0 < ntap) group(t0, ntap - t0);
#pragma unroll
        for (int r = 0; r < kR; r++) {
            const int q = q0 + r;
            if (q < L) {
                const size_t at = row + (size_t)(even ? 2 * q + half : q);
                const double y = negate ? -acc[r] : acc[r];
                out[at] = add ? __dadd_rn(add[at], y) : y;
            }
        }
    }
}

int check_nt(const char* who, int64_t nt) {
    RTMI_ARG(nt <= kMaxNt, "nt must be <= 16384: a trace is held in LDS in one piece");
    return RTMI_OK;
}

// The launch: N traces of nt samples on the current device's null stream; ms, if not NULL, the kernel's event time (waits for it).
int launch(const char* who, const double* d_taps, int64_t N, int64_t nt, const double* d_x, const double* d_add, int negate, double* d_y,
           double* ms) {
    const int L = nt % 2 == 0 ? (int)(nt / 2) : (int)nt;
    const int CH = (L + kR - 1) / kR, chunks = nt % 2 == 0 ? (CH + 31) / 32 * 32 + CH : CH;      // as the kernel counts them
    const int lanes = std::min(kMaxLanes, std::max(64, (chunks + 63) / 64 * 64));
    const size_t lds = (size_t)nt * sizeof(double);
    if (lds > 65536) RTMI_HIP(hipFuncSetAttribute((const void*)k_hilbert, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxNt * sizeof(double))));
    EventMarks<2> ev;
    if (ms) {
        RTMI_HIP(ev.create());
        RTMI_HIP(ev.mark(0));
    }
    hipLaunchKernelGGL(k_hilbert, dim3((unsigned)N), dim3(lanes), lds, nullptr, d_x, d_add, d_y, d_taps, (int)nt, negate ? 1 : 0);
    RTMI_HIP(hipGetLastError());
    if (ms) {
        RTMI_HIP(ev.mark(1));
        RTMI_HIP(ev.wait(1));
        RTMI_HIP(ev.ms(0, 1, ms));
    }
    return RTMI_OK;
}

int upload_taps(const char* who, int64_t nt, double** d_taps) {
    const int64_t K = rt::hilbert_ntaps(nt);
    if (K < 1) return RTMI_OK;
    std::vector<double> t((size_t)K);
    rt::hilbert_taps(nt, t.data());
    RTMI_HIP(hipMalloc((void**)d_taps, (size_t)K * sizeof(double)));
    RTMI_HIP(hipMemcpy(*d_taps, t.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    return RTMI_OK;
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

}  // namespace

// The handle's taps go up at first use and stay until rtmi_kirchhoff_destroy.  The callers have checked the arguments, nt and the
// device.
int rtmi_internal_kirchhoff_hilbert_dev(rtmi_kirchhoff* k, const char* who, const double* d_x, const double* d_add, bool negate,
                                        double* d_y, double* ms) {
    if (!k->htaps) RTMI_RC(upload_taps(who, k->kp.nt, &k->htaps));
    return launch(who, k->htaps, k->kp.N, k->kp.nt, d_x, d_add, negate, d_y, ms);
}

int rtmi_internal_kirchhoff_hilbert_check(const rtmi_kirchhoff* k, const char* who) { return check_nt(who, k->kp.nt); }

RTMI_EXPORT int rtmi_hilbert_taps(int64_t n, double* taps) {
    const char* who = "rtmi_hilbert_taps";
    RTMI_ARG(taps, "null taps");
    RTMI_ARG(n >= 1, "n must be >= 1");
    rt::hilbert_taps(n, taps);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_hilbert(rtmi_kirchhoff* k, const double* x, double* y) {
    const char* who = "rtmi_kirchhoff_hilbert";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(x, "null x");
    RTMI_ARG(y, "null y");
    RTMI_RC(check_nt(who, k->kp.nt));
    RTMI_RC(check_device(k, who));
    const size_t bytes = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    DevMem mem;
    double *dx = nullptr, *dy = nullptr;
    for (double** p : {&dx, &dy})
        if (mem.get(p, bytes) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_kirchhoff_hilbert: hipMalloc failed");
    RTMI_HIP(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
    RTMI_RC(rtmi_internal_kirchhoff_hilbert_dev(k, who, dx, nullptr, false, dy, nullptr));
    RTMI_HIP(hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_hilbert_dev(rtmi_kirchhoff* k, const double* d_x, const double* d_add, int32_t negate, double* d_y) {
    const char* who = "rtmi_kirchhoff_hilbert_dev";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(d_x, "null d_x");
    RTMI_ARG(d_y, "null d_y");
    RTMI_RC(check_nt(who, k->kp.nt));
    const size_t bytes = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    RTMI_ARG(!overlap(d_x, d_y, bytes), "d_y may not be d_x or overlap it: every output reads the whole trace");
    RTMI_ARG(!d_add || d_add == d_y || !overlap(d_add, d_y, bytes), "d_add must be d_y itself or apart from it");
    RTMI_RC(check_device(k, who));
    RTMI_RC(check_device_pointer(k, who, d_x, bytes, "d_x"));
    if (d_add) RTMI_RC(check_device_pointer(k, who, d_add, bytes, "d_add"));
    RTMI_RC(check_device_pointer(k, who, d_y, bytes, "d_y"));
    RTMI_RC(rtmi_internal_kirchhoff_hilbert_dev(k, who, d_x, d_add, negate != 0, d_y, nullptr));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_debug_hilbert(const double* x, int64_t N, int64_t nt, const double* add, int32_t negate, double* y) {
    const char* who = "rtmi_debug_hilbert";
    RTMI_ARG(x, "null x");
    RTMI_ARG(y, "null y");
    RTMI_ARG(N >= 1 && N <= INT32_MAX, "N must be in 1 .. 2^31 - 1 (one block per trace)");
    RTMI_ARG(nt >= 1, "nt must be >= 1");
    RTMI_RC(check_nt(who, nt));
    const size_t bytes = (size_t)N * (size_t)nt * sizeof(double);
    DevMem mem;
    double *dx = nullptr, *dy = nullptr, *dt = nullptr;
    RTMI_HIP(mem.get(&dx, bytes));
    RTMI_HIP(mem.get(&dy, bytes));
    const int rc = upload_taps(who, nt, &dt);
    if (dt) mem.p.push_back(dt);
    RTMI_RC(rc);
    RTMI_HIP(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
    if (add) RTMI_HIP(hipMemcpy(dy, add, bytes, hipMemcpyHostToDevice));
    RTMI_RC(launch(who, dt, N, nt, dx, add ? dy : nullptr, negate, dy, nullptr));
    RTMI_HIP(hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
