// kirchhoff.hip -- Kirchhoff migration and modelling from traveltime tables (rtmi_kirchhoff_create / _migrate / _model /
// _destroy): the diffraction-stack operator pair L^T (traces -> image, optionally split into opening-angle bins) and L
// (reflectivity model -> traces), exact transposes of each other up to rounding.  include/rtmi.h states the operator; DESIGN.md
// section 14 the kernels and the fixed-point derivation.
//   L^T  one lane per image node, x fastest (table reads are coalesced).  The lane walks the traces in the caller's order and
//        adds into an fp64 register (no bins) or into its own column of an LDS array [bin][lane]: no atomics, one fixed order.
//        T, amp and theta of the source are kept while the source index does not change (a wave-uniform test).
//   L    one block per trace.  The trace's samples are two-word (128-bit) fixed-point accumulators in LDS; the lanes sweep the
//        nodes, round each contribution once to an integer number of quanta 2^scale_exp and add it with a returning 64-bit LDS
//        atomic (the carry into the high word is read off the returned old value: rt_fix128.h).  Integer sums
//        commute, so the result has the same bits in every schedule and trace order.  The block converts and stores its trace.
// The tables and the geometry live on the device in the handle; data and image cross the bus on every call.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt_fix128.h"
#include "rtmi_host.h"

namespace {

constexpr int kMaxBins = 32;
constexpr int kWindow = 4096;         // samples of a trace held in LDS at a time: 4096 x 16 B = 64 KiB
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct KArgs {
    const double *T, *amp, *theta;    // [P][nn] (amp, theta: NULL when absent)
    const int32_t *isrc, *irec;       // [N]
    const double* w;                  // [N]; ones when the caller gave none (a factor 1 changes no bit)
    long nn, N, nt;
    double t0, inv_dt, dopen, ntm1;   // ntm1 = nt - 1: floor(f) <= nt - 2 iff f < nt - 1
    int nb;
};

// What one (trace, node) pair reads and derives.  ok: the pair contributes (rtmi.h): every value read is finite, 0 <= j <= nt - 2
// and the bin is below nb.  A non-finite T makes tau, hence f, non-finite, and the range test fails; likewise theta and h.
struct Pair { bool ok; long j; double a, c; int b; };

template <bool AMP, bool BINS>
__device__ __forceinline__ Pair pair_of(const KArgs& A, double Ts, double Tr, double As, double Ar, double Hs, double Hr, double wk) {
    Pair p;
    const double tau = Ts + Tr;
    const double f = (tau - A.t0) * A.inv_dt;
    p.ok = f >= 0.0 && f < A.ntm1;
    const double jf = floor(f);
    p.a = f - jf;
    p.j = p.ok ? (long)jf : 0;
    p.c = wk;
    if (AMP) {
        p.ok = p.ok && fabs(As) < INFINITY && fabs(Ar) < INFINITY;
        p.c = (wk * As) * Ar;
    }
    p.b = 0;
    if (BINS) {
        const double d = Hs - Hr;
        const double h = 0.5 * fabs(d - kTwoPi * rint(d / kTwoPi));
        const double hb = floor(h / A.dopen);
        p.ok = p.ok && hb < (double)A.nb;
        p.b = p.ok ? (int)hb : 0;
    }
    return p;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// ------------------------------------------------------------------------------------------------------------ L^T
// image [nb][nn]; counts [gridDim.x]: the block's contributing pairs (plain stores, summed by the host).
template <bool AMP, bool BINS>
__global__ void k_migrate(KArgs A, const double* __restrict__ data, double* __restrict__ image, unsigned long long* __restrict__ counts) {
    extern __shared__ double acc[];                           // BINS: [nb][blockDim.x]
    __shared__ unsigned long long wcnt[4];
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long x0 = (long)blockIdx.x * BS + tid;
    const bool in = x0 < A.nn;
    const long x = in ? x0 : A.nn - 1;                        // lanes past the image read its last node and store nothing
    double sum = 0.0;
    if (BINS)
        for (int b = 0; b < A.nb; b++) acc[b * BS + tid] = 0.0;
    unsigned long long cnt = 0;
    int sprev = -1;
    double Ts = 0.0, As = 0.0, Hs = 0.0;
#pragma unroll 4
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform: a shot-ordered list re-reads the source rarely
            Ts = A.T[(size_t)s * A.nn + x];
            if (AMP) As = A.amp[(size_t)s * A.nn + x];
            if (BINS) Hs = A.theta[(size_t)s * A.nn + x];
            sprev = s;
        }
        const double Tr = A.T[(size_t)r * A.nn + x];
        const double Ar = AMP ? A.amp[(size_t)r * A.nn + x] : 0.0;
        const double Hr = BINS ? A.theta[(size_t)r * A.nn + x] : 0.0;
        const Pair p = pair_of<AMP, BINS>(A, Ts, Tr, As, Ar, Hs, Hr, wk);
        const double* d = data + (size_t)k * A.nt + p.j;      // j = 0 when the pair does not contribute: always in bounds
        const double d0 = d[0], d1 = d[1];
        const double v = p.c * (d0 + p.a * (d1 - d0));
        if (BINS) {
            if (p.ok) acc[p.b * BS + tid] += v;
        } else {
            sum += p.ok ? v : 0.0;                            // sum is never -0: adding +0 changes no bit
        }
        cnt += (p.ok && in) ? 1ull : 0ull;
    }
    if (in) {
        if (BINS)
            for (int b = 0; b < A.nb; b++) image[(size_t)b * A.nn + x] = acc[b * BS + tid];
        else
            image[x] = sum;
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------ L
// Sample i's accumulator is (lo[i], hi[i]) of rt_fix128.h.
// One block per trace; data [N][nt]; counts [N].  The trace is processed in windows of at most kWindow samples.
template <bool AMP, bool BINS>
__global__ void k_model(KArgs A, const double* __restrict__ m, int e, int W, double* __restrict__ data,
                        unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned long long fix[];               // lo [W], hi [W]
    __shared__ unsigned long long wcnt[4];
    unsigned long long* lo = fix;
    unsigned long long* hi = fix + W;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long k = blockIdx.x;
    const int s = A.isrc[k], r = A.irec[k];
    const double wk = A.w[k];
    const double* Tsp = A.T + (size_t)s * A.nn;
    const double* Trp = A.T + (size_t)r * A.nn;
    const double* Asp = AMP ? A.amp + (size_t)s * A.nn : nullptr;
    const double* Arp = AMP ? A.amp + (size_t)r * A.nn : nullptr;
    const double* Hsp = BINS ? A.theta + (size_t)s * A.nn : nullptr;
    const double* Hrp = BINS ? A.theta + (size_t)r * A.nn : nullptr;
    unsigned long long cnt = 0;
    for (long j0 = 0; j0 < A.nt; j0 += W) {
        const long j1 = (j0 + W < A.nt) ? j0 + W : A.nt;      // the window [j0, j1)
        for (int i = tid; i < W; i += BS) { lo[i] = rt::kFixBias; hi[i] = 0ull; }
        __syncthreads();
#pragma unroll 2
        for (long x = tid; x < A.nn; x += BS) {
            const Pair p = pair_of<AMP, BINS>(A, Tsp[x], Trp[x], AMP ? Asp[x] : 0.0, AMP ? Arp[x] : 0.0, BINS ? Hsp[x] : 0.0,
                                              BINS ? Hrp[x] : 0.0, wk);
            if (!p.ok) continue;
            if (j0 == 0) cnt++;
            if (p.j + 1 < j0 || p.j >= j1) continue;
            const double cm = p.c * m[(size_t)p.b * A.nn + x];
            if (!(fabs(cm) < INFINITY)) continue;             // a non-finite model value contributes nothing
            const double v0 = cm * (1.0 - p.a), v1 = cm * p.a;
            if (p.j >= j0) (void)rt::add128(lo, hi, (int)(p.j - j0), (long long)rint(ldexp(v0, -e)));
            if (p.j + 1 < j1) (void)rt::add128(lo, hi, (int)(p.j + 1 - j0), (long long)rint(ldexp(v1, -e)));
        }
        __syncthreads();
        for (long i = tid; i < j1 - j0; i += BS) data[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(lo[i], hi[i]), e);
        __syncthreads();
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[k] = t;
    }
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct rtmi_kirchhoff {
    rtmi_kirchhoff_params kp{};
    int device = 0, nb = 1;
    size_t nn = 0;
    double max_w = 1.0, max_amp = 1.0;        // over finite values; the order-independent bound of the fixed-point scale
    double *T = nullptr, *amp = nullptr, *theta = nullptr, *w = nullptr, *data = nullptr, *image = nullptr;
    int32_t *isrc = nullptr, *irec = nullptr;
    unsigned long long* counts = nullptr;     // max(N, migrate's blocks)
    size_t ncounts = 0;
    ~rtmi_kirchhoff() {
        for (void* p : {(void*)T, (void*)amp, (void*)theta, (void*)w, (void*)data, (void*)image, (void*)isrc, (void*)irec, (void*)counts})
            if (p) (void)hipFree(p);
    }
    KArgs args() const {
        return KArgs{T, amp, theta, isrc, irec, w, (long)nn, (long)kp.N, (long)kp.nt, kp.t0, 1.0 / kp.dt, kp.dopen,
                     (double)(kp.nt - 1), nb};
    }
};

namespace {

int migrate_block(int nb) { return nb > 16 ? 128 : 256; }    // [bin][lane] fp64 in LDS stays within 32 KiB

int check_device(const rtmi_kirchhoff* k, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == k->device, "the calling thread's current device is not the handle's");
    return RTMI_OK;
}

int read_counts(const rtmi_kirchhoff* k, size_t n, int64_t* total, const char* who) {
    std::vector<unsigned long long> h(n);
    RTMI_HIP(hipMemcpy(h.data(), k->counts, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long t = 0;
    for (unsigned long long v : h) t += v;
    *total = (int64_t)t;
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_create(const rtmi_kirchhoff_params* kp, const double* T, const double* amp, const double* theta,
                                      const int32_t* isrc, const int32_t* irec, const double* w, rtmi_kirchhoff** out) {
    const char* who = "rtmi_kirchhoff_create";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_ARG(kp, "null kp");
    RTMI_ARG(T, "null T");
    RTMI_ARG(isrc, "null isrc");
    RTMI_ARG(irec, "null irec");
    RTMI_ARG(kp->nx >= 1, "nx must be >= 1");
    RTMI_ARG(kp->ny >= 1, "ny must be >= 1");
    RTMI_ARG(kp->P >= 1, "P must be >= 1");
    RTMI_ARG(kp->N >= 1, "N must be >= 1");
    RTMI_ARG(kp->nt >= 2, "nt must be >= 2");
    RTMI_ARG(kp->nx <= (1ll << 31) && kp->ny <= (1ll << 31) && kp->nx * kp->ny <= (1ll << 31), "nx ny must be <= 2^31");
    RTMI_ARG(kp->P <= INT32_MAX, "P must fit the int32 indices");
    RTMI_ARG(kp->N <= INT32_MAX, "N must be below 2^31 (one block per trace)");
    RTMI_ARG(std::isfinite(kp->dt) && kp->dt > 0.0, "dt must be finite and > 0");
    RTMI_ARG(std::isfinite(kp->t0), "t0 must be finite");
    RTMI_ARG(kp->nbin >= 0 && kp->nbin <= kMaxBins, "nbin must be in 0..32");
    if (kp->nbin > 0) {
        RTMI_ARG(theta, "nbin > 0 needs theta");
        RTMI_ARG(std::isfinite(kp->dopen) && kp->dopen > 0.0, "dopen must be finite and > 0");
    }
    for (int64_t k = 0; k < kp->N; k++) {
        RTMI_ARG(isrc[k] >= 0 && isrc[k] < kp->P, "isrc has an index outside [0, P)");
        RTMI_ARG(irec[k] >= 0 && irec[k] < kp->P, "irec has an index outside [0, P)");
    }
    double max_w = 1.0;
    if (w) {
        max_w = 0.0;
        for (int64_t k = 0; k < kp->N; k++) {
            RTMI_ARG(std::isfinite(w[k]), "w has a value that is not finite");
            max_w = std::fmax(max_w, std::fabs(w[k]));
        }
    }
    const size_t nn = (size_t)kp->nx * (size_t)kp->ny, P = (size_t)kp->P, N = (size_t)kp->N, nt = (size_t)kp->nt;
    const int nb = kp->nbin > 0 ? kp->nbin : 1;
    double max_amp = 1.0;
    if (amp) {
        max_amp = 0.0;
        for (size_t i = 0; i < P * nn; i++)
            if (std::isfinite(amp[i])) max_amp = std::fmax(max_amp, std::fabs(amp[i]));
    }
    rtmi_kirchhoff* k = new (std::nothrow) rtmi_kirchhoff;
    if (!k) return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_kirchhoff_create: out of host memory");
    k->kp = *kp;
    k->nb = nb;
    k->nn = nn;
    k->max_w = max_w;
    k->max_amp = max_amp;
    const bool bins = kp->nbin > 0;
    const size_t mblocks = (nn + migrate_block(nb) - 1) / migrate_block(nb);
    k->ncounts = N > mblocks ? N : mblocks;
    auto fail = [&](int code, const std::string& msg) {
        delete k;
        return rtmi_internal_fail(code, (std::string(who) + ": " + msg).c_str());
    };
    hipError_t e = hipGetDevice(&k->device);
    if (e != hipSuccess) return fail(RTMI_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    auto get = [&](void** p, size_t bytes) { return hipMalloc(p, bytes); };
    struct { void** p; size_t bytes; const void* src; } bufs[] = {
        {(void**)&k->T, P * nn * sizeof(double), T},
        {(void**)&k->amp, amp ? P * nn * sizeof(double) : 0, amp},
        {(void**)&k->theta, bins ? P * nn * sizeof(double) : 0, theta},
        {(void**)&k->isrc, N * sizeof(int32_t), isrc},
        {(void**)&k->irec, N * sizeof(int32_t), irec},
        {(void**)&k->w, N * sizeof(double), nullptr},
        {(void**)&k->data, N * nt * sizeof(double), nullptr},
        {(void**)&k->image, (size_t)nb * nn * sizeof(double), nullptr},
        {(void**)&k->counts, k->ncounts * sizeof(unsigned long long), nullptr},
    };
    for (auto& b : bufs) {
        if (!b.bytes) continue;
        e = get(b.p, b.bytes);
        if (e != hipSuccess) return fail(RTMI_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
        if (b.src) {
            e = hipMemcpy(*b.p, b.src, b.bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(RTMI_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
        }
    }
    std::vector<double> ones;
    if (!w) ones.assign(N, 1.0);
    e = hipMemcpy(k->w, w ? w : ones.data(), N * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(RTMI_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    *out = k;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_migrate(rtmi_kirchhoff* k, const double* data, double* image, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_migrate";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(data, "null data");
    RTMI_ARG(image, "null image");
    RTMI_RC(check_device(k, who));
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn;
    const double t_up = now_ms();
    RTMI_HIP(hipMemcpy(k->data, data, N * nt * sizeof(double), hipMemcpyHostToDevice));
    const double upload_ms = now_ms() - t_up;
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const int BS = migrate_block(k->nb);
    const dim3 grid((unsigned)((nn + BS - 1) / BS)), blk(BS);
    const bool bins = k->kp.nbin > 0, has_amp = k->amp != nullptr;
    const size_t lds = bins ? (size_t)k->nb * BS * sizeof(double) : 0;
    const KArgs A = k->args();
    RTMI_HIP(ev.mark(0));
    if (has_amp && bins) hipLaunchKernelGGL((k_migrate<true, true>), grid, blk, lds, nullptr, A, k->data, k->image, k->counts);
    else if (has_amp) hipLaunchKernelGGL((k_migrate<true, false>), grid, blk, lds, nullptr, A, k->data, k->image, k->counts);
    else if (bins) hipLaunchKernelGGL((k_migrate<false, true>), grid, blk, lds, nullptr, A, k->data, k->image, k->counts);
    else hipLaunchKernelGGL((k_migrate<false, false>), grid, blk, lds, nullptr, A, k->data, k->image, k->counts);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    RTMI_HIP(hipMemcpy(image, k->image, (size_t)k->nb * nn * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->upload_ms = upload_ms;
        st->pairs = (int64_t)(N * nn);
        RTMI_RC(read_counts(k, grid.x, &st->contributing, who));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_model(rtmi_kirchhoff* k, const double* model, double* data, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_model";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(model, "null model");
    RTMI_ARG(data, "null data");
    RTMI_RC(check_device(k, who));
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn, nm = (size_t)k->nb * nn;
    // the quantum: |contribution| <= max|w| max|amp|^2 max|m| = f 2^ex with f in [0.5, 1), so it is below 2^57 quanta 2^(ex - 57)
    double max_m = 0.0;
    for (size_t i = 0; i < nm; i++)
        if (std::isfinite(model[i])) max_m = std::fmax(max_m, std::fabs(model[i]));
    const double bound = (k->max_w * k->max_amp) * k->max_amp * max_m;
    const int e = std::isfinite(bound) ? rt::fix_exponent(bound) : 1025 - rt::kFixBits;
    const double t_up = now_ms();
    RTMI_HIP(hipMemcpy(k->image, model, nm * sizeof(double), hipMemcpyHostToDevice));
    const double upload_ms = now_ms() - t_up;
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const int W = (int)(nt < (size_t)kWindow ? nt : (size_t)kWindow);
    const dim3 grid((unsigned)N), blk(256);
    const size_t lds = (size_t)W * 2 * sizeof(unsigned long long);
    const bool bins = k->kp.nbin > 0, has_amp = k->amp != nullptr;
    const KArgs A = k->args();
    RTMI_HIP(ev.mark(0));
    if (has_amp && bins) hipLaunchKernelGGL((k_model<true, true>), grid, blk, lds, nullptr, A, k->image, e, W, k->data, k->counts);
    else if (has_amp) hipLaunchKernelGGL((k_model<true, false>), grid, blk, lds, nullptr, A, k->image, e, W, k->data, k->counts);
    else if (bins) hipLaunchKernelGGL((k_model<false, true>), grid, blk, lds, nullptr, A, k->image, e, W, k->data, k->counts);
    else hipLaunchKernelGGL((k_model<false, false>), grid, blk, lds, nullptr, A, k->image, e, W, k->data, k->counts);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    RTMI_HIP(hipMemcpy(data, k->data, N * nt * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->upload_ms = upload_ms;
        st->pairs = (int64_t)(N * nn);
        st->scale_exp = e;
        RTMI_RC(read_counts(k, N, &st->contributing, who));
    }
    return RTMI_OK;
}

RTMI_EXPORT void rtmi_kirchhoff_destroy(rtmi_kirchhoff* k) { delete k; }
