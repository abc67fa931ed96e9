// rt_kirchhoff.h -- what the Kirchhoff units share (kirchhoff.hip: the migrate / model kernel pair of every kind of handle and its
// one launch path; kirchhoff_aa.hip: the anti-aliased handle, its bank filter and level sum; kirchhoff_lsqr.hip: least-squares
// migration over any handle): the kernel arguments, one (trace, node) pair's arithmetic, the arrivals of a table at a node and
// their phase, a block's count, the handle, its argument checks and uploads.  Everything but the handle and
// the cross-unit entries is in an anonymous namespace: each unit gets its own copy, as with rtmi_host.h.  DESIGN.md sections 14,
// 19, 20, 21, 23 and 25.
#pragma once
#include <hip/hip_runtime.h>

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
constexpr int kMaxLev = RTMI_KIRCHHOFF_MAX_LEVELS;
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

// What the kernels of an anti-aliased handle take besides (rtmi_kirchhoff_create_aa; the others take an empty struct in its place).
struct AAArgs {
    const double* pt;              // [P][K][nn]
    double asrc, arec, amid;
    double thr[kMaxLev - 1];       // (double)hw[l] for l < nlev - 1, +inf from there on: the level is the number of thresholds below sl
    long lstride, cstride;         // doubles from one level to the next (channels N nt) and from channel 0 to channel 1 (N nt)
    int nlev;
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

// The block's sum of cnt into counts[index] (a plain store; the host sums the blocks).  Blocks of at most 512 lanes.
__device__ __forceinline__ void block_count_to(unsigned long long* counts, long index, unsigned long long cnt) {
    __shared__ unsigned long long wcnt[8];
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[index] = t;
    }
}

// kmah on the device: the caustic count mod 4 as int8, -1 where the table's value is not a finite non-negative integer.
constexpr int8_t kBadKmah = -1;

// The K arrivals of one table at one node.  Absent columns are never read.
template <int K> struct Arr { double T[K], A[K], H[K]; int m[K]; };

template <int K, bool AMP, bool BINS, bool PHASE>
__device__ __forceinline__ void load_arr(const KArgs& A, const int8_t* __restrict__ kmah, size_t at, Arr<K>& o) {
#pragma unroll
    for (int i = 0; i < K; i++) {
        const size_t q = at + (size_t)i * A.nn;
        o.T[i] = A.T[q];
        o.A[i] = AMP ? A.amp[q] : 0.0;
        o.H[i] = BINS ? A.theta[q] : 0.0;
        o.m[i] = PHASE ? (int)kmah[q] : 0;
    }
}

// The phase of a pair from its two counts: valid iff neither is kBadKmah; q = (ms + mr) mod 4 picks the channel (odd: 1) and the
// sign (q = 1, 2: minus), rtmi.h's table.
struct Phase { bool valid, odd, neg; };
__device__ __forceinline__ Phase phase_of(int ms, int mr) {
    const int q = ms + mr;
    return Phase{(ms | mr) >= 0, (q & 1) != 0, ((q + 1) & 2) != 0};
}

}  // namespace

struct rtmi_kirchhoff {
    rtmi_kirchhoff_params kp{};
    int device = 0, nb = 1;
    int karr = 0;                             // 0: rtmi_kirchhoff_create's handle; K >= 1: create_multi's, tables [P][K][nn]
    size_t nn = 0;
    double max_w = 1.0, max_amp = 1.0;        // over finite values; the order-independent bound of the fixed-point scale
    double *T = nullptr, *amp = nullptr, *theta = nullptr, *w = nullptr, *data = nullptr, *image = nullptr;
    int32_t *isrc = nullptr, *irec = nullptr;
    int8_t* kmah = nullptr;                   // multi: [P][K][nn], the count mod 4 or kBadKmah; NULL without kmah
    unsigned long long* counts = nullptr;     // max(N, migrate's blocks)
    size_t ncounts = 0;
    unsigned long long* red = nullptr;        // kRedWords words a reduction leaves its result in (k_absmax_finite, kirchhoff_lsqr.hip)
    int cus = 1;                              // the device's compute units: the grid-stride kernels launch a small multiple of it
    // rtmi_kirchhoff_create_aa's handle (nlev >= 1; 0 on every other handle): data is [nlev][channels][N][nt], level 0 the
    // caller's channels, levels 1 .. nlev - 1 the bank of migrate2 and, in model2, the spreads of every level
    int nlev = 0;
    int hw[RTMI_KIRCHHOFF_MAX_LEVELS] = {};
    double asrc = 0.0, arec = 0.0, amid = 0.0;
    double* pt = nullptr;                     // [P][K][nn]
    double* htaps = nullptr;                  // the Hilbert transform's taps for nt (rt_hilbert.h), uploaded at its first use
    double* ftaps = nullptr;                  // rtmi_kirchhoff_set_filter's taps f[0 .. fL), NULL with no filter set (rt_filter.h)
    int fL = 0, forigin = 0;
    ~rtmi_kirchhoff() {
        for (void* p : {(void*)T, (void*)amp, (void*)theta, (void*)w, (void*)data, (void*)image, (void*)isrc, (void*)irec, (void*)kmah, (void*)counts,
                        (void*)pt, (void*)red, (void*)htaps, (void*)ftaps})
            if (p) (void)hipFree(p);
    }
    KArgs args() const {
        return KArgs{T, amp, theta, isrc, irec, w, (long)nn, (long)kp.N, (long)kp.nt, kp.t0, 1.0 / kp.dt, kp.dopen,
                     (double)(kp.nt - 1), nb};
    }
    AAArgs aa_args() const {
        AAArgs Q{};
        Q.pt = pt;
        Q.asrc = asrc; Q.arec = arec; Q.amid = amid;
        for (int l = 0; l < kMaxLev - 1; l++) Q.thr[l] = l < nlev - 1 ? (double)hw[l] : INFINITY;
        Q.cstride = (long)((size_t)kp.N * (size_t)kp.nt);
        Q.lstride = (kmah ? 2 : 1) * Q.cstride;
        Q.nlev = nlev;
        return Q;
    }
};

// The pair on device pointers, the one launch path of the two kernels (kirchhoff.hip): any kind of handle,
// the callers have checked the arguments and the device.  d1 is read, or written, only on a handle with kmah.  The handle's own
// staging buffers may be passed (the host-pointer entries do): nothing is copied then.  st may be NULL; counts: also read back
// and sum the per-block counts into st->contributing (N words), which a solver's loop leaves out.  upload_ms is 0.
int rtmi_internal_kirchhoff_migrate_dev(rtmi_kirchhoff* k, const char* who, const double* d0, const double* d1, double* d_image,
                                        rtmi_kirchhoff_stats* st, bool counts);
int rtmi_internal_kirchhoff_model_dev(rtmi_kirchhoff* k, const char* who, const double* d_model, double* d0, double* d1,
                                      rtmi_kirchhoff_stats* st, bool counts);
// What that path launches around the pair kernel on a handle of rtmi_kirchhoff_create_aa with more than one level
// (kirchhoff_aa.hip), in place over the handle's `data`: before migrate, levels 1 .. nlev - 1 of the bank from level 0
// (k_aa_filter); gather: after model, the sum of the filtered spreads of every level into level 0 (k_aa_gather).
int rtmi_internal_kirchhoff_aa_sweep(rtmi_kirchhoff* k, const char* who, bool gather);
// The Hilbert transform along the handle's traces on device pointers (kirchhoff_hilbert.hip):
// d_y = (d_add ? d_add : +0) +- H d_x over [N][nt], minus with negate; d_y may be d_add, not d_x.  _check: RTMI_ERR_ARG naming nt
// when a trace does not fit the kernel's LDS.  The callers have checked that, the arguments and the device.  The handle's taps
// go up at the first call.  ms, if not NULL: the kernel's event time, waited for; with NULL the call does not wait.
int rtmi_internal_kirchhoff_hilbert_check(const rtmi_kirchhoff* k, const char* who);
int rtmi_internal_kirchhoff_hilbert_dev(rtmi_kirchhoff* k, const char* who, const double* d_x, const double* d_add, bool negate,
                                        double* d_y, double* ms);
// The trace filter on device pointers (kirchhoff_filter.hip): d_y = F d_x over [N][nt], or F^T d_x with
// transpose, with the taps of rtmi_kirchhoff_set_filter; d_y may not be d_x.  The callers have checked that a filter is set
// (k->ftaps), the arguments and the device.  ms as above.
int rtmi_internal_kirchhoff_filter_dev(rtmi_kirchhoff* k, const char* who, const double* d_x, bool transpose, double* d_y, double* ms);

namespace {

int migrate_block(int nb) { return nb > 16 ? 128 : 256; }    // [bin][lane] fp64 in LDS stays within 32 KiB

// `bytes` at p are memory of the handle's device, and the allocation holds them all (rtmi_host.h)
int check_device_pointer(const rtmi_kirchhoff* k, const char* who, const void* p, size_t bytes, const char* name) {
    return check_device_pointer(k->device, who, p, bytes, name);
}

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

// model's quantum: |contribution| <= max|w| max|amp|^2 max|m| = f 2^ex with f in [0.5, 1), so it is below 2^57 quanta 2^(ex - 57);
// max_m: max|m| over the finite values (rtmi_internal_absmax_finite)
int model_exponent(const rtmi_kirchhoff* k, double max_m) {
    const double bound = (k->max_w * k->max_amp) * k->max_amp * max_m;
    return std::isfinite(bound) ? rt::fix_exponent(bound) : 1025 - rt::kFixBits;
}

// All creates.  karr = 0: rtmi_kirchhoff_create (tables [P][nn], no kmah); karr >= 1: create_multi (tables [P][karr][nn]); with
// ap: create_aa (create_multi's tables and pt of their shape, the levels and the lengths of ap).
int create_impl(const char* who, const rtmi_kirchhoff_params* kp, int karr, const double* T, const double* amp, const double* theta,
                const double* kmah, const int32_t* isrc, const int32_t* irec, const double* w, rtmi_kirchhoff** out,
                const rtmi_kirchhoff_aa_params* ap = nullptr, const double* pt = nullptr) {
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
    if (ap) {
        RTMI_ARG(pt, "null pt");
        RTMI_ARG(ap->nlev >= 1 && ap->nlev <= RTMI_KIRCHHOFF_MAX_LEVELS, "nlev must be in 1..8");
        RTMI_ARG(ap->hw[0] == 0, "hw[0] must be 0");
        for (int l = 1; l < ap->nlev; l++) RTMI_ARG(ap->hw[l] > ap->hw[l - 1], "hw must be strictly increasing");
        RTMI_ARG(ap->hw[ap->nlev - 1] <= 64, "hw must be <= 64");
        RTMI_ARG(std::isfinite(ap->asrc) && ap->asrc >= 0.0, "asrc must be finite and >= 0");
        RTMI_ARG(std::isfinite(ap->arec) && ap->arec >= 0.0, "arec must be finite and >= 0");
        RTMI_ARG(std::isfinite(ap->amid) && ap->amid >= 0.0, "amid must be finite and >= 0");
    }
    const size_t nn = (size_t)kp->nx * (size_t)kp->ny, N = (size_t)kp->N, nt = (size_t)kp->nt;
    const size_t P = (size_t)kp->P * (size_t)(karr > 0 ? karr : 1);        // tables of nn nodes
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
    k->karr = karr;
    k->nb = nb;
    k->nn = nn;
    k->max_w = max_w;
    k->max_amp = max_amp;
    if (ap) {
        k->nlev = ap->nlev;
        for (int l = 0; l < ap->nlev; l++) k->hw[l] = ap->hw[l];
        k->asrc = ap->asrc; k->arec = ap->arec; k->amid = ap->amid;
    }
    const size_t levels = ap ? (size_t)ap->nlev : 1;
    const bool bins = kp->nbin > 0;
    const size_t mblocks = (nn + migrate_block(nb) - 1) / migrate_block(nb);
    k->ncounts = N > mblocks ? N : mblocks;
    auto fail = [&](int code, const std::string& msg) {
        delete k;
        return rtmi_internal_fail(code, (std::string(who) + ": " + msg).c_str());
    };
    hipError_t e = hipGetDevice(&k->device);
    if (e != hipSuccess) return fail(RTMI_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    e = hipDeviceGetAttribute(&k->cus, hipDeviceAttributeMultiprocessorCount, k->device);
    if (e != hipSuccess || k->cus < 1) return fail(RTMI_ERR_HIP, std::string("hipDeviceGetAttribute: ") + hipGetErrorString(e));
    auto get = [&](void** p, size_t bytes) { return hipMalloc(p, bytes); };
    struct { void** p; size_t bytes; const void* src; } bufs[] = {
        {(void**)&k->T, P * nn * sizeof(double), T},
        {(void**)&k->amp, amp ? P * nn * sizeof(double) : 0, amp},
        {(void**)&k->theta, bins ? P * nn * sizeof(double) : 0, theta},
        {(void**)&k->pt, ap ? P * nn * sizeof(double) : 0, pt},
        {(void**)&k->isrc, N * sizeof(int32_t), isrc},
        {(void**)&k->irec, N * sizeof(int32_t), irec},
        {(void**)&k->w, N * sizeof(double), nullptr},
        {(void**)&k->kmah, kmah ? P * nn * sizeof(int8_t) : 0, nullptr},
        {(void**)&k->data, levels * (kmah ? 2 : 1) * N * nt * sizeof(double), nullptr},   // with kmah: channel 0, then channel 1
        {(void**)&k->image, (size_t)nb * nn * sizeof(double), nullptr},
        {(void**)&k->counts, k->ncounts * sizeof(unsigned long long), nullptr},
        {(void**)&k->red, kRedWords * sizeof(unsigned long long), nullptr},
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
    if (kmah) {
        std::vector<int8_t> km(P * nn);
        for (size_t i = 0; i < P * nn; i++) {
            const double v = kmah[i];
            km[i] = (std::isfinite(v) && v >= 0.0 && v == std::floor(v)) ? (int8_t)std::fmod(v, 4.0) : kBadKmah;
        }
        e = hipMemcpy(k->kmah, km.data(), P * nn * sizeof(int8_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(RTMI_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    *out = k;
    return RTMI_OK;
}

// create_multi's own checks and the one-arrival parameters of its struct (P: rtmi_kirchhoff_multi_params, rtmi_kirchhoff_aa_params)
template <typename P> int multi_params(const char* who, const P* mp, rtmi_kirchhoff_params* kp) {
    RTMI_ARG(mp->karr >= 1 && mp->karr <= RTMI_KIRCHHOFF_MAX_ARRIVALS, "karr must be in 1..4");
    *kp = rtmi_kirchhoff_params{};
    kp->nx = mp->nx; kp->ny = mp->ny; kp->P = mp->P; kp->N = mp->N; kp->nt = mp->nt;
    kp->t0 = mp->t0; kp->dt = mp->dt; kp->nbin = mp->nbin; kp->dopen = mp->dopen;
    RTMI_ARG(kp->P <= INT32_MAX / RTMI_KIRCHHOFF_MAX_ARRIVALS, "P karr must fit the int32 indices");
    return RTMI_OK;
}

}  // namespace
