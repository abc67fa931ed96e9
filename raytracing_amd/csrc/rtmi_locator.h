// rtmi_locator.h -- the locator handle as its units see it: locate.hip creates and destroys it and searches it with picks by
// least squares, stack.hip searches it with traces (section 30), edt.hip with picks by equal differential
// time (section 31).  The two pick searches share what comes before and after the search itself -- the checks of a call, the
// staged picks, the exact minimum over an event's tiles -- and that is here too.  After rtmi_host.h.
#pragma once
#include "rtmi_host.h"

struct rtmi_locator {
    rtmi_locator_params lp{};
    int device = -1, cus = 0;
    size_t nn = 0;
    double* T = nullptr;          // device [P][ny][nx]
    ~rtmi_locator() {
        if (T) (void)hipFree(T);
    }
};

namespace {

#define RTMI_ALLOC(expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            (void)hipGetLastError();                                                                              \
            return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + #expr + ": " + hipGetErrorString(e_)).c_str()); \
        }                                                                                                         \
    } while (0)

// the calling thread's current device is the handle's
int check_device(const rtmi_locator* loc, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == loc->device, "the calling thread's current device is not the handle's");
    return RTMI_OK;
}

constexpr int kTile = 256;             // nodes of a block, one per lane
constexpr int kChunk = 16;             // events (stack.hip: scan indices) of a block: their running sums live in the lane's registers
constexpr unsigned kNoNode = 0xffffffffu;
constexpr unsigned kAllPicks = (1u << kChunk) - 1;

// ------------------------------------------------------------------ shared by the searches with picks (locate.hip, edt.hip)
// (key, node) of the best candidate of one (event, tile) and what of the tile contributed
struct Partial {
    double key;
    unsigned node;
    int cnt;
};

// An invalid pick is this one NaN in the staged picks; a difference of two finite numbers is never a NaN, so the test is exact.
__device__ __forceinline__ double no_pick() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool is_no_pick(double v) { return ((unsigned)__double2hiint(v) & 0x7fffffffu) >= 0x7ff80000u; }

// (a, na) <- the lesser of (a, na) and (b, nb): by key, then by node.  Keys are never NaN.
__device__ __forceinline__ void take_less(double& a, unsigned& na, double b, unsigned nb) {
    const bool less = b < a || (b == a && nb < na);
    a = less ? b : a;
    na = less ? nb : na;
}

// Per event: ref = the pick of the lowest valid station (no_pick() when there is none, and for the events past E that fill the
// last chunk) and needv = max(need, 1), or the number of valid picks when need is absent.
__device__ __forceinline__ bool valid_pick(const double* __restrict__ t, const double* __restrict__ w, long i) {
    return fabs(t[i]) < INFINITY && (!w || (w[i] > 0.0 && w[i] < INFINITY));
}
__global__ void __launch_bounds__(256) k_locate_prep(const double* __restrict__ t, const double* __restrict__ w, const int32_t* __restrict__ need,
                                                     long E, long Epad, int P, double* __restrict__ ref, int* __restrict__ needv) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Epad) return;
    double r0 = no_pick();
    int nvalid = 0;
    if (e < E)
        for (int r = 0; r < P; r++)
            if (valid_pick(t, w, e * P + r) && nvalid++ == 0) r0 = t[e * P + r];
    const int nd = e < E ? (need ? need[e] : nvalid) : 1;
    ref[e] = r0;
    needv[e] = nd > 1 ? nd : 1;
}

// Picks as the search reads them, one lane per (chunk, station): tr [chunk][P][16] = t - ref (no_pick() where the pick is not
// valid or the event is past E), wv of the same layout, and mask [chunk][P], bit k set where event k of the chunk has a valid
// pick at the station.  The 16 events of a chunk lie side by side, so that one scalar load brings a station's picks for the
// whole chunk, and a station at which the whole chunk has picks -- the usual case -- needs no test per event.
__global__ void __launch_bounds__(256) k_locate_stage(const double* __restrict__ t, const double* __restrict__ w, const double* __restrict__ ref,
                                                      long E, long nchunks, int P, double* __restrict__ tr, double* __restrict__ wv,
                                                      unsigned* __restrict__ mask) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks * P) return;
    const long c = i / P, r = i % P;
    unsigned m = 0;
    for (int k = 0; k < kChunk; k++) {
        const long e = c * kChunk + k;
        double d = no_pick(), wr = 0.0;
        if (e < E && valid_pick(t, w, e * P + r)) {
            d = t[e * P + r] - ref[e];
            if (w) wr = w[e * P + r];
            m |= 1u << k;
        }
        tr[i * kChunk + k] = d;
        if (wv) wv[i * kChunk + k] = wr;
    }
    mask[i] = m;
}

// best[e] = the node of the least (key, node) over the event's partials, -1 when no tile has a candidate
__global__ void __launch_bounds__(256) k_locate_pick(const Partial* __restrict__ part, unsigned ntiles, int32_t* __restrict__ best,
                                                     long long* __restrict__ contributing) {
    const size_t e = blockIdx.x;
    const int tid = (int)threadIdx.x;
    double key = INFINITY;
    unsigned node = kNoNode;
    long long cnt = 0;
    for (unsigned i = tid; i < ntiles; i += 256) {
        const Partial p = part[e * ntiles + i];
        take_less(key, node, p.key, p.node);
        cnt += p.cnt;
    }
    for (int off = 1; off < 64; off <<= 1) {
        take_less(key, node, __shfl_xor(key, off), __shfl_xor(node, off));
        cnt += __shfl_xor(cnt, off);
    }
    __shared__ double wkey[4];
    __shared__ unsigned wnode[4];
    __shared__ long long wcnt[4];
    if ((tid & 63) == 0) {
        wkey[tid >> 6] = key;
        wnode[tid >> 6] = node;
        wcnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; v++) {
            take_less(key, node, wkey[v], wnode[v]);
            cnt += wcnt[v];
        }
        best[e] = node == kNoNode ? -1 : (int32_t)node;
        contributing[e] = cnt;
    }
}

// what every form of a call with picks refuses before it touches the device
int check_picks_call(const char* who, const rtmi_locator* loc, int64_t E, const void* t, const void* res, unsigned* nchunks, unsigned* ntiles) {
    RTMI_ARG(loc, "null handle");
    RTMI_ARG(t, "null t");
    RTMI_ARG(res, "null res");
    RTMI_ARG(E >= 1, "E must be >= 1");
    const int64_t nc = (E + kChunk - 1) / kChunk, nt = (int64_t)((loc->nn + kTile - 1) / kTile);
    RTMI_ARG(nc < ((int64_t)1 << 31) && (double)nc * (double)nt < (double)((int64_t)1 << 31), "more than 2^31 (tile, event chunk) pairs: split E over several calls");
    *nchunks = (unsigned)nc;
    *ntiles = (unsigned)nt;
    return RTMI_OK;
}

}  // namespace
