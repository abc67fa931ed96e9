// rtmi_host.h -- the host-side support layer of every translation unit: the ways out of an entry, one call's device memory and
// event marks, grid sizing, a block's exact maximum, the check of a caller's device pointer, and the checks every entry that reads
// a batch's recorded rows makes.  A new post-trace unit starts
// from this header and from rt_rows.h, the record as its kernels read it (DESIGN.md sections 15 to 17).  Everything is in an
// anonymous namespace: each unit gets its own copy, as with rt_crossing.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rtmi.h"
#include "rtmi_internal.h"

#define RTMI_EXPORT extern "C" __attribute__((visibility("default")))
// The three ways out of an entry.  Each relies on a local `const char* who`, the public entry's name: it begins every message.
#define RTMI_HIP(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return rtmi_internal_fail(RTMI_ERR_HIP, (std::string(who) + ": " + #expr + ": " + hipGetErrorString(e_)).c_str()); \
    } while (0)
#define RTMI_ARG(cond, msg)                                                                               \
    do {                                                                                                  \
        if (!(cond)) return rtmi_internal_fail(RTMI_ERR_ARG, (std::string(who) + ": " + (msg)).c_str()); \
    } while (0)
#define RTMI_RC(expr)                \
    do {                             \
        const int rc_ = (expr);      \
        if (rc_) return rc_;         \
    } while (0)
// The same two for the entries that spell their own name into the message (rtmi.hip, shard.hip): a HIP failure is reported with
// the place in the source instead.
#define HIP_TRY(expr)                                                                                                       \
    do {                                                                                                                    \
        hipError_t e_ = (expr);                                                                                             \
        if (e_ != hipSuccess)                                                                                               \
            return rtmi_internal_fail(RTMI_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                                     std::to_string(__LINE__) + ")").c_str());                              \
    } while (0)
#define ARG_TRY(cond, msg)                                                                  \
    do {                                                                                    \
        if (!(cond)) return rtmi_internal_fail(RTMI_ERR_ARG, std::string(msg).c_str());     \
    } while (0)

namespace {

// device allocations of one call, freed on every way out
struct DevMem {
    std::vector<void*> p;
    template <typename T> hipError_t get(T** out, size_t bytes) {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, bytes ? bytes : 8);
        if (e == hipSuccess) { p.push_back(v); *out = (T*)v; }
        return e;
    }
    ~DevMem() { for (void* v : p) (void)hipFree(v); }
};

// N marks on the null stream of one call and the time between two of them
template <int N> struct EventMarks {
    hipEvent_t e[N] = {};
    hipError_t create() {
        for (hipEvent_t& v : e) {
            const hipError_t r = hipEventCreate(&v);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    hipError_t mark(int i) { return hipEventRecord(e[i], nullptr); }
    hipError_t wait(int i) { return hipEventSynchronize(e[i]); }
    hipError_t ms(int i, int j, double* out) {
        float t = 0.0f;
        const hipError_t r = hipEventElapsedTime(&t, e[i], e[j]);
        *out = t;
        return r;
    }
    ~EventMarks() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
};

// f(T()) with T the element type of a field or batch: the one place where a dtype becomes a template argument
template <typename F> auto by_dtype(int dtype, F&& f) { return dtype == RTMI_F64 ? f(double()) : f(float()); }

// one lane per item, 256 lanes per block
dim3 blocks(long n) { return dim3((unsigned)((n + 255) / 256)); }

// blocks of 256 lanes for a grid-stride pass over n items, each lane taking `per` of them at a time: at most 4 blocks per CU
dim3 stride_blocks(int cus, size_t n, size_t per) {
    const size_t want = (n + 256 * per - 1) / (256 * per), cap = (size_t)4 * (size_t)cus;
    return dim3((unsigned)(want < 1 ? 1 : want < cap ? want : cap));
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The words a handle keeps for the results of its reductions (rtmi_internal_absmax_finite, rt_lsqr_device.h)
constexpr size_t kRedWords = 8;

// The block's largest v (v >= 0, never NaN) into *slot, a double kept as its bits: non-negative doubles order as unsigned integers,
// so one integer atomic max per block is the second stage of the reduction, and fmax is exact: the same bits in every schedule.
// The slot starts from 0.  Blocks of 256 lanes.
__device__ __forceinline__ void block_max_to(unsigned long long* slot, double v) {
    __shared__ double wmax[4];
    for (int off = 1; off < 64; off <<= 1) v = fmax(v, __shfl_xor(v, off));
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) wmax[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const double m = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
        if (m > 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(m));
    }
}

// `bytes` at p are memory of `device`, a handle's (hipPointerGetAttributes), and the allocation holds them all
int check_device_pointer(int device, const char* who, const void* p, size_t bytes, const char* name) {
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();             // a plain host pointer: not an error of the runtime's to keep
    const bool ok = e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device;
    RTMI_ARG(ok, std::string(name) + " is not memory of the handle's device");
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        RTMI_ARG(false, std::string(name) + ": the extent of its allocation could not be read");
    }
    RTMI_ARG((const char*)p + bytes <= (const char*)base + size, std::string(name) + " is shorter than the call needs");
    return RTMI_OK;
}

// slot[o] = the slot of the caller's ray o: the inverse of rtmi_device_view.perm.  A template, so that only the units that launch
// it carry the kernel.
template <typename I> __global__ void k_inverse(const I* perm, I* slot, long R) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < R) slot[perm[k]] = (I)k;
}

// The axes of a regular output grid (P: rtmi_grid_params, rtmi_beam_params)
template <typename P> int check_grid_axes(const char* who, const P& g) {
    RTMI_ARG(g.nx >= 1 && g.ny >= 1, "nx and ny must be >= 1");
    RTMI_ARG((double)g.nx * (double)g.ny <= (double)(1L << 31), "more than 2^31 nodes per source");
    RTMI_ARG(g.gdx > 0.0 && g.gdy > 0.0 && std::isfinite(g.gdx) && std::isfinite(g.gdy), "gdx and gdy must be finite and > 0");
    RTMI_ARG(std::isfinite(g.gx0) && std::isfinite(g.gy0), "gx0 and gy0 must be finite");
    return RTMI_OK;
}

// An entry that reads a batch's recorded rows: what it needs ...
enum : unsigned {
    kRecIsotropic = 1,      // op1..op9 with gamma 1 only
    kRecPoly = 2,           // the field's polynomial view (Recorded::poly)
    kRecFromLaunch = 4,     // every ray's rows must run from its launch point: a batch with rows from rtmi_batch_set_state is refused
    kRecOnDevice = 8,       // the calling thread's current device must be the field's
};
// ... and what it gets
struct Recorded {
    rtmi_device_view v;
    rtmi_params p;
    const rtmi_field* f;
    rtmi_internal_poly poly;
};
// The checks on the host, in this order -- record_stride 1, isotropic, from the launch point, a whole number of fans (fan_size 0:
// not asked), the field's device -- then the view, which drains the rays handed over to the re-trace of critical rays, with the
// batch's stream idle.
int recorded(const char* who, rtmi_batch* b, unsigned needs, int64_t fan_size, Recorded* r) {
    int from_state = 0;
    RTMI_RC(rtmi_internal_batch_info(b, &r->f, &r->p, &from_state));
    RTMI_ARG(r->p.record_stride == 1, "needs the full trajectory (record_stride 1)");
    if (needs & kRecIsotropic)
        RTMI_ARG(r->p.method >= 1 && r->p.method <= 9 && r->p.gamma == 1.0,
                 "isotropic media only (op1..op9, gamma 1): amplitudes come from dynamic ray tracing, which is another system "
                 "in an anisotropic medium");
    if ((needs & kRecFromLaunch) && from_state)
        return rtmi_internal_fail(RTMI_ERR_STATE, (std::string(who) + ": rtmi_batch_set_state gave rays a row other than 0: their "
                                                   "rows before it are not a trajectory from the source (reset the batch)").c_str());
    if (fan_size) {
        int64_t nrays = 0;
        RTMI_RC(rtmi_internal_batch_rays(b, &nrays));
        RTMI_ARG(nrays % fan_size == 0, "the batch's ray count is not a multiple of fan_size");
    }
    if (needs & kRecPoly) RTMI_RC(rtmi_internal_field_poly(r->f, &r->poly));
    if (needs & kRecOnDevice) RTMI_RC(rtmi_internal_on_device(who, r->f));
    RTMI_RC(rtmi_batch_view(b, &r->v));
    RTMI_RC(rtmi_sync(b));
    return RTMI_OK;
}

}  // namespace
