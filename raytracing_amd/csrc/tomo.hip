// tomo.hip -- recorded rays compiled into a sparse ray-tomography matrix that lives on the device (rtmi_tomo_create, _append,
// _read, _info, _apply, _transpose, their _dev forms, rtmi_tomo_lsqr, rtmi_tomo_lsqr_weighted, _destroy).  include/rtmi.h states
// the contract; DESIGN.md section 24 the definitions, the error bound and what was measured; section 26 the weighted solver.
//
// A row of the matrix is one reported traveltime's derivative with respect to the field's samples; it is a list of segments, one
// per cell visit of its ray: the cell's first sample `base` and four weights p[q].  rtmi_tomo_append walks a batch's rows with
// walk_weighted (rt_sens_walk.h), the walk of rtmi_traveltime_backproject with weight 1 on the one observation, twice: a count pass
// (the rows' lengths), a scan on the host over the lengths (rt_tomo.h: the slices' offsets), and a fill pass.  The batch is not
// needed afterwards.  Storage is sliced by 64 rows (rt_tomo.h), so that the products run one lane per row with coalesced loads:
//   k_tomo_apply      y_r = sum over the row's segments, in visit order, of ((p0 x0 + p1 x1) + p2 x2) + p3 x3, x gathered from the
//                     4 samples of the segment's cell; one fixed order, no atomics.
//   k_tomo_transpose  every product p_q w_r is rounded once to a fixed-point integer (quantum from Vmax max|w|, an order-independent
//                     bound), the lanes of a wave whose next segments lie in the same cell add as one (the lane
//                     furthest behind names the cell, so that neighbouring rays stay together although their segment indices
//                     drift apart), and the sums go into two integer words per sample with adds that return nothing (add_split),
//                     read as one integer and rounded once (rt_fix128.h): the same bits in every schedule and order of appends.
// Both are compiled for chunks of C = 8, 4, 2 and 1 columns (vectors are planes: column c of x is x + c xs; the transposed
// product's width 1 is k_tomo_transpose1, the same arithmetic with the integers kept per lane), read a segment once
// for the chunk, and serve the single entries as nrhs = 1 and rtmi_tomo_apply_multi, _transpose_multi with the caller's nrhs
// (DESIGN.md section 28).  The model basis follows (rtmi_tomo_basis_*), then the one solver body,
// tomo_lsqr_run: the loop of rt_lsqr_device.h over the stacked operator [A P | Dx | Dy | Dxx | Dyy] on S planes, which
// rtmi_tomo_lsqr, _lsqr_weighted and _lsqr_basis run with S = 1 and rtmi_tomo_lsqr_multi with the caller's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_fix128.h"
#include "rt_lsqr_device.h"
#include "rt_sens_walk.h"
#include "rt_tomo.h"
#include "rt_tomo_basis.h"
#include "rtmi_host.h"
#include "rt_tomo_reg.h"

static_assert(rt::kTomoSlice == 64, "a slice is a wave");

// The transposed product's accumulators exist this many times; a block of rows adds into copy (block index mod kTomoCopies), and the
// copies' integers are summed before the one rounding.  Rays of one source share their first cells: the copies spread the adds to
// those few addresses.
constexpr int kTomoCopies = 8;
constexpr size_t kTomoRed = (size_t)kMultiMax * kRedM + 2;

// One append's rows
struct TomoBlock {
    int64_t first = 0, rows = 0, segments = 0, padded = 0;
    int32_t* len = nullptr;       // [rows]
    int64_t* off = nullptr;       // [slices + 1]
    int32_t* base = nullptr;      // [padded]
    double* val = nullptr;        // [4 padded]
    void release() {
        for (void* p : {(void*)len, (void*)off, (void*)base, (void*)val})
            if (p) (void)hipFree(p);
        len = nullptr; off = nullptr; base = nullptr; val = nullptr;
    }
    size_t bytes() const {
        return (size_t)rows * sizeof(int32_t) + (size_t)(rt::tomo_slices(rows) + 1) * sizeof(int64_t) + (size_t)padded * (sizeof(int32_t) + 4 * sizeof(double));
    }
};

struct rtmi_tomo {
    int device = 0, cus = 1;
    Axes F{};
    std::vector<TomoBlock> blocks;
    int64_t rows = 0, segments = 0, padded = 0;
    double vmax = 0.0, compile_ms = 0.0;
    // [acc_cols] x [kTomoCopies] x (A [nz], B [nz]): the transposed product's split accumulators (add_split), one set per column:
    // one column at create, grown when a call has more (ensure_cols)
    unsigned long long* acc = nullptr;
    int acc_cols = 0;
    // kTomoRed reduction words: [kMultiMax] x kRedM, the columns' of rt_lsqr_device.h, then a fill pass's max |p| and the atomics
    unsigned long long* red = nullptr;
    hipEvent_t ev[2] = {};
    size_t nz() const { return (size_t)F.qx * (size_t)F.qy; }
    size_t bytes() const {
        size_t b = ((size_t)acc_cols * kTomoCopies * 2 * nz() + kTomoRed) * sizeof(unsigned long long);
        for (const TomoBlock& k : blocks) b += k.bytes();
        return b;
    }
    unsigned long long* red_vmax() const { return red + kTomoRed - 2; }
    unsigned long long* red_atomics() const { return red + kTomoRed - 1; }
    ~rtmi_tomo() {
        for (TomoBlock& b : blocks) b.release();
        if (acc) (void)hipFree(acc);
        if (red) (void)hipFree(red);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// ------------------------------------------------------------------------------------------------------------ compile
// walk_weighted's sinks.  Both end a ray observed at a crossing with that crossing's step: later rows carry no weight.
struct CountSink {
    static constexpr bool kStopAtLast = true;
    int n;
    __device__ __forceinline__ void flush(bool go, int, int, const double (&)[4]) { n += go ? 1 : 0; }
};
struct FillSink {
    static constexpr bool kStopAtLast = true;
    int32_t* base;
    double* val;
    int64_t off;                  // the slice's offset
    int lane, qx, k, cap;         // cap: the row's length from the count pass: nothing is written past it
    double vmax;
    __device__ __forceinline__ void flush(bool go, int cx, int cy, const double (&p)[4]) {
        if (go && k < cap) {
            base[rt::tomo_slot(off, k, lane)] = cy * qx + cx;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                val[rt::tomo_value(off, k, q, lane)] = p[q];
                vmax = fmax(vmax, fabs(p[q]));
            }
            k++;
        }
    }
};

// One lane per ray.  which [R] (the caller's ray order; NULL: every ray's end), rowof [R]: the ray's row in the block, -1 skipped.
// FILL false: len[row] = the row's segments.  FILL true: the segments into the block's storage, and max |p| into *vmax.
template <typename T, bool FILL>
__global__ void __launch_bounds__(256) k_tomo_walk(Rows<T> rec, Args A, const int32_t* __restrict__ which, const int32_t* __restrict__ rowof,
                                                   int32_t* __restrict__ len, const int64_t* __restrict__ off, int32_t* __restrict__ base,
                                                   double* __restrict__ val, unsigned long long* __restrict__ vmax) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < rec.R;
    const long o = in ? rec.caller(k) : 0;
    const long row = in ? (long)rowof[o] : -1;
    long last = (in && row >= 0) ? rec.last(k) : -1;
    if (last >= rec.rec_rows) last = -1;                      // past the record: an empty row
    const int wh = (in && which) ? which[o] : -1;
    const bool line = A.has_line && wh >= 0;
    int K = 0;
    double we = 0.0;
    if (last >= 0) {
        if (wh < 0) {
            we = 1.0;
        } else if (wh < min(count_crossings(rec, k, last, A.L), A.kmax)) {
            K = wh + 1;                                       // crossings 0 .. wh matter to the walk; wh carries the weight
        } else {
            last = -1;                                        // no such crossing: an empty row
        }
    }
    auto wc = [&](int c) { return c == wh ? 1.0 : 0.0; };
    if (!FILL) {
        CountSink sink{0};
        walk_weighted(rec, A, in ? k : 0, last, line, K, we, wc, sink);
        if (row >= 0) len[row] = sink.n;
    } else {
        FillSink sink{base, val, row >= 0 ? off[row >> 6] : 0, (int)(row & 63), A.F.qx, 0, row >= 0 ? len[row] : 0, 0.0};
        walk_weighted(rec, A, in ? k : 0, last, line, K, we, wc, sink);
        block_max_to(vmax, sink.vmax);
    }
}

// ------------------------------------------------------------------------------------------------------------ products
// A product takes nrhs <= kMultiMax vectors through one read of the matrix.  A kernel is compiled for chunks of C = 8, 4, 2 and 1
// columns; a launch takes the widest that nrhs fills, with the chunk in blockIdx.y, so that a product is one launch per append
// whatever nrhs is.  The last chunk may be partial: its missing columns are not written.
int chunk_of(int nrhs) { return nrhs >= 8 ? 8 : nrhs >= 4 ? 4 : nrhs >= 2 ? 2 : 1; }

// One lane per row of a block: y[c][r] for r < rows and the columns c0 .. c0 + C - 1.  A segment's base and p are loaded once, the
// gathers and the five roundings are the column's own.  A column past nrhs reads the last one's x and is not written.
template <int C>
__global__ void __launch_bounds__(256) k_tomo_apply(const int32_t* __restrict__ len, const int64_t* __restrict__ off,
                                                    const int32_t* __restrict__ base, const double* __restrict__ val, long rows, int qx,
                                                    int nrhs, const double* __restrict__ x, size_t xs, double* __restrict__ y, size_t ys) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int c0 = (int)blockIdx.y * C;
    const int lane = (int)(r & 63);
    const int64_t o = off[r >> 6];
    const int n = len[r];
    const double* xc[C];
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; j++) {
        xc[j] = x + (size_t)min(c0 + j, nrhs - 1) * xs;
        acc[j] = 0.0;
    }
    for (int k = 0; k < n; k++) {
        const int b = base[rt::tomo_slot(o, k, lane)];
        const double p0 = val[rt::tomo_value(o, k, 0, lane)], p1 = val[rt::tomo_value(o, k, 1, lane)];
        const double p2 = val[rt::tomo_value(o, k, 2, lane)], p3 = val[rt::tomo_value(o, k, 3, lane)];
#pragma unroll
        for (int j = 0; j < C; j++) {
            const double* z = xc[j] + b;
            const double t = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(p0, z[0]), __dmul_rn(p1, z[1])), __dmul_rn(p2, z[qx])), __dmul_rn(p3, z[qx + 1]));
            acc[j] = __dadd_rn(acc[j], t);
        }
    }
#pragma unroll
    for (int j = 0; j < C; j++)
        if (c0 + j < nrhs) y[(size_t)(c0 + j) * ys + r] = acc[j];
}

// s quanta into sample i of the split accumulators: the low 32 bits of s into A[i], the rest (signed) into B[i], so that
// s = B 2^32 + A holds for the sums as well.  Neither add returns a value, so the wave does not wait for memory; below 2^32 adds
// per sample neither word can wrap.  Returns the atomics issued.
__device__ __forceinline__ int add_split(unsigned long long* A, unsigned long long* B, size_t i, long long s) {
    if (s == 0) return 0;
    atomicAdd(A + i, (unsigned long long)s & 0xffffffffull);
    const long long h = s >> 32;
    if (h == 0) return 1;
    atomicAdd(B + i, (unsigned long long)h);
    return 2;
}

// The transposed product of one column (nrhs = 1): one lane per row of a block, a wave per slice; the lanes step through the
// cells as in k_tomo_transpose below.  With one column a lane forms its four integers when it takes its segment and keeps them,
// not when it joins an add: 60 VGPRs against the template's 66 at C = 1, which by_chunk therefore does not instantiate.  The same
// lanes take part, so the bits and the count of atomics are the template's.  A weight that is not finite counts as 0.
__global__ void __launch_bounds__(256) k_tomo_transpose1(const int32_t* __restrict__ len, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ base, const double* __restrict__ val, long rows, int qx,
                                                         const double* __restrict__ w, int e, unsigned long long* acc, size_t nz,
                                                         unsigned long long* natomics) {
    unsigned long long* const A = acc + (size_t)(blockIdx.x % kTomoCopies) * 2 * nz;
    unsigned long long* const B = A + nz;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < rows;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t o = in ? off[r >> 6] : 0;
    const double wr = in ? w[r] : 0.0;
    const int n = (in && fabs(wr) < INFINITY && wr != 0.0) ? len[r] : 0;
    long long nat = 0;
    int k = 0, b = 0, nb = 0;
    long long m[4] = {0, 0, 0, 0};
    double np[4] = {0.0, 0.0, 0.0, 0.0};
    auto load = [&](int kk) {                                 // segment kk into (nb, np)
        if (kk < n) {
            nb = base[rt::tomo_slot(o, kk, lane)];
#pragma unroll
            for (int q = 0; q < 4; q++) np[q] = val[rt::tomo_value(o, kk, q, lane)];
        }
    };
    auto take = [&]() {                                       // (nb, np) becomes the lane's next segment
        b = nb;
#pragma unroll
        for (int q = 0; q < 4; q++) m[q] = (long long)rint(ldexp(__dmul_rn(np[q], wr), -e));
    };
    load(0);
    take();
    load(1);
    for (;;) {
        const bool pend = k < n;
        if (__ballot(pend) == 0ull) break;
        int kmin = pend ? k : INT32_MAX;
        for (int s = 1; s < 64; s <<= 1) kmin = min(kmin, __shfl_xor(kmin, s));
        const int leader = __ffsll((long long)__ballot(pend && k == kmin)) - 1;
        const int lb = __shfl(b, leader);
        const bool mem = pend && b == lb;
        long long v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = mem ? m[q] : 0;
        if (__popcll(__ballot(mem)) > 1) {
#pragma unroll
            for (int s = 1; s < 64; s <<= 1)
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] += __shfl_xor(v[q], s);
        }
        if (lane == leader) {
            nat += add_split(A, B, (size_t)lb, v[0]);
            nat += add_split(A, B, (size_t)lb + 1, v[1]);
            nat += add_split(A, B, (size_t)lb + qx, v[2]);
            nat += add_split(A, B, (size_t)lb + qx + 1, v[3]);
        }
        if (mem) {
            k++;
            take();
            load(k + 1);
        }
    }
    for (int s = 1; s < 64; s <<= 1) nat += __shfl_xor(nat, s);
    if (lane == 0 && nat) atomicAdd(natomics, (unsigned long long)nat);
}

// Per column of a transposed product: the quantum's exponent; zero: the column contributes nothing and its result is +0.0
// (W = 0); skip: the column is not the call's business, nothing of it is read or written
struct TomoCols {
    int e[kMultiMax];
    unsigned long long zero, skip;
};

// One lane per row of a block, a wave per slice, for the columns c0 .. c0 + C - 1.  A weight that is not finite counts as 0.  The
// leader election, the kmin reduction and the ballot happen once per step for the chunk; the integers, the wave sums and the adds
// are the column's own, into the column's accumulators acc + c (kTomoCopies 2 nz).  A lane takes part when its weight is not zero
// in any column of the chunk; where it is zero its products are integer zeros, which change no sum, and add_split skips them.
template <int C>
__global__ void __launch_bounds__(256) k_tomo_transpose(const int32_t* __restrict__ len, const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ base, const double* __restrict__ val, long rows, int qx,
                                                        int nrhs, const double* __restrict__ w, size_t ws, TomoCols K,
                                                        unsigned long long* acc, size_t nz, unsigned long long* natomics) {
    const int c0 = (int)blockIdx.y * C;
    const size_t copy = (size_t)(blockIdx.x % kTomoCopies) * 2 * nz;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = r < rows;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t o = in ? off[r >> 6] : 0;
    double wr[C];
    int ec[C];
    bool any = false;
#pragma unroll
    for (int j = 0; j < C; j++) {
        const int c = c0 + j;
        const bool use = c < nrhs && !(((K.zero | K.skip) >> (c & 63)) & 1ull);
        double v = (in && use) ? w[(size_t)c * ws + r] : 0.0;
        if (!(fabs(v) < INFINITY)) v = 0.0;
        wr[j] = v;
        ec[j] = K.e[c & 63];
        any = any || v != 0.0;
    }
    const int n = (in && any) ? len[r] : 0;
    long long nat = 0;
    // Neighbouring rays visit much the same cells, but not at the same segment index: a ray that clips a corner has one visit more.
    // So the lanes do not step through k together.  Each holds its next segment; the lane that is furthest behind names a cell,
    // every lane whose next segment is that cell joins its add and moves on, the others wait.  Which lanes add together changes no
    // bit: the sums are integers.  The segment after the next is loaded a step ahead.
    int k = 0, b = 0, nb = 0;
    double p[4] = {0.0, 0.0, 0.0, 0.0}, np[4] = {0.0, 0.0, 0.0, 0.0};
    auto load = [&](int kk) {                                 // segment kk into (nb, np)
        if (kk < n) {
            nb = base[rt::tomo_slot(o, kk, lane)];
#pragma unroll
            for (int q = 0; q < 4; q++) np[q] = val[rt::tomo_value(o, kk, q, lane)];
        }
    };
    auto take = [&]() {                                       // (nb, np) becomes the lane's next segment
        b = nb;
#pragma unroll
        for (int q = 0; q < 4; q++) p[q] = np[q];
    };
    load(0);
    take();
    load(1);
    for (;;) {
        const bool pend = k < n;
        if (__ballot(pend) == 0ull) break;
        int kmin = pend ? k : INT32_MAX;
        for (int s = 1; s < 64; s <<= 1) kmin = min(kmin, __shfl_xor(kmin, s));
        const int leader = __ffsll((long long)__ballot(pend && k == kmin)) - 1;
        const int lb = __shfl(b, leader);
        const bool mem = pend && b == lb;
        const bool several = __popcll(__ballot(mem)) > 1;
#pragma unroll
        for (int j = 0; j < C; j++) {
            if (c0 + j >= nrhs) break;
            long long v[4] = {0, 0, 0, 0};
            if (mem) {
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = (long long)rint(ldexp(__dmul_rn(p[q], wr[j]), -ec[j]));
            }
            if (several) {
#pragma unroll
                for (int s = 1; s < 64; s <<= 1)
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q] += __shfl_xor(v[q], s);
            }
            if (lane == leader) {
                unsigned long long* const A = acc + (size_t)(c0 + j) * kTomoCopies * 2 * nz + copy;
                unsigned long long* const B = A + nz;
                nat += add_split(A, B, (size_t)lb, v[0]);
                nat += add_split(A, B, (size_t)lb + 1, v[1]);
                nat += add_split(A, B, (size_t)lb + qx, v[2]);
                nat += add_split(A, B, (size_t)lb + qx + 1, v[3]);
            }
        }
        if (mem) {
            k++;
            take();
            load(k + 1);
        }
    }
    for (int s = 1; s < 64; s <<= 1) nat += __shfl_xor(nat, s);
    if (lane == 0 && nat) atomicAdd(natomics, (unsigned long long)nat);
}

// (the smoothing rows k_tomo_diff, k_tomo_diff2 and their transposed terms k_tomo_reg_t: rt_tomo_reg.h)

// Sample i of the accumulators acc: the copies' integers B 2^32 + A summed, as the two words of rt_fix128.h (the low one biased),
// rounded once to fp64 and scaled by 2^e
__device__ __forceinline__ double acc_sample(const unsigned long long* __restrict__ acc, size_t nz, long i, int e) {
    unsigned long long a = 0ull, bb = 0ull;                                   // the copies' sums: below 2^32 adds in all, neither wraps
    for (int c = 0; c < kTomoCopies; c++) {
        a += acc[(size_t)c * 2 * nz + i];
        bb += acc[(size_t)c * 2 * nz + nz + i];
    }
    unsigned long long lo = (bb << 32) + a;
    unsigned long long hi = (unsigned long long)((long long)bb >> 32) + (lo < a ? 1ull : 0ull);
    const unsigned long long lo2 = lo + rt::kFixBias;
    hi += lo2 < lo ? 1ull : 0ull;
    return ldexp(rt::fix_to_double(lo2, hi), e);
}

// Per column (blockIdx.y): g + c gs = the column's accumulators, each sample's integer B 2^32 + A rounded once to fp64, +0.0 for a
// zero column; a skipped column is not written.  A regulariser's transposed rows are added afterwards (k_tomo_reg_t).
__global__ void __launch_bounds__(256) k_tomo_finish(const unsigned long long* __restrict__ acc, TomoCols K, size_t nz, double* __restrict__ g,
                                                     size_t gs) {
    const int c = (int)blockIdx.y;
    if ((K.skip >> c) & 1ull) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)nz) return;
    const bool zero = (K.zero >> c) & 1ull;
    g[(size_t)c * gs + i] = zero ? 0.0 : acc_sample(acc + (size_t)c * kTomoCopies * 2 * nz, nz, i, K.e[c]);
}

// ------------------------------------------------------------------------------------------------------------ host
int on_device(const rtmi_tomo* t, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == t->device, "the calling thread's current device is not the handle's");
    return RTMI_OK;
}

void fill_stats(const rtmi_tomo* t, rtmi_tomo_stats* st) {
    *st = rtmi_tomo_stats{};
    st->rows = t->rows; st->segments = t->segments; st->padded_segments = t->padded;
    st->bytes_device = (int64_t)t->bytes();
    st->compile_ms = t->compile_ms;
    st->vmax = t->vmax;
    st->qx = t->F.qx; st->qy = t->F.qy;
}

// f(std::integral_constant<int, C>) for the chunk width of nrhs when that is 8, 4 or 2; false for width 1, which is the caller's
template <typename F> bool by_chunk(int nrhs, F&& f) {
    switch (chunk_of(nrhs)) {
        case 8: f(std::integral_constant<int, 8>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        default: return false;
    }
}

int check_nrhs(const char* who, int32_t nrhs) {
    RTMI_ARG(nrhs >= 1 && nrhs <= kMultiMax, "nrhs must be in 1 .. 64");
    return RTMI_OK;
}

// Accumulators for nrhs columns: kept, and replaced by a larger set when a call has more.  A growth that fails leaves the handle
// without any, and the next call, of whatever width, allocates its own.
int ensure_cols(rtmi_tomo* t, const char* who, int nrhs) {
    if (t->acc_cols >= nrhs) return RTMI_OK;
    if (t->acc) (void)hipFree(t->acc);
    t->acc = nullptr;
    t->acc_cols = 0;
    if (hipMalloc((void**)&t->acc, (size_t)nrhs * kTomoCopies * 2 * t->nz() * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        t->acc = nullptr;
        return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": hipMalloc of the accumulators of " + std::to_string(nrhs) +
                                                   " columns failed").c_str());
    }
    t->acc_cols = nrhs;
    return RTMI_OK;
}

// A product's time: with ms, the kernels' event time between the two marks, waited for; without (the solver, which times its
// operator calls on the wall clock), no marks and no wait: the caller waits for the stream itself
hipError_t mark_begin(rtmi_tomo* t, const double* ms) { return ms ? hipEventRecord(t->ev[0], nullptr) : hipSuccess; }
hipError_t mark_end(rtmi_tomo* t, double* ms) {
    if (!ms) return hipSuccess;
    float f = 0.0f;
    hipError_t e = hipEventRecord(t->ev[1], nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(t->ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&f, t->ev[0], t->ev[1]);
    *ms = f;
    return e;
}

// y + c ys [rows] = A (x + c xs) for c < nrhs, on device pointers the callers have checked: one launch per append.  ms (or
// NULL): see mark_end.
int apply_dev(rtmi_tomo* t, const char* who, int nrhs, const double* d_x, size_t xs, double* d_y, size_t ys, double* ms) {
    RTMI_HIP(mark_begin(t, ms));
    const int C = chunk_of(nrhs);
    for (const TomoBlock& b : t->blocks) {
        const dim3 grid(blocks((long)b.rows).x, (unsigned)((nrhs + C - 1) / C));
        auto launch = [&](auto c) {
            hipLaunchKernelGGL((k_tomo_apply<decltype(c)::value>), grid, dim3(256), 0, nullptr, b.len, b.off, b.base, b.val, (long)b.rows,
                               t->F.qx, nrhs, d_x, xs, d_y + b.first, ys);
        };
        if (!by_chunk(nrhs, launch)) launch(std::integral_constant<int, 1>());
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(mark_end(t, ms));
    return RTMI_OK;
}

// g + c gs [qy][qx] = A^T (w + c ws) for the columns c of `mask`.  Every column has its own W, bound and exponent, from one
// reduction launch and one read-back.  range [nrhs]: the column's bound fl(Vmax max|w|) is not a normal number, and nothing of it
// is written; with `strict` the call then stops before any product.  atomics (or NULL: not read back), exps [nrhs] (or NULL): the
// columns' exponents, 0 for a zero column.
int transpose_dev(rtmi_tomo* t, const char* who, int nrhs, const double* d_w, size_t ws, double* d_g, size_t gs, unsigned long long mask,
                  bool strict, bool* range, double* ms, int64_t* atomics, int32_t* exps) {
    if (ms) *ms = 0.0;
    if (atomics) *atomics = 0;
    const size_t nz = t->nz();
    RTMI_RC(ensure_cols(t, who, nrhs));
    double W[kMultiMax] = {};
    if (t->rows > 0 && t->segments > 0 && t->vmax > 0.0)
        RTMI_RC(absmax(who, Vec{t->red, t->cus, nrhs}, d_w, ws, (size_t)t->rows, mask, W));
    TomoCols K{};
    K.skip = ~mask;
    bool work = false, refused = false;
    for (int c = 0; c < nrhs; c++) {
        range[c] = false;
        if (exps) exps[c] = 0;
        if (!(mask & col_bit(c))) continue;
        if (!(W[c] > 0.0)) {
            K.zero |= col_bit(c);
            continue;
        }
        const double bound = t->vmax * W[c];
        if (!std::isnormal(bound)) {
            range[c] = true;
            refused = true;
            K.skip |= col_bit(c);
            continue;
        }
        K.e[c] = rt::fix_exponent(bound);
        if (exps) exps[c] = K.e[c];
        work = true;
    }
    if (strict && refused) return RTMI_OK;
    RTMI_HIP(mark_begin(t, ms));
    if (work) {
        RTMI_HIP(hipMemsetAsync(t->acc, 0, (size_t)nrhs * kTomoCopies * 2 * nz * sizeof(unsigned long long), nullptr));
        RTMI_HIP(hipMemsetAsync(t->red_atomics(), 0, sizeof(unsigned long long), nullptr));
        const int C = chunk_of(nrhs);
        for (const TomoBlock& b : t->blocks) {
            const dim3 grid(blocks((long)b.rows).x, (unsigned)((nrhs + C - 1) / C));
            const bool wider = by_chunk(nrhs, [&](auto c) {
                hipLaunchKernelGGL((k_tomo_transpose<decltype(c)::value>), grid, dim3(256), 0, nullptr, b.len, b.off, b.base, b.val, (long)b.rows,
                                   t->F.qx, nrhs, d_w + b.first, ws, K, t->acc, nz, t->red_atomics());
            });
            if (!wider)                                       // one column, and it has work: neither zero nor skipped
                hipLaunchKernelGGL(k_tomo_transpose1, grid, dim3(256), 0, nullptr, b.len, b.off, b.base, b.val, (long)b.rows, t->F.qx,
                                   d_w + b.first, K.e[0], t->acc, nz, t->red_atomics());
            RTMI_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_tomo_finish, dim3(blocks((long)nz).x, (unsigned)nrhs), dim3(256), 0, nullptr, t->acc, K, nz, d_g, gs);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(mark_end(t, ms));
    if (work && atomics) {
        unsigned long long n = 0;
        RTMI_HIP(hipMemcpy(&n, t->red_atomics(), sizeof(n), hipMemcpyDeviceToHost));
        *atomics = (int64_t)n;
    }
    return RTMI_OK;
}

int finite_all(const char* who, const double* p, size_t n, const char* msg) {
    for (size_t i = 0; i < n; i++) RTMI_ARG(std::isfinite(p[i]), msg);
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_tomo_create(const rtmi_field* f, rtmi_tomo** out) {
    const char* who = "rtmi_tomo_create";
    RTMI_ARG(f, "null field");
    RTMI_ARG(out, "null out");
    rtmi_internal_poly poly;
    RTMI_RC(rtmi_internal_field_poly(f, &poly));              // RTMI_ERR_ARG unless the current device is the field's
    int qx = 0, qy = 0;
    RTMI_RC(rtmi_field_dims(f, &qx, &qy));
    RTMI_ARG(qx >= 2 && qy >= 2, "the field needs at least 2 samples per axis");
    rtmi_tomo* t = new (std::nothrow) rtmi_tomo;
    if (!t) return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_tomo_create: out of host memory");
    t->F = Axes{poly.ax, poly.bx, poly.inv_hx, poly.ay, poly.by, poly.inv_hy, qx, qy};
    auto fail = [&](int code, const char* what, hipError_t e) {
        delete t;
        return rtmi_internal_fail(code, (std::string(who) + ": " + what + ": " + hipGetErrorString(e)).c_str());
    };
    hipError_t e = hipGetDevice(&t->device);
    if (e != hipSuccess) return fail(RTMI_ERR_HIP, "hipGetDevice", e);
    e = hipDeviceGetAttribute(&t->cus, hipDeviceAttributeMultiprocessorCount, t->device);
    if (e != hipSuccess || t->cus < 1) return fail(RTMI_ERR_HIP, "hipDeviceGetAttribute", e);
    e = hipMalloc((void**)&t->acc, (size_t)kTomoCopies * 2 * t->nz() * sizeof(unsigned long long));
    if (e != hipSuccess) return fail(RTMI_ERR_ALLOC, "hipMalloc", e);
    t->acc_cols = 1;
    e = hipMalloc((void**)&t->red, kTomoRed * sizeof(unsigned long long));
    if (e != hipSuccess) return fail(RTMI_ERR_ALLOC, "hipMalloc", e);
    for (hipEvent_t& v : t->ev) {
        e = hipEventCreate(&v);
        if (e != hipSuccess) return fail(RTMI_ERR_HIP, "hipEventCreate", e);
    }
    *out = t;
    return RTMI_OK;
}

RTMI_EXPORT void rtmi_tomo_destroy(rtmi_tomo* t) { delete t; }

RTMI_EXPORT int rtmi_tomo_append(rtmi_tomo* t, rtmi_batch* b, const double line[3], int32_t kmax, const int32_t* which, int32_t* nseg,
                                 int64_t* first_row) {
    const char* who = "rtmi_tomo_append";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_line(line, kmax, who));
    RTMI_ARG(b, "null batch");
    int64_t R64 = 0;
    RTMI_RC(rtmi_internal_batch_rays(b, &R64));
    const size_t R = (size_t)R64;
    if (which) {
        const int32_t top = line ? kmax - 1 : -1;
        for (size_t m = 0; m < R; m++) {
            RTMI_ARG(which[m] >= RTMI_TOMO_SKIP, "which has a value below RTMI_TOMO_SKIP (-2)");
            RTMI_ARG(line || which[m] < 0, "which names a crossing, which needs a line");
            RTMI_ARG(which[m] <= top, "which has a value above kmax - 1");
        }
    }
    Args A;
    rtmi_device_view v;
    RTMI_RC(prepare(b, which ? line : nullptr, kmax, who, &A, &v));
    RTMI_RC(on_device(t, who));
    const Axes& F = t->F;
    RTMI_ARG(A.F.qx == F.qx && A.F.qy == F.qy && A.F.ax == F.ax && A.F.bx == F.bx && A.F.inv_hx == F.inv_hx && A.F.ay == F.ay &&
                 A.F.by == F.by && A.F.inv_hy == F.inv_hy,
             "the batch's field has other sample axes than the handle's");
    RTMI_ARG((size_t)v.R == R, "the batch's view disagrees with its ray count");
    // rows in the caller's ray order
    std::vector<int32_t> rowof(R);
    int64_t rows = 0;
    for (size_t m = 0; m < R; m++) rowof[m] = (which && which[m] == RTMI_TOMO_SKIP) ? -1 : (int32_t)rows++;
    if (first_row) *first_row = t->rows;
    if (rows == 0) {
        if (nseg)
            for (size_t m = 0; m < R; m++) nseg[m] = -1;
        t->compile_ms = 0.0;
        return RTMI_OK;
    }
    TomoBlock blk;
    blk.first = t->rows;
    blk.rows = rows;
    struct Guard {
        TomoBlock* b;
        ~Guard() { if (b) b->release(); }
    } guard{&blk};
    DevMem mem;
    int32_t *d_which = nullptr, *d_rowof = nullptr;
    RTMI_HIP(mem.get(&d_rowof, R * sizeof(int32_t)));
    RTMI_HIP(hipMemcpy(d_rowof, rowof.data(), R * sizeof(int32_t), hipMemcpyHostToDevice));
    if (which) {
        RTMI_HIP(mem.get(&d_which, R * sizeof(int32_t)));
        RTMI_HIP(hipMemcpy(d_which, which, R * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const int64_t ns = rt::tomo_slices(rows);
    auto get = [&](void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 8) == hipSuccess; };
    const char* no_mem = "rtmi_tomo_append: hipMalloc failed";
    if (!get((void**)&blk.len, (size_t)rows * sizeof(int32_t)) || !get((void**)&blk.off, (size_t)(ns + 1) * sizeof(int64_t)))
        return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem);
    RTMI_HIP(hipMemset(blk.len, 0, (size_t)rows * sizeof(int32_t)));
    const dim3 gr = blocks((long)R), bs(256);
    RTMI_HIP(hipEventRecord(t->ev[0], nullptr));
    by_dtype(v.dtype, [&](auto q) {
        hipLaunchKernelGGL((k_tomo_walk<decltype(q), false>), gr, bs, 0, nullptr, rows_of<decltype(q)>(v), A, d_which, d_rowof, blk.len, nullptr,
                           nullptr, nullptr, nullptr);
    });
    RTMI_HIP(hipGetLastError());
    std::vector<int32_t> len((size_t)rows);
    std::vector<int64_t> off((size_t)ns + 1);
    RTMI_HIP(hipMemcpy(len.data(), blk.len, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    blk.segments = rt::tomo_offsets(len.data(), rows, off.data());
    blk.padded = off[(size_t)ns];
    if (!get((void**)&blk.base, (size_t)blk.padded * sizeof(int32_t)) || !get((void**)&blk.val, (size_t)blk.padded * 4 * sizeof(double)))
        return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem);
    RTMI_HIP(hipMemcpy(blk.off, off.data(), (size_t)(ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemsetAsync(blk.base, 0, (size_t)blk.padded * sizeof(int32_t), nullptr));
    RTMI_HIP(hipMemsetAsync(blk.val, 0, (size_t)blk.padded * 4 * sizeof(double), nullptr));
    RTMI_HIP(hipMemsetAsync(t->red_vmax(), 0, sizeof(unsigned long long), nullptr));
    by_dtype(v.dtype, [&](auto q) {
        hipLaunchKernelGGL((k_tomo_walk<decltype(q), true>), gr, bs, 0, nullptr, rows_of<decltype(q)>(v), A, d_which, d_rowof, blk.len, blk.off,
                           blk.base, blk.val, t->red_vmax());
    });
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipEventRecord(t->ev[1], nullptr));
    RTMI_HIP(hipEventSynchronize(t->ev[1]));
    float ms = 0.0f;
    RTMI_HIP(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]));
    double vmax = 0.0;
    RTMI_HIP(hipMemcpy(&vmax, t->red_vmax(), sizeof(double), hipMemcpyDeviceToHost));
    if (nseg)
        for (size_t m = 0; m < R; m++) nseg[m] = rowof[m] < 0 ? -1 : len[(size_t)rowof[m]];
    t->blocks.push_back(blk);
    guard.b = nullptr;
    t->rows += rows;
    t->segments += blk.segments;
    t->padded += blk.padded;
    t->vmax = std::fmax(t->vmax, vmax);
    t->compile_ms = ms;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_info(const rtmi_tomo* t, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_info";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(st, "null stats");
    fill_stats(t, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_read(const rtmi_tomo* t, int64_t* row_ptr, int32_t* base, double* val) {
    const char* who = "rtmi_tomo_read";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(row_ptr || (!base && !val), "base and val need row_ptr");
    if (!row_ptr) return RTMI_OK;
    RTMI_RC(on_device(t, who));
    int64_t at = 0;
    row_ptr[0] = 0;
    for (const TomoBlock& b : t->blocks) {
        const int64_t ns = rt::tomo_slices(b.rows);
        std::vector<int32_t> len((size_t)b.rows), hb;
        std::vector<int64_t> off((size_t)ns + 1);
        std::vector<double> hv;
        RTMI_HIP(hipMemcpy(len.data(), b.len, (size_t)b.rows * sizeof(int32_t), hipMemcpyDeviceToHost));
        RTMI_HIP(hipMemcpy(off.data(), b.off, (size_t)(ns + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (base) {
            hb.resize((size_t)b.padded);
            RTMI_HIP(hipMemcpy(hb.data(), b.base, (size_t)b.padded * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        if (val) {
            hv.resize((size_t)b.padded * 4);
            RTMI_HIP(hipMemcpy(hv.data(), b.val, (size_t)b.padded * 4 * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int64_t r = 0; r < b.rows; r++) {
            const int64_t o = off[(size_t)(r >> 6)];
            const int lane = (int)(r & 63);
            for (int32_t k = 0; k < len[(size_t)r]; k++, at++) {
                if (base) base[at] = hb[(size_t)rt::tomo_slot(o, k, lane)];
                if (val)
                    for (int q = 0; q < 4; q++) val[4 * at + q] = hv[(size_t)rt::tomo_value(o, k, q, lane)];
            }
            row_ptr[b.first + r + 1] = at;
        }
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_apply_dev(rtmi_tomo* t, const double* d_x, double* d_y, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_apply_dev";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(d_x, "null d_x");
    RTMI_ARG(d_y || t->rows == 0, "null d_y");
    RTMI_RC(on_device(t, who));
    RTMI_RC(check_device_pointer(t->device, who, d_x, t->nz() * sizeof(double), "d_x"));
    if (t->rows) RTMI_RC(check_device_pointer(t->device, who, d_y, (size_t)t->rows * sizeof(double), "d_y"));
    double ms = 0.0;
    RTMI_RC(apply_dev(t, who, 1, d_x, 0, d_y, 0, &ms));
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms;
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_apply(rtmi_tomo* t, const double* x, double* y, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_apply";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(x, "null x");
    RTMI_ARG(y || t->rows == 0, "null y");
    RTMI_RC(finite_all(who, x, t->nz(), "x has a value that is not finite"));
    RTMI_RC(on_device(t, who));
    DevMem mem;
    double *dx = nullptr, *dy = nullptr;
    RTMI_HIP(mem.get(&dx, t->nz() * sizeof(double)));
    RTMI_HIP(mem.get(&dy, (size_t)t->rows * sizeof(double)));
    RTMI_HIP(hipMemcpy(dx, x, t->nz() * sizeof(double), hipMemcpyHostToDevice));
    double ms = 0.0;
    RTMI_RC(apply_dev(t, who, 1, dx, 0, dy, 0, &ms));
    if (t->rows) RTMI_HIP(hipMemcpy(y, dy, (size_t)t->rows * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms;
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_transpose_dev(rtmi_tomo* t, const double* d_w, double* d_g, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_transpose_dev";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(d_w || t->rows == 0, "null d_w");
    RTMI_ARG(d_g, "null d_g");
    RTMI_RC(on_device(t, who));
    if (t->rows) RTMI_RC(check_device_pointer(t->device, who, d_w, (size_t)t->rows * sizeof(double), "d_w"));
    RTMI_RC(check_device_pointer(t->device, who, d_g, t->nz() * sizeof(double), "d_g"));
    bool range = false;
    double ms = 0.0;
    int64_t atomics = 0;
    int32_t e = 0;
    RTMI_RC(transpose_dev(t, who, 1, d_w, 0, d_g, 0, 1ull, true, &range, &ms, &atomics, &e));
    RTMI_ARG(!range, "Vmax max|w| is not a normal number (RTMI_LSQR_RANGE)");
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms; st->atomics = atomics; st->scale_exp = e;
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_transpose(rtmi_tomo* t, const double* w, double* g, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_transpose";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(w || t->rows == 0, "null w");
    RTMI_ARG(g, "null g");
    RTMI_RC(finite_all(who, w, (size_t)t->rows, "w has a value that is not finite"));
    RTMI_RC(on_device(t, who));
    DevMem mem;
    double *dw = nullptr, *dg = nullptr;
    RTMI_HIP(mem.get(&dw, (size_t)t->rows * sizeof(double)));
    RTMI_HIP(mem.get(&dg, t->nz() * sizeof(double)));
    if (t->rows) RTMI_HIP(hipMemcpy(dw, w, (size_t)t->rows * sizeof(double), hipMemcpyHostToDevice));
    bool range = false;
    double ms = 0.0;
    int64_t atomics = 0;
    int32_t e = 0;
    RTMI_RC(transpose_dev(t, who, 1, dw, 0, dg, 0, 1ull, true, &range, &ms, &atomics, &e));
    RTMI_ARG(!range, "Vmax max|w| is not a normal number (RTMI_LSQR_RANGE)");
    RTMI_HIP(hipMemcpy(g, dg, t->nz() * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms; st->atomics = atomics; st->scale_exp = e;
    }
    return RTMI_OK;
}

// ------------------------------------------------------------------------------------------------------------ model basis
// A separable model basis P = Py (x) Px from a coefficient grid c [my][mx] to the field's samples x [qy][qx], its exact transpose,
// second-difference rows, and the solver that takes both (rtmi_tomo_basis_*, rtmi_tomo_lsqr_basis; DESIGN.md section 27;
// rt_tomo_basis.h has the axis rules, the ranges and the pair as host loops).
//   k_basis_prolong     one lane per fine node: up to By Bx reads of c, which is small and stays in L2
//   k_basis_restrict_x  t [qy][mx]: a block takes one fine row and kBasisTile neighbouring coefficients, whose ranges overlap and
//                       together are one run of fine indices; the run goes through LDS in pieces of kBasisChunk samples, in
//                       ascending order, and every lane walks the part of its own range that lies in the piece, ascending
//   k_basis_restrict_y  g [my][mx]: lanes along l (coalesced), a loop over the range of fine rows, ascending
// No atomics: every sum has one owner and one order, the same bits under every launch shape.
struct rtmi_tomo_basis {
    int device = 0, qx = 0, qy = 0, mx = 0, my = 0, bx = 0, by = 0;
    int32_t *fx = nullptr, *fy = nullptr, *lox = nullptr, *hix = nullptr, *loy = nullptr, *hiy = nullptr;
    double *wx = nullptr, *wy = nullptr;
    double* t = nullptr;                        // [qy][mx]: between the two passes of the transposed operator
    size_t nf() const { return (size_t)qx * (size_t)qy; }
    size_t ng() const { return (size_t)mx * (size_t)my; }
    size_t bytes() const {
        return ((size_t)qx + (size_t)qy + 2 * ((size_t)mx + (size_t)my)) * sizeof(int32_t) +
               ((size_t)qx * bx + (size_t)qy * by + (size_t)qy * mx) * sizeof(double);
    }
    ~rtmi_tomo_basis() {
        for (void* p : {(void*)fx, (void*)fy, (void*)lox, (void*)hix, (void*)loy, (void*)hiy, (void*)wx, (void*)wy, (void*)t})
            if (p) (void)hipFree(p);
    }
};

namespace {

constexpr int kBasisTile = 256;       // coefficients of one block of k_basis_restrict_x: one per lane
constexpr int kBasisChunk = 1024;     // fine samples of a row in LDS at a time

__global__ void __launch_bounds__(256) k_basis_prolong(const double* __restrict__ c, int qx, int qy, int mx, int bx, int by,
                                                       const int32_t* __restrict__ fx, const double* __restrict__ wx,
                                                       const int32_t* __restrict__ fy, const double* __restrict__ wy, double* __restrict__ x) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= (long)qx * qy) return;
    const int i = (int)(n / qx), j = (int)(n % qx);
    const double* cc = c + (size_t)fy[i] * mx + fx[j];
    double acc = 0.0;
    for (int a = 0; a < by; a++) {
        double r = 0.0;
        for (int b = 0; b < bx; b++) r = __dadd_rn(r, __dmul_rn(wx[(size_t)j * bx + b], cc[(size_t)a * mx + b]));
        acc = __dadd_rn(acc, __dmul_rn(wy[(size_t)i * by + a], r));
    }
    x[n] = acc;
}

// grid (qy, tiles of l)
__global__ void __launch_bounds__(kBasisTile) k_basis_restrict_x(const double* __restrict__ x, int qx, int mx, int bx,
                                                                  const int32_t* __restrict__ fx, const double* __restrict__ wx,
                                                                  const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                  double* __restrict__ t) {
    __shared__ double row[kBasisChunk];
    const int i = (int)blockIdx.x, l0 = (int)blockIdx.y * kBasisTile, l = l0 + (int)threadIdx.x;
    const int l1 = min(l0 + kBasisTile, mx) - 1;                     // the tile's last coefficient; l0 <= l1 < mx
    const int j0 = lo[l0], j1 = hi[l1];                              // lo and hi are non-decreasing: the tile's run of fine indices
    const bool mine = l < mx;
    const int mlo = mine ? lo[l] : 0, mhi = mine ? hi[l] : 0;
    const double* xr = x + (size_t)i * qx;
    double s = 0.0;
    for (int c0 = j0; c0 < j1; c0 += kBasisChunk) {
        const int c1 = min(c0 + kBasisChunk, j1);
        for (int j = c0 + (int)threadIdx.x; j < c1; j += kBasisTile) row[j - c0] = xr[j];
        __syncthreads();
        for (int j = max(mlo, c0); j < min(mhi, c1); j++) s = __dadd_rn(s, __dmul_rn(wx[(size_t)j * bx + (l - fx[j])], row[j - c0]));
        __syncthreads();
    }
    if (mine) t[(size_t)i * mx + l] = s;
}

// grid (my, blocks of l)
__global__ void __launch_bounds__(256) k_basis_restrict_y(const double* __restrict__ t, int mx, int by, const int32_t* __restrict__ fy,
                                                          const double* __restrict__ wy, const int32_t* __restrict__ lo,
                                                          const int32_t* __restrict__ hi, double* __restrict__ g) {
    const int k = (int)blockIdx.x, l = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (l >= mx) return;
    double s = 0.0;
    for (int i = lo[k]; i < hi[k]; i++) s = __dadd_rn(s, __dmul_rn(wy[(size_t)i * by + (k - fy[i])], t[(size_t)i * mx + l]));
    g[(size_t)k * mx + l] = s;
}

int basis_on_device(const rtmi_tomo_basis* p, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == p->device, "the calling thread's current device is not the basis's");
    return RTMI_OK;
}

// launches only: the callers have checked the pointers and wait for the stream themselves
int basis_prolong_dev(rtmi_tomo_basis* p, const char* who, const double* d_c, double* d_x) {
    hipLaunchKernelGGL(k_basis_prolong, blocks((long)p->nf()), dim3(256), 0, nullptr, d_c, p->qx, p->qy, p->mx, p->bx, p->by, p->fx, p->wx, p->fy,
                       p->wy, d_x);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

int basis_restrict_dev(rtmi_tomo_basis* p, const char* who, const double* d_x, double* d_g) {
    hipLaunchKernelGGL(k_basis_restrict_x, dim3((unsigned)p->qy, (unsigned)((p->mx + kBasisTile - 1) / kBasisTile)), dim3(kBasisTile), 0, nullptr,
                       d_x, p->qx, p->mx, p->bx, p->fx, p->wx, p->lox, p->hix, p->t);
    RTMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_basis_restrict_y, dim3((unsigned)p->my, (unsigned)((p->mx + 255) / 256)), dim3(256), 0, nullptr, p->t, p->mx, p->by, p->fy,
                       p->wy, p->loy, p->hiy, d_g);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

// upload + launch + download of one of the pair: n_in values in, n_out values out
int basis_host_call(rtmi_tomo_basis* p, const char* who, bool restrict_, const double* in, double* out) {
    const size_t n_in = restrict_ ? p->nf() : p->ng(), n_out = restrict_ ? p->ng() : p->nf();
    RTMI_RC(finite_all(who, in, n_in, restrict_ ? "x has a value that is not finite" : "c has a value that is not finite"));
    RTMI_RC(basis_on_device(p, who));
    DevMem mem;
    double *di = nullptr, *dout = nullptr;
    RTMI_HIP(mem.get(&di, n_in * sizeof(double)));
    RTMI_HIP(mem.get(&dout, n_out * sizeof(double)));
    RTMI_HIP(hipMemcpy(di, in, n_in * sizeof(double), hipMemcpyHostToDevice));
    RTMI_RC(restrict_ ? basis_restrict_dev(p, who, di, dout) : basis_prolong_dev(p, who, di, dout));
    RTMI_HIP(hipMemcpy(out, dout, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_bspline_axis(int32_t q, int32_t m, int32_t degree, int32_t* first, double* wgt) {
    const char* who = "rtmi_bspline_axis";
    RTMI_ARG(first, "null first");
    RTMI_ARG(wgt, "null wgt");
    RTMI_ARG(degree == 0 || degree == 1 || degree == 3, "degree must be 0, 1 or 3");
    RTMI_ARG(q >= 2, "q must be >= 2");
    RTMI_ARG(m >= degree + 1, "m must be >= degree + 1");
    RTMI_ARG(rt::bspline_axis(q, m, degree, first, wgt), "sizes the helper cannot do");
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_basis_create(const rtmi_tomo* t, int32_t mx, int32_t bx, const int32_t* first_x, const double* wgt_x, int32_t my,
                                       int32_t by, const int32_t* first_y, const double* wgt_y, rtmi_tomo_basis** out) {
    const char* who = "rtmi_tomo_basis_create";
    RTMI_ARG(t, "null handle");
    RTMI_ARG(first_x, "null first_x");
    RTMI_ARG(wgt_x, "null wgt_x");
    RTMI_ARG(first_y, "null first_y");
    RTMI_ARG(wgt_y, "null wgt_y");
    RTMI_ARG(out, "null out");
    RTMI_ARG(mx >= 1 && my >= 1, "mx and my must be >= 1");
    const int qx = t->F.qx, qy = t->F.qy;
    struct One { const char* name; int q, m, B; const int32_t* first; const double* wgt; };
    for (const One& a : {One{"x", qx, mx, bx, first_x, wgt_x}, One{"y", qy, my, by, first_y, wgt_y}}) {
        int64_t at = -1;
        const char* why = rt::basis_axis_check(a.q, a.m, a.B, a.first, a.wgt, &at);
        if (why) RTMI_ARG(false, std::string("axis ") + a.name + (at >= 0 ? ", index " + std::to_string(at) : std::string()) + ": " + why);
    }
    RTMI_RC(on_device(t, who));
    rtmi_tomo_basis* p = new (std::nothrow) rtmi_tomo_basis;
    if (!p) return rtmi_internal_fail(RTMI_ERR_ALLOC, "rtmi_tomo_basis_create: out of host memory");
    p->device = t->device;
    p->qx = qx; p->qy = qy; p->mx = mx; p->my = my; p->bx = bx; p->by = by;
    std::vector<int32_t> lox((size_t)mx), hix((size_t)mx), loy((size_t)my), hiy((size_t)my);
    rt::basis_ranges(qx, mx, bx, first_x, lox.data(), hix.data());
    rt::basis_ranges(qy, my, by, first_y, loy.data(), hiy.data());
    auto up = [&](auto** dst, const auto* src, size_t n) {
        hipError_t e = hipMalloc((void**)dst, n * sizeof(**dst));
        if (e == hipSuccess) e = hipMemcpy(*dst, src, n * sizeof(**dst), hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up(&p->fx, first_x, (size_t)qx);
    if (e == hipSuccess) e = up(&p->fy, first_y, (size_t)qy);
    if (e == hipSuccess) e = up(&p->wx, wgt_x, (size_t)qx * bx);
    if (e == hipSuccess) e = up(&p->wy, wgt_y, (size_t)qy * by);
    if (e == hipSuccess) e = up(&p->lox, lox.data(), (size_t)mx);
    if (e == hipSuccess) e = up(&p->hix, hix.data(), (size_t)mx);
    if (e == hipSuccess) e = up(&p->loy, loy.data(), (size_t)my);
    if (e == hipSuccess) e = up(&p->hiy, hiy.data(), (size_t)my);
    if (e == hipSuccess) e = hipMalloc((void**)&p->t, (size_t)qy * mx * sizeof(double));
    if (e != hipSuccess) {
        delete p;
        return rtmi_internal_fail(e == hipErrorOutOfMemory ? RTMI_ERR_ALLOC : RTMI_ERR_HIP,
                                  (std::string(who) + ": device memory: " + hipGetErrorString(e)).c_str());
    }
    *out = p;
    return RTMI_OK;
}

RTMI_EXPORT void rtmi_tomo_basis_destroy(rtmi_tomo_basis* p) { delete p; }

RTMI_EXPORT int rtmi_tomo_basis_prolong(rtmi_tomo_basis* p, const double* c, double* x) {
    const char* who = "rtmi_tomo_basis_prolong";
    RTMI_ARG(p, "null handle");
    RTMI_ARG(c, "null c");
    RTMI_ARG(x, "null x");
    return basis_host_call(p, who, false, c, x);
}

RTMI_EXPORT int rtmi_tomo_basis_restrict(rtmi_tomo_basis* p, const double* x, double* g) {
    const char* who = "rtmi_tomo_basis_restrict";
    RTMI_ARG(p, "null handle");
    RTMI_ARG(x, "null x");
    RTMI_ARG(g, "null g");
    return basis_host_call(p, who, true, x, g);
}

RTMI_EXPORT int rtmi_tomo_basis_prolong_dev(rtmi_tomo_basis* p, const double* d_c, double* d_x) {
    const char* who = "rtmi_tomo_basis_prolong_dev";
    RTMI_ARG(p, "null handle");
    RTMI_ARG(d_c, "null d_c");
    RTMI_ARG(d_x, "null d_x");
    RTMI_RC(basis_on_device(p, who));
    RTMI_RC(check_device_pointer(p->device, who, d_c, p->ng() * sizeof(double), "d_c"));
    RTMI_RC(check_device_pointer(p->device, who, d_x, p->nf() * sizeof(double), "d_x"));
    RTMI_RC(basis_prolong_dev(p, who, d_c, d_x));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_basis_restrict_dev(rtmi_tomo_basis* p, const double* d_x, double* d_g) {
    const char* who = "rtmi_tomo_basis_restrict_dev";
    RTMI_ARG(p, "null handle");
    RTMI_ARG(d_x, "null d_x");
    RTMI_ARG(d_g, "null d_g");
    RTMI_RC(basis_on_device(p, who));
    RTMI_RC(check_device_pointer(p->device, who, d_x, p->nf() * sizeof(double), "d_x"));
    RTMI_RC(check_device_pointer(p->device, who, d_g, p->ng() * sizeof(double), "d_g"));
    RTMI_RC(basis_restrict_dev(p, who, d_x, d_g));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    return RTMI_OK;
}

// ------------------------------------------------------------------------------------------------------------ many vectors at once
// The products' entries for nrhs planes (rtmi_tomo_apply_multi, _transpose_multi)
namespace {

// the public transposed calls' end: a refusal that names the first column out of range, else the stats
int transpose_done(const rtmi_tomo* t, const char* who, int nrhs, const bool* range, const int32_t* exps, double ms, int64_t atomics,
                   rtmi_tomo_stats* st) {
    for (int c = 0; c < nrhs; c++)
        RTMI_ARG(!range[c], "column " + std::to_string(c) + ": Vmax max|w| is not a normal number (RTMI_LSQR_RANGE)");
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms; st->atomics = atomics;
        int32_t e = 0;
        bool first = true;
        for (int c = 0; c < nrhs; c++)
            if (exps[c] != 0 && (first || exps[c] > e)) { e = exps[c]; first = false; }
        st->scale_exp = e;
    }
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_tomo_apply_multi_dev(rtmi_tomo* t, int32_t nrhs, const double* d_x, double* d_y, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_apply_multi_dev";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG(d_x, "null d_x");
    RTMI_ARG(d_y || t->rows == 0, "null d_y");
    RTMI_RC(on_device(t, who));
    RTMI_RC(check_device_pointer(t->device, who, d_x, (size_t)nrhs * t->nz() * sizeof(double), "d_x"));
    if (t->rows) RTMI_RC(check_device_pointer(t->device, who, d_y, (size_t)nrhs * (size_t)t->rows * sizeof(double), "d_y"));
    double ms = 0.0;
    RTMI_RC(apply_dev(t, who, nrhs, d_x, t->nz(), d_y, (size_t)t->rows, &ms));
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms;
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_apply_multi(rtmi_tomo* t, int32_t nrhs, const double* x, double* y, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_apply_multi";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG(x, "null x");
    RTMI_ARG(y || t->rows == 0, "null y");
    const size_t nx = (size_t)nrhs * t->nz(), ny = (size_t)nrhs * (size_t)t->rows;
    RTMI_RC(finite_all(who, x, nx, "x has a value that is not finite"));
    RTMI_RC(on_device(t, who));
    DevMem mem;
    double *dx = nullptr, *dy = nullptr;
    RTMI_HIP(mem.get(&dx, nx * sizeof(double)));
    RTMI_HIP(mem.get(&dy, ny * sizeof(double)));
    RTMI_HIP(hipMemcpy(dx, x, nx * sizeof(double), hipMemcpyHostToDevice));
    double ms = 0.0;
    RTMI_RC(apply_dev(t, who, nrhs, dx, t->nz(), dy, (size_t)t->rows, &ms));
    if (ny) RTMI_HIP(hipMemcpy(y, dy, ny * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        fill_stats(t, st);
        st->kernel_ms = ms;
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tomo_transpose_multi_dev(rtmi_tomo* t, int32_t nrhs, const double* d_w, double* d_g, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_transpose_multi_dev";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG(d_w || t->rows == 0, "null d_w");
    RTMI_ARG(d_g, "null d_g");
    RTMI_RC(on_device(t, who));
    if (t->rows) RTMI_RC(check_device_pointer(t->device, who, d_w, (size_t)nrhs * (size_t)t->rows * sizeof(double), "d_w"));
    RTMI_RC(check_device_pointer(t->device, who, d_g, (size_t)nrhs * t->nz() * sizeof(double), "d_g"));
    bool range[kMultiMax];
    int32_t exps[kMultiMax];
    double ms = 0.0;
    int64_t atomics = 0;
    RTMI_RC(transpose_dev(t, who, nrhs, d_w, (size_t)t->rows, d_g, t->nz(), all_cols(nrhs), true, range, &ms, &atomics, exps));
    return transpose_done(t, who, nrhs, range, exps, ms, atomics, st);
}

RTMI_EXPORT int rtmi_tomo_transpose_multi(rtmi_tomo* t, int32_t nrhs, const double* w, double* g, rtmi_tomo_stats* st) {
    const char* who = "rtmi_tomo_transpose_multi";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG(w || t->rows == 0, "null w");
    RTMI_ARG(g, "null g");
    const size_t nw = (size_t)nrhs * (size_t)t->rows, ng = (size_t)nrhs * t->nz();
    RTMI_RC(finite_all(who, w, nw, "w has a value that is not finite"));
    RTMI_RC(on_device(t, who));
    DevMem mem;
    double *dw = nullptr, *dg = nullptr;
    RTMI_HIP(mem.get(&dw, nw * sizeof(double)));
    RTMI_HIP(mem.get(&dg, ng * sizeof(double)));
    if (nw) RTMI_HIP(hipMemcpy(dw, w, nw * sizeof(double), hipMemcpyHostToDevice));
    bool range[kMultiMax];
    int32_t exps[kMultiMax];
    double ms = 0.0;
    int64_t atomics = 0;
    RTMI_RC(transpose_dev(t, who, nrhs, dw, (size_t)t->rows, dg, t->nz(), all_cols(nrhs), true, range, &ms, &atomics, exps));
    RTMI_RC(transpose_done(t, who, nrhs, range, exps, ms, atomics, nullptr));
    RTMI_HIP(hipMemcpy(g, dg, ng * sizeof(double), hipMemcpyDeviceToHost));
    return transpose_done(t, who, nrhs, range, exps, ms, atomics, st);
}

namespace {

// ------------------------------------------------------------------------------------------------------------ solver
// (reg's weights are checked by check_reg, rt_tomo_reg.h)
// Every solver's body, for S columns: the loop of rt_lsqr_device.h over the coefficient grid G ([my][mx] with a basis, [qy][qx]
// without), with first- (d1) and second-difference (d2) rows on G, on planes.  The products and the vector passes are one launch
// for all columns; the basis and regulariser kernels, which work on model-sized vectors, are launched per live column.  The loop
// sees the options row_weight ([S][rows] with wr_cols, else [rows] for all) and col_scale; the start model is a fine one, so its
// residual is taken here, before the loop, and it is added here, after P.  The callers have checked the arguments.
int tomo_lsqr_run(const char* who, rtmi_tomo* t, rtmi_tomo_basis* p, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo, const double* d1,
                  const double* d2, int S, bool wr_cols, const double* rhs, double* c, double* x, double* history, rtmi_lsqr_stats* st) {
    const size_t rows = (size_t)t->rows, nm = t->nz();
    const size_t gx = p ? (size_t)p->mx : (size_t)t->F.qx, gy = p ? (size_t)p->my : (size_t)t->F.qy, ng = gx * gy;
    const size_t n1x = d1 ? gy * (gx - 1) : 0, n1y = d1 ? (gy - 1) * gx : 0;
    const size_t n2x = d2 && gx > 2 ? gy * (gx - 2) : 0, n2y = d2 && gy > 2 ? (gy - 2) * gx : 0;
    const size_t per = rows + n1x + n1y + n2x + n2y;
    const double t_begin = now_ms();
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    RTMI_RC(ensure_cols(t, who, S));
    DevMem mem;
    size_t doubles = 0;
    auto get = [&](double** q, size_t n) {
        doubles += n;
        return mem.get(q, n * sizeof(double)) == hipSuccess;
    };
    double *u = nullptr, *Av = nullptr, *v = nullptr, *w = nullptr, *yd = nullptr, *Atu = nullptr, *xf = nullptr, *gf = nullptr, *x0 = nullptr;
    for (double** q : {&u, &Av})
        if (!get(q, S * per)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    for (double** q : {&v, &w, &yd, &Atu})
        if (!get(q, S * ng)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    if (p)
        for (double** q : {&xf, &gf})
            if (!get(q, S * nm)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    if (lo && lo->x0) {
        if (!get(&x0, nm)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(x0, lo->x0, nm * sizeof(double), hipMemcpyHostToDevice));
    }
    // the row weights cover the `rows` observations; a regulariser's rows carry none
    LsqrOptions O;
    size_t nopt = 0;
    RTMI_RC(lsqr_upload_options(who, mem, lo, S, wr_cols, rows, per, ng, &O, &nopt));
    doubles += nopt;
    const Vec V{t->red, t->cus, S};
    const unsigned long long all = all_cols(S);
    double operator_ms = 0.0;
    auto each = [&](unsigned long long mask, auto&& f) {
        for (int s = 0; s < S; s++)
            if (mask & col_bit(s)) RTMI_RC(f((size_t)s));
        return (int)RTMI_OK;
    };
    // the stacked operator [A P | Dx | Dy | Dxx | Dyy] on the planes s [S][G], and its transpose
    auto Ax = [&](const double* s, double* y, unsigned long long mask) {
        const double t0 = now_ms();
        if (p) RTMI_RC(each(mask, [&](size_t k) { return basis_prolong_dev(p, who, s + k * ng, xf + k * nm); }));
        RTMI_RC(apply_dev(t, who, S, p ? xf : s, nm, y, per, nullptr));
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;                         // the regulariser's forward rows are outside it
        if (d1 || d2)
            RTMI_RC(each(mask, [&](size_t k) {
                const double* sk = s + k * ng;
                double* yk = y + k * per + rows;
                if (d1) hipLaunchKernelGGL(k_tomo_diff, blocks((long)ng), dim3(256), 0, nullptr, sk, (int)gx, (int)gy, d1[0], d1[1], yk, yk + n1x);
                if (d2)
                    hipLaunchKernelGGL(k_tomo_diff2, blocks((long)ng), dim3(256), 0, nullptr, sk, (int)gx, (int)gy, d2[0], d2[1], yk + n1x + n1y,
                                       yk + n1x + n1y + n2x);
                RTMI_HIP(hipGetLastError());
                return (int)RTMI_OK;
            }));
        return (int)RTMI_OK;
    };
    auto At = [&](const double* s, double* g, unsigned long long mask, bool* range) {
        const double t0 = now_ms();
        RTMI_RC(transpose_dev(t, who, S, s, per, p ? gf : g, p ? nm : ng, mask, false, range, nullptr, nullptr, nullptr));
        unsigned long long ok = 0ull;
        for (int k = 0; k < S; k++)
            if ((mask & col_bit(k)) && !range[k]) ok |= col_bit(k);
        if (p || d1 || d2) {
            RTMI_RC(each(ok, [&](size_t k) {
                double* gk = g + k * ng;
                const double* sk = s + k * per + rows;
                if (p) RTMI_RC(basis_restrict_dev(p, who, gf + k * nm, gk));
                if (d1 || d2) {
                    hipLaunchKernelGGL(k_tomo_reg_t, blocks((long)ng), dim3(256), 0, nullptr, gk, (int)gx, (int)gy, d1 ? sk : nullptr,
                                       d1 ? sk + n1x : nullptr, d1 ? d1[0] : 0.0, d1 ? d1[1] : 0.0, d2 ? sk + n1x + n1y : nullptr,
                                       d2 ? sk + n1x + n1y + n2x : nullptr, d2 ? d2[0] : 0.0, d2 ? d2[1] : 0.0);
                    RTMI_HIP(hipGetLastError());
                }
                return (int)RTMI_OK;
            }));
        }
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
        return (int)RTMI_OK;
    };
    // the right-hand sides go up once: column s into the first `rows` values of plane s
    RTMI_HIP(hipMemsetAsync(u, 0, (size_t)S * per * sizeof(double), nullptr));
    RTMI_HIP(hipMemsetAsync(yd, 0, (size_t)S * ng * sizeof(double), nullptr));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    RTMI_HIP(hipMemcpy2D(u, per * sizeof(double), rhs, rows * sizeof(double), rows * sizeof(double), (size_t)S, hipMemcpyHostToDevice));
    if (x0) {                                                                         // u = fl(rhs - A x0) over the data rows; A x0 once
        const double t0 = now_ms();
        RTMI_RC(apply_dev(t, who, 1, x0, 0, Av, 0, nullptr));
        RTMI_RC(lsqr_sub_start(who, V, u, per, Av, rows));
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
    }
    std::vector<rtmi_lsqr_stats> out((size_t)S);
    RTMI_RC(lsqr_loop(who, V, lp, per, ng, LsqrVectors{u, Av, v, w, yd, Atu}, Ax, At, history, out.data(), O));   // yd = fl(dc y): c
    if (c) RTMI_HIP(hipMemcpy(c, yd, (size_t)S * ng * sizeof(double), hipMemcpyDeviceToHost));
    double* xd = yd;
    if (p) {
        RTMI_RC(each(all, [&](size_t k) { return basis_prolong_dev(p, who, yd + k * ng, xf + k * nm); }));
        xd = xf;
    }
    if (x0) RTMI_RC(lsqr_add_start(who, V, xd, nm, x0, nm));
    RTMI_HIP(hipMemcpy(x, xd, (size_t)S * nm * sizeof(double), hipMemcpyDeviceToHost));
    const double total = now_ms() - t_begin;
    const int64_t bytes = (int64_t)(doubles * sizeof(double) + t->bytes() + (p ? p->bytes() : 0));
    for (int s = 0; s < S; s++) {
        out[(size_t)s].total_ms = total;
        out[(size_t)s].operator_ms = operator_ms;
        out[(size_t)s].bytes_device = bytes;
        if (st) st[s] = out[(size_t)s];
    }
    return RTMI_OK;
}

// rtmi_tomo_lsqr and _weighted: their checks, then the body with one column, no basis and the first differences of `smooth`
int tomo_lsqr_single(const char* who, rtmi_tomo* t, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo, const double smooth[2],
                     const double* rhs, double* x, double* history, rtmi_lsqr_stats* st) {
    RTMI_ARG(t, "null handle");
    RTMI_ARG(lp, "null params");
    RTMI_ARG(rhs, "null rhs");
    RTMI_ARG(x, "null x");
    RTMI_RC(lsqr_check_params(who, lp));
    if (smooth)
        RTMI_ARG(std::isfinite(smooth[0]) && smooth[0] >= 0.0 && std::isfinite(smooth[1]) && smooth[1] >= 0.0,
                 "smooth must be finite and >= 0");
    RTMI_ARG(t->rows >= 1, "the handle has no rows");
    RTMI_RC(finite_all(who, rhs, (size_t)t->rows, "rhs has a value that is not finite"));
    RTMI_RC(lsqr_check_options(who, lo, (size_t)t->rows, t->nz()));
    RTMI_RC(on_device(t, who));
    return tomo_lsqr_run(who, t, nullptr, lp, lo, smooth, nullptr, 1, false, rhs, nullptr, x, history, st);
}

// rtmi_tomo_lsqr_basis and _multi, after their own arguments: the basis, the parameters, the nrhs right-hand sides and the options
int check_solve(const char* who, const rtmi_tomo* t, const rtmi_tomo_basis* p, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo,
                size_t nrhs, size_t nwr, const double* rhs, const double* x) {
    if (p)
        RTMI_ARG(p->qx == t->F.qx && p->qy == t->F.qy && p->device == t->device, "the basis was made for another shape or device than the handle's");
    RTMI_ARG(lp, "null params");
    RTMI_ARG(rhs, "null rhs");
    RTMI_ARG(x, "null x");
    RTMI_RC(lsqr_check_params(who, lp));
    RTMI_ARG(t->rows >= 1, "the handle has no rows");
    RTMI_RC(finite_all(who, rhs, nrhs * (size_t)t->rows, "rhs has a value that is not finite"));
    if (lo) {
        rtmi_lsqr_options coarse = *lo, fine = *lo;                               // col_scale has |G| values, x0 qy qx
        coarse.x0 = nullptr;
        fine.row_weight = nullptr; fine.col_scale = nullptr;
        RTMI_RC(lsqr_check_options(who, &coarse, nwr, p ? p->ng() : t->nz()));
        RTMI_RC(lsqr_check_options(who, &fine, 0, t->nz()));
    }
    return on_device(t, who);
}

}  // namespace

RTMI_EXPORT int rtmi_tomo_lsqr(rtmi_tomo* t, const rtmi_lsqr_params* lp, const double smooth[2], const double* rhs, double* x,
                               double* history, rtmi_lsqr_stats* st) {
    return tomo_lsqr_single("rtmi_tomo_lsqr", t, lp, nullptr, smooth, rhs, x, history, st);
}

RTMI_EXPORT int rtmi_tomo_lsqr_weighted(rtmi_tomo* t, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo, const double smooth[2],
                                        const double* rhs, double* x, double* history, rtmi_lsqr_stats* st) {
    return tomo_lsqr_single("rtmi_tomo_lsqr_weighted", t, lp, lo, smooth, rhs, x, history, st);
}

RTMI_EXPORT int rtmi_tomo_lsqr_basis(rtmi_tomo* t, rtmi_tomo_basis* p, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo,
                                     const rtmi_tomo_reg* reg, const double* rhs, double* c, double* x, double* history,
                                     rtmi_lsqr_stats* st) {
    const char* who = "rtmi_tomo_lsqr_basis";
    RTMI_ARG(t, "null handle");
    const double *d1 = nullptr, *d2 = nullptr;
    RTMI_RC(check_reg(who, reg, &d1, &d2));
    RTMI_RC(check_solve(who, t, p, lp, lo, 1, (size_t)t->rows, rhs, x));
    return tomo_lsqr_run(who, t, p, lp, lo, d1, d2, 1, false, rhs, c, x, history, st);
}

RTMI_EXPORT int rtmi_tomo_lsqr_multi(rtmi_tomo* t, rtmi_tomo_basis* p, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo,
                                     const rtmi_tomo_reg* reg, int32_t nrhs, int32_t flags, const double* rhs, double* c, double* x,
                                     double* history, rtmi_lsqr_stats* st) {
    const char* who = "rtmi_tomo_lsqr_multi";
    RTMI_ARG(t, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG((flags & ~RTMI_LSQR_MULTI_ROW_WEIGHT) == 0, "flags has bits other than RTMI_LSQR_MULTI_ROW_WEIGHT");
    const double *d1 = nullptr, *d2 = nullptr;
    RTMI_RC(check_reg(who, reg, &d1, &d2));
    const bool wr_cols = (flags & RTMI_LSQR_MULTI_ROW_WEIGHT) != 0;
    RTMI_RC(check_solve(who, t, p, lp, lo, (size_t)nrhs, (wr_cols ? (size_t)nrhs : 1) * (size_t)t->rows, rhs, x));
    if (history) std::memset(history, 0, (size_t)nrhs * (size_t)lp->iter_lim * 4 * sizeof(double));
    return tomo_lsqr_run(who, t, p, lp, lo, d1, d2, (int)nrhs, wr_cols, rhs, c, x, history, st);
}
