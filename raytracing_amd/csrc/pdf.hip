// pdf.hip -- the location pdf of a search on a locator handle's tables: moments, confidence regions, marginals and samples
// (rtmi_locate_pdf, rtmi_locate_edt_pdf and their _dev forms; include/rtmi.h).  The search is
// rtmi_locate_dev / rtmi_locate_edt_dev on a group of events with its maps written to a buffer of this unit; the kernels here
// read that buffer while it is resident, and no map leaves the device.  The arithmetic of a node and of the results is
// rt_pdf.h's; the kernels only decide who runs it on what.
//   k_pdf_mass      one lane per node of a tile of 256, one block per (run of tiles, event): the mass of every node, the tile's
//                   mass, the block's histogram in LDS, the moments in two-word lane accumulators; flushed by integer atomics
//   k_pdf_scan      one block per event: the tile masses into their inclusive prefix
//   k_pdf_sample    one wave per sample: binary search of the tile, then a wave prefix over its 256 masses, four nodes a lane
//   k_pdf_marginal  one lane per column or row: the integer sum over the event's mass
// Every sum is a sum of integers: the same bits in every schedule.  No atomics on floating point.
#include "rtmi_locator.h"

#include "rt_pdf.h"

namespace {

constexpr size_t kGroupBudget = (size_t)256 << 20;     // the most a group of events takes on the device: maps, histograms, tile masses
constexpr size_t kMaxGroup = 32768;                     // events of a group: blockIdx.y
constexpr unsigned kTilesPerBlock = 64;                 // a block's run of tiles: its histogram is flushed once per run

// what the kernels know of an event (host -> device, per group)
struct PdfEvent {
    int32_t node, p;            // the best node (-1: none); EDT: the power
    double ref, b;              // obj* or value*; least squares: sw* 0.5 / sigma^2
};

// an event's sums on the device, plain two's complement words from 0: rt::PdfSums in words
constexpr int kAccWords = 13;
enum : int { aZ = 0, aRim = 1, aNz = 2, aSx = 3, aSy = 5, aSxx = 7, aSxy = 9, aSyy = 11 };
static_assert(sizeof(rt::PdfSums) == kAccWords * sizeof(unsigned long long), "PdfSums is the accumulator's words");

struct I128 {
    unsigned long long lo;
    long long hi;
};
__device__ __forceinline__ void add_term(I128& a, long long t) {
    const unsigned long long u = (unsigned long long)t;
    a.lo += u;
    a.hi += (t < 0 ? -1 : 0) + (a.lo < u ? 1 : 0);
}
__device__ __forceinline__ I128 wave_sum(I128 a) {
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long lo = (unsigned long long)__shfl_xor((long long)a.lo, off);
        const long long hi = __shfl_xor(a.hi, off);
        a.lo += lo;
        a.hi += hi + (a.lo < lo ? 1 : 0);
    }
    return a;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 1; off < 64; off <<= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}
// w[0], w[1] += a, modulo 2^128: the low word's carry is read from the value its add returned
__device__ __forceinline__ void atomic_add128(unsigned long long* w, I128 a) {
    if (a.lo == 0 && a.hi == 0) return;
    unsigned long long h = (unsigned long long)a.hi;
    if (a.lo) {
        const unsigned long long old = atomicAdd(w, a.lo);
        h += (old + a.lo) < old ? 1ull : 0ull;
    }
    if (h) atomicAdd(w + 1, h);
}

template <bool EDT> __device__ __forceinline__ unsigned long long node_mass(double v, const PdfEvent& ev, const double* tab) {
    return rt::pdf_mass(EDT ? rt::pdf_rho_edt(v, ev.ref, ev.p) : rt::pdf_rho_l2(v, ev.ref, ev.b, tab));
}

// Block (bx, e) walks tiles bx tpb .. of event e of the group.  An event without a best node has mass nowhere: its tiles get 0.
template <bool EDT>
__global__ void __launch_bounds__(kTile) k_pdf_mass(const double* __restrict__ maps, size_t nn, unsigned nx, unsigned ny, unsigned ntiles,
                                                    unsigned tpb, const PdfEvent* __restrict__ evs, unsigned long long* __restrict__ acc,
                                                    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ tile_mass,
                                                    unsigned long long* __restrict__ col, unsigned long long* __restrict__ row) {
    __shared__ double tab[rt::kExpTableLen];
    __shared__ unsigned hcount[rt::kPdfBins];
    __shared__ unsigned long long hmass[rt::kPdfBins];
    __shared__ unsigned long long wsum[2][kTile / 64];
    const int tid = (int)threadIdx.x;
    const size_t e = blockIdx.y;
    if (tid < rt::kExpTableLen) tab[tid] = rt::np_exp_tables()[tid];
    for (int i = tid; i < rt::kPdfBins; i += kTile) {
        hcount[i] = 0u;
        hmass[i] = 0ull;
    }
    __syncthreads();
    const PdfEvent ev = evs[e];
    const bool live = ev.node >= 0;
    const int bx0 = live ? (int)((unsigned)ev.node % nx) : 0, by0 = live ? (int)((unsigned)ev.node / nx) : 0;
    const double* __restrict__ map = maps + e * nn;
    unsigned long long Z = 0, rim = 0, nz = 0;
    I128 Sx{0, 0}, Sy{0, 0}, Sxx{0, 0}, Sxy{0, 0}, Syy{0, 0};
    const unsigned t0 = blockIdx.x * tpb, t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    for (unsigned t = t0; t < t1; t++) {
        const size_t x = (size_t)t * kTile + tid;
        unsigned long long m = 0;
        if (live && x < nn) m = node_mass<EDT>(map[x], ev, tab);
        if (m) {
            const unsigned ix = (unsigned)x % nx, iy = (unsigned)x / nx;
            const long long di = (long long)ix - bx0, dj = (long long)iy - by0, mi = (long long)m * di, mj = (long long)m * dj;
            Z += m;
            nz += 1;
            if (ix == 0 || ix == nx - 1 || iy == 0 || iy == ny - 1) rim += m;
            add_term(Sx, mi);
            add_term(Sy, mj);
            add_term(Sxx, mi * di);
            add_term(Sxy, mi * dj);
            add_term(Syy, mj * dj);
            const int bin = rt::pdf_bin(m);
            atomicAdd(&hcount[bin], 1u);
            atomicAdd(&hmass[bin], m);
            if (col) atomicAdd(col + e * nx + ix, m);    // a wave's lanes are nx-periodic: distinct addresses where nx >= 64
        }
        if (row && __ballot(m != 0)) {                   // a wave's lanes of one row lie side by side: their sum, one atomic per row
            const int lane = tid & 63;
            const unsigned iy = x < nn ? (unsigned)x / nx : kNoNode;
            unsigned long long s = m;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long v = (unsigned long long)__shfl_down((long long)s, off);
                const unsigned jy = __shfl_down(iy, off);
                if (lane + off < 64 && jy == iy) s += v;
            }
            const unsigned py = __shfl_up(iy, 1);
            if (s && (lane == 0 || py != iy)) atomicAdd(row + e * ny + iy, s);
        }
        const unsigned long long ws = wave_sum(m);
        if ((tid & 63) == 0) wsum[t & 1][tid >> 6] = ws;
        __syncthreads();                                 // one per tile: the next tile writes the other half of wsum
        if (tid == 0) tile_mass[e * ntiles + t] = (wsum[t & 1][0] + wsum[t & 1][1]) + (wsum[t & 1][2] + wsum[t & 1][3]);
    }
    if (!live) return;
    __syncthreads();
    for (int i = tid; i < rt::kPdfBins; i += kTile) {
        if (hcount[i]) {
            atomicAdd(hist + (e * rt::kPdfBins + i) * 2, (unsigned long long)hcount[i]);
            atomicAdd(hist + (e * rt::kPdfBins + i) * 2 + 1, hmass[i]);
        }
    }
    Z = wave_sum(Z);
    rim = wave_sum(rim);
    nz = wave_sum(nz);
    Sx = wave_sum(Sx);
    Sy = wave_sum(Sy);
    Sxx = wave_sum(Sxx);
    Sxy = wave_sum(Sxy);
    Syy = wave_sum(Syy);
    if ((tid & 63) == 0 && nz) {
        unsigned long long* a = acc + e * kAccWords;
        atomicAdd(a + aZ, Z);
        if (rim) atomicAdd(a + aRim, rim);
        atomicAdd(a + aNz, nz);
        atomic_add128(a + aSx, Sx);
        atomic_add128(a + aSy, Sy);
        atomic_add128(a + aSxx, Sxx);
        atomic_add128(a + aSxy, Sxy);
        atomic_add128(a + aSyy, Syy);
    }
}

// tile_mass [event][ntiles] -> its inclusive prefix, in place.  Lane l takes a run of ceil(ntiles / 256) tiles.
__global__ void __launch_bounds__(256) k_pdf_scan(unsigned long long* __restrict__ tile_mass, unsigned ntiles) {
    __shared__ unsigned long long part[256];
    const int tid = (int)threadIdx.x;
    unsigned long long* tm = tile_mass + (size_t)blockIdx.x * ntiles;
    const unsigned run = (ntiles + 255) / 256;
    const unsigned a = (unsigned)tid * run < ntiles ? (unsigned)tid * run : ntiles, b = a + run < ntiles ? a + run : ntiles;
    unsigned long long s = 0;
    for (unsigned i = a; i < b; i++) s += tm[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long c = 0;
        for (int i = 0; i < 256; i++) {
            const unsigned long long v = part[i];
            part[i] = c;
            c += v;
        }
    }
    __syncthreads();
    s = part[tid];
    for (unsigned i = a; i < b; i++) {
        s += tm[i];
        tm[i] = s;
    }
}

// Wave w of block (bx, e) draws sample 4 bx + w of event e: the first tile whose inclusive prefix exceeds q, then the first node
// in it.  Lane l recomputes the masses of nodes 4 l .. 4 l + 3 of the tile from the resident map: the mass pass's bits.
template <bool EDT>
__global__ void __launch_bounds__(kTile) k_pdf_sample(const double* __restrict__ maps, size_t nn, unsigned ntiles,
                                                      const PdfEvent* __restrict__ evs, const unsigned long long* __restrict__ acc,
                                                      const unsigned long long* __restrict__ prefix, const double* __restrict__ u,
                                                      int32_t* __restrict__ samples, long S) {
    __shared__ double tab[rt::kExpTableLen];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < rt::kExpTableLen) tab[tid] = rt::np_exp_tables()[tid];
    __syncthreads();
    const size_t e = blockIdx.y;
    const long s = (long)blockIdx.x * (kTile / 64) + (tid >> 6);
    if (s >= S) return;
    const PdfEvent ev = evs[e];
    const unsigned long long Z = acc[e * kAccWords + aZ];
    if (ev.node < 0 || Z == 0) {
        if (lane == 0) samples[e * (size_t)S + s] = -1;
        return;
    }
    unsigned long long q = rt::pdf_sample_quantum(u[e * (size_t)S + s], Z);
    const unsigned long long* pf = prefix + e * ntiles;
    unsigned lo = 0, hi = ntiles - 1;                    // pf[ntiles - 1] = Z > q
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (pf[mid] > q) hi = mid;
        else lo = mid + 1;
    }
    if (lo) q -= pf[lo - 1];
    const size_t x0 = (size_t)lo * kTile + 4 * (size_t)lane;
    unsigned long long m[4], own = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        m[k] = x0 + k < nn ? node_mass<EDT>(maps[e * nn + x0 + k], ev, tab) : 0ull;
        own += m[k];
    }
    unsigned long long incl = own;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v = (unsigned long long)__shfl_up((long long)incl, off);
        if (lane >= off) incl += v;
    }
    const unsigned long long over = __ballot(incl > q);
    if (over == 0) return;                               // the prefix holds the tile's mass: never
    if (lane == __ffsll((long long)over) - 1) {
        unsigned long long c = incl - own;
        int k = 0;
        for (; k < 3; k++) {
            c += m[k];
            if (c > q) break;
        }
        samples[e * (size_t)S + s] = (int32_t)(x0 + k);
    }
}

// sums [event][n] of integer mass over Z: a marginal; NaN for an event without a pdf
__global__ void __launch_bounds__(256) k_pdf_marginal(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ acc,
                                                      long n, long total, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const unsigned long long Z = acc[(i / n) * kAccWords + aZ];
    out[i] = Z ? (double)sums[i] / (double)Z : no_pick();
}

enum Kind { kL2, kEdt };

struct Call {
    Kind kind;
    const rtmi_edt_params* ep;
    const rtmi_pdf_params* pp;
    rtmi_locate_result* res;
    rtmi_edt_result* eres;
};

// what every form of the call refuses before it touches the device
int check_pdf(const char* who, const rtmi_locator* loc, const Call& c, int64_t E, const void* t, bool weights, const rtmi_pdf_result* pdf,
              const void* u, const void* samples) {
    RTMI_ARG(loc, "null handle");                       // check_picks_call's, but for its bound on (tile, chunk) pairs, which
    RTMI_ARG(t, "null t");                               // holds for a group here: group_events sees to it
    RTMI_ARG(E >= 1, "E must be >= 1");
    RTMI_ARG(c.pp, "null pp");
    RTMI_ARG(pdf, "null pdf");
    const rtmi_pdf_params& p = *c.pp;
    RTMI_ARG(loc->lp.nx <= rt::kPdfMaxAxis && loc->lp.ny <= rt::kPdfMaxAxis, "nx or ny is over 65536");
    RTMI_ARG(p.nlevels >= 0 && p.nlevels <= rt::kPdfMaxLevels, "nlevels must be in 0 .. 8");
    for (int k = 0; k < p.nlevels; k++) RTMI_ARG(p.levels[k] > 0.0 && p.levels[k] < 1.0, "levels[" + std::to_string(k) + "] is not in (0, 1)");
    RTMI_ARG(p.S >= 0, "S must be >= 0");
    RTMI_ARG(p.S == 0 || (u && samples), "null u or samples (S > 0)");
    RTMI_ARG(p.power >= 0 && p.power <= 4096, "power must be in 0 .. 4096");
    RTMI_ARG(p.reserved[0] >= 0 && p.reserved[1] >= 0, "reserved[0] and reserved[1] must be >= 0");
    if (c.kind == kL2) {
        RTMI_ARG(std::isfinite(p.sigma) && p.sigma > 0.0, "sigma must be finite and > 0");
    } else {                                             // rtmi_locate_edt's own, restated: its text names that entry
        RTMI_ARG(c.ep, "null ep");
        if (weights) RTMI_ARG(std::isfinite(c.ep->sigma) && c.ep->sigma >= 0.0, "ep->sigma must be finite and >= 0 (with weights)");
        else RTMI_ARG(std::isfinite(c.ep->sigma) && c.ep->sigma > 0.0, "ep->sigma must be finite and > 0 (without weights)");
        RTMI_ARG(c.ep->reserved[0] >= 0, "ep->reserved[0] must be >= 0");
    }
    return RTMI_OK;
}

int check_need(const char* who, const int32_t* need, int64_t E) {
    if (need)
        for (int64_t e = 0; e < E; e++) RTMI_ARG(need[e] >= 0, "need[" + std::to_string(e) + "] is negative");
    return RTMI_OK;
}

int pdf_dev(rtmi_locator* loc, const char* who, const Call& c, int64_t E, const double* d_t, const double* d_w, const int32_t* d_need,
            rtmi_pdf_result* pdf, double* d_mx, double* d_my, const double* d_u, int32_t* d_samples, rtmi_locate_stats* st) {
    const rtmi_pdf_params& pp = *c.pp;
    const size_t nn = loc->nn, P = (size_t)loc->lp.P;
    const unsigned nx = (unsigned)loc->lp.nx, ny = (unsigned)loc->lp.ny, ntiles = (unsigned)((nn + kTile - 1) / kTile);
    const long S = (long)pp.S;
    // an event's share of the group's device memory: its map, histogram, tile masses, sums and marginal sums
    const size_t per_event = nn * sizeof(double) + ((size_t)rt::kPdfBins * 2 + ntiles + kAccWords + nx + ny) * sizeof(unsigned long long);
    size_t group = pp.reserved[0] > 0 ? (size_t)pp.reserved[0] : std::max<size_t>(1, kGroupBudget / per_event);
    group = std::min(std::min(group, (size_t)E), kMaxGroup);
    // the searches take fewer than 2^31 (tile, chunk of 16 events) pairs per call: ntiles <= 2^23, so at least 255 chunks
    group = std::min(group, (size_t)((((uint64_t)1 << 31) - 1) / ntiles) * kChunk);
    const unsigned tpb = pp.reserved[1] > 0 ? (unsigned)std::min<int64_t>(pp.reserved[1], ntiles) : kTilesPerBlock;
    const unsigned bpe = (ntiles + tpb - 1) / tpb;     // blocks per event
    std::vector<rtmi_locate_result> own_l2;
    std::vector<rtmi_edt_result> own_edt;
    rtmi_locate_result* res = c.res;
    rtmi_edt_result* eres = c.eres;
    if (c.kind == kL2 && !res) {
        own_l2.resize((size_t)E);
        res = own_l2.data();
    }
    if (c.kind == kEdt && !eres) {
        own_edt.resize((size_t)E);
        eres = own_edt.data();
    }
    DevMem mem;
    double* maps = nullptr;
    PdfEvent* evs = nullptr;
    unsigned long long *acc = nullptr, *hist = nullptr, *tile_mass = nullptr, *col = nullptr, *row = nullptr;
    RTMI_ALLOC(mem.get(&maps, group * nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&evs, group * sizeof(PdfEvent)));
    RTMI_ALLOC(mem.get(&acc, group * kAccWords * sizeof(unsigned long long)));
    RTMI_ALLOC(mem.get(&hist, group * rt::kPdfBins * 2 * sizeof(unsigned long long)));
    RTMI_ALLOC(mem.get(&tile_mass, group * ntiles * sizeof(unsigned long long)));
    if (d_mx) RTMI_ALLOC(mem.get(&col, group * nx * sizeof(unsigned long long)));
    if (d_my) RTMI_ALLOC(mem.get(&row, group * ny * sizeof(unsigned long long)));
    EventMarks<2> marks;
    RTMI_HIP(marks.create());
    std::vector<PdfEvent> hev(group);
    std::vector<rt::PdfSums> hacc(group);
    std::vector<unsigned long long> hhist(group * rt::kPdfBins * 2), hc(rt::kPdfBins), hm(rt::kPdfBins);
    const rt::LocateGrid g{loc->lp.gx0, loc->lp.gdx, loc->lp.gy0, loc->lp.gdy};
    rtmi_locate_stats total{};
    double pdf_ms = 0.0;
    int64_t ngroups = 0;
    for (size_t e0 = 0; e0 < (size_t)E; e0 += group, ngroups++) {
        const size_t ge = std::min(group, (size_t)E - e0);
        const double* gt = d_t + e0 * P;
        const double* gw = d_w ? d_w + e0 * P : nullptr;
        const int32_t* gneed = d_need ? d_need + e0 : nullptr;
        rtmi_locate_stats gs{};
        if (c.kind == kL2) RTMI_RC(rtmi_locate_dev(loc, (int64_t)ge, gt, gw, gneed, res + e0, maps, &gs));
        else RTMI_RC(rtmi_locate_edt_dev(loc, c.ep, (int64_t)ge, gt, gw, gneed, eres + e0, nullptr, nullptr, maps, &gs));
        total.kernel_ms += gs.kernel_ms;
        total.triples += gs.triples;
        total.contributing += gs.contributing;
        total.reserved[0] += gs.reserved[0];
        for (size_t k = 0; k < ge; k++) {
            PdfEvent& v = hev[k];
            if (c.kind == kL2) {
                const rtmi_locate_result& r = res[e0 + k];
                v = PdfEvent{r.node, 0, r.obj, r.node >= 0 ? rt::pdf_l2_scale(r.sw, pp.sigma) : 0.0};
            } else {
                const rtmi_edt_result& r = eres[e0 + k];
                v = PdfEvent{(int32_t)r.node, pp.power > 0 ? pp.power : (int32_t)std::max<int64_t>(r.n, 1), r.value, 0.0};
            }
        }
        RTMI_HIP(hipMemcpy(evs, hev.data(), ge * sizeof(PdfEvent), hipMemcpyHostToDevice));
        RTMI_HIP(marks.mark(0));
        RTMI_HIP(hipMemsetAsync(acc, 0, ge * kAccWords * sizeof(unsigned long long), nullptr));
        RTMI_HIP(hipMemsetAsync(hist, 0, ge * rt::kPdfBins * 2 * sizeof(unsigned long long), nullptr));
        if (col) RTMI_HIP(hipMemsetAsync(col, 0, ge * nx * sizeof(unsigned long long), nullptr));
        if (row) RTMI_HIP(hipMemsetAsync(row, 0, ge * ny * sizeof(unsigned long long), nullptr));
        const dim3 grid(bpe, (unsigned)ge);
        if (c.kind == kL2) hipLaunchKernelGGL(k_pdf_mass<false>, grid, dim3(kTile), 0, nullptr, maps, nn, nx, ny, ntiles, tpb, evs, acc, hist, tile_mass, col, row);
        else hipLaunchKernelGGL(k_pdf_mass<true>, grid, dim3(kTile), 0, nullptr, maps, nn, nx, ny, ntiles, tpb, evs, acc, hist, tile_mass, col, row);
        RTMI_HIP(hipGetLastError());
        if (S > 0) {
            hipLaunchKernelGGL(k_pdf_scan, dim3((unsigned)ge), dim3(256), 0, nullptr, tile_mass, ntiles);
            RTMI_HIP(hipGetLastError());
            const dim3 sgrid((unsigned)((S + kTile / 64 - 1) / (kTile / 64)), (unsigned)ge);
            const double* gu = d_u + e0 * (size_t)S;
            int32_t* gsm = d_samples + e0 * (size_t)S;
            if (c.kind == kL2) hipLaunchKernelGGL(k_pdf_sample<false>, sgrid, dim3(kTile), 0, nullptr, maps, nn, ntiles, evs, acc, tile_mass, gu, gsm, S);
            else hipLaunchKernelGGL(k_pdf_sample<true>, sgrid, dim3(kTile), 0, nullptr, maps, nn, ntiles, evs, acc, tile_mass, gu, gsm, S);
            RTMI_HIP(hipGetLastError());
        }
        if (d_mx) {
            hipLaunchKernelGGL(k_pdf_marginal, blocks((long)ge * nx), dim3(256), 0, nullptr, col, acc, (long)nx, (long)ge * nx, d_mx + e0 * nx);
            RTMI_HIP(hipGetLastError());
        }
        if (d_my) {
            hipLaunchKernelGGL(k_pdf_marginal, blocks((long)ge * ny), dim3(256), 0, nullptr, row, acc, (long)ny, (long)ge * ny, d_my + e0 * ny);
            RTMI_HIP(hipGetLastError());
        }
        RTMI_HIP(marks.mark(1));
        RTMI_HIP(marks.wait(1));
        double ms = 0.0;
        RTMI_HIP(marks.ms(0, 1, &ms));
        pdf_ms += ms;
        RTMI_HIP(hipMemcpy(hacc.data(), acc, ge * sizeof(rt::PdfSums), hipMemcpyDeviceToHost));
        RTMI_HIP(hipMemcpy(hhist.data(), hist, ge * rt::kPdfBins * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ge; k++) {
            for (int i = 0; i < rt::kPdfBins; i++) {
                hc[(size_t)i] = hhist[(k * rt::kPdfBins + i) * 2];
                hm[(size_t)i] = hhist[(k * rt::kPdfBins + i) * 2 + 1];
            }
            const int32_t node = hev[k].node;
            const rt::PdfStats o = node < 0 ? rt::pdf_none()
                                            : rt::pdf_finalize(hacc[k], hc.data(), hm.data(), (int)((unsigned)node % nx), (int)((unsigned)node / nx),
                                                               g, pp.nlevels, pp.levels);
            rtmi_pdf_result& r = pdf[e0 + k];
            r = rtmi_pdf_result{};
            r.mean_x = o.mean_x;
            r.mean_y = o.mean_y;
            r.area = o.area;
            r.rim_fraction = o.rim_fraction;
            r.nz = o.nz;
            r.mass = o.mass;
            for (int i = 0; i < 3; i++) {
                r.cov[i] = o.cov[i];
                r.ellipse[i] = o.ellipse[i];
            }
            for (int i = 0; i < rt::kPdfMaxLevels; i++) {
                r.level_count[i] = o.level_count[i];
                r.level_area[i] = o.level_area[i];
                r.level_fraction[i] = o.level_fraction[i];
                r.level_rho[i] = o.level_rho[i];
            }
        }
    }
    if (st) {
        *st = total;
        st->kernel_ms += pdf_ms;
        st->reserved[1] = ngroups;                                           // the groups of events the call was walked in
        st->reserved[2] = (int64_t)std::llround(pdf_ms * 1e6);               // this unit's kernels' part of kernel_ms, in nanoseconds
    }
    return RTMI_OK;
}

// the _dev form: the caller's device pointers are checked, then the walk
int pdf_entry_dev(rtmi_locator* loc, const char* who, const Call& c, int64_t E, const double* d_t, const double* d_w, const int32_t* d_need,
                  rtmi_pdf_result* pdf, double* d_mx, double* d_my, const double* d_u, int32_t* d_samples, rtmi_locate_stats* st) {
    RTMI_RC(check_pdf(who, loc, c, E, d_t, d_w != nullptr, pdf, d_u, d_samples));
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P, S = (size_t)c.pp->S;
    RTMI_RC(check_device_pointer(loc->device, who, d_t, picks * sizeof(double), "d_t"));
    if (d_w) RTMI_RC(check_device_pointer(loc->device, who, d_w, picks * sizeof(double), "d_w"));
    if (d_need) RTMI_RC(check_device_pointer(loc->device, who, d_need, (size_t)E * sizeof(int32_t), "d_need"));
    if (d_mx) RTMI_RC(check_device_pointer(loc->device, who, d_mx, (size_t)E * (size_t)loc->lp.nx * sizeof(double), "d_mx"));
    if (d_my) RTMI_RC(check_device_pointer(loc->device, who, d_my, (size_t)E * (size_t)loc->lp.ny * sizeof(double), "d_my"));
    if (S) RTMI_RC(check_device_pointer(loc->device, who, d_u, (size_t)E * S * sizeof(double), "d_u"));
    if (S) RTMI_RC(check_device_pointer(loc->device, who, d_samples, (size_t)E * S * sizeof(int32_t), "d_samples"));
    return pdf_dev(loc, who, c, E, d_t, d_w, d_need, pdf, d_mx, d_my, S ? d_u : nullptr, S ? d_samples : nullptr, st);
}

// the host form: upload, the walk, download
int pdf_entry_host(rtmi_locator* loc, const char* who, const Call& c, int64_t E, const double* t, const double* w, const int32_t* need,
                   rtmi_pdf_result* pdf, double* mx, double* my, const double* u, int32_t* samples, rtmi_locate_stats* st) {
    RTMI_RC(check_pdf(who, loc, c, E, t, w != nullptr, pdf, u, samples));
    RTMI_RC(check_need(who, need, E));
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P, S = (size_t)c.pp->S, nx = (size_t)loc->lp.nx, ny = (size_t)loc->lp.ny;
    DevMem mem;
    double *d_t = nullptr, *d_w = nullptr, *d_mx = nullptr, *d_my = nullptr, *d_u = nullptr;
    int32_t *d_need = nullptr, *d_samples = nullptr;
    const double t0 = now_ms();
    RTMI_ALLOC(mem.get(&d_t, picks * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_t, t, picks * sizeof(double), hipMemcpyHostToDevice));
    if (w) {
        RTMI_ALLOC(mem.get(&d_w, picks * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_w, w, picks * sizeof(double), hipMemcpyHostToDevice));
    }
    if (need) {
        RTMI_ALLOC(mem.get(&d_need, (size_t)E * sizeof(int32_t)));
        RTMI_HIP(hipMemcpy(d_need, need, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (S) {
        RTMI_ALLOC(mem.get(&d_u, (size_t)E * S * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_u, u, (size_t)E * S * sizeof(double), hipMemcpyHostToDevice));
        RTMI_ALLOC(mem.get(&d_samples, (size_t)E * S * sizeof(int32_t)));
    }
    const double upload_ms = now_ms() - t0;
    if (mx) RTMI_ALLOC(mem.get(&d_mx, (size_t)E * nx * sizeof(double)));
    if (my) RTMI_ALLOC(mem.get(&d_my, (size_t)E * ny * sizeof(double)));
    RTMI_RC(pdf_dev(loc, who, c, E, d_t, d_w, d_need, pdf, d_mx, d_my, d_u, d_samples, st));
    if (mx) RTMI_HIP(hipMemcpy(mx, d_mx, (size_t)E * nx * sizeof(double), hipMemcpyDeviceToHost));
    if (my) RTMI_HIP(hipMemcpy(my, d_my, (size_t)E * ny * sizeof(double), hipMemcpyDeviceToHost));
    if (S) RTMI_HIP(hipMemcpy(samples, d_samples, (size_t)E * S * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_locate_pdf(rtmi_locator* loc, const rtmi_pdf_params* pp, int64_t E, const double* t, const double* w,
                                const int32_t* need, rtmi_locate_result* res, rtmi_pdf_result* pdf, double* mx, double* my,
                                const double* u, int32_t* samples, rtmi_locate_stats* st) {
    return pdf_entry_host(loc, "rtmi_locate_pdf", Call{kL2, nullptr, pp, res, nullptr}, E, t, w, need, pdf, mx, my, u, samples, st);
}

RTMI_EXPORT int rtmi_locate_pdf_dev(rtmi_locator* loc, const rtmi_pdf_params* pp, int64_t E, const double* d_t, const double* d_w,
                                    const int32_t* d_need, rtmi_locate_result* res, rtmi_pdf_result* pdf, double* d_mx, double* d_my,
                                    const double* d_u, int32_t* d_samples, rtmi_locate_stats* st) {
    return pdf_entry_dev(loc, "rtmi_locate_pdf_dev", Call{kL2, nullptr, pp, res, nullptr}, E, d_t, d_w, d_need, pdf, d_mx, d_my, d_u,
                         d_samples, st);
}

RTMI_EXPORT int rtmi_locate_edt_pdf(rtmi_locator* loc, const rtmi_edt_params* ep, const rtmi_pdf_params* pp, int64_t E, const double* t,
                                    const double* w, const int32_t* need, rtmi_edt_result* res, rtmi_pdf_result* pdf, double* mx,
                                    double* my, const double* u, int32_t* samples, rtmi_locate_stats* st) {
    return pdf_entry_host(loc, "rtmi_locate_edt_pdf", Call{kEdt, ep, pp, nullptr, res}, E, t, w, need, pdf, mx, my, u, samples, st);
}

RTMI_EXPORT int rtmi_locate_edt_pdf_dev(rtmi_locator* loc, const rtmi_edt_params* ep, const rtmi_pdf_params* pp, int64_t E,
                                        const double* d_t, const double* d_w, const int32_t* d_need, rtmi_edt_result* res,
                                        rtmi_pdf_result* pdf, double* d_mx, double* d_my, const double* d_u, int32_t* d_samples,
                                        rtmi_locate_stats* st) {
    return pdf_entry_dev(loc, "rtmi_locate_edt_pdf_dev", Call{kEdt, ep, pp, nullptr, res}, E, d_t, d_w, d_need, pdf, d_mx, d_my, d_u,
                         d_samples, st);
}
