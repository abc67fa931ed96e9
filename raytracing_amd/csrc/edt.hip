// edt.hip -- robust event location by equal differential time on a locator handle's tables (rtmi_locate_edt, rtmi_locate_edt_dev,
// rtmi_edt_exp; include/rtmi.h).  The arithmetic of a station pair and of a node is rt_edt.h's; the kernels
// here only decide who runs it on what.
//   k_locate_prep    ref and the fewest picks of a candidate; k_locate_stage the chunk's picks as the search reads them;
//   k_locate_pick    the least (key, node) of an event's partials: rtmi_locator.h's, shared with locate.hip
//   k_edt_pairs      weights only: g and h of every (chunk, pair, event) of a group of chunks, so that the search neither divides
//                    nor takes a square root
//   k_edt            one lane per node of a tile of 256, one block per (tile, chunk of 16 events): value at every node, the map,
//                    and one partial (key = -value, node, contributing pairs) per (event, tile)
//   k_edt_window     one wave per event: value and tau at the nine nodes around the best one, the centre's shares and residuals
// No atomics: every result is one lane's own chain of operations or an exact minimum, the same bits on every run.
#include "rtmi_locator.h"

#include "rt_edt.h"
#include "rt_locate.h"

namespace {

constexpr size_t kPairBytes = (size_t)2 * kChunk * sizeof(double);      // g [16] and h [16] of one (chunk, pair)
constexpr size_t kPairBudget = (size_t)256 << 20;                        // the most the staged g and h of one group of chunks take

// what the window kernel leaves per event for the host
struct DevOut {
    int32_t node, n;
    double ref, share_sum;
    double wval[9], wtau[9];
    long long contributing;
};

// rt_np_exp.h's tables into the block's LDS: 32 lanes, then a barrier
__device__ __forceinline__ void stage_exp_tables(double* tab) {
    if (threadIdx.x < rt::kExpTableLen) tab[threadIdx.x] = rt::np_exp_tables()[threadIdx.x];
    __syncthreads();
}

// g and h of the pairs of a group of chunks, one lane per (chunk, a, b) of the full square, the lanes with a < b at work:
// gh [chunk][pair][2][16], pair = a (2 P - a - 1) / 2 + (b - a - 1), the order in which the search walks them.  A pair with a
// pick that is not valid gets zeros, which nobody reads.
__global__ void __launch_bounds__(256) k_edt_pairs(const double* __restrict__ wv, long c0, long gchunks, int P, double s2, double* __restrict__ gh) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long PP = (long)P * P;
    if (i >= gchunks * PP) return;
    const long c = i / PP, a = i % PP / P, b = i % P;
    if (a >= b) return;
    const long npairs = (long)P * (P - 1) / 2, pair = a * (2L * P - a - 1) / 2 + (b - a - 1);
    const double* wa = wv + ((c0 + c) * P + a) * kChunk;
    const double* wb = wv + ((c0 + c) * P + b) * kChunk;
    double* o = gh + (c * npairs + pair) * 2 * kChunk;
    for (int k = 0; k < kChunk; k++) {
        double g = 0.0, h = 0.0;
        if (wa[k] > 0.0 && wb[k] > 0.0) {
            g = rt::edt_g(rt::edt_var(wa[k], s2), rt::edt_var(wb[k], s2));
            h = rt::edt_sqrt(g);
        }
        o[k] = g;
        o[kChunk + k] = h;
    }
}

// What a block of k_edt hands to its walk over the pairs
struct ChunkView {
    const double* __restrict__ T;      // the tables
    size_t nn, xl;                     // nodes per table; the lane's node, the last node for a lane past the grid
    int P;
    bool inb;                          // the lane has a node
    const double* __restrict__ tr;     // the chunk's staged picks [P][16] ...
    const unsigned* __restrict__ mask; // ... and masks [P]
    const double* __restrict__ gh;     // W: the chunk's [pair][2][16]
    double g0;                         // no weights: every pair's g
    const double* tab;                 // rt_np_exp.h's tables in LDS
};

// A lane's walk over the station pairs for the 16 events of its chunk: a ascending outside with d_a of the 16 events in registers,
// b > a ascending inside.  ALL: every event of the chunk has a valid pick at every station, the usual case: no test per event, the
// 16 steps run under one test of the lane's two table values.  Otherwise a step runs where both stations' masks have the event's
// bit.  The steps and their order are the same, so no bit depends on the variant.  T[b][x] is one coalesced load per pair, asked
// for one station ahead and used for the 16 events; the load is unconditional (a lane past the grid reads the last node, the step
// past the last station reads that station again) so that no branch stands between it and the wait for the one before.  The
// picks, masks, g and h are wave-uniform: scalar loads.
template <bool W, bool ALL>
__device__ __forceinline__ void chunk_pairs(const ChunkView& v, double (&S)[kChunk], double (&H)[kChunk], int (&n)[kChunk]) {
    auto table = [&](int r) { return v.T[(size_t)(r < v.P ? r : v.P - 1) * v.nn + v.xl]; };
    int nfin = 0;                           // ALL: every event counts the same stations, those with a finite table value here
    size_t pair = 0;
    for (int a = 0; a < v.P; a++) {
        const double Ta = table(a);
        double Tn = table(a + 1);
        const bool fa = v.inb && fabs(Ta) < INFINITY;
        const unsigned ma = ALL ? kAllPicks : v.mask[a];
        double da[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; k++) da[k] = v.tr[a * kChunk + k] - Ta;
        if (ALL) {
            nfin += fa ? 1 : 0;
        } else {
#pragma unroll
            for (int k = 0; k < kChunk; k++) n[k] += fa && (ma >> k & 1) ? 1 : 0;
        }
        for (int b = a + 1; b < v.P; b++, pair++) {
            const double Tb = Tn;
            Tn = table(b + 1);
            const unsigned m = ALL ? kAllPicks : ma & v.mask[b];
            if (fa && fabs(Tb) < INFINITY) {
#pragma unroll
                for (int k = 0; k < kChunk; k++) {
                    if (ALL || (m >> k & 1)) {
                        const double db = v.tr[b * kChunk + k] - Tb;
                        if (W) {
                            const double g = v.gh[pair * 2 * kChunk + k], h = v.gh[pair * 2 * kChunk + kChunk + k];
                            S[k] = S[k] + h * rt::edt_k(da[k], db, g, v.tab);
                            H[k] = H[k] + h;
                        } else {
                            S[k] = S[k] + rt::edt_k(da[k], db, v.g0, v.tab);
                        }
                    }
                }
            }
        }
    }
    if (ALL) {
#pragma unroll
        for (int k = 0; k < kChunk; k++) n[k] = nfin;
    }
}

// The search.  Block b works on tile b / gchunks and chunk c0 + b % gchunks of the call: the blocks in flight share a few tiles,
// so a table value comes from HBM once and from the caches afterwards.  A lane holds S (and H) of its node for the 16 events of the
// chunk in registers; the reduction is locate.hip's: the wave, the block through LDS, k_locate_pick over the tiles.
template <bool W>
__global__ void __launch_bounds__(kTile) k_edt(const double* __restrict__ T, size_t nn, int P, const double* __restrict__ tr,
                                               const unsigned* __restrict__ mask, const int* __restrict__ needv,
                                               const double* __restrict__ gh, double g0, long E, unsigned c0, unsigned gchunks,
                                               unsigned ntiles, double* __restrict__ maps, Partial* __restrict__ part) {
    __shared__ double tab[rt::kExpTableLen];
    stage_exp_tables(tab);
    const unsigned tile = blockIdx.x / gchunks, cg = blockIdx.x % gchunks, c = c0 + cg;
    const int tid = (int)threadIdx.x;
    const size_t x = (size_t)tile * kTile + tid;
    const bool inb = x < nn;
    const size_t npairs = (size_t)P * (P - 1) / 2;
    const ChunkView v{T, nn, inb ? x : nn - 1, P, inb, tr + (size_t)c * P * kChunk, mask + (size_t)c * P,
                      W ? gh + (size_t)cg * npairs * 2 * kChunk : nullptr, g0, tab};
    bool all = true;
    for (int r = 0; r < P; r++) all = all && v.mask[r] == kAllPicks;

    double S[kChunk], H[kChunk];
    int n[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
        S[k] = 0.0;
        H[k] = 0.0;
        n[k] = 0;
    }
    if (all) chunk_pairs<W, true>(v, S, H, n);
    else chunk_pairs<W, false>(v, S, H, n);

    __shared__ double wkey[kTile / 64][kChunk];
    __shared__ unsigned wnode[kTile / 64][kChunk];
    __shared__ int wcnt[kTile / 64][kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
        const long e = (long)c * kChunk + k;
        const int need = needv[(size_t)c * kChunk + k];
        const bool cand = n[k] >= (need > 2 ? need : 2);
        const int pairs = n[k] * (n[k] - 1) / 2;
        if (!W) H[k] = (double)pairs;
        const double val = cand ? S[k] / H[k] : -INFINITY;
        if (maps && inb && e < E) maps[(size_t)e * nn + x] = val;
        double key = -val < INFINITY ? -val : INFINITY;               // a NaN counts as -inf
        unsigned node = cand && inb ? (unsigned)x : kNoNode;
        int cnt = pairs;
        for (int off = 1; off < 64; off <<= 1) {
            take_less(key, node, __shfl_xor(key, off), __shfl_xor(node, off));
            cnt += __shfl_xor(cnt, off);
        }
        if ((tid & 63) == 0) {
            wkey[tid >> 6][k] = key;
            wnode[tid >> 6][k] = node;
            wcnt[tid >> 6][k] = cnt;
        }
    }
    __syncthreads();
    if (tid < kChunk && (long)c * kChunk + tid < E) {
        double key = wkey[0][tid];
        unsigned node = wnode[0][tid];
        int cnt = wcnt[0][tid];
        for (int w = 1; w < kTile / 64; w++) {
            take_less(key, node, wkey[w][tid], wnode[w][tid]);
            cnt += wcnt[w][tid];
        }
        part[((size_t)c * kChunk + tid) * ntiles + tile] = Partial{key, node, cnt};
    }
}

// The 3 x 3 window around every event's best node: lane l of the event's wave takes row l / 3 and column l % 3 and walks its node
// by rt_edt.h's own loops, the search's steps in the search's order.  g and h are computed here, not read from the staged pairs:
// the same operations on the same operands.  The centre's lane also writes the event's rows of share and resid.
template <bool W>
__global__ void __launch_bounds__(64) k_edt_window(const double* __restrict__ T, size_t nn, long nx, long ny, int P,
                                                   const double* __restrict__ tr, const double* __restrict__ wv,
                                                   const int* __restrict__ needv, const double* __restrict__ ref, double s2, double g0,
                                                   const int32_t* __restrict__ best, const long long* __restrict__ contributing,
                                                   DevOut* __restrict__ out, double* __restrict__ share, double* __restrict__ resid) {
    __shared__ double tab[rt::kExpTableLen];
    stage_exp_tables(tab);
    const size_t e = blockIdx.x;
    const int l = (int)threadIdx.x;
    if (l >= 9) return;
    const int32_t node = best[e];
    DevOut& o = out[e];
    double* sh = share ? share + e * (size_t)P : nullptr;
    double* rs = resid ? resid + e * (size_t)P : nullptr;
    double val = no_pick(), tau = no_pick(), den = no_pick();
    int n = 0;
    bool inside = false;
    if (node >= 0) {
        const long ix = node % nx + (l % 3 - 1), iy = node / nx + (l / 3 - 1);
        if (ix >= 0 && ix < nx && iy >= 0 && iy < ny) {
            inside = true;
            const size_t off = (e / kChunk) * (size_t)P * kChunk + e % kChunk;
            const rt::EdtView v{P, tr + off, W ? wv + off : nullptr, (size_t)kChunk, T + ((size_t)iy * nx + ix), nn, s2, g0, tab};
            const int need = needv[e];
            const rt::EdtNode q = rt::edt_node<W>(v, need > 2 ? need : 2);
            val = q.value;
            n = q.n;
            if (q.cand) {
                tau = rt::edt_tau<W>(v, &den, l == 4 ? sh : nullptr);
                if (l == 4 && rs) rt::edt_resid(v, tau, rs);
            }
        }
    }
    o.wval[l] = val;
    o.wtau[l] = tau;
    if (l == 4) {
        o.node = node;
        o.n = n;
        o.ref = node < 0 ? no_pick() : ref[e];
        o.share_sum = den;
        o.contributing = contributing[e];
        if (!inside) {
            for (int r = 0; r < P; r++) {
                if (sh) sh[r] = no_pick();
                if (rs) rs[r] = no_pick();
            }
        }
    }
}

// what both forms of the call refuse before they touch the device
int check_edt(const char* who, const rtmi_edt_params* ep, bool weights) {
    RTMI_ARG(ep, "null ep");
    if (weights) RTMI_ARG(std::isfinite(ep->sigma) && ep->sigma >= 0.0, "sigma must be finite and >= 0 (with weights)");
    else RTMI_ARG(std::isfinite(ep->sigma) && ep->sigma > 0.0, "sigma must be finite and > 0 (without weights)");
    RTMI_ARG(ep->reserved[0] >= 0, "reserved[0] must be >= 0");
    return RTMI_OK;
}

int edt_dev(rtmi_locator* loc, const char* who, const rtmi_edt_params* ep, int64_t E, unsigned nchunks, unsigned ntiles, const double* d_t,
            const double* d_w, const int32_t* d_need, rtmi_edt_result* res, double* d_share, double* d_resid, double* d_maps,
            rtmi_locate_stats* st) {
    const int P = (int)loc->lp.P;
    const size_t nn = loc->nn, Epad = (size_t)nchunks * kChunk, staged = Epad * (size_t)P, npairs = (size_t)P * (P - 1) / 2;
    const double s2 = ep->sigma * ep->sigma, g0 = rt::edt_g(s2, s2);
    // weights: the chunks of one group, whose staged g and h fit the budget; reserved[0] sets it for tests
    size_t group = nchunks;
    if (d_w && npairs) {
        const size_t fit = kPairBudget / (npairs * kPairBytes);
        group = ep->reserved[0] > 0 ? (size_t)ep->reserved[0] : fit < 1 ? 1 : fit;
        if (group > nchunks) group = nchunks;
    }
    DevMem mem;
    double *tr = nullptr, *wv = nullptr, *ref = nullptr, *gh = nullptr;
    int* needv = nullptr;
    unsigned* mask = nullptr;
    Partial* part = nullptr;
    int32_t* best = nullptr;
    long long* contributing = nullptr;
    DevOut* out = nullptr;
    RTMI_ALLOC(mem.get(&tr, staged * sizeof(double)));
    if (d_w) RTMI_ALLOC(mem.get(&wv, staged * sizeof(double)));
    if (d_w) RTMI_ALLOC(mem.get(&gh, group * npairs * kPairBytes));
    RTMI_ALLOC(mem.get(&ref, Epad * sizeof(double)));
    RTMI_ALLOC(mem.get(&needv, Epad * sizeof(int)));
    RTMI_ALLOC(mem.get(&mask, (size_t)nchunks * P * sizeof(unsigned)));
    RTMI_ALLOC(mem.get(&part, (size_t)E * ntiles * sizeof(Partial)));
    RTMI_ALLOC(mem.get(&best, (size_t)E * sizeof(int32_t)));
    RTMI_ALLOC(mem.get(&contributing, (size_t)E * sizeof(long long)));
    RTMI_ALLOC(mem.get(&out, (size_t)E * sizeof(DevOut)));
    EventMarks<4> ev;
    RTMI_HIP(ev.create());
    RTMI_HIP(ev.mark(0));
    hipLaunchKernelGGL(k_locate_prep, blocks((long)Epad), dim3(256), 0, nullptr, d_t, d_w, d_need, (long)E, (long)Epad, P, ref, needv);
    RTMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_locate_stage, blocks((long)nchunks * P), dim3(256), 0, nullptr, d_t, d_w, ref, (long)E, (long)nchunks, P, tr, wv, mask);
    RTMI_HIP(hipGetLastError());
    unsigned ngroups = 0;
    for (size_t c0 = 0; c0 < nchunks; c0 += group, ngroups++) {
        const unsigned gc = (unsigned)(nchunks - c0 < group ? nchunks - c0 : group);
        if (d_w && npairs) {
            hipLaunchKernelGGL(k_edt_pairs, blocks((long)gc * P * P), dim3(256), 0, nullptr, wv, (long)c0, (long)gc, P, s2, gh);
            RTMI_HIP(hipGetLastError());
        }
        if (c0 == 0) RTMI_HIP(ev.mark(1));
        const dim3 grid(gc * ntiles);
        if (d_w) {
            hipLaunchKernelGGL(k_edt<true>, grid, dim3(kTile), 0, nullptr, loc->T, nn, P, tr, mask, needv, gh, g0, (long)E, (unsigned)c0, gc, ntiles, d_maps, part);
        } else {
            hipLaunchKernelGGL(k_edt<false>, grid, dim3(kTile), 0, nullptr, loc->T, nn, P, tr, mask, needv, gh, g0, (long)E, (unsigned)c0, gc, ntiles, d_maps, part);
        }
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(2));
    hipLaunchKernelGGL(k_locate_pick, dim3((unsigned)E), dim3(256), 0, nullptr, part, ntiles, best, contributing);
    RTMI_HIP(hipGetLastError());
    const long nx = (long)loc->lp.nx, ny = (long)loc->lp.ny;
    if (d_w) {
        hipLaunchKernelGGL(k_edt_window<true>, dim3((unsigned)E), dim3(64), 0, nullptr, loc->T, nn, nx, ny, P, tr, wv, needv, ref, s2, g0, best, contributing, out, d_share, d_resid);
    } else {
        hipLaunchKernelGGL(k_edt_window<false>, dim3((unsigned)E), dim3(64), 0, nullptr, loc->T, nn, nx, ny, P, tr, wv, needv, ref, s2, g0, best, contributing, out, d_share, d_resid);
    }
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(3));
    RTMI_HIP(ev.wait(3));
    std::vector<DevOut> h((size_t)E);
    RTMI_HIP(hipMemcpy(h.data(), out, (size_t)E * sizeof(DevOut), hipMemcpyDeviceToHost));
    const rt::LocateGrid g{loc->lp.gx0, loc->lp.gdx, loc->lp.gy0, loc->lp.gdy};
    const double nan = std::nan("");
    int64_t total = 0;
    for (int64_t e = 0; e < E; e++) {
        const DevOut& o = h[(size_t)e];
        rtmi_edt_result& r = res[e];
        r = rtmi_edt_result{};
        total += o.contributing;
        r.node = o.node;
        for (int k = 0; k < 9; k++) {
            r.win_val[k] = o.wval[k];
            r.win_tau[k] = o.wtau[k];
        }
        r.ref = o.ref;
        if (o.node < 0) {
            r.ix = r.iy = -1;
            r.value = r.t0 = r.share_sum = r.x = r.y = r.t0_refined = r.dx = r.dy = nan;
            continue;
        }
        r.ix = o.node % nx;
        r.iy = o.node / nx;
        r.n = o.n;
        r.npairs = (int64_t)o.n * (o.n - 1) / 2;
        r.value = o.wval[4];
        r.share_sum = o.share_sum;
        r.t0 = o.ref + o.wtau[4];
        double f[9];
        for (int k = 0; k < 9; k++) f[k] = -o.wval[k];
        const rt::LocateRefined q = rt::locate_refine(f, o.wtau, o.ref, 1.0, (int)r.ix, (int)r.iy, g);
        r.x = q.x;
        r.y = q.y;
        r.t0_refined = q.t0;
        r.dx = q.dx;
        r.dy = q.dy;
        r.refined = q.refined;
    }
    if (st) {
        *st = rtmi_locate_stats{};
        double search_ms = 0.0;
        RTMI_HIP(ev.ms(0, 3, &st->kernel_ms));
        RTMI_HIP(ev.ms(1, 2, &search_ms));
        st->reserved[0] = (int64_t)std::llround(search_ms * 1e6);          // k_edt's share of kernel_ms, in nanoseconds
        st->reserved[1] = ngroups;                                           // the groups of chunks the call was walked in
        st->triples = (int64_t)E * (int64_t)nn * (int64_t)npairs;
        st->contributing = total;
    }
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_edt_exp(const double* z, double* out, int64_t n) {
    const char* who = "rtmi_edt_exp";
    RTMI_ARG(n >= 0, "n must be >= 0");
    RTMI_ARG(n == 0 || (z && out), "null z or out");
    for (int64_t i = 0; i < n; i++) RTMI_ARG(z[i] >= rt::kEdtCut && z[i] <= 0.0, "z[" + std::to_string(i) + "] is not in [-700, 0]");
    for (int64_t i = 0; i < n; i++) out[i] = rt::edt_exp(z[i], rt::np_exp_tables());
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_locate_edt_dev(rtmi_locator* loc, const rtmi_edt_params* ep, int64_t E, const double* d_t, const double* d_w,
                                    const int32_t* d_need, rtmi_edt_result* res, double* d_share, double* d_resid, double* d_maps,
                                    rtmi_locate_stats* st) {
    const char* who = "rtmi_locate_edt_dev";
    unsigned nchunks = 0, ntiles = 0;
    RTMI_RC(check_picks_call(who, loc, E, d_t, res, &nchunks, &ntiles));
    RTMI_RC(check_edt(who, ep, d_w != nullptr));
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P;
    RTMI_RC(check_device_pointer(loc->device, who, d_t, picks * sizeof(double), "d_t"));
    if (d_w) RTMI_RC(check_device_pointer(loc->device, who, d_w, picks * sizeof(double), "d_w"));
    if (d_need) RTMI_RC(check_device_pointer(loc->device, who, d_need, (size_t)E * sizeof(int32_t), "d_need"));
    if (d_share) RTMI_RC(check_device_pointer(loc->device, who, d_share, picks * sizeof(double), "d_share"));
    if (d_resid) RTMI_RC(check_device_pointer(loc->device, who, d_resid, picks * sizeof(double), "d_resid"));
    if (d_maps) RTMI_RC(check_device_pointer(loc->device, who, d_maps, (size_t)E * loc->nn * sizeof(double), "d_maps"));
    return edt_dev(loc, who, ep, E, nchunks, ntiles, d_t, d_w, d_need, res, d_share, d_resid, d_maps, st);
}

RTMI_EXPORT int rtmi_locate_edt(rtmi_locator* loc, const rtmi_edt_params* ep, int64_t E, const double* t, const double* w,
                                const int32_t* need, rtmi_edt_result* res, double* share, double* resid, double* maps,
                                rtmi_locate_stats* st) {
    const char* who = "rtmi_locate_edt";
    unsigned nchunks = 0, ntiles = 0;
    RTMI_RC(check_picks_call(who, loc, E, t, res, &nchunks, &ntiles));
    RTMI_RC(check_edt(who, ep, w != nullptr));
    if (need)
        for (int64_t e = 0; e < E; e++) RTMI_ARG(need[e] >= 0, "need[" + std::to_string(e) + "] is negative");
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P;
    DevMem mem;
    double *d_t = nullptr, *d_w = nullptr, *d_maps = nullptr, *d_share = nullptr, *d_resid = nullptr;
    int32_t* d_need = nullptr;
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
    const double upload_ms = now_ms() - t0;
    if (share) RTMI_ALLOC(mem.get(&d_share, picks * sizeof(double)));
    if (resid) RTMI_ALLOC(mem.get(&d_resid, picks * sizeof(double)));
    if (maps) RTMI_ALLOC(mem.get(&d_maps, (size_t)E * loc->nn * sizeof(double)));
    RTMI_RC(edt_dev(loc, who, ep, E, nchunks, ntiles, d_t, d_w, d_need, res, d_share, d_resid, d_maps, st));
    if (share) RTMI_HIP(hipMemcpy(share, d_share, picks * sizeof(double), hipMemcpyDeviceToHost));
    if (resid) RTMI_HIP(hipMemcpy(resid, d_resid, picks * sizeof(double), hipMemcpyDeviceToHost));
    if (maps) RTMI_HIP(hipMemcpy(maps, d_maps, (size_t)E * loc->nn * sizeof(double), hipMemcpyDeviceToHost));
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}
