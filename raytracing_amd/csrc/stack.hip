// stack.hip -- pick-free event detection and location: station traces stacked along the traveltime moveout of every grid node
// for every candidate origin time (rtmi_locate_stack, rtmi_locate_stack_dev; include/rtmi.h), on the tables
// of a locator handle (rtmi_locator.h).  The arithmetic of a (node, origin time, station) is rt_stack.h's one step; the kernels
// here only decide who runs it on what.
//   k_stack_prep     the scan's origin times, the valid stations with their weights, and the fewest stations of a candidate
//   k_stack          one lane per node of a tile of 256, one block per (tile, part of the scan): S at every node and scan index
//                    of the part, a chunk of 16 scan indices at a time; the volume; the lane's own best (S, m) of the part; one
//                    partial (key, node) per (scan index, tile)
//   k_stack_pick     one block per scan index: the greatest (key, least node) of its partials
//   k_stack_merge    one lane per node: the greatest (key, least m) over the parts
//   k_stack_total    the contributing triples of all blocks
//   k_stack_window   27 lanes per event: S at the 3 x 3 x 3 points around it, by the same step in the same order
// No atomics: every result is one lane's own chain of operations or an exact maximum, the same bits on every run and under every
// split of the scan.
#include "rtmi_locator.h"

#include "rt_stack.h"

namespace {

// kTile nodes of a block, one per lane, and kChunk scan indices whose running sums a lane keeps in registers: rtmi_locator.h
constexpr int kBlocksPerCu = 32;        // the search aims at this many blocks per CU, so that the last round of blocks is a small share

// what the window kernel leaves per event for the host
struct DevWin {
    double win[27];
    int32_t n, pad;
};
struct DevEvent {
    int32_t m, node;
};

// What every kernel reads: the tables, the traces, and what k_stack_prep left
struct StackView {
    const double* __restrict__ T;       // [P][nn]
    const double* __restrict__ c;       // [P][nt]
    size_t nn;
    long nt;
    const double* __restrict__ ov;      // [chunks * 16] origin times: wave-uniform, scalar loads
    const int* __restrict__ sidx;       // [nvalid] the valid stations, ascending ...
    const double* __restrict__ swt;     // ... and their weights
    const int* __restrict__ meta;       // nvalid, max(need, 1)
    rt::StackAxis ax;
};

__device__ __forceinline__ double nan_() { return __longlong_as_double(0x7ff8000000000000LL); }

// (a, ia) <- the greater of (a, ia) and (b, ib): by key, then by the lesser index.  Keys are never NaN.
__device__ __forceinline__ void take_more(double& a, unsigned& ia, double b, unsigned ib) {
    const bool more = b > a || (b == a && ib < ia);
    a = more ? b : a;
    ia = more ? ib : ia;
}

__global__ void __launch_bounds__(256) k_stack_prep(const double* __restrict__ w, int P, int need, double o0, double od, long Mpad,
                                                    double* __restrict__ ov, int* __restrict__ sidx, double* __restrict__ swt,
                                                    int* __restrict__ meta) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m < Mpad) ov[m] = o0 + (double)m * od;
    if (m == 0) {
        int nv = 0;
        for (int r = 0; r < P; r++)
            if (!w || (w[r] > 0.0 && w[r] < INFINITY)) {
                sidx[nv] = r;
                swt[nv] = w ? w[r] : 1.0;
                nv++;
            }
        const int nd = need ? need : nv;
        meta[0] = nv;
        meta[1] = nd > 1 ? nd : 1;
    }
}

// The search.  Block (tile, part) walks the chunks of its part of the scan.  Per chunk a lane holds n and s (and sw) of its node
// for the chunk's 16 origin times in registers and walks the valid stations once: T[r][x] is one coalesced load per station and
// chunk, asked for one station ahead (unconditionally: a lane past the grid reads the last node and drops it, the step past the
// last station reads that station again); the origin times and the weights are wave-uniform.  The two trace samples of a step
// are gathered straight from global memory, where the traces (P nt 8 bytes) stay in L2; a step out of range reads samples 0
// and 1, so that no branch stands between the sixteen gathers of a station.
template <bool W>
__global__ void __launch_bounds__(kTile) k_stack(const StackView v, long M, long nchunks, long per_part, unsigned ntiles,
                                                 double* __restrict__ volume, double* __restrict__ bkey, int32_t* __restrict__ bm,
                                                 double* __restrict__ pkey, unsigned* __restrict__ pnode, long long* __restrict__ pcnt) {
    const unsigned tile = blockIdx.x, part = blockIdx.y;
    const int tid = (int)threadIdx.x;
    const size_t nn = v.nn, x = (size_t)tile * kTile + tid;
    const bool inb = x < nn;
    const size_t xl = inb ? x : nn - 1;
    const int nv = v.meta[0], needv = v.meta[1];
    const long cfirst = (long)part * per_part, clast = cfirst + per_part < nchunks ? cfirst + per_part : nchunks;

    __shared__ double wkey[2][kTile / 64][kChunk];
    __shared__ unsigned wnode[2][kTile / 64][kChunk];
    __shared__ long long wcnt[kTile / 64];
    double bestk = -INFINITY;
    int32_t bestm = -1;
    long long cnt = 0;
    auto table = [&](int i) { return v.T[(size_t)v.sidx[i < nv ? i : nv - 1] * nn + xl]; };

    for (long ch = cfirst; ch < clast; ch++) {
        const long mc = ch * kChunk;
        const double* __restrict__ o = v.ov + mc;
        rt::StackSums a[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; k++) a[k] = rt::StackSums{0, 0.0, 0.0};
        double Tn = nv > 0 ? table(0) : 0.0;
        for (int i = 0; i < nv; i++) {
            const double Tv = inb ? Tn : nan_();
            Tn = table(i + 1);
            const double wr = W ? v.swt[i] : 0.0;
            const double* __restrict__ cr = v.c + (size_t)v.sidx[i] * (size_t)v.nt;
#pragma unroll
            for (int k = 0; k < kChunk; k++)
                rt::stack_step<W>(a[k], o[k], Tv, wr, v.ax, [&](long j, double& c0, double& c1) {
                    c0 = cr[j];
                    c1 = cr[j + 1];
                });
        }
        const int buf = (int)(ch & 1);
#pragma unroll
        for (int k = 0; k < kChunk; k++) {
            const long m = mc + k;                                    // wave-uniform
            const bool cand = a[k].n >= needv && m < M;
            const double S = rt::stack_value<W>(a[k], needv);
            if (m < M) {
                cnt += a[k].n;
                if (volume && inb) volume[(size_t)m * nn + x] = S;
            }
            const double key = S > -INFINITY ? S : -INFINITY;         // a NaN counts as -inf
            if (cand && (bestm < 0 || key > bestk)) {                 // m ascends: the first of the greatest stays
                bestk = key;
                bestm = (int32_t)m;
            }
            // the wave's greatest key, then the first lane that holds it among the candidates: the least node.  A lane that is no
            // candidate has the key -inf, which no candidate's key is below, so the greatest key is a candidate's if there is one.
            double kmax = key;
            for (int off = 1; off < 64; off <<= 1) kmax = fmax(kmax, __shfl_xor(kmax, off));
            const unsigned long long who = __ballot(cand && key == kmax);
            if ((tid & 63) == 0) {
                wkey[buf][tid >> 6][k] = who ? kmax : -INFINITY;
                wnode[buf][tid >> 6][k] = who ? (unsigned)x + (unsigned)(__ffsll((long long)who) - 1) : kNoNode;
            }
        }
        // One barrier per chunk: the chunk after the next one writes this buffer again, and no wave gets there before every wave
        // has passed the next chunk's barrier, which the lanes below reach only after their reads.
        __syncthreads();
        if (tid < kChunk && mc + tid < M) {
            double key = wkey[buf][0][tid];
            unsigned node = wnode[buf][0][tid];
            for (int q = 1; q < kTile / 64; q++) take_more(key, node, wkey[buf][q][tid], wnode[buf][q][tid]);
            pkey[(size_t)(mc + tid) * ntiles + tile] = key;
            pnode[(size_t)(mc + tid) * ntiles + tile] = node;
        }
    }
    if (bkey && inb) {
        bkey[(size_t)part * nn + x] = bestk;
        bm[(size_t)part * nn + x] = bestm;
    }
    for (int off = 1; off < 64; off <<= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) pcnt[(size_t)part * ntiles + tile] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

// peak[m] and peak_node[m]: the greatest (key, least node) over the scan index's partials, -inf and -1 when no tile has a candidate
__global__ void __launch_bounds__(256) k_stack_pick(const double* __restrict__ pkey, const unsigned* __restrict__ pnode, unsigned ntiles,
                                                    double* __restrict__ peak, int32_t* __restrict__ peak_node) {
    const size_t m = blockIdx.x;
    const int tid = (int)threadIdx.x;
    double key = -INFINITY;
    unsigned node = kNoNode;
    for (unsigned i = tid; i < ntiles; i += 256) take_more(key, node, pkey[m * ntiles + i], pnode[m * ntiles + i]);
    for (int off = 1; off < 64; off <<= 1) take_more(key, node, __shfl_xor(key, off), __shfl_xor(node, off));
    __shared__ double wkey[4];
    __shared__ unsigned wnode[4];
    if ((tid & 63) == 0) {
        wkey[tid >> 6] = key;
        wnode[tid >> 6] = node;
    }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; q++) take_more(key, node, wkey[q], wnode[q]);
        peak[m] = key;
        peak_node[m] = node == kNoNode ? -1 : (int32_t)node;
    }
}

// best[x] and best_m[x] over the parts, which ascend in m: the first of the greatest stays
__global__ void __launch_bounds__(256) k_stack_merge(const double* __restrict__ bkey, const int32_t* __restrict__ bm, unsigned nparts,
                                                     size_t nn, double* __restrict__ best, int32_t* __restrict__ best_m) {
    const size_t x = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= nn) return;
    double key = -INFINITY;
    int32_t m = -1;
    for (unsigned p = 0; p < nparts; p++) {
        const double k = bkey[(size_t)p * nn + x];
        const int32_t mm = bm[(size_t)p * nn + x];
        if (mm >= 0 && (m < 0 || k > key)) {
            key = k;
            m = mm;
        }
    }
    if (best) best[x] = key;
    if (best_m) best_m[x] = m;
}

__global__ void __launch_bounds__(256) k_stack_total(const long long* __restrict__ pcnt, size_t n, long long* __restrict__ total) {
    const int tid = (int)threadIdx.x;
    long long s = 0;
    for (size_t i = tid; i < n; i += 256) s += pcnt[i];
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
    __shared__ long long ws[4];
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) total[0] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// The 3 x 3 x 3 window of every event: lane l takes scan index m + l / 9 - 1, row iy + (l / 3) % 3 - 1 and column ix + l % 3 - 1.
template <bool W>
__global__ void __launch_bounds__(64) k_stack_window(const StackView v, long nx, long ny, long M, const DevEvent* __restrict__ ev,
                                                     DevWin* __restrict__ out) {
    const size_t e = blockIdx.x;
    const int l = (int)threadIdx.x;
    if (l >= 27) return;
    const long m = (long)ev[e].m + (l / 9 - 1);
    const long node = ev[e].node;
    const long ix = node % nx + (l % 3 - 1), iy = node / nx + ((l / 3) % 3 - 1);
    double S = nan_();
    int n = 0;
    if (m >= 0 && m < M && ix >= 0 && ix < nx && iy >= 0 && iy < ny) {
        const int nv = v.meta[0], needv = v.meta[1];
        const size_t x = (size_t)iy * nx + ix;
        rt::StackSums a{0, 0.0, 0.0};
        for (int i = 0; i < nv; i++) {
            const double* __restrict__ cr = v.c + (size_t)v.sidx[i] * (size_t)v.nt;
            rt::stack_step<W>(a, v.ov[m], v.T[(size_t)v.sidx[i] * v.nn + x], W ? v.swt[i] : 0.0, v.ax, [&](long j, double& c0, double& c1) {
                c0 = cr[j];
                c1 = cr[j + 1];
            });
        }
        S = rt::stack_value<W>(a, needv);
        n = a.n;
    }
    out[e].win[l] = S;
    if (l == 13) out[e].n = n;
}

// How a call splits its scan
struct Geometry {
    long nchunks, per_part;
    unsigned ntiles, nparts;
};

// what every form of the call refuses before it touches the device
int check_call(const char* who, const rtmi_locator* loc, const rtmi_stack_params* sp, const void* c, const void* peak, const void* peak_node,
               const void* events, const void* nev, Geometry* g) {
    RTMI_ARG(loc, "null handle");
    RTMI_ARG(sp, "null sp");
    RTMI_ARG(c, "null c");
    RTMI_ARG(peak, "null peak");
    RTMI_ARG(peak_node, "null peak_node");
    RTMI_ARG(nev, "null nev");
    RTMI_ARG(events || sp->max_events <= 0, "null events with max_events > 0");
    RTMI_ARG(sp->nt >= 2, "nt must be >= 2");
    RTMI_ARG(sp->nt <= (int64_t)1 << 31, "nt is over 2^31");
    RTMI_ARG(sp->M >= 1, "M must be >= 1");
    RTMI_ARG(std::isfinite(sp->cdt) && sp->cdt > 0.0, "cdt must be finite and > 0");
    RTMI_ARG(std::isfinite(sp->od) && sp->od > 0.0, "od must be finite and > 0");
    RTMI_ARG(std::isfinite(sp->ct0), "ct0 must be finite");
    RTMI_ARG(std::isfinite(sp->o0), "o0 must be finite");
    RTMI_ARG(sp->need >= 0, "need is negative");
    RTMI_ARG(sp->min_sep >= 0, "min_sep is negative");
    RTMI_ARG(sp->max_events >= 0, "max_events is negative");
    RTMI_ARG(!std::isnan(sp->threshold), "threshold is NaN");
    const char* limit = "M is over 2^31 - 17, or more than 2^31 (tile of 256 nodes, chunk of 16 scan indices) pairs: split the scan over several calls";
    RTMI_ARG(sp->M <= (int64_t)INT32_MAX - kChunk, limit);           // scan indices are int32; the handle is read from here on
    const int64_t nc = (sp->M - 1) / kChunk + 1, nt = (int64_t)((loc->nn + kTile - 1) / kTile);
    RTMI_ARG((double)nc * (double)nt < (double)((int64_t)1 << 31), limit);
    g->nchunks = (long)nc;
    g->ntiles = (unsigned)nt;
    // parts of whole chunks, enough of them that the blocks fill the device several times over; at most 65535, the grid's second dimension
    const int64_t want = ((int64_t)kBlocksPerCu * (loc->cus > 0 ? loc->cus : 1) + nt - 1) / nt;
    const int64_t parts = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, nc), 65535));
    g->per_part = (long)((nc + parts - 1) / parts);
    g->nparts = (unsigned)((nc + g->per_part - 1) / g->per_part);
    return RTMI_OK;
}

int stack_dev(rtmi_locator* loc, const char* who, const rtmi_stack_params& sp, const Geometry& g, const double* d_c, const double* d_w,
              double* d_peak, int32_t* d_peak_node, double* d_best, int32_t* d_best_m, double* d_volume, rtmi_stack_event* events,
              int64_t* nev, rtmi_stack_stats* st) {
    const int P = (int)loc->lp.P;
    const size_t nn = loc->nn, M = (size_t)sp.M, Mpad = (size_t)g.nchunks * kChunk;
    const bool maps = d_best || d_best_m;
    DevMem mem;
    double *ov = nullptr, *swt = nullptr, *pkey = nullptr, *bkey = nullptr;
    int *sidx = nullptr, *meta = nullptr;
    int32_t* bm = nullptr;
    unsigned* pnode = nullptr;
    long long *pcnt = nullptr, *total = nullptr;
    const size_t nblocks = (size_t)g.ntiles * g.nparts;
    RTMI_ALLOC(mem.get(&ov, Mpad * sizeof(double)));
    RTMI_ALLOC(mem.get(&swt, (size_t)P * sizeof(double)));
    RTMI_ALLOC(mem.get(&sidx, (size_t)P * sizeof(int)));
    RTMI_ALLOC(mem.get(&meta, 2 * sizeof(int)));
    RTMI_ALLOC(mem.get(&pkey, M * g.ntiles * sizeof(double)));
    RTMI_ALLOC(mem.get(&pnode, M * g.ntiles * sizeof(unsigned)));
    RTMI_ALLOC(mem.get(&pcnt, nblocks * sizeof(long long)));
    RTMI_ALLOC(mem.get(&total, sizeof(long long)));
    if (maps) {
        RTMI_ALLOC(mem.get(&bkey, (size_t)g.nparts * nn * sizeof(double)));
        RTMI_ALLOC(mem.get(&bm, (size_t)g.nparts * nn * sizeof(int32_t)));
    }
    const StackView v{loc->T, d_c, nn, (long)sp.nt, ov, sidx, swt, meta, rt::StackAxis{sp.ct0, 1.0 / sp.cdt, (double)(sp.nt - 1)}};
    EventMarks<6> ev;
    RTMI_HIP(ev.create());
    RTMI_HIP(ev.mark(0));
    hipLaunchKernelGGL(k_stack_prep, blocks((long)Mpad), dim3(256), 0, nullptr, d_w, P, (int)std::min<int64_t>(sp.need, INT32_MAX), sp.o0, sp.od,
                       (long)Mpad, ov, sidx, swt, meta);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    const dim3 grid(g.ntiles, g.nparts);
    if (d_w) {
        hipLaunchKernelGGL(k_stack<true>, grid, dim3(kTile), 0, nullptr, v, (long)M, g.nchunks, g.per_part, g.ntiles, d_volume, bkey, bm, pkey, pnode, pcnt);
    } else {
        hipLaunchKernelGGL(k_stack<false>, grid, dim3(kTile), 0, nullptr, v, (long)M, g.nchunks, g.per_part, g.ntiles, d_volume, bkey, bm, pkey, pnode, pcnt);
    }
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(2));
    hipLaunchKernelGGL(k_stack_pick, dim3((unsigned)M), dim3(256), 0, nullptr, pkey, pnode, g.ntiles, d_peak, d_peak_node);
    RTMI_HIP(hipGetLastError());
    if (maps) {
        hipLaunchKernelGGL(k_stack_merge, blocks((long)nn), dim3(256), 0, nullptr, bkey, bm, g.nparts, nn, d_best, d_best_m);
        RTMI_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_stack_total, dim3(1), dim3(256), 0, nullptr, pcnt, nblocks, total);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(3));
    RTMI_HIP(ev.wait(3));

    // the events: chosen on the host from the detection series, their windows by one more kernel
    std::vector<double> peak(M);
    std::vector<int32_t> peak_node(M);
    long long contributing = 0;
    RTMI_HIP(hipMemcpy(peak.data(), d_peak, M * sizeof(double), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(peak_node.data(), d_peak_node, M * sizeof(int32_t), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(&contributing, total, sizeof(long long), hipMemcpyDeviceToHost));
    int remained = 0;
    const std::vector<int64_t> taken = rt::stack_select(peak.data(), peak_node.data(), sp.M, sp.threshold, sp.min_sep, sp.max_events, &remained);
    const size_t K = taken.size();
    *nev = (int64_t)K;
    double window_ms = 0.0;
    if (K) {
        const long nx = (long)loc->lp.nx, ny = (long)loc->lp.ny;
        std::vector<DevEvent> he(K);
        for (size_t k = 0; k < K; k++) he[k] = DevEvent{(int32_t)taken[k], peak_node[(size_t)taken[k]]};
        DevEvent* dev_ev = nullptr;
        DevWin* dev_win = nullptr;
        RTMI_ALLOC(mem.get(&dev_ev, K * sizeof(DevEvent)));
        RTMI_ALLOC(mem.get(&dev_win, K * sizeof(DevWin)));
        RTMI_HIP(hipMemcpy(dev_ev, he.data(), K * sizeof(DevEvent), hipMemcpyHostToDevice));
        RTMI_HIP(ev.mark(4));
        if (d_w) {
            hipLaunchKernelGGL(k_stack_window<true>, dim3((unsigned)K), dim3(64), 0, nullptr, v, nx, ny, (long)M, dev_ev, dev_win);
        } else {
            hipLaunchKernelGGL(k_stack_window<false>, dim3((unsigned)K), dim3(64), 0, nullptr, v, nx, ny, (long)M, dev_ev, dev_win);
        }
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(ev.mark(5));
        RTMI_HIP(ev.wait(5));
        RTMI_HIP(ev.ms(4, 5, &window_ms));
        std::vector<DevWin> hw(K);
        RTMI_HIP(hipMemcpy(hw.data(), dev_win, K * sizeof(DevWin), hipMemcpyDeviceToHost));
        const rt::LocateGrid lg{loc->lp.gx0, loc->lp.gdx, loc->lp.gy0, loc->lp.gdy};
        for (size_t k = 0; k < K; k++) {
            rtmi_stack_event& r = events[k];
            r = rtmi_stack_event{};
            r.m = he[k].m;
            r.node = he[k].node;
            r.ix = (int32_t)(he[k].node % nx);
            r.iy = (int32_t)(he[k].node / nx);
            r.n = hw[k].n;
            r.value = hw[k].win[13];
            r.t0 = sp.o0 + (double)r.m * sp.od;
            for (int q = 0; q < 27; q++) r.win[q] = hw[k].win[q];
            const rt::StackRefined f = rt::stack_refine(r.win, r.t0, sp.od, r.ix, r.iy, lg);
            r.x = f.x;
            r.y = f.y;
            r.t0_refined = f.t0;
            r.dx = f.dx;
            r.dy = f.dy;
            r.dm = f.dm;
            r.refined = f.refined;
        }
    }
    if (st) {
        *st = rtmi_stack_stats{};
        double front_ms = 0.0, search_ms = 0.0;
        RTMI_HIP(ev.ms(0, 3, &front_ms));
        RTMI_HIP(ev.ms(1, 2, &search_ms));
        st->kernel_ms = front_ms + window_ms;
        st->reserved[0] = (int64_t)std::llround(search_ms * 1e6);            // k_stack's share of kernel_ms, in nanoseconds
        st->reserved[1] = (int64_t)g.nparts;                                   // the parts the scan was split into
        st->triples = (int64_t)nn * sp.M * P;
        st->contributing = contributing;
        st->truncated = remained;
    }
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_locate_stack_dev(rtmi_locator* loc, const rtmi_stack_params* sp, const double* d_c, const double* d_w, double* d_peak,
                                      int32_t* d_peak_node, double* d_best, int32_t* d_best_m, double* d_volume, rtmi_stack_event* events,
                                      int64_t* nev, rtmi_stack_stats* st) {
    const char* who = "rtmi_locate_stack_dev";
    Geometry g{};
    RTMI_RC(check_call(who, loc, sp, d_c, d_peak, d_peak_node, events, nev, &g));
    RTMI_RC(check_device(loc, who));
    const size_t P = (size_t)loc->lp.P, M = (size_t)sp->M, nn = loc->nn;
    RTMI_RC(check_device_pointer(loc->device, who, d_c, P * (size_t)sp->nt * sizeof(double), "d_c"));
    if (d_w) RTMI_RC(check_device_pointer(loc->device, who, d_w, P * sizeof(double), "d_w"));
    RTMI_RC(check_device_pointer(loc->device, who, d_peak, M * sizeof(double), "d_peak"));
    RTMI_RC(check_device_pointer(loc->device, who, d_peak_node, M * sizeof(int32_t), "d_peak_node"));
    if (d_best) RTMI_RC(check_device_pointer(loc->device, who, d_best, nn * sizeof(double), "d_best"));
    if (d_best_m) RTMI_RC(check_device_pointer(loc->device, who, d_best_m, nn * sizeof(int32_t), "d_best_m"));
    if (d_volume) RTMI_RC(check_device_pointer(loc->device, who, d_volume, M * nn * sizeof(double), "d_volume"));
    return stack_dev(loc, who, *sp, g, d_c, d_w, d_peak, d_peak_node, d_best, d_best_m, d_volume, events, nev, st);
}

RTMI_EXPORT int rtmi_locate_stack(rtmi_locator* loc, const rtmi_stack_params* sp, const double* c, const double* w, double* peak,
                                  int32_t* peak_node, double* best, int32_t* best_m, double* volume, rtmi_stack_event* events, int64_t* nev,
                                  rtmi_stack_stats* st) {
    const char* who = "rtmi_locate_stack";
    Geometry g{};
    RTMI_RC(check_call(who, loc, sp, c, peak, peak_node, events, nev, &g));
    RTMI_RC(check_device(loc, who));
    const size_t P = (size_t)loc->lp.P, M = (size_t)sp->M, nn = loc->nn, samples = P * (size_t)sp->nt;
    DevMem mem;
    double *d_c = nullptr, *d_w = nullptr, *d_peak = nullptr, *d_best = nullptr, *d_volume = nullptr;
    int32_t *d_peak_node = nullptr, *d_best_m = nullptr;
    const double t0 = now_ms();
    RTMI_ALLOC(mem.get(&d_c, samples * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_c, c, samples * sizeof(double), hipMemcpyHostToDevice));
    if (w) {
        RTMI_ALLOC(mem.get(&d_w, P * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_w, w, P * sizeof(double), hipMemcpyHostToDevice));
    }
    const double upload_ms = now_ms() - t0;
    RTMI_ALLOC(mem.get(&d_peak, M * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_peak_node, M * sizeof(int32_t)));
    if (best) RTMI_ALLOC(mem.get(&d_best, nn * sizeof(double)));
    if (best_m) RTMI_ALLOC(mem.get(&d_best_m, nn * sizeof(int32_t)));
    if (volume) RTMI_ALLOC(mem.get(&d_volume, M * nn * sizeof(double)));
    RTMI_RC(stack_dev(loc, who, *sp, g, d_c, d_w, d_peak, d_peak_node, d_best, d_best_m, d_volume, events, nev, st));
    RTMI_HIP(hipMemcpy(peak, d_peak, M * sizeof(double), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(peak_node, d_peak_node, M * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (best) RTMI_HIP(hipMemcpy(best, d_best, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (best_m) RTMI_HIP(hipMemcpy(best_m, d_best_m, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (volume) RTMI_HIP(hipMemcpy(volume, d_volume, M * nn * sizeof(double), hipMemcpyDeviceToHost));
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}
