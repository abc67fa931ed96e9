// locate.hip -- event location by grid search over traveltime tables (rtmi_locator_*, rtmi_locate; include/rtmi.h, DESIGN.md
// section 29).  The arithmetic of a node is rt_locate.h's two steps; the kernels here only decide who runs them on what.
//   k_locate_prep    one lane per event: ref and the fewest picks of a candidate                               (rtmi_locator.h,
//   k_locate_stage   one lane per (chunk of 16 events, station): the chunk's picks as the search reads them     shared with
//   k_locate_pick    one block per event: the least (key, node) of its partials                                 edt.hip)
//   k_locate         one lane per node of a tile of 256, one block per (tile, chunk of 16 events): obj at every node, the map,
//                    and one partial (key, node, contributing) per (event, tile)
//   k_locate_window  one wave per event: obj and tau at the nine nodes around the best one, by the same two steps
// No atomics: every result is one lane's own chain of operations or an exact minimum, the same bits on every run.
#include "rtmi_locator.h"

#include "rt_locate.h"

namespace {

// what the window kernel leaves per event for the host
struct DevOut {
    int32_t node, n;
    double sw, ref;
    double wobj[9], wtau[9];
    long long contributing;
};

// One node's sums over the stations for one event of the chunk, as k_locate_window walks them: the same two steps in the same
// order as k_locate's loops, so the same bits.
template <bool W>
__device__ void node_objective(const double* __restrict__ T, size_t nn, int P, size_t x, const double* __restrict__ tr,
                               const double* __restrict__ wv, int needv, int* n_out, double* sw_out, double* obj, double* tau_out) {
    rt::LocateSums a{0, 0.0, 0.0};
    for (int r = 0; r < P; r++) {
        const double trv = tr[(size_t)r * kChunk];
        if (is_no_pick(trv)) continue;
        const double Tv = T[(size_t)r * nn + x];
        if (fabs(Tv) < INFINITY) rt::locate_pass1<W>(a, trv, W ? wv[(size_t)r * kChunk] : 0.0, Tv);
    }
    const double sw = W ? a.sw : (double)a.n;
    const bool cand = a.n >= needv;
    const double tau = cand ? a.sd / sw : no_pick();
    double q = 0.0;
    if (cand) {
        for (int r = 0; r < P; r++) {
            const double trv = tr[(size_t)r * kChunk];
            if (is_no_pick(trv)) continue;
            const double Tv = T[(size_t)r * nn + x];
            if (fabs(Tv) < INFINITY) rt::locate_pass2<W>(q, tau, trv, W ? wv[(size_t)r * kChunk] : 0.0, Tv);
        }
    }
    *n_out = a.n;
    *sw_out = sw;
    *obj = cand ? q / sw : INFINITY;
    *tau_out = tau;
}

// What a block of k_locate hands to its two passes
struct ChunkView {
    const double* __restrict__ T;      // the tables
    size_t nn, xl;                     // nodes per table; the lane's node, the last node for a lane past the grid
    int P;
    bool inb;                          // the lane has a node
    const double* __restrict__ tr;     // the chunk's staged picks [P][16], ...
    const double* __restrict__ wv;     // ... weights (W only) ...
    const unsigned* __restrict__ mask; // ... and masks [P]
    const int* __restrict__ needv;     // [16]
};

// The two passes of a lane over the stations for the 16 events of its chunk.  ALL: every event of the chunk has a valid pick at
// every station, the usual case: no test per event, the step runs under one test of the lane's table value.  Otherwise a step
// runs where the station's mask has the event's bit.  The steps and their order are the same, so no bit depends on the variant.
// The next station's value is asked for before this one's is used: a lane's only vector load per station and pass.  The load is
// unconditional (a lane past the grid reads the last node, the step past the last station reads that station again) so that no
// branch stands between it and the wait for the one before.
template <bool W, bool ALL>
__device__ __forceinline__ void chunk_passes(const ChunkView& v, rt::LocateSums (&a)[kChunk], double (&tau)[kChunk], double (&q)[kChunk],
                                             bool (&cand)[kChunk]) {
    auto table = [&](int r) { return v.T[(size_t)(r < v.P ? r : v.P - 1) * v.nn + v.xl]; };
    double Tn = table(0);
    int nfin = 0;                           // ALL: every event counts the same stations, those with a finite table value here
    for (int r = 0; r < v.P; r++) {
        const double Tv = Tn;
        Tn = table(r + 1);
        const bool fin = v.inb && fabs(Tv) < INFINITY;
        if (ALL) {
            if (fin) {
                nfin++;
#pragma unroll
                for (int k = 0; k < kChunk; k++) rt::locate_pass1<W>(a[k], v.tr[r * kChunk + k], W ? v.wv[r * kChunk + k] : 0.0, Tv);
            }
        } else {
            const unsigned m = v.mask[r];
#pragma unroll
            for (int k = 0; k < kChunk; k++)
                if (fin && (m >> k & 1)) rt::locate_pass1<W>(a[k], v.tr[r * kChunk + k], W ? v.wv[r * kChunk + k] : 0.0, Tv);
        }
    }
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
        if (ALL) a[k].n = nfin;
        if (!W) a[k].sw = (double)a[k].n;
        cand[k] = a[k].n >= v.needv[k];
        tau[k] = cand[k] ? a[k].sd / a[k].sw : no_pick();
        q[k] = 0.0;
    }
    Tn = table(0);
    for (int r = 0; r < v.P; r++) {
        const double Tv = Tn;
        Tn = table(r + 1);
        const bool fin = v.inb && fabs(Tv) < INFINITY;
        if (ALL) {
            if (fin) {
#pragma unroll
                for (int k = 0; k < kChunk; k++) rt::locate_pass2<W>(q[k], tau[k], v.tr[r * kChunk + k], W ? v.wv[r * kChunk + k] : 0.0, Tv);
            }
        } else {
            const unsigned m = v.mask[r];
#pragma unroll
            for (int k = 0; k < kChunk; k++)
                if (fin && (m >> k & 1)) rt::locate_pass2<W>(q[k], tau[k], v.tr[r * kChunk + k], W ? v.wv[r * kChunk + k] : 0.0, Tv);
        }
    }
}

// The search.  Block b works on tile b / nchunks and chunk b % nchunks: the blocks in flight share a few tiles, so a table value
// comes from HBM once and from the caches for the other chunks.  A lane holds its node's sums for the 16 events of the chunk in
// registers and walks the stations twice, reading T[r][x] once per pass and chunk, not once per event; the picks of a station are
// wave-uniform (scalar loads).
template <bool W>
__global__ void __launch_bounds__(kTile) k_locate(const double* __restrict__ T, size_t nn, int P, const double* __restrict__ tr,
                                                  const double* __restrict__ wv, const unsigned* __restrict__ mask,
                                                  const int* __restrict__ needv, long E, unsigned nchunks, unsigned ntiles,
                                                  double* __restrict__ maps, Partial* __restrict__ part) {
    const unsigned tile = blockIdx.x / nchunks, c = blockIdx.x % nchunks;
    const int tid = (int)threadIdx.x;
    const size_t x = (size_t)tile * kTile + tid;
    const bool inb = x < nn;
    const ChunkView v{T, nn, inb ? x : nn - 1, P, inb, tr + (size_t)c * P * kChunk, W ? wv + (size_t)c * P * kChunk : nullptr,
                      mask + (size_t)c * P, needv + (size_t)c * kChunk};
    bool all = true;
    for (int r = 0; r < P; r++) all = all && v.mask[r] == kAllPicks;

    rt::LocateSums a[kChunk];
    double tau[kChunk], q[kChunk];
    bool cand[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; k++) a[k] = rt::LocateSums{0, 0.0, 0.0};
    if (all) chunk_passes<W, true>(v, a, tau, q, cand);
    else chunk_passes<W, false>(v, a, tau, q, cand);

    __shared__ double wkey[kTile / 64][kChunk];
    __shared__ unsigned wnode[kTile / 64][kChunk];
    __shared__ int wcnt[kTile / 64][kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
        const long e = (long)c * kChunk + k;
        const double obj = cand[k] ? q[k] / a[k].sw : INFINITY;
        if (maps && inb && e < E) maps[(size_t)e * nn + x] = obj;
        double key = obj < INFINITY ? obj : INFINITY;                 // a NaN counts as +inf
        unsigned node = cand[k] && inb ? (unsigned)x : kNoNode;
        int cnt = a[k].n;
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
        for (int v = 1; v < kTile / 64; v++) {
            take_less(key, node, wkey[v][tid], wnode[v][tid]);
            cnt += wcnt[v][tid];
        }
        part[((size_t)c * kChunk + tid) * ntiles + tile] = Partial{key, node, cnt};
    }
}

// The 3 x 3 window around every event's best node: lane l of the event's wave takes row l / 3 and column l % 3.
template <bool W>
__global__ void __launch_bounds__(64) k_locate_window(const double* __restrict__ T, size_t nn, long nx, long ny, int P,
                                                      const double* __restrict__ tr, const double* __restrict__ wv,
                                                      const int* __restrict__ needv, const double* __restrict__ ref,
                                                      const int32_t* __restrict__ best, const long long* __restrict__ contributing,
                                                      DevOut* __restrict__ out) {
    const size_t e = blockIdx.x;
    const int l = (int)threadIdx.x;
    if (l >= 9) return;
    const int32_t node = best[e];
    DevOut& o = out[e];
    if (l == 4) {
        o.node = node;
        o.ref = node < 0 ? no_pick() : ref[e];
        o.contributing = contributing[e];
    }
    double obj = no_pick(), tau = no_pick(), sw = no_pick();
    int n = 0;
    if (node >= 0) {
        const long ix = node % nx + (l % 3 - 1), iy = node / nx + (l / 3 - 1);
        if (ix >= 0 && ix < nx && iy >= 0 && iy < ny) {
            const size_t off = (e / kChunk) * (size_t)P * kChunk + e % kChunk;
            node_objective<W>(T, nn, P, (size_t)iy * nx + ix, tr + off, W ? wv + off : nullptr, needv[e], &n, &sw, &obj, &tau);
        }
    }
    o.wobj[l] = obj;
    o.wtau[l] = tau;
    if (l == 4) {
        o.n = n;
        o.sw = sw;
    }
}

int locate_dev(rtmi_locator* loc, const char* who, int64_t E, unsigned nchunks, unsigned ntiles, const double* d_t, const double* d_w,
               const int32_t* d_need, rtmi_locate_result* res, double* d_maps, rtmi_locate_stats* st) {
    const int P = (int)loc->lp.P;
    const size_t nn = loc->nn, Epad = (size_t)nchunks * kChunk, staged = Epad * (size_t)P;
    DevMem mem;
    double *tr = nullptr, *wv = nullptr, *ref = nullptr;
    int* needv = nullptr;
    unsigned* mask = nullptr;
    Partial* part = nullptr;
    int32_t* best = nullptr;
    long long* contributing = nullptr;
    DevOut* out = nullptr;
    RTMI_ALLOC(mem.get(&tr, staged * sizeof(double)));
    if (d_w) RTMI_ALLOC(mem.get(&wv, staged * sizeof(double)));
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
    RTMI_HIP(ev.mark(1));
    const dim3 grid(nchunks * ntiles);
    if (d_w) {
        hipLaunchKernelGGL(k_locate<true>, grid, dim3(kTile), 0, nullptr, loc->T, nn, P, tr, wv, mask, needv, (long)E, nchunks, ntiles, d_maps, part);
    } else {
        hipLaunchKernelGGL(k_locate<false>, grid, dim3(kTile), 0, nullptr, loc->T, nn, P, tr, wv, mask, needv, (long)E, nchunks, ntiles, d_maps, part);
    }
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(2));
    hipLaunchKernelGGL(k_locate_pick, dim3((unsigned)E), dim3(256), 0, nullptr, part, ntiles, best, contributing);
    RTMI_HIP(hipGetLastError());
    const long nx = (long)loc->lp.nx, ny = (long)loc->lp.ny;
    if (d_w) {
        hipLaunchKernelGGL(k_locate_window<true>, dim3((unsigned)E), dim3(64), 0, nullptr, loc->T, nn, nx, ny, P, tr, wv, needv, ref, best, contributing, out);
    } else {
        hipLaunchKernelGGL(k_locate_window<false>, dim3((unsigned)E), dim3(64), 0, nullptr, loc->T, nn, nx, ny, P, tr, wv, needv, ref, best, contributing, out);
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
        rtmi_locate_result& r = res[e];
        r = rtmi_locate_result{};
        total += o.contributing;
        r.node = o.node;
        for (int k = 0; k < 9; k++) {
            r.win_obj[k] = o.wobj[k];
            r.win_tau[k] = o.wtau[k];
        }
        r.ref = o.ref;
        if (o.node < 0) {
            r.ix = r.iy = -1;
            r.sw = r.obj = r.t0 = r.x = r.y = r.t0_refined = r.dx = r.dy = r.cov[0] = r.cov[1] = r.cov[2] = nan;
            continue;
        }
        r.ix = (int32_t)(o.node % nx);
        r.iy = (int32_t)(o.node / nx);
        r.n = o.n;
        r.sw = o.sw;
        r.obj = o.wobj[4];
        r.t0 = o.ref + o.wtau[4];
        const rt::LocateRefined f = rt::locate_refine(o.wobj, o.wtau, o.ref, o.sw, r.ix, r.iy, g);
        r.x = f.x;
        r.y = f.y;
        r.t0_refined = f.t0;
        r.dx = f.dx;
        r.dy = f.dy;
        r.cov[0] = f.cov[0];
        r.cov[1] = f.cov[1];
        r.cov[2] = f.cov[2];
        r.refined = f.refined;
    }
    if (st) {
        *st = rtmi_locate_stats{};
        double search_ms = 0.0;
        RTMI_HIP(ev.ms(0, 3, &st->kernel_ms));
        RTMI_HIP(ev.ms(1, 2, &search_ms));
        st->reserved[0] = (int64_t)std::llround(search_ms * 1e6);          // k_locate's share of kernel_ms, in nanoseconds
        st->triples = (int64_t)E * (int64_t)nn * P;
        st->contributing = total;
    }
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_locator_create(const rtmi_locator_params* lp, const double* T, rtmi_locator** out) {
    const char* who = "rtmi_locator_create";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_ARG(lp, "null lp");
    RTMI_ARG(T, "null T");
    RTMI_ARG(lp->P >= 1, "P must be >= 1");
    RTMI_ARG(lp->P <= RTMI_LOCATE_MAX_TABLES, "P is over RTMI_LOCATE_MAX_TABLES (512)");
    RTMI_RC(check_grid_axes(who, *lp));
    rtmi_locator* loc = new rtmi_locator;
    struct Guard {
        rtmi_locator* p;
        ~Guard() { delete p; }
    } guard{loc};
    loc->lp = *lp;
    loc->nn = (size_t)lp->nx * (size_t)lp->ny;
    RTMI_HIP(hipGetDevice(&loc->device));
    RTMI_HIP(hipDeviceGetAttribute(&loc->cus, hipDeviceAttributeMultiprocessorCount, loc->device));
    const size_t bytes = (size_t)lp->P * loc->nn * sizeof(double);
    RTMI_ALLOC(hipMalloc((void**)&loc->T, bytes));
    RTMI_HIP(hipMemcpy(loc->T, T, bytes, hipMemcpyHostToDevice));
    guard.p = nullptr;
    *out = loc;
    return RTMI_OK;
}

RTMI_EXPORT void rtmi_locator_destroy(rtmi_locator* loc) { delete loc; }

RTMI_EXPORT int rtmi_locate_dev(rtmi_locator* loc, int64_t E, const double* d_t, const double* d_w, const int32_t* d_need,
                                rtmi_locate_result* res, double* d_maps, rtmi_locate_stats* st) {
    const char* who = "rtmi_locate_dev";
    unsigned nchunks = 0, ntiles = 0;
    RTMI_RC(check_picks_call(who, loc, E, d_t, res, &nchunks, &ntiles));
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P;
    RTMI_RC(check_device_pointer(loc->device, who, d_t, picks * sizeof(double), "d_t"));
    if (d_w) RTMI_RC(check_device_pointer(loc->device, who, d_w, picks * sizeof(double), "d_w"));
    if (d_need) RTMI_RC(check_device_pointer(loc->device, who, d_need, (size_t)E * sizeof(int32_t), "d_need"));
    if (d_maps) RTMI_RC(check_device_pointer(loc->device, who, d_maps, (size_t)E * loc->nn * sizeof(double), "d_maps"));
    return locate_dev(loc, who, E, nchunks, ntiles, d_t, d_w, d_need, res, d_maps, st);
}

RTMI_EXPORT int rtmi_locate(rtmi_locator* loc, int64_t E, const double* t, const double* w, const int32_t* need,
                            rtmi_locate_result* res, double* maps, rtmi_locate_stats* st) {
    const char* who = "rtmi_locate";
    unsigned nchunks = 0, ntiles = 0;
    RTMI_RC(check_picks_call(who, loc, E, t, res, &nchunks, &ntiles));
    if (need)
        for (int64_t e = 0; e < E; e++) RTMI_ARG(need[e] >= 0, "need[" + std::to_string(e) + "] is negative");
    RTMI_RC(check_device(loc, who));
    const size_t picks = (size_t)E * (size_t)loc->lp.P;
    DevMem mem;
    double *d_t = nullptr, *d_w = nullptr, *d_maps = nullptr;
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
    if (maps) RTMI_ALLOC(mem.get(&d_maps, (size_t)E * loc->nn * sizeof(double)));
    RTMI_RC(locate_dev(loc, who, E, nchunks, ntiles, d_t, d_w, d_need, res, d_maps, st));
    if (maps) RTMI_HIP(hipMemcpy(maps, d_maps, (size_t)E * loc->nn * sizeof(double), hipMemcpyDeviceToHost));
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}
