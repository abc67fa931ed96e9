// eikonal.hip -- the eikonal continuation of traveltime tables: the first-order Godunov upwind scheme for |grad T| = n by fast
// sweeping, seeded by a table's covered nodes and a small analytic ball round the source (rtmi_eikonal_fill and its _dev form;
// include/rtmi.h).  The arithmetic of a node is rt_eikonal.h's; the kernel only decides who runs it when.
//   k_eikonal<LDS, FACTORED>  one workgroup per source, the round loop inside.  A sweep walks the anti-diagonals of the grid in the
//                   sweep's own directions; the nodes of one diagonal do not read one another, so the lanes take them side by
//                   side (striding where a diagonal is longer than the block) and a block barrier parts two diagonals: the
//                   serial sweep's bits.  LDS: the source's working table, the slowness and the node states live in the block's
//                   LDS; otherwise in a work space in global memory, which the L2 holds.  FACTORED: the source-factored scheme
//                   (DESIGN.md section 39): the update is rt::eik_update_factored, which evaluates T0 = n_src r at the node and
//                   at its two parents in registers -- no table of it, so both schemes have the same LDS rule and work space.
// Every loop bound and every barrier is uniform across the block and max_rounds bounds the whole; no block waits for another.
// No atomics on floating point.
#include "rtmi_host.h"

#include "rt_eikonal.h"
#include "rt_eikonal_host.h"

namespace {

constexpr size_t kLdsBudget = (size_t)128 << 10;        // the LDS path's share of a CU's 160 KiB: T, n (8 bytes each) and the state per node
constexpr size_t kLdsPerNode = 2 * sizeof(double) + 1;
constexpr size_t kWorkBudget = (size_t)1 << 30;         // the global path's work space of one group of sources
constexpr int kOutWords = 4;                            // per source: rounds | clean << 32, free nodes, filled nodes, changes

struct EikArgs {
    rt::EikGrid g;
    long nx, ny;
    double ball;
    int max_rounds;
    const double* n;            // [ny][nx]
    const double* src;          // [S][2]
    const double* n_src;        // [S]
    double* T;                  // [S][ny][nx] or NULL
    uint8_t* filled;            // [S][ny][nx] or NULL
    double* work;               // global path: [S][ny][nx]
    uint8_t* state;             // global path: [S][ny][nx]
    unsigned long long* out;    // [S][kOutWords]
};

template <bool LDS, bool FACTORED> __global__ void __launch_bounds__(kMaxBlock) k_eikonal(const EikArgs a) {
    extern __shared__ double lds[];                     // LDS: [T | n | state]
    __shared__ unsigned long long red[2][kMaxBlock / 64];
    const int tid = (int)threadIdx.x, bd = (int)blockDim.x;
    const long nx = a.nx, ny = a.ny, nn = nx * ny;
    const size_t s = blockIdx.x;
    const double inf = rt::eik_inf();
    double* w;
    const double* nv;
    uint8_t* st;
    if constexpr (LDS) {
        w = lds;
        nv = lds + nn;
        st = (uint8_t*)(lds + 2 * nn);
    } else {
        w = a.work + s * (size_t)nn;
        nv = a.n;
        st = a.state + s * (size_t)nn;
    }
    const double xs = a.src[2 * s], ys = a.src[2 * s + 1], n_src = a.n_src[s];
    double* Tg = a.T ? a.T + s * (size_t)nn : nullptr;
    // the states and the starting values
    unsigned long long nfree = 0, nopen = 0, nseed = 0;
    for (long x = tid; x < nn; x += bd) {
        const double sl = a.n[x];
        double w0;
        const uint8_t state = rt::eik_init(a.g, x % nx, x / nx, sl, Tg ? Tg[x] : rt::eik_nan(), xs, ys, n_src, a.ball, &w0);
        if constexpr (LDS) lds[nn + x] = sl;
        w[x] = w0;
        st[x] = state;
        if (state != rt::kEikFrozen) nfree++;
        if (state == rt::kEikFree) nopen++;
        else if (w0 < inf) nseed++;
    }
    nfree = block_sum(red, 0, nfree);
    nopen = block_sum(red, 1, nopen);
    nseed = block_sum(red, 0, nseed);       // its barrier also parts the starting values from the first diagonal's reads
    int rounds = 0, clean = 1;
    unsigned long long changes = 0;
    if (nopen > 0 && nseed > 0) {
        const long ndiag = nx + ny - 1;
        while (rounds < a.max_rounds) {
            rounds++;
            unsigned long long mine = 0;
            for (int k = 0; k < 4; k++) {
                const bool xup = k == 0 || k == 3, yup = k < 2;
                for (long d = 0; d < ndiag; d++) {
                    // the diagonal p + q = d in the sweep's own coordinates: q in [q0, q1]
                    const long q0 = d - (nx - 1) > 0 ? d - (nx - 1) : 0, q1 = d < ny - 1 ? d : ny - 1;
                    for (long q = q0 + tid; q <= q1; q += bd) {
                        const long p = d - q, i = xup ? p : nx - 1 - p, j = yup ? q : ny - 1 - q, x = j * nx + i;
                        if (st[x] != rt::kEikFree) continue;
                        const double l = i > 0 ? w[x - 1] : inf, r = i + 1 < nx ? w[x + 1] : inf;
                        const double dn = j > 0 ? w[x - nx] : inf, up = j + 1 < ny ? w[x + nx] : inf;
                        double t;
                        if constexpr (FACTORED) t = rt::eik_update_factored(a.g, i, j, xs, ys, n_src, l, r, dn, up, nv[x]);
                        else t = rt::eik_update(a.g, rt::eik_min(l, r), rt::eik_min(dn, up), nv[x]);
                        if (t < w[x]) {
                            w[x] = t;
                            mine++;
                        }
                    }
                    __syncthreads();
                }
            }
            const unsigned long long changed = block_sum(red, rounds & 1, mine);
            changes += changed;
            clean = changed == 0;
            if (clean) break;
        }
    }
    // the free nodes' values out; obstacles and seeded nodes are not written
    unsigned long long nfilled = 0;
    for (long x = tid; x < nn; x += bd) {
        const bool open = st[x] != rt::kEikFrozen;
        const double v = w[x];
        const bool got = open && v < inf;
        if (open && Tg) Tg[x] = got ? v : rt::eik_nan();
        if (a.filled) a.filled[s * (size_t)nn + x] = got ? 1 : 0;
        if (got) nfilled++;
    }
    nfilled = block_sum(red, (rounds & 1) ^ 1, nfilled);
    if (tid == 0) {
        unsigned long long* o = a.out + s * kOutWords;
        o[0] = (unsigned long long)(unsigned)rounds | (unsigned long long)(unsigned)clean << 32;
        o[1] = nfree;
        o[2] = nfilled;
        o[3] = changes;
    }
}

int eikonal_dev(const char* who, const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src, const double* d_n_src,
                double* d_T, int32_t* rounds, uint8_t* d_filled, rtmi_eikonal_stats* stats) {
    rtmi_eikonal_stats total{};
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny;
    const size_t lds_bytes = (nn * kLdsPerNode + 7) / 8 * 8;
    // reserved[0]: 1 takes the global path where the LDS path would do, for tests; no result depends on it
    const bool lds = lds_bytes <= kLdsBudget && ep->reserved[0] != 1;
    total.path = lds ? RTMI_EIKONAL_LDS : RTMI_EIKONAL_GLOBAL;
    if (S > 0) {
        const long diag = (long)std::min(ep->nx, ep->ny);
        const int block = (int)std::min<long>(kMaxBlock, (diag + 63) / 64 * 64);
        const size_t group = lds ? (size_t)S : std::min((size_t)S, std::max<size_t>(1, kWorkBudget / (nn * (sizeof(double) + 1))));
        DevMem mem;
        EikArgs a{};
        a.g = rt::eik_grid(ep->gx0, ep->gdx, ep->gy0, ep->gdy);
        a.nx = (long)ep->nx;
        a.ny = (long)ep->ny;
        a.ball = ep->ball;
        a.max_rounds = ep->max_rounds > 0 ? ep->max_rounds : rt::kEikDefaultRounds;
        a.n = d_n;
        if (!lds) {
            RTMI_ALLOC(mem.get(&a.work, group * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.state, group * nn));
        }
        unsigned long long* d_out = nullptr;
        RTMI_ALLOC(mem.get(&d_out, (size_t)S * kOutWords * sizeof(unsigned long long)));
        const bool factored = eikonal_fills_factored(ep);
        auto* const kernel = lds ? (factored ? k_eikonal<true, true> : k_eikonal<true, false>)
                                 : (factored ? k_eikonal<false, true> : k_eikonal<false, false>);
        if (lds && lds_bytes > 65536)
            RTMI_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        EventMarks<2> marks;
        RTMI_HIP(marks.create());
        RTMI_HIP(marks.mark(0));
        for (size_t s0 = 0; s0 < (size_t)S; s0 += group) {
            const size_t gs = std::min(group, (size_t)S - s0);
            a.src = d_src + 2 * s0;
            a.n_src = d_n_src + s0;
            a.T = d_T ? d_T + s0 * nn : nullptr;
            a.filled = d_filled ? d_filled + s0 * nn : nullptr;
            a.out = d_out + s0 * kOutWords;
            hipLaunchKernelGGL(kernel, dim3((unsigned)gs), dim3(block), lds ? lds_bytes : 0, nullptr, a);
            RTMI_HIP(hipGetLastError());
        }
        RTMI_HIP(marks.mark(1));
        RTMI_HIP(marks.wait(1));
        RTMI_HIP(marks.ms(0, 1, &total.kernel_ms));
        std::vector<unsigned long long> out((size_t)S * kOutWords);
        RTMI_HIP(hipMemcpy(out.data(), d_out, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < (size_t)S; s++) {
            const unsigned long long* o = &out[s * kOutWords];
            const int32_t r = (int32_t)(o[0] & 0xffffffffull), clean = (int32_t)(o[0] >> 32);
            if (rounds) {
                rounds[2 * s] = r;
                rounds[2 * s + 1] = clean;
            }
            total.free_nodes += (int64_t)o[1];
            total.filled += (int64_t)o[2];
            total.changes += (int64_t)o[3];
            total.rounds_max = std::max(total.rounds_max, r);
        }
        total.unreached = total.free_nodes - total.filled;
    }
    if (stats) *stats = total;
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_fill_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                      const double* d_n_src, double* d_T, int32_t* rounds, uint8_t* d_filled,
                                      rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_fill_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    RTMI_RC(check_eikonal_scheme(who, ep));
    if (S > 0) {
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t nn = (size_t)ep->nx * (size_t)ep->ny;
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        if (d_T) RTMI_RC(check_device_pointer(device, who, d_T, (size_t)S * nn * sizeof(double), "d_T"));
        if (d_filled) RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
    }
    return eikonal_dev(who, ep, d_n, S, d_src, d_n_src, d_T, rounds, d_filled, stats);
}

RTMI_EXPORT int rtmi_eikonal_fill(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src, const double* n_src,
                                  double* T, int32_t* rounds, uint8_t* filled, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_fill";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    RTMI_RC(check_eikonal_scheme(who, ep));
    if (S == 0) return eikonal_dev(who, ep, nullptr, 0, nullptr, nullptr, nullptr, rounds, nullptr, stats);
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    double *d_n = nullptr, *d_src = nullptr, *d_n_src = nullptr, *d_T = nullptr;
    uint8_t* d_filled = nullptr;
    RTMI_ALLOC(mem.get(&d_n, nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_src, (size_t)S * 2 * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_n_src, (size_t)S * sizeof(double)));
    if (T) RTMI_ALLOC(mem.get(&d_T, tab * sizeof(double)));
    if (filled) RTMI_ALLOC(mem.get(&d_filled, tab));
    RTMI_HIP(hipMemcpy(d_n, n, nn * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_src, src, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_n_src, n_src, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    if (T) RTMI_HIP(hipMemcpy(d_T, T, tab * sizeof(double), hipMemcpyHostToDevice));
    RTMI_RC(eikonal_dev(who, ep, d_n, S, d_src, d_n_src, d_T, rounds, d_filled, stats));
    if (T) RTMI_HIP(hipMemcpy(T, d_T, tab * sizeof(double), hipMemcpyDeviceToHost));
    if (filled) RTMI_HIP(hipMemcpy(filled, d_filled, tab, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
