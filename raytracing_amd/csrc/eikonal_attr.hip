// eikonal_attr.hip -- launch angle, direction and spreading at the nodes the eikonal fill gave a value: what the rays know at
// the covered nodes, carried through the causal network of parents that the table defines (rtmi_eikonal_attributes and its _dev
// form; include/rtmi.h).  The arithmetic of a node is rt_eikonal_attr.h's; the kernels only decide who
// runs it when.
//   k_eikonal_attr<LDS>   the launch angle.  One workgroup per source, the round loop inside, built as k_eikonal_lin: a setup pass
//                   turns T, n and filled into each node's code and weight w = cb / (ca + cb) once and sets the starting values
//                   (the ball from the host's table of atan2, free nodes NaN); then the sweeps walk the anti-diagonals, the lanes
//                   side by side on one diagonal and a block barrier between two.  LDS: the values, the weights and the codes (17
//                   bytes per node) live in the block's LDS and the nodes of the ball and the free nodes are written out at the
//                   end; otherwise the values live in the output and the rest in a work space in global memory.
//   k_eikonal_attr_nodes  dir, J and G, after the sweeps on the same stream: one lane per (source, node) of the whole call.  It
//                   finds the node's class and parents again through eik_lin_node and reads the final launch angle of the four
//                   neighbours.
// Every loop bound and every barrier is uniform across the block and max_rounds bounds the whole; no block waits for another.
// No atomics.
#include "rtmi_host.h"

#include "rt_eikonal_attr.h"
#include "rt_eikonal_host.h"

namespace {

constexpr size_t kLdsBudget = (size_t)128 << 10;        // the LDS path's share of a CU's 160 KiB
constexpr size_t kLdsPerNode = 2 * sizeof(double) + 1;  // value, weight and the code
constexpr size_t kWorkBudget = (size_t)1 << 30;         // the work space of one group of sources
constexpr int kOutWords = 4;                            // per source: rounds | clean << 32, free and ball nodes, changes, strays
constexpr int kBoxWords = 5;                            // per source: i0, i1, j0, j1 of the ball's box and where its table starts

struct AttrArgs {
    rt::EikGrid g;
    long nx, ny;
    double ball;
    int max_rounds;
    size_t S;                   // k_eikonal_attr_nodes: the sources of the call
    const double* n;            // [ny][nx]
    const double* src;          // [S][2]
    const double* n_src;        // [S]
    const double* T;            // [S][ny][nx]
    const uint8_t* filled;      // [S][ny][nx]
    const long* box;            // [S][kBoxWords]
    const double* ball_theta0;  // atan2(dy, dx) over every source's box, row by row
    double* theta0;             // [S][ny][nx], in and out
    double* dir;                // [S][2][ny][nx] or NULL
    double *J, *G;              // [S][ny][nx] or NULL
    double* w;                  // global path: [S][ny][nx]
    uint8_t* code;              // global path: [S][ny][nx]
    unsigned long long* out;    // [S][kOutWords]
};

template <bool LDS> __global__ void __launch_bounds__(kMaxBlock) k_eikonal_attr(const AttrArgs a) {
    extern __shared__ double lds[];                     // LDS: [v | w | code]
    __shared__ unsigned long long red[2][kMaxBlock / 64];
    const int tid = (int)threadIdx.x, bd = (int)blockDim.x;
    const long nx = a.nx, ny = a.ny, nn = nx * ny;
    const size_t s = blockIdx.x;
    const double xs = a.src[2 * s], ys = a.src[2 * s + 1], n_src = a.n_src[s];
    const double* Ts = a.T + s * (size_t)nn;
    const uint8_t* fs = a.filled + s * (size_t)nn;
    double* vg = a.theta0 + s * (size_t)nn;
    const long* box = a.box + s * kBoxWords;
    const long bi0 = box[0], bi1 = box[1], bj0 = box[2], bj1 = box[3], bw = bi1 - bi0 + 1;
    const double* tab = a.ball_theta0 + box[4];
    double *v, *w;
    uint8_t* code;
    if constexpr (LDS) {
        v = lds;
        w = lds + nn;
        code = (uint8_t*)(lds + 2 * nn);
    } else {
        v = vg;
        w = a.w + s * (size_t)nn;
        code = a.code + s * (size_t)nn;
    }
    // the classes, the weights and the starting values
    unsigned long long nfree = 0, nnodes = 0, nstray = 0;
    for (long x = tid; x < nn; x += bd) {
        const long i = x % nx, j = x / nx;
        const rt::EikLinNode c = rt::eik_lin_node(a.g, nx, ny, i, j, a.n, Ts, fs, xs, ys, n_src, a.ball);
        const uint8_t cls = rt::eik_lin_class(c.code);
        w[x] = rt::eik_attr_weight(c);
        code[x] = c.code;
        if (cls == rt::kLinBall) {
            // a node of the ball outside the box reads nothing: the host sees the count and calls again with the whole grid as the box
            const bool in = i >= bi0 && i <= bi1 && j >= bj0 && j <= bj1;
            v[x] = in ? tab[(j - bj0) * bw + (i - bi0)] : rt::eik_nan();
            if (!in) nstray++;
        } else if (cls == rt::kLinFree) {
            v[x] = rt::eik_nan();
        } else if constexpr (LDS) {
            v[x] = vg[x];
        }
        if (cls >= rt::kLinFree) nnodes++;
        if (cls == rt::kLinFree) nfree++;
    }
    nnodes = block_sum(red, 0, nnodes);
    nstray = block_sum(red, 1, nstray);
    nfree = block_sum(red, 0, nfree);       // its barrier also parts the starting values from the first diagonal's reads
    int rounds = 0, clean = 1;
    unsigned long long changes = 0;
    if (nfree > 0) {
        const long ndiag = nx + ny - 1;
        while (rounds < a.max_rounds) {
            rounds++;
            unsigned long long mine = 0;
            for (int k = 0; k < 4; k++) {
                const bool xup = rt::eik_lin_xup(false, k), yup = rt::eik_lin_yup(false, k);
                for (long d = 0; d < ndiag; d++) {
                    // the diagonal p + q = d in the sweep's own coordinates: q in [q0, q1]
                    const long q0 = d - (nx - 1) > 0 ? d - (nx - 1) : 0, q1 = d < ny - 1 ? d : ny - 1;
                    for (long q = q0 + tid; q <= q1; q += bd) {
                        const long p = d - q, i = xup ? p : nx - 1 - p, j = yup ? q : ny - 1 - q, x = j * nx + i;
                        const uint8_t c = code[x];
                        if (rt::eik_lin_class(c) != rt::kLinFree) continue;
                        const double t = rt::eik_attr_gather(nx, x, c, w[x], v);
                        if (rt::eik_bits(t) != rt::eik_bits(v[x])) {
                            v[x] = t;
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
    if constexpr (LDS)
        for (long x = tid; x < nn; x += bd)
            if (rt::eik_lin_class(code[x]) >= rt::kLinFree) vg[x] = v[x];
    if (tid == 0) {
        unsigned long long* o = a.out + s * kOutWords;
        o[0] = (unsigned long long)(unsigned)rounds | (unsigned long long)(unsigned)clean << 32;
        o[1] = nnodes;
        o[2] = changes;
        o[3] = nstray;
    }
}

__global__ void __launch_bounds__(256) k_eikonal_attr_nodes(const AttrArgs a, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long nn = a.nx * a.ny, x = t % nn, i = x % a.nx, j = x / a.nx;
    const size_t s = (size_t)(t / nn);
    const double xs = a.src[2 * s], ys = a.src[2 * s + 1];
    const double* Ts = a.T + s * (size_t)nn;
    const rt::EikLinNode c = rt::eik_lin_node(a.g, a.nx, a.ny, i, j, a.n, Ts, a.filled + s * (size_t)nn, xs, ys, a.n_src[s], a.ball);
    if (rt::eik_lin_class(c.code) < rt::kLinFree) return;
    double* px = a.dir ? a.dir + s * 2 * (size_t)nn : nullptr;
    rt::eik_attr_node(a.g, a.nx, a.ny, i, j, a.n, Ts, c, xs, ys, a.theta0 + s * (size_t)nn, px, px ? px + nn : nullptr,
                      a.J ? a.J + s * (size_t)nn : nullptr, a.G ? a.G + s * (size_t)nn : nullptr);
}

// The table of atan2 over every source's box, by the host's libm.  whole: every box is the grid
void ball_tables(const rtmi_eikonal_params* ep, const rt::EikGrid& g, size_t S, const double* src, bool whole, std::vector<long>* box,
                 std::vector<double>* tab) {
    box->assign(S * kBoxWords, 0);
    tab->clear();
    for (size_t s = 0; s < S; s++) {
        long* b = &(*box)[s * kBoxWords];
        const double xs = src[2 * s], ys = src[2 * s + 1];
        rt::eik_lin_ball_box(g, (long)ep->nx, (long)ep->ny, xs, ys, ep->ball, &b[0], &b[1], &b[2], &b[3]);
        if (whole) {
            b[0] = b[2] = 0;
            b[1] = (long)ep->nx - 1;
            b[3] = (long)ep->ny - 1;
        }
        if (b[1] < b[0] || b[3] < b[2]) {               // empty: no node can be of the ball
            b[0] = b[2] = 0;
            b[1] = b[3] = -1;
        }
        b[4] = (long)tab->size();
        for (long j = b[2]; j <= b[3]; j++)
            for (long i = b[0]; i <= b[1]; i++) {
                double dx, dy;
                rt::eik_attr_radius(g, i, j, xs, ys, &dx, &dy);
                tab->push_back(std::atan2(dy, dx));
            }
    }
}

// One call on device memory: a holds the caller's pointers for all S sources, src the sources on the host
int attr_dev(const char* who, const rtmi_eikonal_params* ep, int64_t S, const double* src, AttrArgs a, int32_t* rounds,
             rtmi_eikonal_stats* stats) {
    rtmi_eikonal_stats total{};
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny;
    const size_t lds_bytes = (nn * kLdsPerNode + 7) / 8 * 8;
    // reserved[0]: 1 takes the global path where the LDS path would do, for tests; no result depends on it
    const bool lds = lds_bytes <= kLdsBudget && ep->reserved[0] != 1;
    total.path = lds ? RTMI_EIKONAL_LDS : RTMI_EIKONAL_GLOBAL;
    if (S > 0) {
        const long diag = (long)std::min(ep->nx, ep->ny);
        const int block = (int)std::min<long>(kMaxBlock, (diag + 63) / 64 * 64);
        const size_t per = lds ? 0 : sizeof(double) + 1;
        const size_t group = per ? std::min((size_t)S, std::max<size_t>(1, kWorkBudget / (nn * per))) : (size_t)S;
        DevMem mem;
        a.g = rt::eik_grid(ep->gx0, ep->gdx, ep->gy0, ep->gdy);
        a.nx = (long)ep->nx;
        a.ny = (long)ep->ny;
        a.ball = ep->ball;
        a.max_rounds = ep->max_rounds > 0 ? ep->max_rounds : rt::kEikDefaultRounds;
        a.S = (size_t)S;
        if (!lds) {
            RTMI_ALLOC(mem.get(&a.w, group * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.code, group * nn));
        }
        unsigned long long* d_out = nullptr;
        RTMI_ALLOC(mem.get(&d_out, (size_t)S * kOutWords * sizeof(unsigned long long)));
        if (lds && lds_bytes > 65536)
            RTMI_HIP(hipFuncSetAttribute((const void*)k_eikonal_attr<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        std::vector<unsigned long long> out((size_t)S * kOutWords);
        EventMarks<2> marks;
        RTMI_HIP(marks.create());
        // once with the ball's boxes; again with the whole grid as every box if a node of the ball lay outside its box
        for (int pass = 0; pass < 2; pass++) {
            std::vector<long> box;
            std::vector<double> tab;
            ball_tables(ep, a.g, (size_t)S, src, pass == 1, &box, &tab);
            long* d_box = nullptr;
            double* d_tab = nullptr;
            RTMI_ALLOC(mem.get(&d_box, box.size() * sizeof(long)));
            RTMI_ALLOC(mem.get(&d_tab, tab.size() * sizeof(double)));
            RTMI_HIP(hipMemcpy(d_box, box.data(), box.size() * sizeof(long), hipMemcpyHostToDevice));
            if (!tab.empty()) RTMI_HIP(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
            a.ball_theta0 = d_tab;
            const AttrArgs all = a;
            RTMI_HIP(marks.mark(0));
            for (size_t s0 = 0; s0 < (size_t)S; s0 += group) {
                const size_t gs = std::min(group, (size_t)S - s0);
                AttrArgs b = all;
                b.src = all.src + 2 * s0;
                b.n_src = all.n_src + s0;
                b.T = all.T + s0 * nn;
                b.filled = all.filled + s0 * nn;
                b.theta0 = all.theta0 + s0 * nn;
                b.box = d_box + s0 * kBoxWords;
                b.out = d_out + s0 * kOutWords;
                if (lds) hipLaunchKernelGGL((k_eikonal_attr<true>), dim3((unsigned)gs), dim3(block), lds_bytes, nullptr, b);
                else hipLaunchKernelGGL((k_eikonal_attr<false>), dim3((unsigned)gs), dim3(block), 0, nullptr, b);
                RTMI_HIP(hipGetLastError());
            }
            if (a.dir || a.J || a.G) {
                const long lanes = (long)((size_t)S * nn);
                hipLaunchKernelGGL(k_eikonal_attr_nodes, blocks(lanes), dim3(256), 0, nullptr, all, lanes);
                RTMI_HIP(hipGetLastError());
            }
            RTMI_HIP(marks.mark(1));
            RTMI_HIP(marks.wait(1));
            double ms = 0.0;
            RTMI_HIP(marks.ms(0, 1, &ms));
            total.kernel_ms += ms;
            RTMI_HIP(hipMemcpy(out.data(), d_out, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            unsigned long long strays = 0;
            for (size_t s = 0; s < (size_t)S; s++) strays += out[s * kOutWords + 3];
            if (strays == 0) break;
        }
        for (size_t s = 0; s < (size_t)S; s++) {
            const unsigned long long* o = &out[s * kOutWords];
            const int32_t r = (int32_t)(o[0] & 0xffffffffull), clean = (int32_t)(o[0] >> 32);
            if (rounds) {
                rounds[2 * s] = r;
                rounds[2 * s + 1] = clean;
            }
            total.free_nodes += (int64_t)o[1];
            total.changes += (int64_t)o[2];
            total.rounds_max = std::max(total.rounds_max, r);
        }
        total.filled = total.free_nodes;
    }
    if (stats) *stats = total;
    return RTMI_OK;
}

// the pointers both forms need with S > 0, after check_eikonal
int check_attr(const char* who, const void* T, const void* filled, const void* theta0) {
    RTMI_ARG(T, "null T");
    RTMI_ARG(filled, "null filled");
    RTMI_ARG(theta0, "null theta0");
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_attributes_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                            const double* d_n_src, const double* d_T, const uint8_t* d_filled, double* d_theta0,
                                            double* d_dir, double* d_J, double* d_G, int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_attributes_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    AttrArgs a{};
    std::vector<double> src;
    if (S > 0) {
        RTMI_RC(check_attr(who, d_T, d_filled, d_theta0));
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn * sizeof(double);
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        RTMI_RC(check_device_pointer(device, who, d_T, tab, "d_T"));
        RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
        RTMI_RC(check_device_pointer(device, who, d_theta0, tab, "d_theta0"));
        if (d_dir) RTMI_RC(check_device_pointer(device, who, d_dir, 2 * tab, "d_dir"));
        if (d_J) RTMI_RC(check_device_pointer(device, who, d_J, tab, "d_J"));
        if (d_G) RTMI_RC(check_device_pointer(device, who, d_G, tab, "d_G"));
        // the sources come back for the ball's table of atan2: 16 bytes each
        src.resize((size_t)S * 2);
        RTMI_HIP(hipMemcpy(src.data(), d_src, src.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.theta0 = d_theta0; a.dir = d_dir; a.J = d_J; a.G = d_G;
    return attr_dev(who, ep, S, src.data(), a, rounds, stats);
}

RTMI_EXPORT int rtmi_eikonal_attributes(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src, const double* n_src,
                                        const double* T, const uint8_t* filled, double* theta0, double* dir, double* J, double* G,
                                        int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_attributes";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    AttrArgs a{};
    if (S == 0) return attr_dev(who, ep, 0, nullptr, a, rounds, stats);
    RTMI_RC(check_attr(who, T, filled, theta0));
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    double *d_n = nullptr, *d_src = nullptr, *d_n_src = nullptr, *d_T = nullptr;
    uint8_t* d_filled = nullptr;
    RTMI_ALLOC(mem.get(&d_n, nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_src, (size_t)S * 2 * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_n_src, (size_t)S * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_T, tab * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_filled, tab));
    RTMI_HIP(hipMemcpy(d_n, n, nn * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_src, src, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_n_src, n_src, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_T, T, tab * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d_filled, filled, tab, hipMemcpyHostToDevice));
    // every output is in and out: dead nodes and seeds keep their bits
    struct InOut {
        double* host;
        double** dev;
        size_t count;
    };
    double *d_theta0 = nullptr, *d_dir = nullptr, *d_J = nullptr, *d_G = nullptr;
    const InOut io[4] = {{theta0, &d_theta0, tab}, {dir, &d_dir, 2 * tab}, {J, &d_J, tab}, {G, &d_G, tab}};
    for (const InOut& v : io)
        if (v.host) {
            RTMI_ALLOC(mem.get(v.dev, v.count * sizeof(double)));
            RTMI_HIP(hipMemcpy(*v.dev, v.host, v.count * sizeof(double), hipMemcpyHostToDevice));
        }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.theta0 = d_theta0; a.dir = d_dir; a.J = d_J; a.G = d_G;
    RTMI_RC(attr_dev(who, ep, S, src, a, rounds, stats));
    for (const InOut& v : io)
        if (v.host) RTMI_HIP(hipMemcpy(v.host, *v.dev, v.count * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}
