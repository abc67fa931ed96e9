// eikonal_lin.hip -- the eikonal fill linearised about its result: the tangent dT = J dn and the adjoint g = J^T r of the
// converged Godunov scheme, as sweeps over the causal network of parents that the table defines (rtmi_eikonal_tangent,
// rtmi_eikonal_adjoint and their _dev forms; include/rtmi.h).  The arithmetic of a node is
// rt_eikonal_lin.h's; the kernel only decides who runs it when.
//   k_eikonal_lin<LDS, ADJ>  one workgroup per source, the round loop inside.  A setup pass turns T, n and filled into each
//                   node's ca, cb and code once; then the sweeps walk the anti-diagonals as k_eikonal does: a node's gather
//                   reads the diagonals d - 1 and d + 1 only, so the lanes take one diagonal side by side and a block barrier
//                   parts two diagonals: the serial sweep's bits.  The adjoint also turns the codes into each node's mask of the
//                   neighbours that name it as a parent, so that its gather reads no neighbour's code.  LDS: the values, ca, cb,
//                   the codes and the masks (26 bytes per node) live in the block's LDS; otherwise the values live in the output
//                   table and the rest in a work space in global memory.  A node's constant term is read by that node alone and
//                   stays in global memory on both paths: r itself (adjoint) or cs dn in a work space (tangent).
// Every loop bound and every barrier is uniform across the block and max_rounds bounds the whole; no block waits for another.
// No atomics on floating point; g_src is summed by one lane in node order.
// FACT (ep->scheme == RTMI_EIKONAL_FACTORED_LIN) is the factored update linearised: only the setup differs.  A
// free node's coefficients come from the corrected readings, T0 and rr recomputed in registers as k_eikonal<..., FACTORED> does; csrc
// goes into the tangent's constant term, and the adjoint recomputes it from ca, cb and the code in the g_src pass, which the lanes
// take a row each before one lane adds the ny row sums from a small work space.  The sweeps are the same code.
#include "rtmi_host.h"

#include "rt_eikonal_lin.h"
#include "rt_eikonal_host.h"

namespace {

constexpr size_t kLdsBudget = (size_t)128 << 10;        // the LDS path's share of a CU's 160 KiB
constexpr size_t kLdsPerNode = 3 * sizeof(double) + 2;  // value, ca, cb, the code and the adjoint's mask
constexpr size_t kWorkBudget = (size_t)1 << 30;         // the work space of one group of sources
constexpr int kOutWords = 3;                            // per source: rounds | clean << 32, free and ball nodes, changes

struct LinArgs {
    rt::EikGrid g;
    long nx, ny;
    double ball;
    int max_rounds;
    const double* n;            // [ny][nx]
    const double* src;          // [S][2]
    const double* n_src;        // [S]
    const double* T;            // [S][ny][nx]
    const uint8_t* filled;      // [S][ny][nx]
    const double* dn;           // tangent: [ny][nx]
    const double* dn_src;       // tangent: [S] or NULL
    const double* seed;         // tangent: [S][ny][nx] or NULL
    const double* r;            // adjoint: [S][ny][nx]
    double* v;                  // [S][ny][nx]: dT or lam
    double* gout;               // adjoint: [S][ny][nx] or NULL
    double* g_src;              // adjoint: [S] or NULL
    double *ca, *cb;            // global path: [S][ny][nx]
    uint8_t *code, *kids;       // global path: [S][ny][nx]; kids: adjoint
    union {                     // one slot, so that the argument block keeps its size
        double* k;              // tangent: [S][ny][nx]
        double* gpart;          // adjoint, FACT: [S][ny], the rows' shares of g_src
    };
    unsigned long long* out;    // [S][kOutWords]
};

template <bool LDS, bool ADJ, bool FACT> __global__ void __launch_bounds__(kMaxBlock) k_eikonal_lin(const LinArgs a) {
    extern __shared__ double lds[];                     // LDS: [v | ca | cb | code | kids]
    __shared__ unsigned long long red[2][kMaxBlock / 64];
    const int tid = (int)threadIdx.x, bd = (int)blockDim.x;
    const long nx = a.nx, ny = a.ny, nn = nx * ny;
    const size_t s = blockIdx.x;
    const double xs = a.src[2 * s], ys = a.src[2 * s + 1], n_src = a.n_src[s];
    const double* Ts = a.T + s * (size_t)nn;
    const uint8_t* fs = a.filled + s * (size_t)nn;
    double* vg = a.v + s * (size_t)nn;
    double *v, *ca, *cb;
    uint8_t *code, *kids;
    if constexpr (LDS) {
        v = lds;
        ca = lds + nn;
        cb = lds + 2 * nn;
        code = (uint8_t*)(lds + 3 * nn);
        kids = code + nn;
    } else {
        v = vg;
        ca = a.ca + s * (size_t)nn;
        cb = a.cb + s * (size_t)nn;
        code = a.code + s * (size_t)nn;
        kids = ADJ ? a.kids + s * (size_t)nn : nullptr;
    }
    // a node's constant term: r (adjoint), cs dn (tangent)
    const double* kr;
    if constexpr (ADJ) kr = a.r + s * (size_t)nn;
    else kr = a.k + s * (size_t)nn;
    long bi0 = 0, bi1 = -1, bj0 = 0, bj1 = -1;
    if constexpr (ADJ) rt::eik_lin_ball_box(a.g, nx, ny, xs, ys, a.ball, &bi0, &bi1, &bj0, &bj1);
    // the classes, the coefficients and the starting values
    unsigned long long nfree = 0, nnodes = 0, nstray = 0;
    for (long x = tid; x < nn; x += bd) {
        const long i = x % nx, j = x / nx;
        const rt::EikLinNode c = rt::eik_lin_node_of<FACT>(a.g, nx, ny, i, j, a.n, Ts, fs, xs, ys, n_src, a.ball);
        const uint8_t cls = rt::eik_lin_class(c.code);
        ca[x] = c.ca;
        cb[x] = c.cb;
        code[x] = c.code;
        if constexpr (ADJ) {
            v[x] = cls == rt::kLinDead ? 0.0 : kr[x];
            if (cls == rt::kLinBall && !(i >= bi0 && i <= bi1 && j >= bj0 && j <= bj1)) nstray++;
        } else {
            double k;
            if constexpr (FACT)
                v[x] = rt::eik_flin_tangent_init(c, a.dn[x], a.dn_src ? a.dn_src[s] : 0.0, a.seed ? a.seed[s * (size_t)nn + x] : 0.0, &k);
            else
                v[x] = rt::eik_lin_tangent_init(c, a.dn[x], a.dn_src ? a.dn_src[s] : 0.0, a.seed ? a.seed[s * (size_t)nn + x] : 0.0, &k);
            a.k[s * (size_t)nn + x] = k;
        }
        if (cls >= rt::kLinFree) nnodes++;
        if (cls == rt::kLinFree) nfree++;
    }
    nnodes = block_sum(red, 0, nnodes);
    nstray = block_sum(red, 1, nstray);     // its barrier also parts the codes from the reads of the masks' pass
    if constexpr (ADJ)
        for (long x = tid; x < nn; x += bd) kids[x] = rt::eik_lin_kids(nx, ny, x % nx, x / nx, code);
    nfree = block_sum(red, 0, nfree);       // its barrier also parts the starting values from the first diagonal's reads
    int rounds = 0, clean = 1;
    unsigned long long changes = 0;
    if (nfree > 0) {
        const long ndiag = nx + ny - 1;
        while (rounds < a.max_rounds) {
            rounds++;
            unsigned long long mine = 0;
            for (int k = 0; k < 4; k++) {
                const bool xup = rt::eik_lin_xup(ADJ, k), yup = rt::eik_lin_yup(ADJ, k);
                for (long d = 0; d < ndiag; d++) {
                    // the diagonal p + q = d in the sweep's own coordinates: q in [q0, q1]
                    const long q0 = d - (nx - 1) > 0 ? d - (nx - 1) : 0, q1 = d < ny - 1 ? d : ny - 1;
                    for (long q = q0 + tid; q <= q1; q += bd) {
                        const long p = d - q, i = xup ? p : nx - 1 - p, j = yup ? q : ny - 1 - q, x = j * nx + i;
                        const uint8_t c = code[x];
                        double t;
                        if constexpr (ADJ) {
                            if (rt::eik_lin_class(c) == rt::kLinDead) continue;
                            t = rt::eik_lin_adjoint_gather(nx, x, kids[x], kr[x], ca, cb, v);
                        } else {
                            if (rt::eik_lin_class(c) != rt::kLinFree) continue;
                            t = rt::eik_lin_tangent_gather(nx, x, c, ca[x], cb[x], kr[x], v);
                        }
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
    // the values out, and what the adjoint derives from them
    for (long x = tid; x < nn; x += bd) {
        const double val = v[x];
        if constexpr (LDS) vg[x] = val;
        if constexpr (ADJ) {
            if (a.gout) {
                double gv = 0.0;
                if (rt::eik_lin_class(code[x]) >= rt::kLinFree)
                    gv = rt::eik_lin_node_of<FACT>(a.g, nx, ny, x % nx, x / nx, a.n, Ts, fs, xs, ys, n_src, a.ball).cs * val;
                a.gout[s * (size_t)nn + x] = gv;
            }
        }
    }
    if constexpr (ADJ && FACT) {
        if (a.g_src) {                       // uniform across the block
            // a lane per row, then one lane over the ny row sums in ascending j
            double* part = a.gpart + s * (size_t)ny;
            for (long j = tid; j < ny; j += bd) rt::eik_flin_g_src_row<1>(a.g, nx, j, xs, ys, n_src, code, ca, cb, v, &part[j]);
            __syncthreads();
            if (tid == 0) {
                double acc = 0.0;
                for (long j = 0; j < ny; j++) acc = acc + part[j];
                a.g_src[s] = acc;
            }
        }
    } else if constexpr (ADJ) {
        if (a.g_src && tid == 0) {
            // nstray is 0 unless the box missed a node of the ball: then every node is looked at
            const long i0 = nstray ? 0 : bi0, i1 = nstray ? nx - 1 : bi1, j0 = nstray ? 0 : bj0, j1 = nstray ? ny - 1 : bj1;
            double acc = 0.0;
            for (long j = j0; j <= j1; j++)
                for (long i = i0; i <= i1; i++)
                    if (rt::eik_lin_class(code[j * nx + i]) == rt::kLinBall) acc = acc + rt::eik_lin_csrc(a.g, i, j, xs, ys) * v[j * nx + i];
            a.g_src[s] = acc;
        }
    }
    if (tid == 0) {
        unsigned long long* o = a.out + s * kOutWords;
        o[0] = (unsigned long long)(unsigned)rounds | (unsigned long long)(unsigned)clean << 32;
        o[1] = nnodes;
        o[2] = changes;
    }
}

// One call on device memory: a holds the caller's pointers for all S sources
template <bool ADJ> int lin_dev(const char* who, const rtmi_eikonal_params* ep, int64_t S, LinArgs a, int32_t* rounds,
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
        // the work space per node and source: ca, cb, the code and the adjoint's mask off the LDS path, and the tangent's constant term
        const size_t per = (lds ? 0 : 2 * sizeof(double) + 1) + (ADJ ? (lds ? 0 : 1) : sizeof(double));
        const size_t group = per ? std::min((size_t)S, std::max<size_t>(1, kWorkBudget / (nn * per))) : (size_t)S;
        DevMem mem;
        a.g = rt::eik_grid(ep->gx0, ep->gdx, ep->gy0, ep->gdy);
        a.nx = (long)ep->nx;
        a.ny = (long)ep->ny;
        a.ball = ep->ball;
        a.max_rounds = ep->max_rounds > 0 ? ep->max_rounds : rt::kEikDefaultRounds;
        if (!lds) {
            RTMI_ALLOC(mem.get(&a.ca, group * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.cb, group * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.code, group * nn));
            if (ADJ) RTMI_ALLOC(mem.get(&a.kids, group * nn));
        }
        if (!ADJ) RTMI_ALLOC(mem.get(&a.k, group * nn * sizeof(double)));
        const bool fact = ep->scheme == RTMI_EIKONAL_FACTORED_LIN;
        if (ADJ && fact && a.g_src) RTMI_ALLOC(mem.get(&a.gpart, group * (size_t)ep->ny * sizeof(double)));
        unsigned long long* d_out = nullptr;
        RTMI_ALLOC(mem.get(&d_out, (size_t)S * kOutWords * sizeof(unsigned long long)));
        auto* const kernel = lds ? (fact ? k_eikonal_lin<true, ADJ, true> : k_eikonal_lin<true, ADJ, false>)
                                 : (fact ? k_eikonal_lin<false, ADJ, true> : k_eikonal_lin<false, ADJ, false>);
        if (lds && lds_bytes > 65536)
            RTMI_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        const LinArgs all = a;
        EventMarks<2> marks;
        RTMI_HIP(marks.create());
        RTMI_HIP(marks.mark(0));
        for (size_t s0 = 0; s0 < (size_t)S; s0 += group) {
            const size_t gs = std::min(group, (size_t)S - s0);
            a.src = all.src + 2 * s0;
            a.n_src = all.n_src + s0;
            a.T = all.T + s0 * nn;
            a.filled = all.filled + s0 * nn;
            a.dn_src = all.dn_src ? all.dn_src + s0 : nullptr;
            a.seed = all.seed ? all.seed + s0 * nn : nullptr;
            a.r = all.r ? all.r + s0 * nn : nullptr;
            a.v = all.v + s0 * nn;
            a.gout = all.gout ? all.gout + s0 * nn : nullptr;
            a.g_src = all.g_src ? all.g_src + s0 : nullptr;
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
            total.changes += (int64_t)o[2];
            total.rounds_max = std::max(total.rounds_max, r);
        }
        total.filled = total.free_nodes;
    }
    if (stats) *stats = total;
    return RTMI_OK;
}

// the pointers every form needs with S > 0, after check_eikonal
int check_lin(const char* who, const void* T, const void* filled, const void* in, const char* in_name, const void* out, const char* out_name) {
    RTMI_ARG(T, "null T");
    RTMI_ARG(filled, "null filled");
    RTMI_ARG(in, std::string("null ") + in_name);
    RTMI_ARG(out, std::string("null ") + out_name);
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_tangent_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                         const double* d_n_src, const double* d_T, const uint8_t* d_filled, const double* d_dn,
                                         const double* d_dn_src, const double* d_dT_seed, double* d_dT, int32_t* rounds,
                                         rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_tangent_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    LinArgs a{};
    if (S > 0) {
        RTMI_RC(check_lin(who, d_T, d_filled, d_dn, "dn", d_dT, "dT"));
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn * sizeof(double);
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        RTMI_RC(check_device_pointer(device, who, d_T, tab, "d_T"));
        RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
        RTMI_RC(check_device_pointer(device, who, d_dn, nn * sizeof(double), "d_dn"));
        if (d_dn_src) RTMI_RC(check_device_pointer(device, who, d_dn_src, (size_t)S * sizeof(double), "d_dn_src"));
        if (d_dT_seed) RTMI_RC(check_device_pointer(device, who, d_dT_seed, tab, "d_dT_seed"));
        RTMI_RC(check_device_pointer(device, who, d_dT, tab, "d_dT"));
    }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.dn = d_dn; a.dn_src = d_dn_src; a.seed = d_dT_seed; a.v = d_dT;
    return lin_dev<false>(who, ep, S, a, rounds, stats);
}

RTMI_EXPORT int rtmi_eikonal_adjoint_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                         const double* d_n_src, const double* d_T, const uint8_t* d_filled, const double* d_r,
                                         double* d_lam, double* d_g, double* d_g_src, int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_adjoint_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    LinArgs a{};
    if (S > 0) {
        RTMI_RC(check_lin(who, d_T, d_filled, d_r, "r", d_lam, "lam"));
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn * sizeof(double);
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        RTMI_RC(check_device_pointer(device, who, d_T, tab, "d_T"));
        RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
        RTMI_RC(check_device_pointer(device, who, d_r, tab, "d_r"));
        RTMI_RC(check_device_pointer(device, who, d_lam, tab, "d_lam"));
        if (d_g) RTMI_RC(check_device_pointer(device, who, d_g, tab, "d_g"));
        if (d_g_src) RTMI_RC(check_device_pointer(device, who, d_g_src, (size_t)S * sizeof(double), "d_g_src"));
    }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.r = d_r; a.v = d_lam; a.gout = d_g; a.g_src = d_g_src;
    return lin_dev<true>(who, ep, S, a, rounds, stats);
}

namespace {

// the inputs both host forms upload
struct LinUpload {
    double *n = nullptr, *src = nullptr, *n_src = nullptr, *T = nullptr;
    uint8_t* filled = nullptr;
};

int upload_lin(const char* who, DevMem& mem, const rtmi_eikonal_params* ep, int64_t S, const double* n, const double* src,
               const double* n_src, const double* T, const uint8_t* filled, LinUpload* u) {
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    RTMI_ALLOC(mem.get(&u->n, nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&u->src, (size_t)S * 2 * sizeof(double)));
    RTMI_ALLOC(mem.get(&u->n_src, (size_t)S * sizeof(double)));
    RTMI_ALLOC(mem.get(&u->T, tab * sizeof(double)));
    RTMI_ALLOC(mem.get(&u->filled, tab));
    RTMI_HIP(hipMemcpy(u->n, n, nn * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(u->src, src, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(u->n_src, n_src, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(u->T, T, tab * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(u->filled, filled, tab, hipMemcpyHostToDevice));
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_tangent(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src, const double* n_src,
                                     const double* T, const uint8_t* filled, const double* dn, const double* dn_src,
                                     const double* dT_seed, double* dT, int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_tangent";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    LinArgs a{};
    if (S == 0) return lin_dev<false>(who, ep, 0, a, rounds, stats);
    RTMI_RC(check_lin(who, T, filled, dn, "dn", dT, "dT"));
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    LinUpload u;
    RTMI_RC(upload_lin(who, mem, ep, S, n, src, n_src, T, filled, &u));
    double *d_dn = nullptr, *d_dn_src = nullptr, *d_seed = nullptr, *d_dT = nullptr;
    RTMI_ALLOC(mem.get(&d_dn, nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_dT, tab * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_dn, dn, nn * sizeof(double), hipMemcpyHostToDevice));
    if (dn_src) {
        RTMI_ALLOC(mem.get(&d_dn_src, (size_t)S * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_dn_src, dn_src, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    }
    if (dT_seed) {
        RTMI_ALLOC(mem.get(&d_seed, tab * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_seed, dT_seed, tab * sizeof(double), hipMemcpyHostToDevice));
    }
    a.n = u.n; a.src = u.src; a.n_src = u.n_src; a.T = u.T; a.filled = u.filled;
    a.dn = d_dn; a.dn_src = d_dn_src; a.seed = d_seed; a.v = d_dT;
    RTMI_RC(lin_dev<false>(who, ep, S, a, rounds, stats));
    RTMI_HIP(hipMemcpy(dT, d_dT, tab * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_adjoint(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src, const double* n_src,
                                     const double* T, const uint8_t* filled, const double* r, double* lam, double* g, double* g_src,
                                     int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_adjoint";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    LinArgs a{};
    if (S == 0) return lin_dev<true>(who, ep, 0, a, rounds, stats);
    RTMI_RC(check_lin(who, T, filled, r, "r", lam, "lam"));
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    LinUpload u;
    RTMI_RC(upload_lin(who, mem, ep, S, n, src, n_src, T, filled, &u));
    double *d_r = nullptr, *d_lam = nullptr, *d_g = nullptr, *d_g_src = nullptr;
    RTMI_ALLOC(mem.get(&d_r, tab * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_lam, tab * sizeof(double)));
    if (g) RTMI_ALLOC(mem.get(&d_g, tab * sizeof(double)));
    if (g_src) RTMI_ALLOC(mem.get(&d_g_src, (size_t)S * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_r, r, tab * sizeof(double), hipMemcpyHostToDevice));
    a.n = u.n; a.src = u.src; a.n_src = u.n_src; a.T = u.T; a.filled = u.filled;
    a.r = d_r; a.v = d_lam; a.gout = d_g; a.g_src = d_g_src;
    RTMI_RC(lin_dev<true>(who, ep, S, a, rounds, stats));
    RTMI_HIP(hipMemcpy(lam, d_lam, tab * sizeof(double), hipMemcpyDeviceToHost));
    if (g) RTMI_HIP(hipMemcpy(g, d_g, tab * sizeof(double), hipMemcpyDeviceToHost));
    if (g_src) RTMI_HIP(hipMemcpy(g_src, d_g_src, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// Several right-hand sides per source in one call (rtmi_eikonal_tangent_multi, rtmi_eikonal_adjoint_multi and their _dev forms;
// DESIGN.md section 37).  Column c of every output has the bits the single entry gives on column c alone: columns never read one
// another, a column's sweep is the fixed sweep above, and a round after a column's first clean round reproduces every value bit
// for bit, so a chunk sweeps until its last column is clean and each column reports its own first clean round.
//   k_eikonal_lin_setup, _kids   global path: ca, cb, the codes and the adjoint's masks of a group of sources, one lane per
//                   (source, node), once per source: 18 bytes per node and source that the chunks of the source share
//   k_eikonal_lin_multi<LDS, ADJ, C>  one workgroup per (source, chunk of C columns), the chunk in blockIdx.y.  The working
//                   values and the constant terms of a chunk are column-minor, [node][C], so a node's C values are one access of
//                   8 C bytes and the node's code, mask, ca and cb are read once for the C columns.  LDS: the values and the
//                   source's coefficients (8 C + 18 bytes per node) in the block's LDS, computed by the block itself; else the
//                   values in a work space.  The constant terms are in a work space on both paths.  A partial chunk's missing
//                   columns are columns of zeros that no one reads or writes out.  The read-out pass writes the public planes.
// Every loop bound and every barrier is uniform across the block, max_rounds bounds the whole, no block reads what another block of
// the same launch writes, and there are no atomics.
namespace {

constexpr int kMultiWidths[] = {1, 4, 8};                // the compiled chunk widths

struct LinMultiArgs {
    rt::EikGrid g;
    long nx, ny;
    double ball;
    int max_rounds;
    int K;                      // columns of the call
    int c0;                     // the first column of this launch
    size_t S, s0;               // sources of the call (the planes' stride); the first source of this launch
    const double* n;            // [ny][nx]
    const double* src;          // [S][2]
    const double* n_src;        // [S]
    const double* T;            // [S][ny][nx]
    const uint8_t* filled;      // [S][ny][nx]
    union {                     // one slot, so that the argument block keeps its size
        const double* dn;       // tangent: [K][ny][nx]
        double* gpart;          // adjoint, FACT: [chunks][gs][ny][C], the rows' shares of g_src
    };
    const double* dn_src;       // tangent: [K][S] or NULL
    const double* seed;         // tangent: [K][S][ny][nx] or NULL
    const double* r;            // adjoint: [K][S][ny][nx]
    double* v;                  // [K][S][ny][nx]: dT or lam
    double* gout;               // adjoint: [K][S][ny][nx] or NULL
    double* g_src;              // adjoint: [K][S] or NULL
    double *ca, *cb;            // global path: [gs][ny][nx], the launch's sources
    uint8_t *code, *kids;       // global path: [gs][ny][nx]; kids: adjoint
    double* wv;                 // global path: [chunks][gs][ny nx][C], the working values
    double* wk;                 // [chunks][gs][ny nx][C], the constant terms
    unsigned long long* out;    // [K][S][kOutWords]
};

template <bool FACT> __global__ void __launch_bounds__(256) k_eikonal_lin_setup(const LinMultiArgs a, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long nn = a.nx * a.ny, x = t % nn;
    const size_t s = a.s0 + (size_t)(t / nn);
    const rt::EikLinNode c = rt::eik_lin_node_of<FACT>(a.g, a.nx, a.ny, x % a.nx, x / a.nx, a.n, a.T + s * (size_t)nn,
                                                       a.filled + s * (size_t)nn, a.src[2 * s], a.src[2 * s + 1], a.n_src[s], a.ball);
    a.ca[t] = c.ca;
    a.cb[t] = c.cb;
    a.code[t] = c.code;
}

__global__ void __launch_bounds__(256) k_eikonal_lin_kids(const LinMultiArgs a, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long nn = a.nx * a.ny, x = t % nn;
    a.kids[t] = rt::eik_lin_kids(a.nx, a.ny, x % a.nx, x / a.nx, a.code + (t - x));
}

// the block's sums of C values, the same in every lane
template <int C> __device__ __forceinline__ void block_sum_cols(unsigned long long (*red)[kMaxBlock / 64][C], int slot,
                                                               unsigned long long* v) {
    const int tid = (int)threadIdx.x, waves = (int)(blockDim.x >> 6);
#pragma unroll
    for (int c = 0; c < C; c++) {
        for (int off = 1; off < 64; off <<= 1) v[c] += (unsigned long long)__shfl_xor((long long)v[c], off);
        if ((tid & 63) == 0) red[slot][tid >> 6][c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; c++) {
        unsigned long long s = 0;
        for (int k = 0; k < waves; k++) s += red[slot][k][c];
        v[c] = s;
    }
}

template <bool LDS, bool ADJ, int C, bool FACT> __global__ void __launch_bounds__(kMaxBlock) k_eikonal_lin_multi(const LinMultiArgs a) {
    extern __shared__ double lds[];                     // LDS: [v [nn][C] | ca | cb | code | kids]
    __shared__ unsigned long long red[2][kMaxBlock / 64];
    __shared__ unsigned long long redc[2][kMaxBlock / 64][C];
    const int tid = (int)threadIdx.x, bd = (int)blockDim.x;
    const long nx = a.nx, ny = a.ny, nn = nx * ny;
    const size_t sl = blockIdx.x, s = a.s0 + sl, S = a.S;
    const int col0 = a.c0 + (int)blockIdx.y * C;
    const int ncol = a.K - col0 < C ? a.K - col0 : C;
    const size_t slot = (size_t)blockIdx.y * gridDim.x + sl;
    const double xs = a.src[2 * s], ys = a.src[2 * s + 1], n_src = a.n_src[s];
    const double* Ts = a.T + s * (size_t)nn;
    const uint8_t* fs = a.filled + s * (size_t)nn;
    double *v, *ca, *cb;
    uint8_t *code, *kids;
    if constexpr (LDS) {
        v = lds;
        ca = lds + (size_t)C * nn;
        cb = ca + nn;
        code = (uint8_t*)(cb + nn);
        kids = code + nn;
    } else {
        v = a.wv + slot * (size_t)nn * C;
        ca = a.ca + sl * (size_t)nn;
        cb = a.cb + sl * (size_t)nn;
        code = a.code + sl * (size_t)nn;
        kids = ADJ ? a.kids + sl * (size_t)nn : nullptr;
    }
    double* kr = a.wk + slot * (size_t)nn * C;          // a node's constant terms: r (adjoint), cs dn (tangent)
    long bi0 = 0, bi1 = -1, bj0 = 0, bj1 = -1;
    if constexpr (ADJ) rt::eik_lin_ball_box(a.g, nx, ny, xs, ys, a.ball, &bi0, &bi1, &bj0, &bj1);
    // the classes, the coefficients where the block keeps its own, and every column's starting values and constant terms
    unsigned long long nfree = 0, nnodes = 0, nstray = 0;
    for (long x = tid; x < nn; x += bd) {
        const long i = x % nx, j = x / nx;
        rt::EikLinNode c{0.0, 0.0, 0.0, 0.0, 0};
        if constexpr (LDS || !ADJ) {
            c = rt::eik_lin_node_of<FACT>(a.g, nx, ny, i, j, a.n, Ts, fs, xs, ys, n_src, a.ball);
            if constexpr (LDS) {
                ca[x] = c.ca;
                cb[x] = c.cb;
                code[x] = c.code;
            }
        } else {
            c.code = code[x];
        }
        const uint8_t cls = rt::eik_lin_class(c.code);
        double val[C], k[C];
#pragma unroll
        for (int q = 0; q < C; q++) {
            val[q] = 0.0;
            k[q] = 0.0;
            if (q < ncol) {
                const size_t col = (size_t)(col0 + q), plane = (col * S + s) * (size_t)nn;
                if constexpr (ADJ) {
                    k[q] = a.r[plane + x];
                    val[q] = cls == rt::kLinDead ? 0.0 : k[q];
                } else {
                    if constexpr (FACT)
                        val[q] = rt::eik_flin_tangent_init(c, a.dn[col * (size_t)nn + x], a.dn_src ? a.dn_src[col * S + s] : 0.0,
                                                           a.seed ? a.seed[plane + x] : 0.0, &k[q]);
                    else
                        val[q] = rt::eik_lin_tangent_init(c, a.dn[col * (size_t)nn + x], a.dn_src ? a.dn_src[col * S + s] : 0.0,
                                                          a.seed ? a.seed[plane + x] : 0.0, &k[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < C; q++) {
            v[x * C + q] = val[q];
            kr[x * C + q] = k[q];
        }
        if constexpr (ADJ)
            if (cls == rt::kLinBall && !(i >= bi0 && i <= bi1 && j >= bj0 && j <= bj1)) nstray++;
        if (cls >= rt::kLinFree) nnodes++;
        if (cls == rt::kLinFree) nfree++;
    }
    nnodes = block_sum(red, 0, nnodes);
    nstray = block_sum(red, 1, nstray);     // its barrier also parts the codes from the reads of the masks' pass
    if constexpr (ADJ && LDS)
        for (long x = tid; x < nn; x += bd) kids[x] = rt::eik_lin_kids(nx, ny, x % nx, x / nx, code);
    nfree = block_sum(red, 0, nfree);       // its barrier also parts the starting values from the first diagonal's reads
    // per column: the first round that changed nothing, or max_rounds and not clean.  All of it is uniform across the block
    int rounds[C], clean[C];
    unsigned long long changes[C];
    bool done[C];
#pragma unroll
    for (int q = 0; q < C; q++) {
        rounds[q] = 0;
        clean[q] = 1;
        changes[q] = 0;
        done[q] = q >= ncol;
    }
    if (nfree > 0) {
        const long ndiag = nx + ny - 1;
        int round = 0;
        bool all = false;
        while (!all && round < a.max_rounds) {
            round++;
            unsigned long long mine[C];
#pragma unroll
            for (int q = 0; q < C; q++) mine[q] = 0;
            for (int k = 0; k < 4; k++) {
                const bool xup = rt::eik_lin_xup(ADJ, k), yup = rt::eik_lin_yup(ADJ, k);
                for (long d = 0; d < ndiag; d++) {
                    // the diagonal p + q = d in the sweep's own coordinates: q in [q0, q1]
                    const long q0 = d - (nx - 1) > 0 ? d - (nx - 1) : 0, q1 = d < ny - 1 ? d : ny - 1;
                    for (long q = q0 + tid; q <= q1; q += bd) {
                        const long p = d - q, i = xup ? p : nx - 1 - p, j = yup ? q : ny - 1 - q, x = j * nx + i;
                        const uint8_t c = code[x];
                        double t[C];
                        if constexpr (ADJ) {
                            if (rt::eik_lin_class(c) == rt::kLinDead) continue;
                            rt::eik_lin_adjoint_gather_cols<C>(nx, x, kids[x], kr, ca, cb, v, t);
                        } else {
                            if (rt::eik_lin_class(c) != rt::kLinFree) continue;
                            rt::eik_lin_tangent_gather_cols<C>(nx, x, c, ca[x], cb[x], kr, v, t);
                        }
#pragma unroll
                        for (int w = 0; w < C; w++)
                            if (rt::eik_bits(t[w]) != rt::eik_bits(v[x * C + w])) {
                                v[x * C + w] = t[w];
                                mine[w]++;
                            }
                    }
                    __syncthreads();
                }
            }
            block_sum_cols<C>(redc, round & 1, mine);
            all = true;
#pragma unroll
            for (int q = 0; q < C; q++) {
                if (!done[q]) {
                    changes[q] += mine[q];
                    rounds[q] = round;
                    clean[q] = mine[q] == 0;
                    done[q] = mine[q] == 0;
                }
                all = all && done[q];
            }
        }
    }
    // the values out to the public planes, and what the adjoint derives from them
    for (long x = tid; x < nn; x += bd) {
        double cs = 0.0;
        bool live = false;
        if constexpr (ADJ) {
            if (a.gout && rt::eik_lin_class(code[x]) >= rt::kLinFree) {
                live = true;
                cs = rt::eik_lin_node_of<FACT>(a.g, nx, ny, x % nx, x / nx, a.n, Ts, fs, xs, ys, n_src, a.ball).cs;
            }
        }
#pragma unroll
        for (int q = 0; q < C; q++) {
            if (q < ncol) {
                const size_t plane = ((size_t)(col0 + q) * S + s) * (size_t)nn;
                const double val = v[x * C + q];
                a.v[plane + x] = val;
                if constexpr (ADJ) {
                    if (a.gout) {
                        double gv = 0.0;
                        if (live) gv = cs * val;
                        a.gout[plane + x] = gv;
                    }
                }
            }
        }
    }
    if constexpr (ADJ && FACT) {
        if (a.g_src) {                       // uniform across the block
            // a lane per row for the chunk's columns, then one lane per column over the ny row sums in ascending j
            double* part = a.gpart + slot * (size_t)ny * C;
            for (long j = tid; j < ny; j += bd) {
                double row[C];
                rt::eik_flin_g_src_row<C>(a.g, nx, j, xs, ys, n_src, code, ca, cb, v, row);
#pragma unroll
                for (int q = 0; q < C; q++) part[j * C + q] = row[q];
            }
            __syncthreads();
            if (tid < ncol) {
                double acc = 0.0;
                for (long j = 0; j < ny; j++) acc = acc + part[j * C + tid];
                a.g_src[(size_t)(col0 + tid) * S + s] = acc;
            }
        }
    } else if constexpr (ADJ) {
        if (a.g_src && tid < ncol) {
            // one lane per column, in node order.  nstray is 0 unless the box missed a node of the ball: then every node is looked at
            const long i0 = nstray ? 0 : bi0, i1 = nstray ? nx - 1 : bi1, j0 = nstray ? 0 : bj0, j1 = nstray ? ny - 1 : bj1;
            double acc = 0.0;
            for (long j = j0; j <= j1; j++)
                for (long i = i0; i <= i1; i++)
                    if (rt::eik_lin_class(code[j * nx + i]) == rt::kLinBall)
                        acc = acc + rt::eik_lin_csrc(a.g, i, j, xs, ys) * v[(j * nx + i) * C + tid];
            a.g_src[(size_t)(col0 + tid) * S + s] = acc;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < C; q++) {
            if (q < ncol) {
                unsigned long long* o = a.out + ((size_t)(col0 + q) * S + s) * kOutWords;
                o[0] = (unsigned long long)(unsigned)rounds[q] | (unsigned long long)(unsigned)clean[q] << 32;
                o[1] = nnodes;
                o[2] = changes[q];
            }
        }
    }
}

// How a call at chunk width C goes out: its path, and the sources (gs) and chunks (gc) of one launch, which keep the work space under
// the budget: per source ca, cb, the code and the mask off the LDS path; per workgroup the constant terms, and the values off it
struct MultiPlan {
    int C;
    bool lds;
    size_t lds_bytes, chunks, gs, gc;
};

MultiPlan multi_plan(int C, int K, size_t S, size_t nn, bool force_global) {
    MultiPlan p{};
    p.C = C;
    p.lds_bytes = (nn * ((size_t)C * sizeof(double) + kLdsPerNode - sizeof(double)) + 7) / 8 * 8;
    p.lds = p.lds_bytes <= kLdsBudget && !force_global;
    p.chunks = (size_t)(K + C - 1) / C;
    const size_t per_src = p.lds ? 0 : nn * (kLdsPerNode - sizeof(double));
    const size_t per_wg = nn * (size_t)C * sizeof(double) * (p.lds ? 1 : 2);
    p.gs = std::min(S, kWorkBudget / (per_src + p.chunks * per_wg));
    p.gc = p.chunks;
    if (p.gs == 0) {
        p.gs = 1;
        p.gc = std::min(p.chunks, std::max<size_t>(1, (kWorkBudget - std::min(kWorkBudget, per_src)) / per_wg));
    }
    p.gc = std::min<size_t>(p.gc, 65535);
    return p;
}

// The chunk width of a call: the widest compiled width that K fills and whose launches, under the work budget, still hold at least
// one workgroup per CU, so the narrowest chunks that keep every CU busy; 1 where no width does.  Measured against the widest width
// that K fills.  forced: ep->reserved[1], a compiled width for tests; no result depends on the width
MultiPlan multi_choose(int K, size_t S, size_t nn, int cus, bool force_global, int64_t forced) {
    if (forced) return multi_plan((int)forced, K, S, nn, force_global);
    MultiPlan best = multi_plan(1, K, S, nn, force_global);
    for (int w : kMultiWidths) {
        if (w > K) continue;
        const MultiPlan p = multi_plan(w, K, S, nn, force_global);
        if (p.gs * p.gc >= (size_t)cus) best = p;
    }
    return best;
}

template <bool ADJ, int C, bool FACT> int lin_multi_launch(const char* who, bool lds, size_t lds_bytes, dim3 grid, int block,
                                                           const LinMultiArgs& a) {
    if (lds) {
        // the kernel's static LDS (red and redc) counts against the 64 KiB that need no attribute
        if (lds_bytes + sizeof(unsigned long long) * 2 * (kMaxBlock / 64) * (1 + C) > 65536)
            RTMI_HIP(hipFuncSetAttribute((const void*)k_eikonal_lin_multi<true, ADJ, C, FACT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kLdsBudget));
        hipLaunchKernelGGL((k_eikonal_lin_multi<true, ADJ, C, FACT>), grid, dim3(block), lds_bytes, nullptr, a);
    } else {
        hipLaunchKernelGGL((k_eikonal_lin_multi<false, ADJ, C, FACT>), grid, dim3(block), 0, nullptr, a);
    }
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

// the launch at the call's chunk width
template <bool ADJ, bool FACT> int lin_multi_launch_width(const char* who, int C, bool lds, size_t lds_bytes, dim3 grid, int block,
                                                          const LinMultiArgs& a) {
    if (C == 1) return lin_multi_launch<ADJ, 1, FACT>(who, lds, lds_bytes, grid, block, a);
    if (C == 4) return lin_multi_launch<ADJ, 4, FACT>(who, lds, lds_bytes, grid, block, a);
    return lin_multi_launch<ADJ, 8, FACT>(who, lds, lds_bytes, grid, block, a);
}

// One batched call on device memory: a holds the caller's pointers for all S sources and K columns
template <bool ADJ> int lin_multi_dev(const char* who, const rtmi_eikonal_params* ep, int64_t S, int K, LinMultiArgs a, int32_t* rounds,
                                      rtmi_eikonal_stats* stats) {
    rtmi_eikonal_stats total{};
    const size_t nn = (size_t)ep->nx * (size_t)ep->ny;
    int device = 0, cus = 0;
    if (S > 0) {
        RTMI_HIP(hipGetDevice(&device));
        RTMI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    }
    const MultiPlan plan = multi_choose(K, (size_t)S, nn, cus, ep->reserved[0] == 1, ep->reserved[1]);
    const int C = plan.C;
    const size_t lds_bytes = plan.lds_bytes;
    const bool lds = plan.lds;
    total.path = lds ? RTMI_EIKONAL_LDS : RTMI_EIKONAL_GLOBAL;
    if (S > 0) {
        const long diag = (long)std::min(ep->nx, ep->ny);
        const int block = (int)std::min<long>(kMaxBlock, (diag + 63) / 64 * 64);
        const size_t chunks = plan.chunks, gs = plan.gs, gc = plan.gc;
        DevMem mem;
        a.g = rt::eik_grid(ep->gx0, ep->gdx, ep->gy0, ep->gdy);
        a.nx = (long)ep->nx;
        a.ny = (long)ep->ny;
        a.ball = ep->ball;
        a.max_rounds = ep->max_rounds > 0 ? ep->max_rounds : rt::kEikDefaultRounds;
        a.K = K;
        a.S = (size_t)S;
        if (!lds) {
            RTMI_ALLOC(mem.get(&a.ca, gs * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.cb, gs * nn * sizeof(double)));
            RTMI_ALLOC(mem.get(&a.code, gs * nn));
            if (ADJ) RTMI_ALLOC(mem.get(&a.kids, gs * nn));
            RTMI_ALLOC(mem.get(&a.wv, gs * gc * nn * (size_t)C * sizeof(double)));
        }
        RTMI_ALLOC(mem.get(&a.wk, gs * gc * nn * (size_t)C * sizeof(double)));
        const bool fact = ep->scheme == RTMI_EIKONAL_FACTORED_LIN;
        if (ADJ && fact && a.g_src) RTMI_ALLOC(mem.get(&a.gpart, gs * gc * (size_t)ep->ny * (size_t)C * sizeof(double)));
        unsigned long long* d_out = nullptr;
        RTMI_ALLOC(mem.get(&d_out, (size_t)K * (size_t)S * kOutWords * sizeof(unsigned long long)));
        a.out = d_out;
        EventMarks<2> marks;
        RTMI_HIP(marks.create());
        RTMI_HIP(marks.mark(0));
        for (size_t s0 = 0; s0 < (size_t)S; s0 += gs) {
            const size_t ns = std::min(gs, (size_t)S - s0);
            a.s0 = s0;
            if (!lds) {
                const long lanes = (long)(ns * nn);
                hipLaunchKernelGGL(fact ? k_eikonal_lin_setup<true> : k_eikonal_lin_setup<false>, blocks(lanes), dim3(256), 0, nullptr, a, lanes);
                if (ADJ) hipLaunchKernelGGL(k_eikonal_lin_kids, blocks(lanes), dim3(256), 0, nullptr, a, lanes);
                RTMI_HIP(hipGetLastError());
            }
            for (size_t ch = 0; ch < chunks; ch += gc) {
                const size_t nc = std::min(gc, chunks - ch);
                a.c0 = (int)(ch * (size_t)C);
                const dim3 grid((unsigned)ns, (unsigned)nc);
                if (fact) RTMI_RC((lin_multi_launch_width<ADJ, true>(who, C, lds, lds_bytes, grid, block, a)));
                else RTMI_RC((lin_multi_launch_width<ADJ, false>(who, C, lds, lds_bytes, grid, block, a)));
            }
        }
        RTMI_HIP(marks.mark(1));
        RTMI_HIP(marks.wait(1));
        RTMI_HIP(marks.ms(0, 1, &total.kernel_ms));
        std::vector<unsigned long long> out((size_t)K * (size_t)S * kOutWords);
        RTMI_HIP(hipMemcpy(out.data(), d_out, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t cs = 0; cs < (size_t)K * (size_t)S; cs++) {
            const unsigned long long* o = &out[cs * kOutWords];
            const int32_t r = (int32_t)(o[0] & 0xffffffffull), clean = (int32_t)(o[0] >> 32);
            if (rounds) {
                rounds[2 * cs] = r;
                rounds[2 * cs + 1] = clean;
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

// after check_eikonal: the column count, and the width that tests may force
int check_nrhs(const char* who, const rtmi_eikonal_params* ep, int32_t nrhs) {
    RTMI_ARG(nrhs >= 1 && nrhs <= RTMI_LSQR_MULTI_MAX, "nrhs must be in [1, " + std::to_string(RTMI_LSQR_MULTI_MAX) + "], got " + std::to_string(nrhs));
    bool known = ep->reserved[1] == 0;
    for (int w : kMultiWidths) known = known || ep->reserved[1] == w;
    RTMI_ARG(known, "reserved[1] must be 0 or a compiled chunk width (1, 4, 8)");
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_tangent_multi_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                               const double* d_n_src, const double* d_T, const uint8_t* d_filled, int32_t nrhs,
                                               const double* d_dn, const double* d_dn_src, const double* d_dT_seed, double* d_dT,
                                               int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_tangent_multi_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    RTMI_RC(check_nrhs(who, ep, nrhs));
    LinMultiArgs a{};
    if (S > 0) {
        RTMI_RC(check_lin(who, d_T, d_filled, d_dn, "dn", d_dT, "dT"));
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t K = (size_t)nrhs, nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn * sizeof(double);
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        RTMI_RC(check_device_pointer(device, who, d_T, tab, "d_T"));
        RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
        RTMI_RC(check_device_pointer(device, who, d_dn, K * nn * sizeof(double), "d_dn"));
        if (d_dn_src) RTMI_RC(check_device_pointer(device, who, d_dn_src, K * (size_t)S * sizeof(double), "d_dn_src"));
        if (d_dT_seed) RTMI_RC(check_device_pointer(device, who, d_dT_seed, K * tab, "d_dT_seed"));
        RTMI_RC(check_device_pointer(device, who, d_dT, K * tab, "d_dT"));
    }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.dn = d_dn; a.dn_src = d_dn_src; a.seed = d_dT_seed; a.v = d_dT;
    return lin_multi_dev<false>(who, ep, S, nrhs, a, rounds, stats);
}

RTMI_EXPORT int rtmi_eikonal_adjoint_multi_dev(const rtmi_eikonal_params* ep, const double* d_n, int64_t S, const double* d_src,
                                               const double* d_n_src, const double* d_T, const uint8_t* d_filled, int32_t nrhs,
                                               const double* d_r, double* d_lam, double* d_g, double* d_g_src, int32_t* rounds,
                                               rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_adjoint_multi_dev";
    RTMI_RC(check_eikonal(who, ep, d_n, S, d_src, d_n_src));
    RTMI_RC(check_nrhs(who, ep, nrhs));
    LinMultiArgs a{};
    if (S > 0) {
        RTMI_RC(check_lin(who, d_T, d_filled, d_r, "r", d_lam, "lam"));
        int device = 0;
        RTMI_HIP(hipGetDevice(&device));
        const size_t K = (size_t)nrhs, nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn * sizeof(double);
        RTMI_RC(check_device_pointer(device, who, d_n, nn * sizeof(double), "d_n"));
        RTMI_RC(check_device_pointer(device, who, d_src, (size_t)S * 2 * sizeof(double), "d_src"));
        RTMI_RC(check_device_pointer(device, who, d_n_src, (size_t)S * sizeof(double), "d_n_src"));
        RTMI_RC(check_device_pointer(device, who, d_T, tab, "d_T"));
        RTMI_RC(check_device_pointer(device, who, d_filled, (size_t)S * nn, "d_filled"));
        RTMI_RC(check_device_pointer(device, who, d_r, K * tab, "d_r"));
        RTMI_RC(check_device_pointer(device, who, d_lam, K * tab, "d_lam"));
        if (d_g) RTMI_RC(check_device_pointer(device, who, d_g, K * tab, "d_g"));
        if (d_g_src) RTMI_RC(check_device_pointer(device, who, d_g_src, K * (size_t)S * sizeof(double), "d_g_src"));
    }
    a.n = d_n; a.src = d_src; a.n_src = d_n_src; a.T = d_T; a.filled = d_filled;
    a.r = d_r; a.v = d_lam; a.gout = d_g; a.g_src = d_g_src;
    return lin_multi_dev<true>(who, ep, S, nrhs, a, rounds, stats);
}

RTMI_EXPORT int rtmi_eikonal_tangent_multi(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src,
                                           const double* n_src, const double* T, const uint8_t* filled, int32_t nrhs, const double* dn,
                                           const double* dn_src, const double* dT_seed, double* dT, int32_t* rounds,
                                           rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_tangent_multi";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    RTMI_RC(check_nrhs(who, ep, nrhs));
    LinMultiArgs a{};
    if (S == 0) return lin_multi_dev<false>(who, ep, 0, nrhs, a, rounds, stats);
    RTMI_RC(check_lin(who, T, filled, dn, "dn", dT, "dT"));
    const size_t K = (size_t)nrhs, nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    LinUpload u;
    RTMI_RC(upload_lin(who, mem, ep, S, n, src, n_src, T, filled, &u));
    double *d_dn = nullptr, *d_dn_src = nullptr, *d_seed = nullptr, *d_dT = nullptr;
    RTMI_ALLOC(mem.get(&d_dn, K * nn * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_dT, K * tab * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_dn, dn, K * nn * sizeof(double), hipMemcpyHostToDevice));
    if (dn_src) {
        RTMI_ALLOC(mem.get(&d_dn_src, K * (size_t)S * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_dn_src, dn_src, K * (size_t)S * sizeof(double), hipMemcpyHostToDevice));
    }
    if (dT_seed) {
        RTMI_ALLOC(mem.get(&d_seed, K * tab * sizeof(double)));
        RTMI_HIP(hipMemcpy(d_seed, dT_seed, K * tab * sizeof(double), hipMemcpyHostToDevice));
    }
    a.n = u.n; a.src = u.src; a.n_src = u.n_src; a.T = u.T; a.filled = u.filled;
    a.dn = d_dn; a.dn_src = d_dn_src; a.seed = d_seed; a.v = d_dT;
    RTMI_RC(lin_multi_dev<false>(who, ep, S, nrhs, a, rounds, stats));
    RTMI_HIP(hipMemcpy(dT, d_dT, K * tab * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_adjoint_multi(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src,
                                           const double* n_src, const double* T, const uint8_t* filled, int32_t nrhs, const double* r,
                                           double* lam, double* g, double* g_src, int32_t* rounds, rtmi_eikonal_stats* stats) {
    const char* who = "rtmi_eikonal_adjoint_multi";
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    RTMI_RC(check_nrhs(who, ep, nrhs));
    LinMultiArgs a{};
    if (S == 0) return lin_multi_dev<true>(who, ep, 0, nrhs, a, rounds, stats);
    RTMI_RC(check_lin(who, T, filled, r, "r", lam, "lam"));
    const size_t K = (size_t)nrhs, nn = (size_t)ep->nx * (size_t)ep->ny, tab = (size_t)S * nn;
    DevMem mem;
    LinUpload u;
    RTMI_RC(upload_lin(who, mem, ep, S, n, src, n_src, T, filled, &u));
    double *d_r = nullptr, *d_lam = nullptr, *d_g = nullptr, *d_g_src = nullptr;
    RTMI_ALLOC(mem.get(&d_r, K * tab * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_lam, K * tab * sizeof(double)));
    if (g) RTMI_ALLOC(mem.get(&d_g, K * tab * sizeof(double)));
    if (g_src) RTMI_ALLOC(mem.get(&d_g_src, K * (size_t)S * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_r, r, K * tab * sizeof(double), hipMemcpyHostToDevice));
    a.n = u.n; a.src = u.src; a.n_src = u.n_src; a.T = u.T; a.filled = u.filled;
    a.r = d_r; a.v = d_lam; a.gout = d_g; a.g_src = d_g_src;
    RTMI_RC(lin_multi_dev<true>(who, ep, S, nrhs, a, rounds, stats));
    RTMI_HIP(hipMemcpy(lam, d_lam, K * tab * sizeof(double), hipMemcpyDeviceToHost));
    if (g) RTMI_HIP(hipMemcpy(g, d_g, K * tab * sizeof(double), hipMemcpyDeviceToHost));
    if (g_src) RTMI_HIP(hipMemcpy(g_src, d_g_src, K * (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}
