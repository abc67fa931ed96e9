// eikonal_tomo.hip -- first-arrival eikonal tomography that stays on the device (rtmi_eikonal_tomo_create, _destroy, _info,
// _table, _apply, _transpose, _residual, _relinearise, their _dev forms, and rtmi_eikonal_tomo_lsqr).  include/rtmi.h states the
// contract; DESIGN.md section 36 the definitions and what was measured; rt_eikonal_tomo.h holds the host arithmetic.
//
// A handle keeps the medium, the tables of S sources, the bilinear weights of the R receivers and of the sources, and the lists
// of the transposed product on the device.  The sweeps are eikonal_lin.hip's, called through rtmi_eikonal_tangent_dev and
// rtmi_eikonal_adjoint_dev, and the fill is eikonal.hip's rtmi_eikonal_fill_dev; what is here is what goes round them:
//   k_etomo_sample    one lane per (plane, point): out = sample(v_plane, point), +0.0 (or nothing) where the point's flag is 0.
//                     The forward product's rows from dT, and dn_src and n_src of the sources from dn and n.
//   k_etomo_live      one lane per (source, receiver): the row is live iff none of the receiver's four corners is dead
//   k_etomo_spread    one lane per (source, touched node): the node's segment of the (receiver, corner) list in list order, a
//                     gather, so no atomics; r is zeroed by a plain pass first
//   k_etomo_reduce    one lane per node: the sum over the sources in increasing s, then the node's segment of the (source,
//                     corner) list; consecutive lanes read consecutive nodes of each g_s.  A value that is not finite sets a flag
//                     word (an integer atomic), which is the solver's A^T bound.
//   k_etomo_residual  one lane per (source, receiver): pick - sample(T_s, rec_k) on a live row with a pick, else +0.0
// Every loop bound comes from the host-built tables.  No floating-point atomics.  The solver is the loop of rt_lsqr_device.h with
// one column over [A | Dx | Dy | Dxx | Dyy] on the node grid, the regulariser rows those of rt_tomo_reg.h.
// Several columns per call (rtmi_eikonal_tomo_apply_multi, _transpose_multi, their _dev forms, _lsqr_multi, _set_column_group;
// DESIGN.md section 37): the sample, spread and reduce kernels take the column in blockIdx.y, the sweeps are the batched ones of
// eikonal_lin.hip, the work tables hold a group of columns, and the loop runs its columns in lock-step.
#include <cstring>
#include <new>
#include <type_traits>

#include "rt_lsqr_device.h"

#include "rt_eikonal_host.h"
#include "rt_eikonal_tomo.h"
#include "rt_tomo_reg.h"

struct rtmi_eikonal_tomo {
    int device = 0, cus = 0;
    rtmi_eikonal_params ep{};
    int64_t S = 0, R = 0;
    size_t nn = 0;
    bool self = false;                  // the tables are the handle's own fill from the ball
    DevMem mem;
    double *n = nullptr, *src = nullptr, *n_src = nullptr, *T = nullptr;
    uint8_t *filled = nullptr, *live = nullptr, *inside = nullptr;
    int32_t *ridx = nullptr, *sidx = nullptr;           // [R][4], [S][4]: the corner nodes
    double *rw = nullptr, *sw = nullptr;                // [R][4], [S][4]: their weights
    int64_t nt = 0;                                     // nodes the receivers touch
    int32_t *tnode = nullptr, *toff = nullptr, *tpair = nullptr;
    int32_t *soff = nullptr, *spair = nullptr;          // [nn + 1] and the (source, corner) pairs
    // The work tables hold `cols` columns and are the handle's own allocations, not mem's: a call that sweeps more grows them
    double *tab = nullptr, *r = nullptr, *g = nullptr;  // [cols][S][nn]: dT or lam; the adjoint's right-hand side; g
    double *dn_src = nullptr, *g_src = nullptr;         // [cols][S]
    int cols = 0;
    int cg = 0;                                         // rtmi_eikonal_tomo_set_column_group: columns swept together; 0: the default
    unsigned long long* red = nullptr;                  // kRedWords: a Vec's, and [4] k_etomo_reduce's flag
    unsigned long long* redm = nullptr;                 // many columns': kMultiMax x kRedM of a Vec, then kMultiMax flags; on first use
    size_t bytes = 0;
    std::vector<uint8_t> live_h;
    std::vector<int64_t> live_per;
    int64_t live_rows = 0;
    int32_t path = 0, fill_rounds = 0;
    double** table(int i) { return i == 0 ? &tab : i == 1 ? &r : i == 2 ? &g : i == 3 ? &dn_src : &g_src; }
    ~rtmi_eikonal_tomo() {
        for (int i = 0; i < 5; i++) (void)hipFree(*table(i));
    }
};

namespace {

constexpr size_t kFlagWord = 4;
static_assert(kFlagWord >= kRedM && kFlagWord < kRedWords, "the flag is a word of the handle's that no Vec pass touches");

__global__ void __launch_bounds__(256) k_etomo_sample(const double* __restrict__ v, size_t vs, const int32_t* __restrict__ idx,
                                                      const double* __restrict__ w, const uint8_t* __restrict__ flag, size_t fs, long P,
                                                      long total, bool keep, double* __restrict__ out, size_t vcs, size_t ocs) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    v += blockIdx.y * vcs;                              // the column in blockIdx.y: its planes of v and of out
    out += blockIdx.y * ocs;
    const long k = t % P, s = t / P;
    if (!flag[(size_t)s * fs + k]) {
        if (!keep) out[t] = 0.0;
        return;
    }
    const double* p = v + (size_t)s * vs;
    const int32_t* i = idx + 4 * k;
    out[t] = rt::etomo_sample(p[i[0]], p[i[1]], p[i[2]], p[i[3]], w + 4 * k);
}

__global__ void __launch_bounds__(256) k_etomo_live(const double* __restrict__ n, const double* __restrict__ T, size_t nn,
                                                    const int32_t* __restrict__ idx, long R, long total, uint8_t* __restrict__ live) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long k = t % R, s = t / R;
    live[t] = rt::etomo_live(n, T + (size_t)s * nn, idx + 4 * k) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_etomo_spread(const double* __restrict__ y, const uint8_t* __restrict__ live, long R, long nt,
                                                      const int32_t* __restrict__ tnode, const int32_t* __restrict__ toff,
                                                      const int32_t* __restrict__ tpair, const double* __restrict__ w, size_t nn, long total,
                                                      double* __restrict__ r, size_t ycs, size_t rcs) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    y += blockIdx.y * ycs;                              // the column in blockIdx.y
    r += blockIdx.y * rcs;
    const long q = t % nt, s = t / nt;
    double acc = 0.0;
    for (int32_t p = toff[q]; p < toff[q + 1]; p++) {
        const int32_t pr = tpair[p];
        const long row = s * R + (pr >> 2);
        if (live[row]) acc = acc + w[pr] * y[row];
    }
    r[(size_t)s * nn + tnode[q]] = acc;
}

__global__ void __launch_bounds__(256) k_etomo_reduce(const double* __restrict__ g, const double* __restrict__ g_src, long S, long nn,
                                                      const int32_t* __restrict__ soff, const int32_t* __restrict__ spair,
                                                      const double* __restrict__ sw, double* __restrict__ G, unsigned long long* flag,
                                                      size_t gcs, size_t scs) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= nn) return;
    g += blockIdx.y * gcs;                              // the column in blockIdx.y: its planes, its G and its flag word
    g_src += blockIdx.y * scs;
    G += blockIdx.y * (size_t)nn;
    flag += blockIdx.y;
    double acc = 0.0;
    for (long s = 0; s < S; s++) acc = acc + g[(size_t)s * nn + x];
    for (int32_t p = soff[x]; p < soff[x + 1]; p++) {
        const int32_t pr = spair[p];
        acc = acc + sw[pr] * g_src[pr >> 2];
    }
    G[x] = acc;
    if (!(fabs(acc) < INFINITY)) atomicMax(flag, 1ull);
}

__global__ void __launch_bounds__(256) k_etomo_residual(const double* __restrict__ T, size_t nn, const int32_t* __restrict__ idx,
                                                        const double* __restrict__ w, const uint8_t* __restrict__ live,
                                                        const double* __restrict__ picks, long R, long total, double* __restrict__ res) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long k = t % R, s = t / R;
    const double pick = picks[t];
    double v = 0.0;
    if (live[t] && pick == pick) {
        const double* p = T + (size_t)s * nn;
        const int32_t* i = idx + 4 * k;
        v = pick - rt::etomo_sample(p[i[0]], p[i[1]], p[i[2]], p[i[3]], w + 4 * k);
    }
    res[t] = v;
}

int on_device(const rtmi_eikonal_tomo* h, const char* who) {
    int dev = -1;
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_ARG(dev == h->device, "the calling thread's current device is not the handle's");
    return RTMI_OK;
}

int not_clean(const char* who, const rtmi_eikonal_tomo* h, const std::vector<int32_t>& rounds, const char* what) {
    for (int64_t s = 0; s < h->S; s++)
        if (!rounds[2 * (size_t)s + 1])
            return rtmi_internal_fail(RTMI_ERR_STATE, (std::string(who) + ": " + what + " of source " + std::to_string(s) +
                                                       " did not converge within max_rounds").c_str());
    return RTMI_OK;
}

// the same for the kc columns from column c0 on of a batched sweep: rounds [kc][S][2]
int not_clean(const char* who, const rtmi_eikonal_tomo* h, const std::vector<int32_t>& rounds, int kc, int c0, const char* what) {
    for (int c = 0; c < kc; c++)
        for (int64_t s = 0; s < h->S; s++)
            if (!rounds[2 * ((size_t)c * (size_t)h->S + (size_t)s) + 1])
                return rtmi_internal_fail(RTMI_ERR_STATE, (std::string(who) + ": " + what + " of source " + std::to_string(s) + ", column " +
                                                           std::to_string(c0 + c) + " did not converge within max_rounds").c_str());
    return RTMI_OK;
}

// The work tables for `want` columns: kept, and replaced by a larger set when a call sweeps more together.  A growth that fails
// leaves the tables the handle had, so every call that they serve still works
int ensure_cols(rtmi_eikonal_tomo* h, const char* who, int want) {
    if (h->cols >= want) return RTMI_OK;
    const size_t tab = (size_t)h->S * h->nn * sizeof(double), vec = (size_t)h->S * sizeof(double);
    double* fresh[5] = {};
    for (int i = 0; i < 5; i++)
        if (hipMalloc((void**)&fresh[i], (size_t)want * (i < 3 ? tab : vec)) != hipSuccess) {
            (void)hipGetLastError();
            for (int k = 0; k < i; k++) (void)hipFree(fresh[k]);
            return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": hipMalloc of the work tables of " + std::to_string(want) +
                                                       " columns failed").c_str());
        }
    for (int i = 0; i < 5; i++) {
        (void)hipFree(*h->table(i));
        *h->table(i) = fresh[i];
    }
    h->bytes += (size_t)(want - h->cols) * (3 * tab + 2 * vec);
    h->cols = want;
    return RTMI_OK;
}

// the columns a batched call sweeps together: the caller's, or as many as keep the work tables under 8 GiB
int column_group(const rtmi_eikonal_tomo* h, int K) {
    const size_t per = (size_t)h->S * (3 * h->nn + 2) * sizeof(double);
    const size_t fit = std::max<size_t>(1, ((size_t)8 << 30) / per);
    return (int)std::min<size_t>((size_t)K, h->cg > 0 ? (size_t)h->cg : fit);
}

// the sources' samples of a model-sized vector: out [S]; keep: a source outside the grid keeps its value, else it gets +0.0
int sample_sources(const rtmi_eikonal_tomo* h, const char* who, const double* d_v, bool keep, double* out) {
    hipLaunchKernelGGL(k_etomo_sample, blocks((long)h->S), dim3(256), 0, nullptr, d_v, (size_t)0, h->sidx, h->sw, h->inside, (size_t)0,
                       (long)h->S, (long)h->S, keep, out, (size_t)0, (size_t)0);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

// The tables of a self-filled handle from the ball, and every handle's live rows
int refill(rtmi_eikonal_tomo* h, const char* who) {
    const size_t rows = (size_t)h->S * (size_t)h->R;
    if (h->self) {
        RTMI_HIP(hipMemset(h->T, 0xff, (size_t)h->S * h->nn * sizeof(double)));       // every input NaN: the point-source solve
        std::vector<int32_t> rounds(2 * (size_t)h->S);
        rtmi_eikonal_stats es{};
        RTMI_RC(rtmi_eikonal_fill_dev(&h->ep, h->n, h->S, h->src, h->n_src, h->T, rounds.data(), h->filled, &es));
        RTMI_RC(not_clean(who, h, rounds, "the fill"));
        h->fill_rounds = es.rounds_max;
    }
    hipLaunchKernelGGL(k_etomo_live, blocks((long)rows), dim3(256), 0, nullptr, h->n, h->T, h->nn, h->ridx, (long)h->R, (long)rows, h->live);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h->live_h.data(), h->live, rows, hipMemcpyDeviceToHost));
    h->live_rows = 0;
    for (int64_t s = 0; s < h->S; s++) {
        int64_t c = 0;
        for (int64_t k = 0; k < h->R; k++) c += h->live_h[(size_t)(s * h->R + k)];
        h->live_per[(size_t)s] = c;
        h->live_rows += c;
    }
    return RTMI_OK;
}

struct ProductTimes {
    double sweep_ms = 0.0, kernel_ms = 0.0, reduce_ms = 0.0;
    int32_t rounds_max = 0;
};

void fill_stats(const rtmi_eikonal_tomo* h, const ProductTimes& pt, rtmi_eikonal_tomo_stats* st) {
    if (!st) return;
    *st = rtmi_eikonal_tomo_stats{};
    st->rows = h->S * h->R;
    st->live_rows = h->live_rows;
    st->S = h->S;
    st->R = h->R;
    st->nx = h->ep.nx;
    st->ny = h->ep.ny;
    st->touched = h->nt;
    st->bytes_device = (int64_t)h->bytes;
    st->self_filled = h->self ? 1 : 0;
    st->path = h->path;
    st->rounds_max = pt.rounds_max ? pt.rounds_max : h->fill_rounds;
    st->sweep_ms = pt.sweep_ms;
    st->kernel_ms = pt.kernel_ms;
    st->reduce_ms = pt.reduce_ms;
}

// y = A dn on device pointers: the sources' samples, the tangent sweep, the receivers' samples
int apply_dev(rtmi_eikonal_tomo* h, const char* who, const double* d_dn, double* d_y, ProductTimes* pt) {
    const long rows = (long)(h->S * h->R);
    EventMarks<4> marks;
    RTMI_HIP(marks.create());
    RTMI_HIP(marks.mark(0));
    RTMI_RC(sample_sources(h, who, d_dn, false, h->dn_src));
    RTMI_HIP(marks.mark(1));
    std::vector<int32_t> rounds(2 * (size_t)h->S);
    rtmi_eikonal_stats es{};
    RTMI_RC(rtmi_eikonal_tangent_dev(&h->ep, h->n, h->S, h->src, h->n_src, h->T, h->filled, d_dn, h->dn_src, nullptr, h->tab, rounds.data(), &es));
    RTMI_RC(not_clean(who, h, rounds, "the tangent sweep"));
    RTMI_HIP(marks.mark(2));
    hipLaunchKernelGGL(k_etomo_sample, blocks(rows), dim3(256), 0, nullptr, h->tab, h->nn, h->ridx, h->rw, h->live, (size_t)h->R, (long)h->R,
                       rows, false, d_y, (size_t)0, (size_t)0);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(marks.mark(3));
    RTMI_HIP(marks.wait(3));
    if (pt) {
        double a = 0.0, b = 0.0;
        RTMI_HIP(marks.ms(0, 1, &a));
        RTMI_HIP(marks.ms(2, 3, &b));
        pt->kernel_ms += a + b;
        pt->sweep_ms += es.kernel_ms;
        pt->rounds_max = std::max(pt->rounds_max, es.rounds_max);
    }
    return RTMI_OK;
}

// G = A^T y on device pointers: the spread, the adjoint sweep, the sum.  *range: a value of G is not finite
int transpose_dev(rtmi_eikonal_tomo* h, const char* who, const double* d_y, double* d_G, bool* range, ProductTimes* pt) {
    const size_t tab = (size_t)h->S * h->nn;
    EventMarks<4> marks;
    RTMI_HIP(marks.create());
    RTMI_HIP(marks.mark(0));
    RTMI_HIP(hipMemsetAsync(h->r, 0, tab * sizeof(double), nullptr));
    const long lanes = (long)(h->S * h->nt);
    hipLaunchKernelGGL(k_etomo_spread, blocks(lanes), dim3(256), 0, nullptr, d_y, h->live, (long)h->R, (long)h->nt, h->tnode, h->toff, h->tpair,
                       h->rw, h->nn, lanes, h->r, (size_t)0, (size_t)0);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(marks.mark(1));
    std::vector<int32_t> rounds(2 * (size_t)h->S);
    rtmi_eikonal_stats es{};
    RTMI_RC(rtmi_eikonal_adjoint_dev(&h->ep, h->n, h->S, h->src, h->n_src, h->T, h->filled, h->r, h->tab, h->g, h->g_src, rounds.data(), &es));
    RTMI_RC(not_clean(who, h, rounds, "the adjoint sweep"));
    RTMI_HIP(marks.mark(2));
    RTMI_HIP(hipMemsetAsync(h->red + kFlagWord, 0, sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(k_etomo_reduce, blocks((long)h->nn), dim3(256), 0, nullptr, h->g, h->g_src, (long)h->S, (long)h->nn, h->soff, h->spair,
                       h->sw, d_G, h->red + kFlagWord, (size_t)0, (size_t)0);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(marks.mark(3));
    unsigned long long flag = 0;
    RTMI_HIP(hipMemcpy(&flag, h->red + kFlagWord, sizeof flag, hipMemcpyDeviceToHost));
    if (range) *range = flag != 0;
    if (pt) {
        double a = 0.0, b = 0.0;
        RTMI_HIP(marks.ms(0, 1, &a));
        RTMI_HIP(marks.ms(2, 3, &b));
        pt->kernel_ms += a + b;
        pt->reduce_ms += b;
        pt->sweep_ms += es.kernel_ms;
        pt->rounds_max = std::max(pt->rounds_max, es.rounds_max);
    }
    return RTMI_OK;
}

// ----------------------------------------------------------------------------------------------- several columns per product
// Column c of a batched product is the product above on column c: the sweeps are rtmi_eikonal_tangent_multi_dev and
// rtmi_eikonal_adjoint_multi_dev, whose columns have the single sweeps' bits, and the kernels round them take the column in
// blockIdx.y.  K columns are walked in runs of at most column_group() consecutive columns of `mask`; a column outside it is
// neither read nor written.

// the many columns' reduction words, on first use
int ensure_redm(rtmi_eikonal_tomo* h, const char* who) {
    if (h->redm) return RTMI_OK;
    const size_t words = (size_t)kMultiMax * kRedM + (size_t)kMultiMax;
    RTMI_ALLOC(h->mem.get(&h->redm, words * sizeof(unsigned long long)));
    RTMI_HIP(hipMemset(h->redm, 0, words * sizeof(unsigned long long)));
    h->bytes += words * sizeof(unsigned long long);
    return RTMI_OK;
}

// f(c0, kc) for every run of consecutive columns of mask, cut at cg columns
template <typename F> int by_runs(int K, unsigned long long mask, int cg, F&& f) {
    for (int c0 = 0; c0 < K;) {
        if (!(mask & col_bit(c0))) { c0++; continue; }
        int kc = 1;
        while (kc < cg && c0 + kc < K && (mask & col_bit(c0 + kc))) kc++;
        RTMI_RC(f(c0, kc));
        c0 += kc;
    }
    return RTMI_OK;
}

// y + c ys = A (dn + c nn) for the columns c < K of mask, on device pointers
int apply_multi_dev(rtmi_eikonal_tomo* h, const char* who, int K, const double* d_dn, double* d_y, size_t ys, unsigned long long mask,
                    ProductTimes* pt) {
    const long rows = (long)(h->S * h->R);
    const int cg = column_group(h, K);
    RTMI_RC(ensure_cols(h, who, cg));
    const size_t tab = (size_t)h->S * h->nn;
    std::vector<int32_t> rounds(2 * (size_t)cg * (size_t)h->S);
    const double t0 = now_ms();
    RTMI_RC(by_runs(K, mask, cg, [&](int c0, int kc) {
        const double* dn = d_dn + (size_t)c0 * h->nn;
        hipLaunchKernelGGL(k_etomo_sample, dim3(blocks((long)h->S).x, (unsigned)kc), dim3(256), 0, nullptr, dn, (size_t)0, h->sidx, h->sw,
                           h->inside, (size_t)0, (long)h->S, (long)h->S, false, h->dn_src, h->nn, (size_t)h->S);
        RTMI_HIP(hipGetLastError());
        rtmi_eikonal_stats es{};
        RTMI_RC(rtmi_eikonal_tangent_multi_dev(&h->ep, h->n, h->S, h->src, h->n_src, h->T, h->filled, kc, dn, h->dn_src, nullptr, h->tab,
                                               rounds.data(), &es));
        RTMI_RC(not_clean(who, h, rounds, kc, c0, "the tangent sweep"));
        hipLaunchKernelGGL(k_etomo_sample, dim3(blocks(rows).x, (unsigned)kc), dim3(256), 0, nullptr, h->tab, h->nn, h->ridx, h->rw, h->live,
                           (size_t)h->R, (long)h->R, rows, false, d_y + (size_t)c0 * ys, tab, ys);
        RTMI_HIP(hipGetLastError());
        if (pt) {
            pt->sweep_ms += es.kernel_ms;
            pt->rounds_max = std::max(pt->rounds_max, es.rounds_max);
        }
        return (int)RTMI_OK;
    }));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    if (pt) pt->kernel_ms += now_ms() - t0 - pt->sweep_ms;
    return RTMI_OK;
}

// G + c nn = A^T (y + c ys) for the columns c < K of mask.  range [K] (or NULL): a value of the column's G is not finite
int transpose_multi_dev(rtmi_eikonal_tomo* h, const char* who, int K, const double* d_y, size_t ys, double* d_G, unsigned long long mask,
                        bool* range, ProductTimes* pt) {
    const int cg = column_group(h, K);
    RTMI_RC(ensure_cols(h, who, cg));
    RTMI_RC(ensure_redm(h, who));
    unsigned long long* flags = h->redm + (size_t)kMultiMax * kRedM;
    const size_t tab = (size_t)h->S * h->nn;
    const long lanes = (long)(h->S * h->nt);
    std::vector<int32_t> rounds(2 * (size_t)cg * (size_t)h->S);
    const double t0 = now_ms();
    RTMI_RC(by_runs(K, mask, cg, [&](int c0, int kc) {
        RTMI_HIP(hipMemsetAsync(h->r, 0, (size_t)kc * tab * sizeof(double), nullptr));
        hipLaunchKernelGGL(k_etomo_spread, dim3(blocks(lanes).x, (unsigned)kc), dim3(256), 0, nullptr, d_y + (size_t)c0 * ys, h->live, (long)h->R,
                           (long)h->nt, h->tnode, h->toff, h->tpair, h->rw, h->nn, lanes, h->r, ys, tab);
        RTMI_HIP(hipGetLastError());
        rtmi_eikonal_stats es{};
        RTMI_RC(rtmi_eikonal_adjoint_multi_dev(&h->ep, h->n, h->S, h->src, h->n_src, h->T, h->filled, kc, h->r, h->tab, h->g, h->g_src,
                                               rounds.data(), &es));
        RTMI_RC(not_clean(who, h, rounds, kc, c0, "the adjoint sweep"));
        RTMI_HIP(hipMemsetAsync(flags, 0, (size_t)kc * sizeof(unsigned long long), nullptr));
        hipLaunchKernelGGL(k_etomo_reduce, dim3(blocks((long)h->nn).x, (unsigned)kc), dim3(256), 0, nullptr, h->g, h->g_src, (long)h->S,
                           (long)h->nn, h->soff, h->spair, h->sw, d_G + (size_t)c0 * h->nn, flags, tab, (size_t)h->S);
        RTMI_HIP(hipGetLastError());
        unsigned long long f[kMultiMax];
        RTMI_HIP(hipMemcpy(f, flags, (size_t)kc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (range)
            for (int c = 0; c < kc; c++) range[c0 + c] = f[c] != 0;
        if (pt) {
            pt->sweep_ms += es.kernel_ms;
            pt->rounds_max = std::max(pt->rounds_max, es.rounds_max);
        }
        return (int)RTMI_OK;
    }));
    if (pt) pt->kernel_ms += now_ms() - t0 - pt->sweep_ms;
    return RTMI_OK;
}

int check_nrhs(const char* who, int32_t nrhs) {
    RTMI_ARG(nrhs >= 1 && nrhs <= kMultiMax, "nrhs must be in [1, " + std::to_string(kMultiMax) + "], got " + std::to_string(nrhs));
    return RTMI_OK;
}

int residual_dev(rtmi_eikonal_tomo* h, const char* who, const double* d_picks, double* d_res) {
    const long rows = (long)(h->S * h->R);
    hipLaunchKernelGGL(k_etomo_residual, blocks(rows), dim3(256), 0, nullptr, h->T, h->nn, h->ridx, h->rw, h->live, d_picks, (long)h->R, rows,
                       d_res);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipStreamSynchronize(nullptr));
    return RTMI_OK;
}

// a caller's device vector of `count` doubles
int check_vec(const rtmi_eikonal_tomo* h, const char* who, const void* p, size_t count, const char* name) {
    RTMI_ARG(p, std::string("null ") + name);
    return check_device_pointer(h->device, who, p, count * sizeof(double), name);
}

// One entry on host pointers: upload `in` (nin doubles), the _dev body, download `out` (nout doubles) when it succeeded
template <typename F> int host_call(rtmi_eikonal_tomo* h, const char* who, const double* in, size_t nin, const char* in_name, double* out,
                                    size_t nout, const char* out_name, F&& body) {
    RTMI_ARG(h, "null handle");
    RTMI_ARG(in, std::string("null ") + in_name);
    RTMI_ARG(out, std::string("null ") + out_name);
    RTMI_RC(on_device(h, who));
    DevMem mem;
    double *d_in = nullptr, *d_out = nullptr;
    RTMI_ALLOC(mem.get(&d_in, nin * sizeof(double)));
    RTMI_ALLOC(mem.get(&d_out, nout * sizeof(double)));
    RTMI_HIP(hipMemcpy(d_in, in, nin * sizeof(double), hipMemcpyHostToDevice));
    RTMI_RC(body(d_in, d_out));
    RTMI_HIP(hipMemcpy(out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_tomo_create(const rtmi_eikonal_params* ep, const double* n, int64_t S, const double* src, const double* n_src,
                                         const double* T, const uint8_t* filled, int64_t R, const double* rec, rtmi_eikonal_tomo** out) {
    const char* who = "rtmi_eikonal_tomo_create";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_RC(check_eikonal(who, ep, n, S, src, n_src));
    RTMI_RC(check_eikonal_scheme(who, ep));      // the handle's own fill and every relinearise read it
    RTMI_ARG(S >= 1, "S must be >= 1");
    RTMI_ARG(R >= 1, "R must be >= 1");
    RTMI_ARG(rec, "null rec");
    RTMI_ARG((T == nullptr) == (filled == nullptr), "exactly one of T and filled is null: give both (a fill's result) or neither");
    RTMI_ARG((double)S * (double)R < (double)(1L << 29), "S R must be below 2^29");
    const long nx = (long)ep->nx, ny = (long)ep->ny;
    const size_t nn = (size_t)nx * (size_t)ny;
    const rt::EikGrid g = rt::eik_grid(ep->gx0, ep->gdx, ep->gy0, ep->gdy);
    for (int64_t k = 0; k < R; k++)
        RTMI_ARG(rt::etomo_receiver_ok(g, nx, ny, rec[2 * k], rec[2 * k + 1]),
                 "rec: receiver " + std::to_string(k) + " is not finite or lies outside the grid");
    // the tables of weights and the lists, on the host
    std::vector<int32_t> ridx(4 * (size_t)R), sidx(4 * (size_t)S);
    std::vector<double> rw(4 * (size_t)R), sw(4 * (size_t)S);
    std::vector<uint8_t> inside((size_t)S);
    for (int64_t k = 0; k < R; k++) {
        const rt::EtomoCell c = rt::etomo_cell(g, nx, ny, rec[2 * k], rec[2 * k + 1], false);
        for (int q = 0; q < 4; q++) { ridx[4 * k + q] = (int32_t)c.idx[q]; rw[4 * k + q] = c.w[q]; }
    }
    for (int64_t s = 0; s < S; s++) {
        const rt::EtomoCell c = rt::etomo_cell(g, nx, ny, src[2 * s], src[2 * s + 1], true);
        for (int q = 0; q < 4; q++) { sidx[4 * s + q] = (int32_t)c.idx[q]; sw[4 * s + q] = c.w[q]; }
        inside[(size_t)s] = c.inside ? 1 : 0;
    }
    const rt::EtomoLists LR = rt::etomo_lists(ridx.data(), (long)R, nullptr), LS = rt::etomo_lists(sidx.data(), (long)S, inside.data());
    std::vector<int32_t> soff(nn + 1, 0);
    for (size_t q = 0; q < LS.node.size(); q++) soff[(size_t)LS.node[q] + 1] = LS.off[q + 1] - LS.off[q];
    for (size_t x = 0; x < nn; x++) soff[x + 1] += soff[x];

    rtmi_eikonal_tomo* h = new (std::nothrow) rtmi_eikonal_tomo;
    if (!h) return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": out of host memory").c_str());
    struct Guard {
        rtmi_eikonal_tomo* h;
        ~Guard() { delete h; }
    } guard{h};
    RTMI_HIP(hipGetDevice(&h->device));
    RTMI_HIP(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device));
    h->ep = *ep;
    h->S = S;
    h->R = R;
    h->nn = nn;
    h->self = T == nullptr;
    h->nt = (int64_t)LR.node.size();
    const size_t rows = (size_t)S * (size_t)R, tab = (size_t)S * nn;
    h->live_h.assign(rows, 0);
    h->live_per.assign((size_t)S, 0);
    auto up = [&](auto** d, const auto* src_, size_t count) {
        using E = std::remove_const_t<std::remove_pointer_t<decltype(src_)>>;
        const size_t b = count * sizeof(E);
        h->bytes += b;
        if (h->mem.get(d, b) != hipSuccess) return hipErrorOutOfMemory;
        return src_ && b ? hipMemcpy(*d, src_, b, hipMemcpyHostToDevice) : hipSuccess;
    };
    RTMI_ALLOC(up(&h->n, n, nn));
    RTMI_ALLOC(up(&h->src, src, 2 * (size_t)S));
    RTMI_ALLOC(up(&h->n_src, n_src, (size_t)S));
    RTMI_ALLOC(up(&h->T, T, tab));
    RTMI_ALLOC(up(&h->filled, filled, tab));
    RTMI_ALLOC(up(&h->inside, inside.data(), (size_t)S));
    RTMI_ALLOC(up(&h->ridx, ridx.data(), ridx.size()));
    RTMI_ALLOC(up(&h->rw, rw.data(), rw.size()));
    RTMI_ALLOC(up(&h->sidx, sidx.data(), sidx.size()));
    RTMI_ALLOC(up(&h->sw, sw.data(), sw.size()));
    RTMI_ALLOC(up(&h->tnode, LR.node.data(), LR.node.size()));
    RTMI_ALLOC(up(&h->toff, LR.off.data(), LR.off.size()));
    RTMI_ALLOC(up(&h->tpair, LR.pair.data(), LR.pair.size()));
    RTMI_ALLOC(up(&h->soff, soff.data(), soff.size()));
    RTMI_ALLOC(up(&h->spair, LS.pair.data(), LS.pair.size()));
    RTMI_ALLOC(up(&h->live, (const uint8_t*)nullptr, rows));
    RTMI_RC(ensure_cols(h, who, 1));
    RTMI_ALLOC(up(&h->red, (const unsigned long long*)nullptr, kRedWords));
    RTMI_HIP(hipMemset(h->red, 0, kRedWords * sizeof(unsigned long long)));
    rtmi_eikonal_stats sweeps{};                              // a call with no source does no work and names the sweeps' path
    RTMI_RC(rtmi_eikonal_tangent_dev(ep, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sweeps));
    h->path = sweeps.path;
    RTMI_RC(refill(h, who));
    guard.h = nullptr;
    *out = h;
    return RTMI_OK;
}

RTMI_EXPORT void rtmi_eikonal_tomo_destroy(rtmi_eikonal_tomo* h) { delete h; }

RTMI_EXPORT int rtmi_eikonal_tomo_info(const rtmi_eikonal_tomo* h, rtmi_eikonal_tomo_stats* st, int64_t* live_per_source) {
    const char* who = "rtmi_eikonal_tomo_info";
    RTMI_ARG(h, "null handle");
    fill_stats(h, ProductTimes{}, st);
    if (live_per_source) std::memcpy(live_per_source, h->live_per.data(), (size_t)h->S * sizeof(int64_t));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_table(const rtmi_eikonal_tomo* h, double* T, uint8_t* filled, uint8_t* live) {
    const char* who = "rtmi_eikonal_tomo_table";
    RTMI_ARG(h, "null handle");
    RTMI_RC(on_device(h, who));
    const size_t tab = (size_t)h->S * h->nn;
    if (T) RTMI_HIP(hipMemcpy(T, h->T, tab * sizeof(double), hipMemcpyDeviceToHost));
    if (filled) RTMI_HIP(hipMemcpy(filled, h->filled, tab, hipMemcpyDeviceToHost));
    if (live) std::memcpy(live, h->live_h.data(), h->live_h.size());
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_apply_dev(rtmi_eikonal_tomo* h, const double* d_dn, double* d_y, rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_apply_dev";
    RTMI_ARG(h, "null handle");
    RTMI_RC(on_device(h, who));
    RTMI_RC(check_vec(h, who, d_dn, h->nn, "d_dn"));
    RTMI_RC(check_vec(h, who, d_y, (size_t)(h->S * h->R), "d_y"));
    ProductTimes pt;
    RTMI_RC(apply_dev(h, who, d_dn, d_y, &pt));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_apply(rtmi_eikonal_tomo* h, const double* dn, double* y, rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_apply";
    ProductTimes pt;
    RTMI_RC(host_call(h, who, dn, h ? h->nn : 0, "dn", y, h ? (size_t)(h->S * h->R) : 0, "y",
                      [&](const double* a, double* b) { return apply_dev(h, who, a, b, &pt); }));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_transpose_dev(rtmi_eikonal_tomo* h, const double* d_y, double* d_G, rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_transpose_dev";
    RTMI_ARG(h, "null handle");
    RTMI_RC(on_device(h, who));
    RTMI_RC(check_vec(h, who, d_y, (size_t)(h->S * h->R), "d_y"));
    RTMI_RC(check_vec(h, who, d_G, h->nn, "d_G"));
    ProductTimes pt;
    RTMI_RC(transpose_dev(h, who, d_y, d_G, nullptr, &pt));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_transpose(rtmi_eikonal_tomo* h, const double* y, double* G, rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_transpose";
    ProductTimes pt;
    RTMI_RC(host_call(h, who, y, h ? (size_t)(h->S * h->R) : 0, "y", G, h ? h->nn : 0, "G",
                      [&](const double* a, double* b) { return transpose_dev(h, who, a, b, nullptr, &pt); }));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_residual_dev(rtmi_eikonal_tomo* h, const double* d_picks, double* d_res) {
    const char* who = "rtmi_eikonal_tomo_residual_dev";
    RTMI_ARG(h, "null handle");
    RTMI_RC(on_device(h, who));
    RTMI_RC(check_vec(h, who, d_picks, (size_t)(h->S * h->R), "d_picks"));
    RTMI_RC(check_vec(h, who, d_res, (size_t)(h->S * h->R), "d_res"));
    return residual_dev(h, who, d_picks, d_res);
}

RTMI_EXPORT int rtmi_eikonal_tomo_residual(rtmi_eikonal_tomo* h, const double* picks, double* res) {
    const char* who = "rtmi_eikonal_tomo_residual";
    const size_t rows = h ? (size_t)(h->S * h->R) : 0;
    return host_call(h, who, picks, rows, "picks", res, rows, "res", [&](const double* a, double* b) { return residual_dev(h, who, a, b); });
}

namespace {

// the new medium is on the device already (h->n); n_src: given on the host, on the device, or sampled from n
int relinearise(rtmi_eikonal_tomo* h, const char* who, const double* n_src, bool n_src_dev) {
    if (n_src) RTMI_HIP(hipMemcpy(h->n_src, n_src, (size_t)h->S * sizeof(double), n_src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    else RTMI_RC(sample_sources(h, who, h->n, true, h->n_src));
    return refill(h, who);
}

int check_relinearise(const rtmi_eikonal_tomo* h, const char* who, const void* n) {
    RTMI_ARG(h, "null handle");
    RTMI_ARG(n, "null n");
    if (!h->self)
        return rtmi_internal_fail(RTMI_ERR_STATE, (std::string(who) + ": the handle's tables came from the caller (T and filled): "
                                                   "only a handle that filled its own can be re-linearised").c_str());
    return on_device(h, who);
}

}  // namespace

RTMI_EXPORT int rtmi_eikonal_tomo_relinearise(rtmi_eikonal_tomo* h, const double* n, const double* n_src) {
    const char* who = "rtmi_eikonal_tomo_relinearise";
    RTMI_RC(check_relinearise(h, who, n));
    RTMI_HIP(hipMemcpy(h->n, n, h->nn * sizeof(double), hipMemcpyHostToDevice));
    return relinearise(h, who, n_src, false);
}

RTMI_EXPORT int rtmi_eikonal_tomo_relinearise_dev(rtmi_eikonal_tomo* h, const double* d_n, const double* d_n_src) {
    const char* who = "rtmi_eikonal_tomo_relinearise_dev";
    RTMI_RC(check_relinearise(h, who, d_n));
    RTMI_RC(check_vec(h, who, d_n, h->nn, "d_n"));
    if (d_n_src) RTMI_RC(check_vec(h, who, d_n_src, (size_t)h->S, "d_n_src"));
    RTMI_HIP(hipMemcpy(h->n, d_n, h->nn * sizeof(double), hipMemcpyDeviceToDevice));
    return relinearise(h, who, d_n_src, true);
}

RTMI_EXPORT int rtmi_eikonal_tomo_lsqr(rtmi_eikonal_tomo* h, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo, const rtmi_tomo_reg* reg,
                                       const double* rhs, double* x, double* history, rtmi_lsqr_stats* st) {
    const char* who = "rtmi_eikonal_tomo_lsqr";
    RTMI_ARG(h, "null handle");
    RTMI_ARG(lp, "null params");
    RTMI_ARG(rhs, "null rhs");
    RTMI_ARG(x, "null x");
    RTMI_RC(lsqr_check_params(who, lp));
    const double *d1 = nullptr, *d2 = nullptr;
    RTMI_RC(check_reg(who, reg, &d1, &d2));
    const size_t rows = (size_t)(h->S * h->R), ng = h->nn, gx = (size_t)h->ep.nx, gy = (size_t)h->ep.ny;
    for (size_t i = 0; i < rows; i++) RTMI_ARG(std::isfinite(rhs[i]), "rhs has a value that is not finite");
    RTMI_RC(lsqr_check_options(who, lo, rows, ng));
    if (lo && lo->row_weight)
        for (size_t i = 0; i < rows; i++)
            RTMI_ARG(h->live_h[i] || lo->row_weight[i] == 0.0, "row_weight is not zero on dead row " + std::to_string(i));
    RTMI_RC(on_device(h, who));
    const size_t n1x = d1 ? gy * (gx - 1) : 0, n1y = d1 ? (gy - 1) * gx : 0;
    const size_t n2x = d2 && gx > 2 ? gy * (gx - 2) : 0, n2y = d2 && gy > 2 ? (gy - 2) * gx : 0;
    const size_t per = rows + n1x + n1y + n2x + n2y;
    const double t_begin = now_ms();
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    DevMem mem;
    size_t doubles = 0;
    auto get = [&](double** q, size_t n) {
        doubles += n;
        return mem.get(q, n * sizeof(double)) == hipSuccess;
    };
    double *u = nullptr, *Av = nullptr, *v = nullptr, *w = nullptr, *xd = nullptr, *Atu = nullptr, *x0 = nullptr;
    for (double** q : {&u, &Av})
        if (!get(q, per)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    for (double** q : {&v, &w, &xd, &Atu})
        if (!get(q, ng)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    if (lo && lo->x0) {
        if (!get(&x0, ng)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(x0, lo->x0, ng * sizeof(double), hipMemcpyHostToDevice));
    }
    // the row weights cover the S R observations; a regulariser's rows carry none
    LsqrOptions O;
    size_t nopt = 0;
    RTMI_RC(lsqr_upload_options(who, mem, lo, 1, false, rows, per, ng, &O, &nopt));
    doubles += nopt;
    const Vec V{h->red, h->cus, 1};
    double operator_ms = 0.0;
    // the stacked operator [A | Dx | Dy | Dxx | Dyy] on the node grid, and its transpose
    auto Ax = [&](const double* s, double* y, unsigned long long) {
        const double t0 = now_ms();
        RTMI_RC(apply_dev(h, who, s, y, nullptr));
        operator_ms += now_ms() - t0;                         // the regulariser's forward rows are outside it
        double* yk = y + rows;
        if (d1) hipLaunchKernelGGL(k_tomo_diff, blocks((long)ng), dim3(256), 0, nullptr, s, (int)gx, (int)gy, d1[0], d1[1], yk, yk + n1x);
        if (d2)
            hipLaunchKernelGGL(k_tomo_diff2, blocks((long)ng), dim3(256), 0, nullptr, s, (int)gx, (int)gy, d2[0], d2[1], yk + n1x + n1y,
                               yk + n1x + n1y + n2x);
        RTMI_HIP(hipGetLastError());
        return (int)RTMI_OK;
    };
    auto At = [&](const double* s, double* g, unsigned long long, bool* range) {
        const double t0 = now_ms();
        RTMI_RC(transpose_dev(h, who, s, g, &range[0], nullptr));
        if (!range[0] && (d1 || d2)) {
            const double* sk = s + rows;
            hipLaunchKernelGGL(k_tomo_reg_t, blocks((long)ng), dim3(256), 0, nullptr, g, (int)gx, (int)gy, d1 ? sk : nullptr,
                               d1 ? sk + n1x : nullptr, d1 ? d1[0] : 0.0, d1 ? d1[1] : 0.0, d2 ? sk + n1x + n1y : nullptr,
                               d2 ? sk + n1x + n1y + n2x : nullptr, d2 ? d2[0] : 0.0, d2 ? d2[1] : 0.0);
            RTMI_HIP(hipGetLastError());
        }
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
        return (int)RTMI_OK;
    };
    // the right-hand side goes up once, into the first S R values of u
    RTMI_HIP(hipMemsetAsync(u, 0, per * sizeof(double), nullptr));
    RTMI_HIP(hipMemsetAsync(xd, 0, ng * sizeof(double), nullptr));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    RTMI_HIP(hipMemcpy(u, rhs, rows * sizeof(double), hipMemcpyHostToDevice));
    if (x0) {                                                                         // u = fl(rhs - A x0) over the data rows; A x0 once
        const double t0 = now_ms();
        RTMI_RC(apply_dev(h, who, x0, Av, nullptr));
        RTMI_RC(lsqr_sub_start(who, V, u, per, Av, rows));
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
    }
    rtmi_lsqr_stats out{};
    RTMI_RC(lsqr_loop(who, V, lp, per, ng, LsqrVectors{u, Av, v, w, xd, Atu}, Ax, At, history, &out, O));
    if (x0) RTMI_RC(lsqr_add_start(who, V, xd, ng, x0, ng));
    RTMI_HIP(hipMemcpy(x, xd, ng * sizeof(double), hipMemcpyDeviceToHost));
    out.total_ms = now_ms() - t_begin;
    out.operator_ms = operator_ms;
    out.bytes_device = (int64_t)(doubles * sizeof(double) + h->bytes);
    if (st) *st = out;
    return RTMI_OK;
}

// ------------------------------------------------------------------------------------------------ several columns: the entries
RTMI_EXPORT int rtmi_eikonal_tomo_set_column_group(rtmi_eikonal_tomo* h, int32_t cg) {
    const char* who = "rtmi_eikonal_tomo_set_column_group";
    RTMI_ARG(h, "null handle");
    RTMI_ARG(cg >= 0 && cg <= kMultiMax, "cg must be in [0, " + std::to_string(kMultiMax) + "], got " + std::to_string(cg));
    h->cg = cg;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_apply_multi_dev(rtmi_eikonal_tomo* h, int32_t nrhs, const double* d_dn, double* d_y,
                                                  rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_apply_multi_dev";
    RTMI_ARG(h, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_RC(on_device(h, who));
    const size_t rows = (size_t)(h->S * h->R);
    RTMI_RC(check_vec(h, who, d_dn, (size_t)nrhs * h->nn, "d_dn"));
    RTMI_RC(check_vec(h, who, d_y, (size_t)nrhs * rows, "d_y"));
    ProductTimes pt;
    RTMI_RC(apply_multi_dev(h, who, nrhs, d_dn, d_y, rows, all_cols(nrhs), &pt));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_transpose_multi_dev(rtmi_eikonal_tomo* h, int32_t nrhs, const double* d_y, double* d_G,
                                                      rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_transpose_multi_dev";
    RTMI_ARG(h, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_RC(on_device(h, who));
    const size_t rows = (size_t)(h->S * h->R);
    RTMI_RC(check_vec(h, who, d_y, (size_t)nrhs * rows, "d_y"));
    RTMI_RC(check_vec(h, who, d_G, (size_t)nrhs * h->nn, "d_G"));
    ProductTimes pt;
    RTMI_RC(transpose_multi_dev(h, who, nrhs, d_y, rows, d_G, all_cols(nrhs), nullptr, &pt));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_apply_multi(rtmi_eikonal_tomo* h, int32_t nrhs, const double* dn, double* y, rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_apply_multi";
    RTMI_ARG(h, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    const size_t rows = (size_t)(h->S * h->R);
    ProductTimes pt;
    RTMI_RC(host_call(h, who, dn, (size_t)nrhs * h->nn, "dn", y, (size_t)nrhs * rows, "y", [&](const double* a, double* b) {
        return apply_multi_dev(h, who, nrhs, a, b, rows, all_cols(nrhs), &pt);
    }));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_eikonal_tomo_transpose_multi(rtmi_eikonal_tomo* h, int32_t nrhs, const double* y, double* G,
                                                  rtmi_eikonal_tomo_stats* st) {
    const char* who = "rtmi_eikonal_tomo_transpose_multi";
    RTMI_ARG(h, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    const size_t rows = (size_t)(h->S * h->R);
    ProductTimes pt;
    RTMI_RC(host_call(h, who, y, (size_t)nrhs * rows, "y", G, (size_t)nrhs * h->nn, "G", [&](const double* a, double* b) {
        return transpose_multi_dev(h, who, nrhs, a, rows, b, all_cols(nrhs), nullptr, &pt);
    }));
    fill_stats(h, pt, st);
    return RTMI_OK;
}

// The solver on K columns: the loop of rt_lsqr_device.h in lock-step over planes, as rtmi_tomo_lsqr_multi runs it; the products are
// the batched ones on the columns still in the loop, the regulariser kernels are launched per live column.  Column c has the bits of
// rtmi_eikonal_tomo_lsqr on column c: every pass of the loop treats its columns alone, and so do the products.
RTMI_EXPORT int rtmi_eikonal_tomo_lsqr_multi(rtmi_eikonal_tomo* h, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo,
                                             const rtmi_tomo_reg* reg, int32_t nrhs, int32_t flags, const double* rhs, double* x,
                                             double* history, rtmi_lsqr_stats* st) {
    const char* who = "rtmi_eikonal_tomo_lsqr_multi";
    RTMI_ARG(h, "null handle");
    RTMI_RC(check_nrhs(who, nrhs));
    RTMI_ARG((flags & ~RTMI_LSQR_MULTI_ROW_WEIGHT) == 0, "flags has bits other than RTMI_LSQR_MULTI_ROW_WEIGHT");
    RTMI_ARG(lp, "null params");
    RTMI_ARG(rhs, "null rhs");
    RTMI_ARG(x, "null x");
    RTMI_RC(lsqr_check_params(who, lp));
    const double *d1 = nullptr, *d2 = nullptr;
    RTMI_RC(check_reg(who, reg, &d1, &d2));
    const int K = (int)nrhs;
    const bool wr_cols = (flags & RTMI_LSQR_MULTI_ROW_WEIGHT) != 0;
    const size_t rows = (size_t)(h->S * h->R), ng = h->nn, gx = (size_t)h->ep.nx, gy = (size_t)h->ep.ny;
    for (size_t i = 0; i < (size_t)K * rows; i++)
        RTMI_ARG(std::isfinite(rhs[i]), "rhs has a value that is not finite in column " + std::to_string(i / rows));
    const size_t nwr = (wr_cols ? (size_t)K : 1) * rows;
    RTMI_RC(lsqr_check_options(who, lo, nwr, ng));
    if (lo && lo->row_weight)
        for (size_t i = 0; i < nwr; i++)
            RTMI_ARG(h->live_h[i % rows] || lo->row_weight[i] == 0.0, "row_weight is not zero on dead row " + std::to_string(i % rows) +
                                                                           (wr_cols ? " of column " + std::to_string(i / rows) : std::string()));
    RTMI_RC(on_device(h, who));
    const size_t n1x = d1 ? gy * (gx - 1) : 0, n1y = d1 ? (gy - 1) * gx : 0;
    const size_t n2x = d2 && gx > 2 ? gy * (gx - 2) : 0, n2y = d2 && gy > 2 ? (gy - 2) * gx : 0;
    const size_t per = rows + n1x + n1y + n2x + n2y;
    const double t_begin = now_ms();
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    RTMI_RC(ensure_redm(h, who));
    DevMem mem;
    size_t doubles = 0;
    auto get = [&](double** q, size_t n) {
        doubles += n;
        return mem.get(q, n * sizeof(double)) == hipSuccess;
    };
    double *u = nullptr, *Av = nullptr, *v = nullptr, *w = nullptr, *xd = nullptr, *Atu = nullptr, *x0 = nullptr;
    for (double** q : {&u, &Av})
        if (!get(q, (size_t)K * per)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    for (double** q : {&v, &w, &xd, &Atu})
        if (!get(q, (size_t)K * ng)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    if (lo && lo->x0) {
        if (!get(&x0, ng)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(x0, lo->x0, ng * sizeof(double), hipMemcpyHostToDevice));
    }
    LsqrOptions O;
    size_t nopt = 0;
    RTMI_RC(lsqr_upload_options(who, mem, lo, K, wr_cols, rows, per, ng, &O, &nopt));
    doubles += nopt;
    const Vec V{h->redm, h->cus, K};
    double operator_ms = 0.0;
    auto each = [&](unsigned long long mask, auto&& f) {
        for (int c = 0; c < K; c++)
            if (mask & col_bit(c)) RTMI_RC(f((size_t)c));
        return (int)RTMI_OK;
    };
    auto Ax = [&](const double* s, double* y, unsigned long long mask) {
        const double t0 = now_ms();
        RTMI_RC(apply_multi_dev(h, who, K, s, y, per, mask, nullptr));
        operator_ms += now_ms() - t0;                         // the regulariser's forward rows are outside it
        if (d1 || d2)
            RTMI_RC(each(mask, [&](size_t c) {
                const double* sc = s + c * ng;
                double* yk = y + c * per + rows;
                if (d1) hipLaunchKernelGGL(k_tomo_diff, blocks((long)ng), dim3(256), 0, nullptr, sc, (int)gx, (int)gy, d1[0], d1[1], yk, yk + n1x);
                if (d2)
                    hipLaunchKernelGGL(k_tomo_diff2, blocks((long)ng), dim3(256), 0, nullptr, sc, (int)gx, (int)gy, d2[0], d2[1], yk + n1x + n1y,
                                       yk + n1x + n1y + n2x);
                RTMI_HIP(hipGetLastError());
                return (int)RTMI_OK;
            }));
        return (int)RTMI_OK;
    };
    auto At = [&](const double* s, double* g, unsigned long long mask, bool* range) {
        const double t0 = now_ms();
        RTMI_RC(transpose_multi_dev(h, who, K, s, per, g, mask, range, nullptr));
        unsigned long long ok = 0ull;
        for (int c = 0; c < K; c++)
            if ((mask & col_bit(c)) && !range[c]) ok |= col_bit(c);
        if (d1 || d2)
            RTMI_RC(each(ok, [&](size_t c) {
                const double* sk = s + c * per + rows;
                hipLaunchKernelGGL(k_tomo_reg_t, blocks((long)ng), dim3(256), 0, nullptr, g + c * ng, (int)gx, (int)gy, d1 ? sk : nullptr,
                                   d1 ? sk + n1x : nullptr, d1 ? d1[0] : 0.0, d1 ? d1[1] : 0.0, d2 ? sk + n1x + n1y : nullptr,
                                   d2 ? sk + n1x + n1y + n2x : nullptr, d2 ? d2[0] : 0.0, d2 ? d2[1] : 0.0);
                RTMI_HIP(hipGetLastError());
                return (int)RTMI_OK;
            }));
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
        return (int)RTMI_OK;
    };
    // the right-hand sides go up once: column c into the first S R values of plane c
    RTMI_HIP(hipMemsetAsync(u, 0, (size_t)K * per * sizeof(double), nullptr));
    RTMI_HIP(hipMemsetAsync(xd, 0, (size_t)K * ng * sizeof(double), nullptr));
    RTMI_HIP(hipStreamSynchronize(nullptr));
    RTMI_HIP(hipMemcpy2D(u, per * sizeof(double), rhs, rows * sizeof(double), rows * sizeof(double), (size_t)K, hipMemcpyHostToDevice));
    if (x0) {                                                                         // u = fl(rhs - A x0) over the data rows; A x0 once
        const double t0 = now_ms();
        RTMI_RC(apply_dev(h, who, x0, Av, nullptr));
        RTMI_RC(lsqr_sub_start(who, V, u, per, Av, rows));
        RTMI_HIP(hipStreamSynchronize(nullptr));
        operator_ms += now_ms() - t0;
    }
    if (history) std::memset(history, 0, (size_t)K * (size_t)lp->iter_lim * 4 * sizeof(double));
    std::vector<rtmi_lsqr_stats> out((size_t)K);
    RTMI_RC(lsqr_loop(who, V, lp, per, ng, LsqrVectors{u, Av, v, w, xd, Atu}, Ax, At, history, out.data(), O));
    if (x0) RTMI_RC(lsqr_add_start(who, V, xd, ng, x0, ng));
    RTMI_HIP(hipMemcpy(x, xd, (size_t)K * ng * sizeof(double), hipMemcpyDeviceToHost));
    const double total = now_ms() - t_begin;
    for (int c = 0; c < K; c++) {
        out[(size_t)c].total_ms = total;
        out[(size_t)c].operator_ms = operator_ms;
        out[(size_t)c].bytes_device = (int64_t)(doubles * sizeof(double) + h->bytes);
        if (st) st[c] = out[(size_t)c];
    }
    return RTMI_OK;
}
