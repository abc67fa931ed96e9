// kirchhoff_lsqr.hip -- least-squares Kirchhoff migration that stays on the device (rtmi_kirchhoff_lsqr, rtmi_kirchhoff_lsqr_full,
// rtmi_kirchhoff_lsqr_filtered, rtmi_kirchhoff_lsqr_weighted, rtmi_debug_fix_norm):
// LSQR over the pair of kirchhoff.hip / kirchhoff_aa.hip on device pointers, every vector on the device from the one upload of the
// data to the one download of the model.  include/rtmi.h states the contract; DESIGN.md section 21 the definitions, the memory and
// what was measured; rt_lsqr.h the scalar recurrence (host, scipy's operation order).  _lsqr_full on a handle with kmah solves
// for the full trace ch0 + H ch1 with the Hilbert transform of kirchhoff_hilbert.hip around the pair;
// rtmi_kirchhoff_lsqr_filtered puts the trace filter of kirchhoff_filter.hip and its transpose around that.
// The loop, its vector passes and the order-independent norm are rt_lsqr_device.h's, shared with tomo.hip: a solve here is that
// loop with one column.  A start model is taken out of the data before the loop and added to the model after it, here.
#include "rt_hilbert.h"
#include "rt_kirchhoff.h"
#include "rt_lsqr_device.h"

namespace {

// Both solvers.  full: on a handle with kmah the operator is that of the full trace, A x = ch0 + H ch1 with (ch0, ch1) =
// model2(x), and A^T u = migrate2(u, -H u), its transpose in every bit; on any other handle `full` changes nothing.  filtered
// (with full): on a handle with a filter set, with B that operator, A x = F (B x) and A^T u = B^T (F^T u); F is out of place, so
// the call holds one more N nt vector, Fb, for B v and for F^T u, which are never live together.  With no filter set `filtered`
// changes nothing.  lo: the options of rtmi_kirchhoff_lsqr_weighted, uploaded once; NULL, or every pointer of
// it NULL, allocates nothing and runs the loop as it ran before there were options.  With x0 the right-hand side is
// fl(wr fl(data - A x0)), one forward product and one pass that also does the loop's fl(wr u), and x = fl(x0 + x) after its fl(dc x).
int lsqr_run(const char* who, bool full, bool filtered, rtmi_kirchhoff* k, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo,
             const double* data, double* x, double* history, rtmi_lsqr_stats* st) {
    RTMI_ARG(k, "null handle");
    RTMI_ARG(lp, "null params");
    RTMI_ARG(data, "null data");
    RTMI_ARG(x, "null x");
    RTMI_RC(lsqr_check_params(who, lp));
    RTMI_ARG(full || !k->kmah, "the handle has kmah: its trace is ch0 + H ch1, which rtmi_kirchhoff_lsqr_full solves for");
    const bool hil = full && k->kmah, fil = filtered && k->ftaps;
    if (hil) RTMI_RC(rtmi_internal_kirchhoff_hilbert_check(k, who));
    const size_t per = (size_t)k->kp.N * (size_t)k->kp.nt, nm = (size_t)k->nb * k->nn;
    for (size_t i = 0; i < per; i++) RTMI_ARG(std::isfinite(data[i]), "data has a value that is not finite");
    RTMI_RC(lsqr_check_options(who, lo, per, nm));
    RTMI_RC(check_device(k, who));
    const double t_begin = now_ms();
    DevMem mem;
    double *u = nullptr, *Av = nullptr, *v = nullptr, *w = nullptr, *xd = nullptr, *Atu = nullptr;
    double *Av1 = nullptr, *Hu = nullptr;                                             // channel 1 of A v, and -H u: with hil only
    double* Fb = nullptr;                                                             // B v, then F^T u: with fil only
    double* x0 = nullptr;
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    const struct { double** p; bool wanted; } traces[] = {{&u, true}, {&Av, true}, {&Av1, hil}, {&Hu, hil}, {&Fb, fil}};
    for (const auto& a : traces)
        if (a.wanted && mem.get(a.p, per * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    for (double** p : {&v, &w, &xd, &Atu})
        if (mem.get(p, nm * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
    LsqrOptions O;
    size_t nopt = 0;
    RTMI_RC(lsqr_upload_options(who, mem, lo, 1, false, per, per, nm, &O, &nopt));
    if (lo && lo->x0) {
        if (mem.get(&x0, nm * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(x0, lo->x0, nm * sizeof(double), hipMemcpyHostToDevice));
        nopt += nm;
    }
    const Vec V{k->red, k->cus, 1};
    rtmi_lsqr_stats out{};
    // the call's vectors, the handle's staging (with kmah: two channels per level) and, with hil and with fil, their taps
    const size_t staging = (size_t)(k->nlev ? k->nlev : 1) * (k->kmah ? 2 : 1) * per + nm;
    const size_t ntaps = (hil ? (size_t)rt::hilbert_ntaps(k->kp.nt) : 0) + (fil ? (size_t)k->fL : 0);
    out.bytes_device = (int64_t)(((hil ? 4 : 2) * per + (fil ? per : 0) + 4 * nm + nopt + staging + ntaps) * sizeof(double) +
                                 (k->ncounts + kRedWords) * sizeof(unsigned long long));
    double operator_ms = 0.0;
    rtmi_kirchhoff_stats ks{};

    // t = A^T s and t = A s; the Hilbert and filter kernels' event time counts as the operator's
    auto At = [&](const double* s, double* t, unsigned long long, bool* range) {
        range[0] = false;
        double ms = 0.0, fms = 0.0;
        if (fil) {
            RTMI_RC(rtmi_internal_kirchhoff_filter_dev(k, who, s, true, Fb, &fms));
            s = Fb;
        }
        if (hil) RTMI_RC(rtmi_internal_kirchhoff_hilbert_dev(k, who, s, nullptr, true, Hu, &ms));
        RTMI_RC(rtmi_internal_kirchhoff_migrate_dev(k, who, s, hil ? Hu : nullptr, t, &ks, false));
        operator_ms += ks.kernel_ms + ms + fms;
        return (int)RTMI_OK;
    };
    auto Ax = [&](const double* s, double* t, unsigned long long) {
        double ms = 0.0, fms = 0.0;
        double* b = fil ? Fb : t;                                                     // B s
        RTMI_RC(rtmi_internal_kirchhoff_model_dev(k, who, s, b, hil ? Av1 : nullptr, &ks, false));
        if (hil) RTMI_RC(rtmi_internal_kirchhoff_hilbert_dev(k, who, Av1, b, false, b, &ms));
        if (fil) RTMI_RC(rtmi_internal_kirchhoff_filter_dev(k, who, b, false, t, &fms));
        operator_ms += ks.kernel_ms + ms + fms;
        return (int)RTMI_OK;
    };

    RTMI_HIP(hipMemcpy(u, data, per * sizeof(double), hipMemcpyHostToDevice));       // the data go up once
    RTMI_HIP(hipMemsetAsync(xd, 0, nm * sizeof(double), nullptr));
    double start_ms = 0.0;                                                            // the start model's two passes: vector time
    auto timed = [&](auto&& pass) {
        const double t0 = now_ms();
        RTMI_RC(pass());
        RTMI_HIP(hipStreamSynchronize(nullptr));
        start_ms += now_ms() - t0;
        return (int)RTMI_OK;
    };
    if (x0) {
        RTMI_RC(Ax(x0, Av, 1ull));
        RTMI_RC(timed([&]() { return lsqr_sub_start(who, V, u, per, Av, per, O.wr, O.wrs); }));   // both in one pass: the same two roundings
        O.rhs_weighted = O.wr != nullptr;
    }
    RTMI_RC(lsqr_loop(who, V, lp, per, nm, LsqrVectors{u, Av, v, w, xd, Atu}, Ax, At, history, &out, O));
    if (x0) RTMI_RC(timed([&]() { return lsqr_add_start(who, V, xd, nm, x0, nm); }));
    out.vector_ms += start_ms;
    RTMI_HIP(hipMemcpy(x, xd, nm * sizeof(double), hipMemcpyDeviceToHost));           // the model comes down once
    out.total_ms = now_ms() - t_begin;
    out.operator_ms = operator_ms;
    if (st) *st = out;
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_lsqr(rtmi_kirchhoff* k, const rtmi_lsqr_params* lp, const double* data, double* x, double* history,
                                    rtmi_lsqr_stats* st) {
    return lsqr_run("rtmi_kirchhoff_lsqr", false, false, k, lp, nullptr, data, x, history, st);
}

RTMI_EXPORT int rtmi_kirchhoff_lsqr_full(rtmi_kirchhoff* k, const rtmi_lsqr_params* lp, const double* data, double* x, double* history,
                                         rtmi_lsqr_stats* st) {
    return lsqr_run("rtmi_kirchhoff_lsqr_full", true, false, k, lp, nullptr, data, x, history, st);
}

RTMI_EXPORT int rtmi_kirchhoff_lsqr_filtered(rtmi_kirchhoff* k, const rtmi_lsqr_params* lp, const double* data, double* x,
                                             double* history, rtmi_lsqr_stats* st) {
    return lsqr_run("rtmi_kirchhoff_lsqr_filtered", true, true, k, lp, nullptr, data, x, history, st);
}

RTMI_EXPORT int rtmi_kirchhoff_lsqr_weighted(rtmi_kirchhoff* k, const rtmi_lsqr_params* lp, const rtmi_lsqr_options* lo, int32_t op,
                                             const double* data, double* x, double* history, rtmi_lsqr_stats* st) {
    const char* who = "rtmi_kirchhoff_lsqr_weighted";
    RTMI_ARG(op == RTMI_LSQR_OP_PLAIN || op == RTMI_LSQR_OP_FULL || op == RTMI_LSQR_OP_FILTERED, "op must be one of RTMI_LSQR_OP_");
    return lsqr_run(who, op != RTMI_LSQR_OP_PLAIN, op == RTMI_LSQR_OP_FILTERED, k, lp, lo, data, x, history, st);
}

RTMI_EXPORT int rtmi_debug_fix_norm(const double* x, int64_t n, double* norm, int32_t* e) {
    const char* who = "rtmi_debug_fix_norm";
    RTMI_ARG(x, "null x");
    RTMI_ARG(norm, "null norm");
    RTMI_ARG(e, "null e");
    RTMI_ARG(n >= 1, "n must be >= 1");
    for (int64_t i = 0; i < n; i++) RTMI_ARG(std::isfinite(x[i]), "x has a value that is not finite");
    int dev = 0;
    Vec V{nullptr, 1, 1};
    RTMI_HIP(hipGetDevice(&dev));
    RTMI_HIP(hipDeviceGetAttribute(&V.cus, hipDeviceAttributeMultiprocessorCount, dev));
    DevMem mem;
    double* d = nullptr;
    RTMI_HIP(mem.get(&d, (size_t)n * sizeof(double)));
    RTMI_HIP(mem.get(&V.red, kRedM * sizeof(unsigned long long)));
    RTMI_HIP(hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    double M = 0.0;
    bool range = false;
    int ee = 0;
    RTMI_RC(absmax(who, V, d, (size_t)n, (size_t)n, 1ull, &M));
    RTMI_RC(norms(who, V, d, (size_t)n, (size_t)n, 1ull, &M, norm, &range, &ee));
    RTMI_ARG(!range, "max|x|^2 is not a normal number (RTMI_LSQR_RANGE)");
    *e = ee;
    return RTMI_OK;
}
