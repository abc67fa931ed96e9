// twopoint.hip -- receiver-line crossings of recorded rays (rtmi_crossings) and two-point ray tracing from sources to
// receivers on a line (rtmi_two_point): the shooting method of the reference's paper setting, in its two-point form.
// Batches are read through the checks of rtmi_host.h (recorded) and the public rtmi_batch_view; the refinement relaunches its
// batch through rtmi_internal_relaunch.
//
// The crossing arithmetic (rt_crossing.h) is written in one fixed order (compiled with -ffp-contract=off, sin/cos glibc's own
// through rt_libm.h) so that tests/crossing_ref.py, a numpy restatement, gives the same bits; the receiver angle goes through the
// device's atan2 (within an ulp of numpy's).  DESIGN.md section 9 describes the rules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_crossing.h"
#include "rt_rows.h"
#include "rtmi_host.h"

namespace {

// One lane per ray (slot k), looping over its rows.  x and y are read on every row; the other columns only on a step that
// crosses.  count[o] = crossings (-1: the trajectory reaches past rec_rows), out[kmax][6][R] = u x y T theta s.
template <typename T> __global__ void k_crossings(Rows<T> rec, Line L, int kmax, int32_t* count, double* out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rec.R) return;
    const long R = rec.R;
    const long o = rec.caller(k);
    const size_t P = rec.pitch();
    const T* col = rec.row(0, k);
    const long last = rec.last(k);
    int n = 0;
    if (last >= rec.rec_rows) {
        n = -1;
    } else {
        double x0 = (double)col[COL_X * R], y0 = (double)col[COL_Y * R];
        double f0 = (L.a * x0 + L.b * y0) - L.c;
        for (long i = 1; i <= last; i++) {
            const double x1 = (double)col[(size_t)i * P], y1 = (double)col[(size_t)i * P + COL_Y * R];
            const double f1 = (L.a * x1 + L.b * y1) - L.c;
            if (crosses(f0, f1)) {
                if (n < kmax) {
                    const T* r0 = col + (size_t)(i - 1) * P;
                    const T* r1 = col + (size_t)i * P;
                    const double th0 = (double)r0[COL_TH * R], th1 = (double)r1[COL_TH * R];
                    const double c0 = cos_g(th0), s0 = sin_g(th0), c1 = cos_g(th1), s1 = sin_g(th1);
                    const double dx = x1 - x0, dy = y1 - y0;
                    const double len = sqrt(dx * dx + dy * dy);
                    const double tx0 = len * c0, ty0 = len * s0, tx1 = len * c1, ty1 = len * s1;
                    const double d0 = len * (L.a * c0 + L.b * s0), d1 = len * (L.a * c1 + L.b * s1);
                    const double tau = cross_tau(f0, d0, f1, d1);
                    const Basis h = basis(tau), hd = dbasis(tau);
                    const double x = herm(h, x0, tx0, x1, tx1), y = herm(h, y0, ty0, y1, ty1);
                    const double m0 = (double)r0[COL_PX * R] * c0 + (double)r0[COL_PY * R] * s0;     // p . (cos, sin) = dT/ds
                    const double m1 = (double)r1[COL_PX * R] * c1 + (double)r1[COL_PY * R] * s1;
                    const double tt = herm(h, (double)r0[COL_T * R], len * m0, (double)r1[COL_T * R], len * m1);
                    const double th = atan2(herm(hd, y0, ty0, y1, ty1), herm(hd, x0, tx0, x1, tx1));
                    const double v[6] = {L.a * y - L.b * x, x, y, tt, th, (double)(i - 1) + tau};
                    for (int q = 0; q < 6; q++) out[((size_t)n * 6 + q) * R + o] = v[q];
                }
                n++;
            }
            x0 = x1; y0 = y1; f0 = f1;
        }
    }
    count[o] = n;
    for (int c = n < 0 ? 0 : n; c < kmax; c++)
        for (int q = 0; q < 6; q++) out[((size_t)c * 6 + q) * R + o] = NAN;
}

// k_crossings on the rows of a view, enqueued on st
int crossings_launch(const rtmi_device_view& v, const Line& L, int kmax, int32_t* d_count, double* d_out, hipStream_t st, const char* who) {
    by_dtype(v.dtype, [&](auto t) { hipLaunchKernelGGL(k_crossings<decltype(t)>, blocks((long)v.R), dim3(256), 0, st, rows_of<decltype(t)>(v), L, kmax, d_count, d_out); });
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}
// Crossings read rows wherever they came from: a batch continued from rtmi_batch_set_state is not refused.
int crossings_device(rtmi_batch* b, const Line& L, int kmax, int32_t* d_count, double* d_out, hipStream_t st, const char* who) {
    Recorded r;
    RTMI_RC(recorded(who, b, 0, 0, &r));
    return crossings_launch(r.v, L, kmax, d_count, d_out, st, who);
}

// ------------------------------------------------------------------ two-point
enum : int32_t { ST_EMPTY = -1, ST_ACTIVE = 0, ST_CONVERGED = RTMI_ARRIVAL_CONVERGED, ST_STALLED = RTMI_ARRIVAL_STALLED,
                 ST_TRUNCATED = RTMI_ARRIVAL_TRUNCATED };

// One bracket (source, receiver, slot): the crossing index it follows and the Illinois state on theta.
struct Bracket {
    double ta, tb, fa, fb;    // theta ends and u - u_j there
    double th;                // the angle traced next / last traced
    int32_t c, side, status, iters;
    int32_t key;              // m * kmax + c: the fan pair and crossing it came from (the sort key)
    int32_t pad_;
    double res[6];            // u x y T theta(receiver) at the converged crossing
};

__device__ __forceinline__ double falsi(double ta, double tb, double fa, double fb) {
    const double t = (ta * fb - tb * fa) / (fb - fa);
    const double lo = fmin(ta, tb), hi = fmax(ta, tb);
    return (t > lo && t < hi) ? t : ta + 0.5 * (tb - ta);
}

// the max of istep over rays -> *m (initialised to 0)
__global__ void k_max_istep(const int32_t* istep, long R, int32_t* m) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < R) atomicMax(m, istep[k]);
}

// One thread per (source, fan pair m, crossing c): every receiver u_j in [min, max) of the pair's two u gets a bracket.
__global__ void k_brackets(const int32_t* count, const double* cr, long Rg, int S, int M, int kmax, const double* thetas,
                           const double* ru, int J, int A, int32_t* nslot, Bracket* br, unsigned long long* overflow) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)(M - 1) * kmax;
    if (t >= (long)S * per) return;
    const int s = (int)(t / per), m = (int)(t % per / kmax), c = (int)(t % kmax);
    const long r0 = (long)s * M + m, r1 = r0 + 1;
    const int n = min(count[r0], count[r1]);
    if (c >= n) return;
    const double ua = cr[(size_t)c * 6 * Rg + r0], ub = cr[(size_t)c * 6 * Rg + r1];
    const double lo = fmin(ua, ub), hi = fmax(ua, ub);
    if (!(lo < hi)) return;
    int j0 = 0, j1 = J;                                // first j with ru[j] >= lo
    while (j0 < j1) {
        const int mid = (j0 + j1) >> 1;
        if (ru[mid] < lo) j0 = mid + 1; else j1 = mid;
    }
    for (int j = j0; j < J && ru[j] < hi; j++) {
        const int slot = atomicAdd(nslot + (size_t)s * J + j, 1);
        if (slot >= A) { atomicAdd(overflow, 1ull); continue; }
        Bracket& q = br[((size_t)s * J + j) * A + slot];
        q.ta = thetas[m]; q.tb = thetas[m + 1];
        q.fa = ua - ru[j]; q.fb = ub - ru[j];
        q.th = q.fa == 0.0 ? q.ta : q.fb == 0.0 ? q.tb : falsi(q.ta, q.tb, q.fa, q.fb);
        q.c = c; q.side = 0; q.status = ST_ACTIVE; q.iters = 0; q.key = m * kmax + c;
    }
}

// Per (source, receiver): slots in (m, c) order, so that the result does not depend on the order of the atomics; empty
// slots are marked.  Then the theta to trace and the per-ray max_size (1 for a slot with nothing to trace).
__global__ void k_sort_brackets(int SJ, int A, const int32_t* nslot, Bracket* br, double* th, int32_t* ms, int32_t max_size) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= SJ) return;
    Bracket* q = br + (size_t)t * A;
    const int n = min(nslot[t], A);
    for (int i = 1; i < n; i++)
        for (int j = i; j > 0 && q[j - 1].key > q[j].key; j--) { const Bracket w = q[j]; q[j] = q[j - 1]; q[j - 1] = w; }
    for (int i = 0; i < A; i++) {
        if (i >= n) q[i].status = ST_EMPTY;
        th[(size_t)t * A + i] = i < n ? q[i].th : 0.0;
        ms[(size_t)t * A + i] = i < n ? max_size : 1;
    }
}

// After a trace of every active bracket's theta: converged / stalled / truncated, or the next Illinois angle.
__global__ void k_update(long NB, int J, int A, const double* ru, const int32_t* count, const double* cr, double tol, Bracket* br,
                         double* th, int32_t* ms, int32_t* active) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NB) return;
    Bracket& q = br[t];
    if (q.status != ST_ACTIVE) return;
    const double uj = ru[(t / A) % J];
    q.iters++;
    const int n = count[t];
    if (n < 0) { q.status = ST_TRUNCATED; ms[t] = 1; return; }
    if (n <= q.c) { q.status = ST_STALLED; ms[t] = 1; return; }      // the branch is lost: a discontinuity in theta
    const double u = cr[(size_t)q.c * 6 * NB + t];
    const double f = u - uj;
    if (fabs(f) <= tol) {
        q.status = ST_CONVERGED;
        for (int c = 0; c < 5; c++) q.res[c] = cr[((size_t)q.c * 6 + c) * NB + t];
        q.res[5] = f;
        ms[t] = 1;
        return;
    }
    // Illinois: a retained end whose side is kept twice in a row has its value halved
    if ((f < 0.0) == (q.fb < 0.0)) {
        q.tb = q.th; q.fb = f;
        if (q.side == -1) q.fa *= 0.5;
        q.side = -1;
    } else {
        q.ta = q.th; q.fa = f;
        if (q.side == 1) q.fb *= 0.5;
        q.side = 1;
    }
    if (q.ta == q.tb || nextafter(q.ta, q.tb) == q.tb) { q.status = ST_STALLED; ms[t] = 1; return; }
    q.th = falsi(q.ta, q.tb, q.fa, q.fb);
    th[t] = q.th;
    atomicAdd(active, 1);
}

// Per (source, receiver): converged arrivals first, by T (ties in (m, c) order), then the others in (m, c) order.
// out[A][9] per pair: launch theta, T, u, x, y, theta at the receiver, u - u_j, iterations, status.
__global__ void k_output(int SJ, int A, const Bracket* br, double* out, int32_t* cnt, int32_t* bad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= SJ) return;
    const Bracket* q = br + (size_t)t * A;
    double* o = out + (size_t)t * A * 9;
    int nc = 0, nb = 0, w = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int i = 0; i < A; i++) {
            const bool conv = q[i].status == ST_CONVERGED;
            if (q[i].status == ST_EMPTY || conv != (pass == 0)) continue;
            int at = w;
            if (conv) {    // insertion by T among the converged ones written so far (stable: keeps (m, c) order on ties)
                while (at > 0 && o[(size_t)(at - 1) * 9 + 1] > q[i].res[3]) {
                    for (int f = 0; f < 9; f++) o[(size_t)at * 9 + f] = o[(size_t)(at - 1) * 9 + f];
                    at--;
                }
                nc++;
            } else {
                nb++;
            }
            double* e = o + (size_t)at * 9;
            e[0] = q[i].th;
            e[1] = conv ? q[i].res[3] : NAN;
            e[2] = conv ? q[i].res[0] : NAN;
            e[3] = conv ? q[i].res[1] : NAN;
            e[4] = conv ? q[i].res[2] : NAN;
            e[5] = conv ? q[i].res[4] : NAN;
            e[6] = conv ? q[i].res[5] : NAN;
            e[7] = (double)q[i].iters;
            e[8] = (double)(q[i].status == ST_ACTIVE ? ST_STALLED : q[i].status);     // max_iter ran out: reported as stalled
            w++;
        }
    }
    for (int i = w; i < A; i++) {
        double* e = o + (size_t)i * 9;
        for (int f = 0; f < 8; f++) e[f] = NAN;
        e[8] = (double)ST_EMPTY;
    }
    cnt[t] = nc;
    bad[t] = nb;
}

struct BatchGuard {
    rtmi_batch* b = nullptr;
    ~BatchGuard() { rtmi_batch_destroy(b); }
};
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

RTMI_EXPORT int rtmi_crossings(rtmi_batch* b, const double line[3], int32_t kmax, int32_t* count, double* out) {
    const char* who = "rtmi_crossings";
    RTMI_ARG(b && line && count && out, "null");
    RTMI_ARG(kmax >= 1, "kmax must be >= 1");
    Line L;
    RTMI_ARG(make_line(line, &L), "the line needs (a, b) != (0, 0) and finite coefficients");
    Recorded r;
    RTMI_RC(recorded(who, b, 0, 0, &r));
    const size_t R = (size_t)r.v.R;
    DevMem mem;
    int32_t* dc = nullptr;
    double* dout = nullptr;
    RTMI_HIP(mem.get(&dc, R * sizeof(int32_t)));
    RTMI_HIP(mem.get(&dout, (size_t)kmax * 6 * R * sizeof(double)));
    RTMI_RC(crossings_launch(r.v, L, kmax, dc, dout, nullptr, who));
    RTMI_HIP(hipMemcpy(count, dc, R * sizeof(int32_t), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(out, dout, (size_t)kmax * 6 * R * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_two_point(const rtmi_field* f, const rtmi_params* p, int32_t S, const double* sx, const double* sy, int32_t M,
                               const double* thetas, const double line[3], int32_t J, const double* receivers_u,
                               const rtmi_two_point_params* tp, int32_t* count, int32_t* nbad, double* arrivals,
                               rtmi_two_point_stats* stats) {
    const char* who = "rtmi_two_point";
    RTMI_ARG(f && p && sx && sy && thetas && line && receivers_u && count && nbad && arrivals, "null");
    RTMI_ARG(S >= 1 && M >= 2 && J >= 1, "needs S >= 1 sources, M >= 2 launch angles and J >= 1 receivers");
    RTMI_ARG(p->dtype == RTMI_F64, "fp64 only");
    Line L;
    RTMI_ARG(make_line(line, &L), "the line needs (a, b) != (0, 0) and finite coefficients");
    for (int j = 0; j < J; j++)
        RTMI_ARG(std::isfinite(receivers_u[j]) && (j == 0 || receivers_u[j] > receivers_u[j - 1]),
               "receivers_u must be finite and strictly increasing");
    for (int m = 0; m < M; m++) RTMI_ARG(std::isfinite(thetas[m]), "launch angles must be finite");
    rtmi_two_point_params q{};
    if (tp) q = *tp;
    const int A = q.max_arrivals ? q.max_arrivals : 4, K = q.max_crossings ? q.max_crossings : 4;
    const int max_iter = q.max_iter ? q.max_iter : 60;
    const double tol = q.tol != 0.0 ? q.tol : 1e-10;
    const int64_t budget = q.mem_budget ? q.mem_budget : (int64_t)8 << 30;
    RTMI_ARG(A >= 1 && A <= 64 && K >= 1 && K <= 64 && max_iter >= 1 && tol > 0 && budget > 0,
           "max_arrivals and max_crossings must be in [1, 64], max_iter >= 1, tol > 0, mem_budget > 0");
    RTMI_ARG((int64_t)S * M < (1ll << 31) && (int64_t)S * J * A < (1ll << 31), "too many rays");

    rtmi_two_point_stats st{};
    StreamGuard sg;
    RTMI_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    const hipStream_t strm = sg.s;
    rtmi_params pb = *p;
    pb.sort_rays = 0; pb.ext_s_ray = nullptr; pb.ext_n_ray = nullptr; pb.no_n_ray = 1; pb.lazy_clear = 0;
    DevMem mem;
    int32_t* dmax = nullptr;
    double *dth = nullptr, *dru = nullptr;
    RTMI_HIP(mem.get(&dmax, sizeof(int32_t)));
    RTMI_HIP(mem.get(&dth, (size_t)M * 8));
    RTMI_HIP(mem.get(&dru, (size_t)J * 8));
    RTMI_HIP(hipMemcpy(dth, thetas, (size_t)M * 8, hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(dru, receivers_u, (size_t)J * 8, hipMemcpyHostToDevice));

    // 1. the count pass: every source's fan without a record; its longest ray sizes the record
    auto t0 = std::chrono::steady_clock::now();
    std::vector<double> hx, hy, ht;
    try {
        hx.resize((size_t)S * M); hy.resize((size_t)S * M); ht.resize((size_t)S * M);
    } catch (const std::exception& e) {
        return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + e.what()).c_str());
    }
    for (int s = 0; s < S; s++)
        for (int m = 0; m < M; m++) { hx[(size_t)s * M + m] = sx[s]; hy[(size_t)s * M + m] = sy[s]; ht[(size_t)s * M + m] = thetas[m]; }
    int32_t fan_rows = 0;
    {
        rtmi_params pc = pb;
        pc.record_stride = 0; pc.rec_rows = 0;
        BatchGuard bc;
        RTMI_RC(rtmi_batch_create(f, &pc, (int64_t)S * M, hx.data(), hy.data(), ht.data(), (void*)strm, &bc.b));
        RTMI_RC(rtmi_run(bc.b));
        rtmi_device_view v;
        RTMI_RC(rtmi_batch_view(bc.b, &v));
        RTMI_HIP(hipMemsetAsync(dmax, 0, sizeof(int32_t), strm));
        hipLaunchKernelGGL(k_max_istep, blocks((long)v.R), dim3(256), 0, strm, v.istep, (long)v.R, dmax);
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(hipMemcpyAsync(&fan_rows, dmax, sizeof(int32_t), hipMemcpyDeviceToHost, strm));
        RTMI_HIP(hipStreamSynchronize(strm));
    }
    const int64_t rec_fan = (int64_t)fan_rows + 1;
    // refinement rays may run a little longer than any fan ray; those that run past the record are reported as truncated
    const int64_t rec_ref = std::min<int64_t>(p->max_size, rec_fan + rec_fan / 8 + 16);
    const int64_t per_src = 48 * std::max<int64_t>((int64_t)M * rec_fan, (int64_t)J * A * rec_ref);
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(S, budget / per_src));
    st.rec_rows = rec_fan;
    st.fan_ms += ms_since(t0);

    for (int s0 = 0; s0 < S; s0 += G) {
        const int Sg = std::min(G, S - s0);
        const long Rf = (long)Sg * M, NB = (long)Sg * J * A;
        DevMem gm;
        int32_t *fc = nullptr, *nslot = nullptr, *ms = nullptr, *rc = nullptr, *active = nullptr, *dcnt = nullptr, *dbad = nullptr;
        double *fcr = nullptr, *rcr = nullptr, *th = nullptr, *dout = nullptr;
        Bracket* br = nullptr;
        unsigned long long* dover = nullptr;
        RTMI_HIP(gm.get(&fc, Rf * 4)); RTMI_HIP(gm.get(&fcr, (size_t)K * 6 * Rf * 8));
        RTMI_HIP(gm.get(&nslot, (size_t)Sg * J * 4)); RTMI_HIP(gm.get(&br, NB * sizeof(Bracket)));
        RTMI_HIP(gm.get(&ms, NB * 4)); RTMI_HIP(gm.get(&th, NB * 8));
        RTMI_HIP(gm.get(&rc, NB * 4)); RTMI_HIP(gm.get(&rcr, (size_t)K * 6 * NB * 8));
        RTMI_HIP(gm.get(&active, 4)); RTMI_HIP(gm.get(&dover, 8));
        RTMI_HIP(gm.get(&dcnt, (size_t)Sg * J * 4)); RTMI_HIP(gm.get(&dbad, (size_t)Sg * J * 4)); RTMI_HIP(gm.get(&dout, NB * 9 * 8));

        // 2. the fan, recorded, and its crossings
        t0 = std::chrono::steady_clock::now();
        {
            rtmi_params pf = pb;
            pf.record_stride = 1; pf.rec_rows = rec_fan;
            BatchGuard bf;
            RTMI_RC(rtmi_batch_create(f, &pf, Rf, hx.data() + (size_t)s0 * M, hy.data() + (size_t)s0 * M, ht.data() + (size_t)s0 * M,
                                    (void*)strm, &bf.b));
            RTMI_RC(rtmi_run(bf.b));
            RTMI_RC(crossings_device(bf.b, L, K, fc, fcr, strm, who));
            RTMI_HIP(hipStreamSynchronize(strm));
        }
        st.fan_ms += ms_since(t0);

        // 3. brackets
        t0 = std::chrono::steady_clock::now();
        RTMI_HIP(hipMemsetAsync(nslot, 0, (size_t)Sg * J * 4, strm));
        RTMI_HIP(hipMemsetAsync(dover, 0, 8, strm));
        const long nt = (long)Sg * (M - 1) * K;
        hipLaunchKernelGGL(k_brackets, blocks(nt), dim3(256), 0, strm, fc, fcr, Rf, Sg, M, K, dth, dru, J, A, nslot,
                           br, dover);
        hipLaunchKernelGGL(k_sort_brackets, blocks(Sg * J), dim3(256), 0, strm, Sg * J, A, nslot, br, th, ms,
                           p->max_size);
        RTMI_HIP(hipGetLastError());
        unsigned long long over = 0;
        RTMI_HIP(hipMemcpyAsync(&over, dover, 8, hipMemcpyDeviceToHost, strm));
        RTMI_HIP(hipStreamSynchronize(strm));
        st.overflow += over;
        st.bracket_ms += ms_since(t0);

        // 4. refinement: one ray per bracket per iteration; brackets that are done get max_size 1 and take no step
        t0 = std::chrono::steady_clock::now();
        {
            rtmi_params pr = pb;
            pr.record_stride = 1; pr.rec_rows = rec_ref;
            pr.launch_mode = RTMI_LAUNCH_PLAIN;
            std::vector<double> hxr((size_t)NB), hyr((size_t)NB), htr((size_t)NB, 0.0);
            for (long t = 0; t < NB; t++) { hxr[t] = sx[s0 + t / ((long)J * A)]; hyr[t] = sy[s0 + t / ((long)J * A)]; }
            BatchGuard brt;
            RTMI_RC(rtmi_batch_create(f, &pr, NB, hxr.data(), hyr.data(), htr.data(), (void*)strm, &brt.b));
            int it = 0;
            for (; it < max_iter; it++) {
                RTMI_RC(rtmi_internal_relaunch(brt.b, th, ms));
                RTMI_RC(rtmi_run(brt.b));
                RTMI_RC(crossings_device(brt.b, L, K, rc, rcr, strm, who));
                RTMI_HIP(hipMemsetAsync(active, 0, 4, strm));
                hipLaunchKernelGGL(k_update, blocks(NB), dim3(256), 0, strm, NB, J, A, dru, rc, rcr, tol, br, th, ms,
                                   active);
                RTMI_HIP(hipGetLastError());
                int32_t h_active = 0;
                RTMI_HIP(hipMemcpyAsync(&h_active, active, 4, hipMemcpyDeviceToHost, strm));
                RTMI_HIP(hipStreamSynchronize(strm));
                if (h_active == 0) { it++; break; }
            }
            st.iterations = std::max(st.iterations, it);
        }
        st.refine_ms += ms_since(t0);

        // 5. output
        hipLaunchKernelGGL(k_output, blocks(Sg * J), dim3(256), 0, strm, Sg * J, A, br, dout, dcnt, dbad);
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(hipMemcpyAsync(arrivals + (size_t)s0 * J * A * 9, dout, NB * 9 * 8, hipMemcpyDeviceToHost, strm));
        RTMI_HIP(hipMemcpyAsync(count + (size_t)s0 * J, dcnt, (size_t)Sg * J * 4, hipMemcpyDeviceToHost, strm));
        RTMI_HIP(hipMemcpyAsync(nbad + (size_t)s0 * J, dbad, (size_t)Sg * J * 4, hipMemcpyDeviceToHost, strm));
        RTMI_HIP(hipStreamSynchronize(strm));
        st.groups++;
    }
    if (stats) *stats = st;
    return RTMI_OK;
}
