// paraxial.hip -- dynamic (paraxial) ray tracing along recorded rays (rtmi_paraxial): geometrical spreading, the caustic
// index and the ray amplitude of every ray, at the end of the ray and at its crossings of a receiver line; and the
// derivatives of the two gradient fits the kernel evaluates them with (rtmi_field_eval_dgrad).  DESIGN.md section 10.
//
// A post-pass over a batch's record, like k_crossings: one lane per ray walks its rows 0 .. last, reads x, y and theta of
// every row and looks the field up once per row (a step's end lookup is the next step's start lookup).  The lookup is the
// fast-form step methods' own cell polynomial (rt_polytab.h), differentiated: n from the bilinear part, g and its Jacobian
// from the two bicubics.  A wave whose lanes share one cell reads the cell's 36 coefficients through the scalar cache, as
// rt::PolyGather does; otherwise every lane reads its own.  Arithmetic is fp64 in one fixed order (-ffp-contract=off, sin/cos
// glibc's own through rt_libm.h) so that tests/paraxial_ref.py, a numpy restatement, follows it operation for operation.
// Batches are read through the public rtmi_batch_view; the field and the batch's parameters through two internal hooks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_crossing.h"
#include "rt_polytab.h"
#include "rt_rows.h"
#include "rtmi_host.h"

namespace {

constexpr int kCols = 7;        // Q1 P1 Q2 P2 J G kmah
constexpr int kStride = rt::kPolyStride;

// rtmi_internal_poly with the table typed (T: the field's dtype)
template <typename T> struct PolyF {
    const T* poly;
    long flat;
    int ncx, ncy;
    double ax, bx, inv_hx, ay, by, inv_hy;
};

// n, g = (dn/dx, dn/dy) and the Jacobian of g: gxy = d(dn/dx)/dy and so on
struct NG2 { double n, gx, gy, gxx, gxy, gyx, gyy; };
struct CellPos { int cell; double u, v; };

template <typename T> __device__ __forceinline__ CellPos locate(const PolyF<T>& F, double x, double y) {
    const rt::PolyPos c = rt::locate(F, F.ncx, F.ncy, x, y);
    return CellPos{c.jy * F.ncx + c.jx, c.u, c.v};
}

// The flat-cell map (rt::FieldDev::flat, rt_polytab.h): a flat cell's entry is its constant n, an ordinary cell's a NaN pattern
template <typename T> __device__ __forceinline__ bool flat_cell(const PolyF<T>& F, int cell, double& c) {
    if (!F.flat) return false;
    if constexpr (sizeof(T) == 8) {
        const unsigned long long b = reinterpret_cast<const unsigned long long*>(F.poly)[(long)cell - F.flat];
        if ((unsigned)(b >> 32) == 0xffffffffu) return false;
        c = __builtin_bit_cast(double, b);
    } else {
        const unsigned b = reinterpret_cast<const unsigned*>(F.poly)[(long)cell - F.flat];
        if (b == 0xffffffffu) return false;
        c = (double)__builtin_bit_cast(float, b);
    }
    return true;
}

// One cell's polynomials and their derivatives at (u, v).  ROW(k) yields row k's four coefficients (powers 0..3 of u) as fp64:
// rows 0-3 the d/dx spline (k the power of v), 4-7 the d/dy spline, 8 n's bilinear b0 + b1 u + b2 v + b3 u v.  Value and
// Horner order as rt::poly_bicubic / poly_bilinear (the same bits as the step kernels' lookup); d/du and d/dv by Horner too.
template <typename ROW> __device__ __forceinline__ NG2 eval_cell(ROW row, double u, double v, double ihx, double ihy) {
    double g[2], gu[2], gv[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        double r[4], dr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double4 a = row(4 * s + k);
            r[k] = __builtin_fma(__builtin_fma(__builtin_fma(a.w, u, a.z), u, a.y), u, a.x);
            dr[k] = __builtin_fma(__builtin_fma(3.0 * a.w, u, 2.0 * a.z), u, a.y);
        }
        g[s] = __builtin_fma(__builtin_fma(__builtin_fma(r[3], v, r[2]), v, r[1]), v, r[0]);
        gu[s] = __builtin_fma(__builtin_fma(__builtin_fma(dr[3], v, dr[2]), v, dr[1]), v, dr[0]);
        gv[s] = __builtin_fma(__builtin_fma(3.0 * r[3], v, 2.0 * r[2]), v, r[1]);
    }
    const double4 b = row(8);
    NG2 o;
    o.n = __builtin_fma(__builtin_fma(b.w, u, b.z), v, __builtin_fma(b.y, u, b.x));
    o.gx = g[0]; o.gy = g[1];
    o.gxx = gu[0] * ihx; o.gxy = gv[0] * ihy;
    o.gyx = gu[1] * ihx; o.gyy = gv[1] * ihy;
    return o;
}

template <typename T> using Quad = T __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ double4 widen(Quad<T> q) { return double4{(double)q.x, (double)q.y, (double)q.z, (double)q.w}; }

// The lookup at (x, y) of every lane that is executing.  Wave-uniform cell (the common case: neighbouring rays of a fan): the
// map entry and the 36 coefficients through the scalar cache; otherwise per-lane vector loads.  Same numbers, same arithmetic.
template <typename T> __device__ __forceinline__ NG2 lookup(const PolyF<T>& F, double x, double y) {
    const CellPos c = locate(F, x, y);
    double cf;
    const int cu = __builtin_amdgcn_readfirstlane(c.cell);
    if (__builtin_amdgcn_ballot_w64(c.cell != cu) == 0ull) {
        if (flat_cell(F, cu, cf)) return NG2{cf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        typedef const Quad<T> __attribute__((address_space(4)))* SP;
        SP p = (SP)(F.poly + (size_t)cu * kStride);
        asm volatile("" : "+s"(p));
        return eval_cell([&](int k) { return widen<T>(p[k]); }, c.u, c.v, F.inv_hx, F.inv_hy);
    }
    if (flat_cell(F, c.cell, cf)) return NG2{cf, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const Quad<T>* p = reinterpret_cast<const Quad<T>*>(F.poly + (size_t)c.cell * kStride);
    return eval_cell([&](int k) { return widen<T>(p[k]); }, c.u, c.v, F.inv_hx, F.inv_hy);
}

// K = n_ee - 2 n_e^2 / n for the ray normal e = (-sin theta, cos theta): dP/ds = K Q
__device__ __forceinline__ double kappa(const NG2& f, double c, double s) {
    const double ex = -s, ey = c;
    const double ne = f.gx * ex + f.gy * ey;
    const double nee = ex * (f.gxx * ex + f.gxy * ey) + ey * (f.gyx * ex + f.gyy * ey);
    return nee - 2.0 * ne * ne / f.n;
}

// The plane-wave (Q1, P1) and point-source (Q2, P2) solutions of dQ/ds = P / n, dP/ds = K Q
struct Tube { double q1, p1, q2, p2; };
// One step of length h, kick-drift-kick (Stormer-Verlet): ka, kb = K at its ends, wm = the mean of 1/n at its ends.  Each of
// the three updates is a shear, so the step's matrix has determinant 1 and Q1 P2 - Q2 P1 stays 1 to rounding.
__device__ __forceinline__ void kdk(Tube& t, double h, double ka, double kb, double wm) {
    const double a = 0.5 * h * ka, d = h * wm, b = 0.5 * h * kb;
    t.p1 = t.p1 + a * t.q1; t.p2 = t.p2 + a * t.q2;
    t.q1 = t.q1 + d * t.p1; t.q2 = t.q2 + d * t.p2;
    t.p1 = t.p1 + b * t.q1; t.p2 = t.p2 + b * t.q2;
}
// a caustic: Q2 changes sign (a row exactly at Q2 = 0 counts once, on the way in)
__device__ __forceinline__ int sign_change(double a, double b) { return ((a > 0.0 && b <= 0.0) || (a < 0.0 && b >= 0.0)) ? 1 : 0; }

// the 7 columns of one answer: Q1 P1 Q2 P2, J = n0 Q2, G = (n_r |J|)^-1/2, kmah
__device__ __forceinline__ void put(double* out, long R, long o, const Tube& t, double n0, double nr, int kmah) {
    const double J = n0 * t.q2;
    const double v[kCols] = {t.q1, t.p1, t.q2, t.p2, J, 1.0 / sqrt(nr * fabs(J)), (double)kmah};
#pragma unroll
    for (int q = 0; q < kCols; q++) out[(size_t)q * R + o] = v[q];
}
__device__ __forceinline__ void put_nan(double* out, long R, long o) {
#pragma unroll
    for (int q = 0; q < kCols; q++) out[(size_t)q * R + o] = NAN;
}

struct ParaxArgs {
    Line L;
    int has_line, kmax;
    int32_t* count;             // [R] or NULL
    double* at_line;            // [kmax][7][R] (has_line)
    double* at_end;             // [7][R]
    double* row_J;              // [rec_rows][R] or NULL: J after every row, slot order (rtmi_internal_paraxial_rows)
    int32_t* row_kmah;          // [rec_rows][R], with row_J
    double* row_tube;           // [rec_rows][5][R] or NULL: Q1 P1 Q2 P2 n after every row, slot order (rtmi_internal_paraxial_tube)
};

__device__ __forceinline__ void put_tube(double* out, long R, long i, long k, const Tube& t, double n) {
    double* p = out + (size_t)i * 5 * R + k;
    p[0] = t.q1; p[R] = t.p1; p[2 * R] = t.q2; p[3 * R] = t.p2; p[4 * R] = n;
}

// One lane per ray (slot k); answers in the caller's order.  A crossing of the line (the rule and tau* of rtmi_crossings) gets
// a partial step of length tau* L with K and 1/n interpolated linearly in tau along the step.
template <typename T> __global__ void k_paraxial(PolyF<T> F, Rows<T> rec, ParaxArgs A) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rec.R) return;
    const long R = rec.R;
    const long o = rec.caller(k);
    const size_t P = rec.pitch();
    const T* col = rec.row(0, k);
    const long last = A.row_tube ? rec.last_recorded(k) : rec.last(k);    // beams take a truncated ray's recorded rows
    const Line L = A.L;
    int n = 0;
    if (last >= rec.rec_rows) {
        n = -1;
        put_nan(A.at_end, R, o);
    } else {
        double x0 = (double)col[COL_X * R], y0 = (double)col[COL_Y * R];
        const double th0 = (double)col[COL_TH * R];
        double c0 = cos_g(th0), s0 = sin_g(th0);
        NG2 f = lookup(F, x0, y0);
        const double nsrc = f.n;
        double k0 = kappa(f, c0, s0), w0 = 1.0 / f.n, nl = f.n;
        double f0 = (L.a * x0 + L.b * y0) - L.c;
        Tube t{1.0, 0.0, 0.0, 1.0};
        int kmah = 0;
        if (A.row_J) { A.row_J[k] = nsrc * t.q2; A.row_kmah[k] = 0; }
        if (A.row_tube) put_tube(A.row_tube, R, 0, k, t, nsrc);
        // the next row's three loads go out a step ahead
        double xn = 0.0, yn = 0.0, tn = 0.0;
        if (last >= 1) { xn = (double)col[P]; yn = (double)col[P + COL_Y * R]; tn = (double)col[P + COL_TH * R]; }
        for (long i = 1; i <= last; i++) {
            const double x1 = xn, y1 = yn, th1 = tn;
            if (i < last) {
                const T* r = col + (size_t)(i + 1) * P;
                xn = (double)r[COL_X * R]; yn = (double)r[COL_Y * R]; tn = (double)r[COL_TH * R];
            }
            const double c1 = cos_g(th1), s1 = sin_g(th1);
            f = lookup(F, x1, y1);
            const double k1 = kappa(f, c1, s1), w1 = 1.0 / f.n;
            const double dx = x1 - x0, dy = y1 - y0;
            const double len = sqrt(dx * dx + dy * dy);
            if (A.has_line) {
                const double f1 = (L.a * x1 + L.b * y1) - L.c;
                if (crosses(f0, f1)) {
                    if (n < A.kmax) {
                        const double d0 = len * (L.a * c0 + L.b * s0), d1 = len * (L.a * c1 + L.b * s1);
                        const double tau = cross_tau(f0, d0, f1, d1);
                        const double kt = k0 + tau * (k1 - k0), wt = w0 + tau * (w1 - w0);
                        Tube u = t;
                        kdk(u, tau * len, k0, kt, 0.5 * (w0 + wt));
                        put(A.at_line + (size_t)n * kCols * R, R, o, u, nsrc, 1.0 / wt, kmah + sign_change(t.q2, u.q2));
                    }
                    n++;
                }
                f0 = f1;
            }
            const double q2 = t.q2;
            kdk(t, len, k0, k1, 0.5 * (w0 + w1));
            kmah += sign_change(q2, t.q2);
            if (A.row_J) { A.row_J[(size_t)i * R + k] = nsrc * t.q2; A.row_kmah[(size_t)i * R + k] = kmah; }
            if (A.row_tube) put_tube(A.row_tube, R, i, k, t, f.n);
            x0 = x1; y0 = y1; c0 = c1; s0 = s1; k0 = k1; w0 = w1; nl = f.n;
        }
        put(A.at_end, R, o, t, nsrc, nl, kmah);
    }
    if (A.count) A.count[o] = n;
    if (A.has_line)
        for (int c = n < 0 ? 0 : n; c < A.kmax; c++) put_nan(A.at_line + (size_t)c * kCols * R, R, o);
}

template <typename T> __global__ void k_field_dgrad(PolyF<T> F, long npts, const double* x, const double* y, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    const NG2 f = lookup(F, x[i], y[i]);
    out[i] = f.gxx;
    out[npts + i] = f.gxy;
    out[2 * npts + i] = f.gyx;
    out[3 * npts + i] = f.gyy;
}

template <typename T> PolyF<T> poly_f(const rtmi_internal_poly& v) {
    return PolyF<T>{(const T*)v.poly, v.flat, v.ncx, v.ncy, v.ax, v.bx, v.inv_hx, v.ay, v.by, v.inv_hy};
}

// k_paraxial on a batch's rows
int launch(const char* who, const Recorded& r, const ParaxArgs& a) {
    by_dtype(r.v.dtype, [&](auto t) {
        hipLaunchKernelGGL(k_paraxial<decltype(t)>, blocks((long)r.v.R), dim3(256), 0, nullptr, poly_f<decltype(t)>(r.poly), rows_of<decltype(t)>(r.v), a);
    });
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}
constexpr unsigned kNeeds = kRecIsotropic | kRecPoly | kRecFromLaunch;

}  // namespace

RTMI_EXPORT int rtmi_paraxial(rtmi_batch* b, const double line[3], int32_t kmax, int32_t* count, double* at_line, double* at_end) {
    const char* who = "rtmi_paraxial";
    RTMI_ARG(b && at_end, "null");
    Line L{0.0, 0.0, 0.0};
    if (line) {
        RTMI_ARG(count && at_line, "a line needs count and at_line");
        RTMI_ARG(kmax >= 1, "kmax must be >= 1");
        RTMI_ARG(make_line(line, &L), "the line needs (a, b) != (0, 0) and finite coefficients");
    }
    Recorded r;
    RTMI_RC(recorded(who, b, kNeeds, 0, &r));
    const size_t R = (size_t)r.v.R;
    const int K = line ? kmax : 0;
    DevMem mem;
    int32_t* dc = nullptr;
    double *dl = nullptr, *de = nullptr;
    RTMI_HIP(mem.get(&dc, R * sizeof(int32_t)));
    RTMI_HIP(mem.get(&de, (size_t)kCols * R * sizeof(double)));
    if (K) RTMI_HIP(mem.get(&dl, (size_t)K * kCols * R * sizeof(double)));
    RTMI_RC(launch(who, r, ParaxArgs{L, line ? 1 : 0, K, dc, dl, de, nullptr, nullptr, nullptr}));
    RTMI_HIP(hipMemcpy(at_end, de, (size_t)kCols * R * sizeof(double), hipMemcpyDeviceToHost));
    if (count) RTMI_HIP(hipMemcpy(count, dc, R * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (K) RTMI_HIP(hipMemcpy(at_line, dl, (size_t)K * kCols * R * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

namespace {
// rtmi_paraxial's kernel with its per-row outputs (row_J and row_kmah, or row_tube) into DEVICE buffers; rtmi_paraxial's checks
int paraxial_rows(const char* who, rtmi_batch* b, double* row_J, int32_t* row_kmah, double* row_tube) {
    Recorded r;
    RTMI_RC(recorded(who, b, kNeeds, 0, &r));
    DevMem mem;
    double* de = nullptr;
    RTMI_HIP(mem.get(&de, (size_t)kCols * (size_t)r.v.R * sizeof(double)));
    RTMI_RC(launch(who, r, ParaxArgs{Line{0.0, 0.0, 0.0}, 0, 0, nullptr, nullptr, de, row_J, row_kmah, row_tube}));
    RTMI_HIP(hipDeviceSynchronize());
    return RTMI_OK;
}
}  // namespace

// J = n0 Q2 and kmah after every recorded row of every ray, into DEVICE buffers of the batch's device ([rec_rows][R], slot order;
// rows past a ray's last row are left as they were).  The J of a ray's last row is rtmi_paraxial's at_end J, bit for bit: the
// same kernel with the same arithmetic, storing what it carries.  The checks are rtmi_paraxial's, under the caller's name.
int rtmi_internal_paraxial_rows(const char* who, rtmi_batch* b, double* row_J, int32_t* row_kmah) {
    RTMI_ARG(b && row_J && row_kmah, "null");
    return paraxial_rows(who, b, row_J, row_kmah, nullptr);
}

// Q1 P1 Q2 P2 and n after every recorded row ([rec_rows][5][R], slot order), the same kernel storing what it carries; a ray
// that runs past rec_rows is walked over its recorded rows.  For the Gaussian beams (beams.hip).
int rtmi_internal_paraxial_tube(const char* who, rtmi_batch* b, double* row_tube) {
    RTMI_ARG(b && row_tube, "null");
    return paraxial_rows(who, b, nullptr, nullptr, row_tube);
}

RTMI_EXPORT int rtmi_debug_paraxial_rows(rtmi_batch* b, double* J, int32_t* kmah) {
    const char* who = "rtmi_debug_paraxial_rows";
    RTMI_ARG(b && J && kmah, "null");
    rtmi_device_view v;
    RTMI_RC(rtmi_batch_view(b, &v));
    const size_t R = (size_t)v.R, n = (size_t)v.rec_rows * R;
    DevMem mem;
    double* dj = nullptr;
    int32_t* dk = nullptr;
    RTMI_HIP(mem.get(&dj, n * sizeof(double)));
    RTMI_HIP(mem.get(&dk, n * sizeof(int32_t)));
    RTMI_HIP(hipMemset(dj, 0xff, n * sizeof(double)));
    RTMI_HIP(hipMemset(dk, 0xff, n * sizeof(int32_t)));
    RTMI_RC(rtmi_internal_paraxial_rows(who, b, dj, dk));
    std::vector<double> hj(n);
    std::vector<int32_t> hk(n), perm(v.perm ? R : 0);
    RTMI_HIP(hipMemcpy(hj.data(), dj, n * sizeof(double), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(hk.data(), dk, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (v.perm) RTMI_HIP(hipMemcpy(perm.data(), v.perm, R * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)v.rec_rows; i++)
        for (size_t k = 0; k < R; k++) {
            const size_t o = v.perm ? (size_t)perm[k] : k;
            J[i * R + o] = hj[i * R + k];
            kmah[i * R + o] = hk[i * R + k];
        }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_field_eval_dgrad(const rtmi_field* f, int64_t npts, const double* x, const double* y, double* gx_x,
                                      double* gx_y, double* gy_x, double* gy_y) {
    const char* who = "rtmi_field_eval_dgrad";
    RTMI_ARG(f && x && y && gx_x && gx_y && gy_x && gy_y, "null");
    RTMI_ARG(npts >= 0, "npts < 0");
    rtmi_internal_poly pv;
    RTMI_RC(rtmi_internal_field_poly(f, &pv));
    if (npts == 0) return RTMI_OK;
    const size_t nb = (size_t)npts * sizeof(double);
    DevMem mem;
    double* d = nullptr;
    RTMI_HIP(mem.get(&d, 6 * nb));
    RTMI_HIP(hipMemcpy(d, x, nb, hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(d + npts, y, nb, hipMemcpyHostToDevice));
    const dim3 g = blocks(npts), blk(256);
    by_dtype(pv.dtype, [&](auto t) {
        hipLaunchKernelGGL(k_field_dgrad<decltype(t)>, g, blk, 0, nullptr, poly_f<decltype(t)>(pv), (long)npts, d, d + npts, d + 2 * npts);
    });
    RTMI_HIP(hipGetLastError());
    double* outs[4] = {gx_x, gx_y, gy_x, gy_y};
    for (int q = 0; q < 4; q++) RTMI_HIP(hipMemcpy(outs[q], d + (2 + q) * npts, nb, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
