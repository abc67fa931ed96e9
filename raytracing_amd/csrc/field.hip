// field.hip -- the field build of librtmi.so: a scenario's (or the caller's) samples of n on a regular grid, their gradients, the
// FITPACK fit behind the reference's RectBivariateSpline, and the arrays and per-cell polynomial table (rt_polytab.h) the step
// kernels look up.  Runs once per field; the lookups themselves are rtmi.hip's (rt_device.h belongs to that unit alone, DESIGN.md
// section 16).  Reference lines are RT_bench.py file:line of neyuru/RayTracing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "rt_np_exp.h"
#include "rt_polytab.h"
#include "rtmi_field.h"

// Steep cells (k_polytab): lambda * (the grid's shorter side) >= kSteepRate.  40: the interface scenario's sigmoid (lambda up
// to 36 on a 12 x 28 grid) has a band of them 0.07 wide; the fisheye (lambda <= 2, 9 x 9) and vert_heterogeneous (0.2) have none.
constexpr double kSteepRate = 40.0;

// ================================================================== field build kernels (fp64)
// np.exp on a float64 array as the reference's numpy evaluates it (RT_bench.py:107 calls it on the meshgrid): on the
// AVX512 machines numpy's wheels dispatch to Intel SVML's __svml_exp8_ha (numpy/_core/src/umath/svml, BSD-3), which is not
// libm's exp in the last bit for 4.5 % of arguments.  The routine's main path restated (oracle/rt_oracle.c np_exp has the
// same text; tools/check_np_exp.py: 0 mismatches against np.exp on 2.6e7 arguments): N = floor(x*log2(e)*16)/16 -- an fma
// rounded toward zero onto a 2^-4 grid -- r = x - N*ln2 in two pieces, a degree-6 polynomial in three interleaved pairs,
// 2^(j/16) from a 16-entry table with its correction term, scaled by 2^floor(N).  |x| >= 707.7 (SVML's scalar fall-back):
// ocml's exp -- there 1 + e rounds to e or to 1 and the interface's n is sqrt(2) or 1 whatever the last bits of e.
// The main path is rt_np_exp.h's, one text with the host's and with rt_edt.h's.
// On the device: tests/test_gpu_elementary.py (rtmi_debug_exp, below) -- the oracle's bits on 2.6e6 main-path arguments.
__device__ static double np_exp(double x) {
    if (!(fabs(x) < 0x1.61da04cbafe44p+9)) return exp(x);
    return rt::np_exp_main(x, rt::np_exp_tables());
}

__device__ static double scenario_n(int sc, double a, double b) {
    if (sc == RTMI_INTERFACE)  // :107 (exp overflows to inf for y < -3.55, result sqrt(2): same as numpy)
        return __dsqrt_rn(2.0) - (__dsqrt_rn(2.0) - 1.0) / (1.0 + np_exp(-b / 0.005));
    if (sc == RTMI_FISHEYE)    // :111
        return 1.0 / (1.0 + a * a + b * b);
    return 1.0 / (18.0 + 2.0 * b);  // :115-116
}

// element i of numpy.linspace(a, b, q) with step h (linspace() below, on the device)
__device__ static double axis_at(int i, int q, double a, double h, double b) { return i >= q - 1 ? b : (double)i * h + a; }

__global__ void k_sample(int sc, double* Z, int qx, int qy, double ax, double hx, double bx, double ay, double hy,
                         double by) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= qx || i >= qy) return;
    const double x = axis_at(j, qx, ax, hx, bx), y = axis_at(i, qy, ay, hy, by);
    Z[(size_t)i * qx + j] = scenario_n(sc, x, y);  // meshgrid X[i,j]=x[j], Y[i,j]=y[i] (:430-432)
}

// np.gradient(Z, delta, edge_order=2) along one axis (:450); numpy's evaluation order (contraction is off).
__global__ void k_gradient(const double* Z, double* out, int qx, int qy, int axis, double dx) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= qx || i >= qy) return;
    const int n = axis == 0 ? qy : qx, p = axis == 0 ? i : j;
    const long s = axis == 0 ? qx : 1;
    const double* c = Z + (size_t)i * qx + j;
    double r;
    if (p == 0) {
        r = (-1.5 / dx) * c[0] + (2.0 / dx) * c[s] + (-0.5 / dx) * c[2 * s];
    } else if (p == n - 1) {
        r = (0.5 / dx) * c[-2 * s] + (-2.0 / dx) * c[-s] + (1.5 / dx) * c[0];
    } else {
        r = (c[s] - c[-s]) / (2.0 * dx);
    }
    out[(size_t)i * qx + j] = r;
}

// FITPACK regrid with s = 0 (fpregr.f -> fpgrre.f, p = -1), the fit behind RectBivariateSpline (:456-457): the
// interpolating spline's coefficients as the least-squares solution of (spy) c (spx)' = z by Givens rotations.  Each data
// row of an axis' observation matrix is rotated into a band triangle (fpgivs / fprota); the rotations depend on the axis
// alone, so the host works them out once per axis (fp_axis_build) and the device applies them to all right-hand sides at
// once -- first along FITPACK's x (the rows of our [qy][qx] arrays: the reference passes (y, x, Z)), then along its y --
// followed by the two back substitutions (fpback).  Same operations in the same order as the Fortran (scipy's wheels carry
// no FMA; this library is compiled with -ffp-contract=off), so the coefficient arrays are scipy's get_coeffs() bit for bit
// -- where rounds 1-2's banded LU of the same system landed 1.3e-15 away, enough to move interface x op3/4/5 by 2e-7.
//
// k_givens: lane = one right-hand side (stride ls), it = data rows of the axis (stride is).  Data row it touches triangle
// rows nr[it] .. nr[it]+3; nr never decreases and a triangle row is final once nr has passed it, so the four live rows
// are a register window: no read-modify-write of memory at all (out starts as the zero matrix of the Fortran).
__global__ void k_givens(const double* in, double* out, int m, int nlines, long is, long ls, const int* nr, const double* cs) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlines) return;
    const double* src = in + (size_t)t * ls;
    double* dst = out + (size_t)t * ls;
    double w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    int base = 0;
    for (int it = 0; it < m; it++) {
        for (const int number = nr[it]; base < number; ++base) {
            dst[(size_t)base * is] = w0;
            w0 = w1; w1 = w2; w2 = w3; w3 = 0;
        }
        double right = src[(size_t)it * is];
        const double* r = cs + (size_t)it * 8;
#define RT_ROTA_(W, I)                                                                  \
        if (!(r[2 * I] == 0.0 && r[2 * I + 1] == 0.0)) {   /* (0, 0): piv == 0, no rotation */ \
            const double c = r[2 * I], sn = r[2 * I + 1], s1 = right, s2 = W;               \
            W = c * s2 + sn * s1;        /* fprota: b = cos*b + sin*a */                    \
            right = c * s1 - sn * s2;    /*         a = cos*a - sin*b */                    \
        }
        RT_ROTA_(w0, 0) RT_ROTA_(w1, 1) RT_ROTA_(w2, 2) RT_ROTA_(w3, 3)
#undef RT_ROTA_
    }
    if (base < m) dst[(size_t)base * is] = w0;
    if (base + 1 < m) dst[(size_t)(base + 1) * is] = w1;
    if (base + 2 < m) dst[(size_t)(base + 2) * is] = w2;
    if (base + 3 < m) dst[(size_t)(base + 3) * is] = w3;
}
// fpback with bandwidth 4: a[n][4] is the band triangle; one line (stride ls) per lane, elements es apart
__global__ void k_fpback(double* d, int n, int nlines, long es, long ls, const double* a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlines) return;
    double* z = d + (size_t)t * ls;
    double c1 = z[(size_t)(n - 1) * es] / a[(size_t)(n - 1) * 4], c2 = 0, c3 = 0;   // c[i+1], c[i+2], c[i+3]
    z[(size_t)(n - 1) * es] = c1;
    for (int i = n - 2, j = 2; i >= 0; i--, j++) {
        const double* ai = a + (size_t)i * 4;
        double store = z[(size_t)i * es];
        store = store - c1 * ai[1];
        if (j > 2) store = store - c2 * ai[2];
        if (j > 3) store = store - c3 * ai[3];
        const double v = store / ai[0];
        z[(size_t)i * es] = v;
        c3 = c2; c2 = c1; c1 = v;
    }
}

template <typename T> __global__ void k_pack(const double* Z, const double* cdy, const double* cdx, T* zn, T* g, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    zn[i] = (T)Z[i];
    g[2 * i] = (T)cdx[i];      // d/dx spline = grd[1] (:154)
    g[2 * i + 1] = (T)cdy[i];  // d/dy spline = grd[0] (:155)
}

// The per-cell polynomial table (rt_polytab.h): one thread per cell, fp64 conversion, stored in the field's dtype; and the
// flat-cell map in front of it (rt::poly_cell_flat; thr from the grid's largest gradient-spline coefficient, k_absmax).
// A cell's STEEPNESS lambda = sqrt(max |Hessian of n| / min n) over its four corners, from the cell's own polynomials: the
// gradient splines' first derivatives (d/du, d/dv of both, scaled to x and y) are the Hessian the reference's field has there;
// its infinity norm bounds |w' H w| for every unit w.  A ray that runs along the iso-lines of a transition drifts away from
// its neighbours like exp(lambda s) on the side where n curves upwards: lambda = 36 per unit length in the interface scenario's
// sigmoid, 2 at most in the fisheye, 0.2 in vert_heterogeneous.  Kept (as float bits in the map entry's low word, fp64 fields
// only) when lambda >= lam0 = kSteepRate / (the grid's shorter side): a transition sharp against the size of the scene.
template <typename T>
__global__ void k_polytab(const double* Z, const double* cdx, const double* cdy, int qx, int qy, const double* Cx, const double* Lx,
                          const double* Cy, const double* Ly, T* out, T* flatn, const unsigned long long* gmax_bits,
                          unsigned long long* nflat, double inv_hx, double inv_hy, double lam0) {
    const int jx = blockIdx.x * blockDim.x + threadIdx.x, jy = blockIdx.y;
    bool flat = false, steep = false;
    if (jx < qx - 1 && jy < qy - 1) {
        double c[36];
        rt::poly_cell_convert(Z, cdx, cdy, qx, qy, jx, jy, Cx, Lx, Cy, Ly, c);
        const size_t cell = (size_t)jy * (qx - 1) + jx;
        T* o = out + cell * rt::kPolyStride;
        for (int i = 0; i < 36; i++) o[i] = (T)c[i];
        for (int i = 36; i < rt::kPolyStride; i++) o[i] = T(0);
        flat = rt::poly_cell_flat(c, __builtin_bit_cast(double, *gmax_bits) * rt::kPolyFlatRel);
        typedef typename rt::FlatBits<T>::type B;
        B entry = flat ? __builtin_bit_cast(B, (T)c[32]) : ~(B)0;
        if constexpr (sizeof(T) == 8) {
            if (!flat) {
                double hmax = 0.0, nmin = INFINITY;
                for (int corner = 0; corner < 4; corner++) {
                    const double u = corner & 1, v = corner >> 1;
                    double H[2][2];     // [spline s: 0 = dn/dx, 1 = dn/dy][0: d/dx, 1: d/dy]
                    for (int sp = 0; sp < 2; sp++) {
                        const double* A = c + 16 * sp;      // A[4k + p]: u^p v^k
                        double du = 0.0, dv = 0.0, vk = 1.0;
                        for (int k = 0; k < 4; k++) {
                            du += vk * (A[4 * k + 1] + u * (2.0 * A[4 * k + 2] + u * 3.0 * A[4 * k + 3]));
                            vk *= v;
                        }
                        double up = 1.0;
                        for (int pq = 0; pq < 4; pq++) {
                            dv += up * (A[4 + pq] + v * (2.0 * A[8 + pq] + v * 3.0 * A[12 + pq]));
                            up *= u;
                        }
                        H[sp][0] = du * inv_hx; H[sp][1] = dv * inv_hy;
                    }
                    hmax = fmax(hmax, fmax(fabs(H[0][0]) + fabs(H[0][1]), fabs(H[1][0]) + fabs(H[1][1])));
                    nmin = fmin(nmin, c[32] + u * c[33] + v * c[34] + u * v * c[35]);
                }
                const double lam = nmin > 0.0 ? sqrt(hmax / nmin) : 0.0;
                steep = lam >= lam0 && lam < 3.0e38;
                entry = rt::steep_entry_bits(steep ? (float)lam : 0.f);
            }
        }
        reinterpret_cast<B*>(flatn)[cell] = entry;
    }
    const unsigned long long votes = rt_ballot(flat), svotes = rt_ballot(steep);                 // one atomic per wave
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(nflat, (unsigned long long)__popcll(votes));
    if ((threadIdx.x & 63) == 0 && svotes) atomicAdd(nflat + 1, (unsigned long long)__popcll(svotes));
}
// x-invariant ("layered") fields (rt_device.h, "the lookup by depth alone"; include/rtmi.h).  k_layered_check counts the cells
// that break the rule's conditions: a sample of the cell's corners whose bit pattern differs from its row's first (exact, no
// tolerance), or residue the rule would drop that is not small -- a coefficient of the d/dx polynomial or a u-dependent one of
// the d/dy polynomial beyond 2^-40 of the grid's largest gradient-spline coefficient, a u-dependent one of n's beyond 2^-40 of
// its constant term (a NaN fails every comparison).  Reads the finished table.
constexpr double kLayerRel = 0x1p-40;
template <typename T>
__global__ void k_layered_check(const double* Z, int qx, int qy, const T* poly, const unsigned long long* gmax_bits, unsigned long long* nbad) {
    const int jx = blockIdx.x * blockDim.x + threadIdx.x, jy = blockIdx.y;
    bool bad = false;
    if (jx < qx - 1 && jy < qy - 1) {
        const unsigned long long* r0 = reinterpret_cast<const unsigned long long*>(Z) + (size_t)jy * qx;
        const unsigned long long* r1 = r0 + qx;
        bad = r0[jx] != r0[0] || r0[jx + 1] != r0[0] || r1[jx] != r1[0] || r1[jx + 1] != r1[0];
        const T* c = poly + ((size_t)jy * (qx - 1) + jx) * rt::kPolyStride;
        const double thr = __builtin_bit_cast(double, *gmax_bits) * kLayerRel;
        for (int i = 0; i < 16; i++) bad = bad || !(fabs((double)c[i]) <= thr);
        for (int k = 0; k < 4; k++)
            for (int p = 1; p < 4; p++) bad = bad || !(fabs((double)c[16 + 4 * k + p]) <= thr);
        const double tn = fabs((double)c[32]) * kLayerRel;
        bad = bad || !(fabs((double)c[33]) <= tn) || !(fabs((double)c[35]) <= tn);
    }
    const unsigned long long votes = rt_ballot(bad);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(nbad, (unsigned long long)__popcll(votes));
}
// The row table of a layered field: row jy's {g0, g1, g2, g3, b0, b2, 0, 0} -- the u-free coefficients of cell (ncx / 2, jy), the
// table's own bits -- rt::kLayerStride * (jy + 1) elements in front of the table (rt::layer_row).
template <typename T> __global__ void k_layered_rows(T* poly, int ncx, int ncy) {
    const int jy = blockIdx.x * blockDim.x + threadIdx.x;
    if (jy >= ncy) return;
    const T* c = poly + ((size_t)jy * ncx + ncx / 2) * rt::kPolyStride;
    T* o = poly - (size_t)rt::kLayerStride * ((size_t)jy + 1);
    o[0] = c[16]; o[1] = c[20]; o[2] = c[24]; o[3] = c[28];
    o[4] = c[32]; o[5] = c[34]; o[6] = T(0); o[7] = T(0);
}
// max |v| over two arrays as the bit pattern of a non-negative double (ordered like the integers)
__global__ void k_absmax(const double* a, const double* b, size_t n, unsigned long long* out) {
    unsigned long long m = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, fabs(a[i])), v = __builtin_bit_cast(unsigned long long, fabs(b[i]));
        m = u > m ? u : m;
        m = v > m ? v : m;                    // (a NaN coefficient orders above everything: no cell is flat then)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(m, o, 64); m = w > m ? w : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// ------------------------------------------------------------------ host side of the field build
namespace {
// FITPACK fpbspl (k=3) on the host, for the collocation matrix only.
void host_bspl3(const std::vector<double>& t, double x, int l, double h[4]) {
    double hh[4];
    h[0] = 1.0;
    for (int j = 1; j <= 3; j++) {
        for (int i = 0; i < j; i++) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 0; i < j; i++) {
            const int li = l + 1 + i, lj = li - j;
            const double f = hh[i] / (t[li] - t[lj]);
            h[i] = h[i] + f * (t[li] - x);
            h[i + 1] = f * (x - t[lj]);
        }
    }
}
// One axis of fpgrre: the Givens rotations that take the axis' observation matrix (one cubic B-spline row per data point,
// interpolating not-a-knot knots t = [x0 x4, x[2..m-3], x[m-1] x4]) to its band triangle.  Out: nr[it] = first triangle row
// data row it touches, cs[it][i] = (cos, sin) of its i-th rotation ((0, 0): none, the pivot was zero), a[m][4] the triangle.
struct FpAxis { std::vector<int> nr; std::vector<double> cs, a; };
FpAxis fp_axis_build(const std::vector<double>& x) {
    const int m = (int)x.size();
    std::vector<double> t(m + 4);
    for (int i = 0; i <= 3; i++) { t[i] = x[0]; t[m + 3 - i] = x[m - 1]; }
    for (int i = 4, j = 2; i < m; i++, j++) t[i] = x[j];
    FpAxis A;
    A.nr.assign(m, 0); A.cs.assign((size_t)m * 8, 0.0); A.a.assign((size_t)m * 4, 0.0);
    int l = 3, number = 0;
    for (int it = 0; it < m; it++) {
        while (!(x[it] < t[l + 1] || l == m - 1)) { l++; number++; }
        double h[4];
        host_bspl3(t, x[it], l, h);
        A.nr[it] = number;
        for (int i = 0, irot = number; i < 4; i++, irot++) {
            const double piv = h[i];
            if (piv == 0.0) continue;
            double& ww = A.a[(size_t)irot * 4];
            const double store = std::fabs(piv);                 // fpgivs
            double dd;
            if (store >= ww) { const double q = ww / piv; dd = store * std::sqrt(1.0 + q * q); }
            else { const double q = piv / ww; dd = ww * std::sqrt(1.0 + q * q); }
            const double c = ww / dd, sn = piv / dd;
            ww = dd;
            A.cs[(size_t)it * 8 + 2 * i] = c; A.cs[(size_t)it * 8 + 2 * i + 1] = sn;
            for (int j = i + 1, i2 = 1; j < 4; j++, i2++) {      // fprota on the rest of the row
                const double s1 = h[j], s2 = A.a[(size_t)irot * 4 + i2];
                A.a[(size_t)irot * 4 + i2] = c * s2 + sn * s1;
                h[j] = c * s1 - sn * s2;
            }
        }
    }
    return A;
}
// Per cell index j of an axis, rt::ex::kAxisTab = 24 doubles (rt::ex::AxisTab): the correctly rounded reciprocals of the seven knot
// differences rt::ex::axis_exact divides by (same knots by the same operations as the device forms them: x is numpy.linspace as
// linspace() below restates it; then an IEEE division) -- 1/(x[j+1]-x[j]), 1/(k1-k0), 1/(k1-tm1), 1/(k2-k0), 1/(k1-tm2),
// 1/(k2-tm1), 1/(k3-k0), 0 -- then x[j], x[j+1], the six knots tm2 .. k3 and the seven differences (and a 0) in the same order.
std::vector<double> fp_axis_tab_build(const std::vector<double>& x) {
    constexpr int S = rt::ex::kAxisTab;
    const int m = (int)x.size();
    std::vector<double> out((size_t)m * S, 0.0);
    auto knot = [&](int l) { return l <= 3 ? x[0] : (l >= m ? x[m - 1] : x[l - 2]); };   // rt::knot3
    for (int j = 0; j < m - 1; j++) {
        int l = j + 2;
        l = l < 3 ? 3 : (l > m - 1 ? m - 1 : l);
        const double tm2 = knot(l - 2), tm1 = knot(l - 1), k0 = knot(l), k1 = knot(l + 1), k2 = knot(l + 2), k3 = knot(l + 3);
        double* o = &out[(size_t)j * S];
        const double d[7] = {x[j + 1] - x[j], k1 - k0, k1 - tm1, k2 - k0, k1 - tm2, k2 - tm1, k3 - k0};
        for (int i = 0; i < 7; i++) { o[i] = 1.0 / d[i]; o[16 + i] = d[i]; }
        o[8] = x[j]; o[9] = x[j + 1];
        o[10] = tm2; o[11] = tm1; o[12] = k0; o[13] = k1; o[14] = k2; o[15] = k3;
    }
    for (int i = 0; i < S; i++) out[(size_t)(m - 1) * S + i] = out[(size_t)(m - 2) * S + i];
    return out;
}
std::vector<double> linspace(double a, double b, int n) {
    std::vector<double> v(n);
    const double step = (b - a) / (double)(n - 1);
    for (int i = 0; i < n; i++) v[i] = (double)i * step + a;
    v[n - 1] = b;
    return v;
}
}  // namespace

// `work`: the call's device buffers (field_finish frees them once nothing can still read them)
static int field_finish_impl(const char* who, rtmi_field* f, double delta, DevMem& work) {
    const int qx = f->qx, qy = f->qy;
    const size_t nz = (size_t)qx * qy;
    hipStream_t st = f->stream;
    RTMI_HIP(hipMalloc(&f->dCdy, nz * sizeof(double)));
    RTMI_HIP(hipMalloc(&f->dCdx, nz * sizeof(double)));
    dim3 blk(256), grd((qx + 255) / 256, qy);
    hipLaunchKernelGGL(k_gradient, grd, blk, 0, st, f->dZ, f->dCdy, qx, qy, 0, delta);  // GradX = d/dy (Q2)
    hipLaunchKernelGGL(k_gradient, grd, blk, 0, st, f->dZ, f->dCdx, qx, qy, 1, delta);  // GradY = d/dx
    RTMI_HIP(hipGetLastError());
    // RectBivariateSpline(y, x, Grad) (:456-457) = FITPACK regrid, s = 0: Givens QR along y (FITPACK's x), then along x
    const FpAxis AX = fp_axis_build(linspace(f->ax, f->bx, qx));
    const FpAxis AY = fp_axis_build(linspace(f->ay, f->by, qy));
    double* dlux = nullptr;     // rotations + triangles of both axes
    double* g = nullptr;        // the work matrix
    const size_t nax = (size_t)qx * 12, nay = (size_t)qy * 12;                 // cs [m][8] + a [m][4]
    RTMI_HIP(work.get(&dlux, (nax + nay) * sizeof(double) + (size_t)(qx + qy) * sizeof(int)));
    RTMI_HIP(work.get(&g, nz * sizeof(double)));
    double *csx = dlux, *ax4 = dlux + (size_t)qx * 8, *csy = dlux + nax, *ay4 = csy + (size_t)qy * 8;
    int *nrx = (int*)(dlux + nax + nay), *nry = nrx + qx;
    RTMI_HIP(hipMemcpyAsync(csx, AX.cs.data(), (size_t)qx * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(ax4, AX.a.data(), (size_t)qx * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(csy, AY.cs.data(), (size_t)qy * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(ay4, AY.a.data(), (size_t)qy * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(nrx, AX.nr.data(), (size_t)qx * sizeof(int), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(nry, AY.nr.data(), (size_t)qy * sizeof(int), hipMemcpyHostToDevice, st));
    for (double* c : {f->dCdy, f->dCdx}) {
        // rows of z into FITPACK-x's triangle (one lane per column), columns of g into FITPACK-y's (one lane per row)
        hipLaunchKernelGGL(k_givens, dim3((qx + 63) / 64), dim3(64), 0, st, c, g, qy, qx, (long)qx, 1L, nry, csy);
        hipLaunchKernelGGL(k_givens, dim3((qy + 63) / 64), dim3(64), 0, st, g, c, qx, qy, 1L, (long)qx, nrx, csx);
        // (ry) c1 = h along x for every row, then c (rx)' = c1 along y for every column
        hipLaunchKernelGGL(k_fpback, dim3((qy + 63) / 64), dim3(64), 0, st, c, qx, qy, 1L, (long)qx, ax4);
        hipLaunchKernelGGL(k_fpback, dim3((qx + 63) / 64), dim3(64), 0, st, c, qy, qx, (long)qx, 1L, ay4);
    }
    RTMI_HIP(hipGetLastError());
    const bool f64 = f->dtype == RTMI_F64;
    const size_t esz = f64 ? 8 : 4;
    RTMI_HIP(hipMalloc(&f->zn, nz * esz));
    RTMI_HIP(hipMalloc(&f->g, 2 * nz * esz));
    by_dtype(f->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_pack<T>, blocks((long)nz), dim3(256), 0, st, f->dZ, f->dCdy, f->dCdx, (T*)f->zn, (T*)f->g, nz);
    });
    RTMI_HIP(hipGetLastError());
    {   // reciprocals of the knot differences for the reference-order lookup (rt_exact.h)
        const std::vector<double> RX = fp_axis_tab_build(linspace(f->ax, f->bx, qx)), RY = fp_axis_tab_build(linspace(f->ay, f->by, qy));
        RTMI_HIP(hipMalloc(&f->rdiv, (RX.size() + RY.size()) * sizeof(double)));
        RTMI_HIP(hipMemcpyAsync(f->rdiv, RX.data(), RX.size() * sizeof(double), hipMemcpyHostToDevice, st));
        RTMI_HIP(hipMemcpyAsync(f->rdiv + RX.size(), RY.data(), RY.size() * sizeof(double), hipMemcpyHostToDevice, st));
        RTMI_HIP(hipStreamSynchronize(st));  // the host vectors go out of scope
    }
    // one polynomial per cell for the fast-form lookups: per-axis basis tables on the host (long double), cells on the device
    const double ihx = f64 ? 1.0 / f->hx : (double)(float)(1.0 / f->hx);
    const double ihy = f64 ? 1.0 / f->hy : (double)(float)(1.0 / f->hy);
    const rt::PolyAxis PX = rt::poly_axis_build(linspace(f->ax, f->bx, qx), f64 ? f->ax : (double)(float)f->ax, ihx);
    const rt::PolyAxis PY = rt::poly_axis_build(linspace(f->ay, f->by, qy), f64 ? f->ay : (double)(float)f->ay, ihy);
    const size_t ncell = (size_t)(qx - 1) * (qy - 1);
    const size_t nax2 = (size_t)(qx - 1) * 20, nay2 = (size_t)(qy - 1) * 20;
    double* dpoly = nullptr;    // per-axis tables of the cell polynomials
    RTMI_HIP(work.get(&dpoly, (nax2 + nay2) * sizeof(double)));
    double *dCx = dpoly, *dLx = dpoly + (size_t)(qx - 1) * 16, *dCy = dpoly + nax2, *dLy = dCy + (size_t)(qy - 1) * 16;
    RTMI_HIP(hipMemcpyAsync(dCx, PX.C.data(), PX.C.size() * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(dLx, PX.L.data(), PX.L.size() * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(dCy, PY.C.data(), PY.C.size() * sizeof(double), hipMemcpyHostToDevice, st));
    RTMI_HIP(hipMemcpyAsync(dLy, PY.L.data(), PY.L.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // one allocation: the flat-cell map (one entry per cell, padded to 32 entries), then the table
    f->flat_pad = (long)((ncell + 31) / 32 * 32);
    RTMI_HIP(hipMalloc(&f->poly_base, ((size_t)f->flat_pad + ncell * rt::kPolyStride) * esz));
    f->poly = (char*)f->poly_base + (size_t)f->flat_pad * esz;
    unsigned long long* dcnt = nullptr;      // [0] bits of max |gradient-spline coefficient|, [1] flat cells, [2] steep cells
    RTMI_HIP(work.get(&dcnt, 3 * sizeof(unsigned long long)));
    unsigned long long hcnt[3] = {0, 0, 0};
    // steep: lambda >= kSteepRate / the grid's shorter side
    const double lam0 = kSteepRate / std::fmin(f->bx - f->ax, f->by - f->ay);
    RTMI_HIP(hipMemsetAsync(dcnt, 0, sizeof(hcnt), st));
    hipLaunchKernelGGL(k_absmax, dim3(256), dim3(256), 0, st, f->dCdx, f->dCdy, nz, dcnt);
    const dim3 pg((qx - 1 + 63) / 64, qy - 1), pb(64);
    by_dtype(f->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_polytab<T>, pg, pb, 0, st, f->dZ, f->dCdx, f->dCdy, qx, qy, dCx, dLx, dCy, dLy, (T*)f->poly, (T*)f->poly_base, dcnt,
                           dcnt + 1, ihx, ihy, lam0);
    });
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpyAsync(hcnt, dcnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    RTMI_HIP(hipStreamSynchronize(st));  // the host vectors and tables go out of scope
    f->flat_cells = (long)hcnt[1];
    f->steep_cells = (long)hcnt[2];
    memcpy(&f->gmax, &hcnt[0], sizeof(double));
    // x-invariant?  Only a field without flat and steep cells can be (the map's region then holds the row table), and the grid
    // must be wide enough for the region to hold a line per row.
    if (f->flat_cells == 0 && f->steep_cells == 0 && (size_t)rt::kLayerStride * (qy - 1) <= (size_t)f->flat_pad) {
        unsigned long long nbad = 0;
        RTMI_HIP(hipMemsetAsync(dcnt + 1, 0, sizeof(nbad), st));
        by_dtype(f->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_layered_check<T>, pg, pb, 0, st, f->dZ, qx, qy, (const T*)f->poly, dcnt, dcnt + 1);
        });
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(hipMemcpyAsync(&nbad, dcnt + 1, sizeof(nbad), hipMemcpyDeviceToHost, st));
        RTMI_HIP(hipStreamSynchronize(st));
        if (nbad == 0) {
            by_dtype(f->dtype, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(k_layered_rows<T>, dim3((qy - 1 + 63) / 64), dim3(64), 0, st, (T*)f->poly, qx - 1, qy - 1);
            });
            RTMI_HIP(hipGetLastError());
            RTMI_HIP(hipStreamSynchronize(st));
            f->layered = 1;
        }
    }
    if (getenv("RTMI_DEBUG")) fprintf(stderr, "rtmi: field %d x %d: %ld of %zu cells flat, %ld steep (lambda >= %.3g)\n", qx, qy, (long)hcnt[1], ncell, (long)hcnt[2], lam0);
    return RTMI_OK;
}

static int field_finish(const char* who, rtmi_field* f, double delta) {
    DevMem work;
    int rc;
    try {
        rc = field_finish_impl(who, f, delta, work);
    } catch (const std::exception& e) {   // host vectors of the collocation factorisation
        rc = rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string("field build: ") + e.what()).c_str());
    }
    if (rc) (void)hipStreamSynchronize(f->stream);   // nothing may still read the work buffers
    return rc;
}

RTMI_EXPORT void rtmi_field_destroy(rtmi_field* f) {
    if (!f) return;
    (void)hipFree(f->dZ); (void)hipFree(f->dCdy); (void)hipFree(f->dCdx); (void)hipFree(f->zn); (void)hipFree(f->g);
    (void)hipFree(f->poly_base);
    (void)hipFree(f->rdiv);
    delete f;
}

static int field_alloc(int dtype, int qx, int qy, void* stream, rtmi_field** out) {
    const char* who = "field";
    RTMI_ARG(out, "out is null");
    RTMI_ARG(dtype == RTMI_F64 || dtype == RTMI_F32, "dtype must be RTMI_F64 or RTMI_F32");
    RTMI_ARG(qx >= 8 && qy >= 8, "grid must be at least 8x8 (cubic not-a-knot fit)");
    RTMI_ARG((size_t)qx * qy < (1ull << 31) && qx < (1 << 24) && qy < (1 << 24), "grid too large");
    rtmi_field* f = new (std::nothrow) rtmi_field();
    if (!f) return rtmi_internal_fail(RTMI_ERR_ALLOC, "field: host allocation failed");
    f->dtype = dtype; f->qx = qx; f->qy = qy; f->stream = (hipStream_t)stream;
    *out = f;
    RTMI_HIP(hipGetDevice(&f->device));
    RTMI_HIP(hipMalloc(&f->dZ, (size_t)qx * qy * sizeof(double)));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_field_build(int scenario, double xi, double xs, double yi, double ys, double delta, int dtype,
                                 void* stream, rtmi_field** out) {
    const char* who = "rtmi_field_build";
    RTMI_ARG(scenario >= RTMI_INTERFACE && scenario <= RTMI_ANISOTROPY, "scenario must be 1..4");
    RTMI_ARG(delta > 0 && xs > xi && ys > yi, "need delta > 0 and xs > xi, ys > yi");
    const int qx = (int)((xs - xi + 6) / delta + 1);  // :426
    const int qy = (int)((ys - yi + 6) / delta + 1);  // :427
    rtmi_field* f = nullptr;
    int rc = field_alloc(dtype, qx, qy, stream, &f);
    if (rc) { rtmi_field_destroy(f); return rc; }
    f->ax = xi - 3; f->bx = xs + 3; f->hx = (f->bx - f->ax) / (double)(qx - 1);  // :429 linspace
    f->ay = yi - 3; f->by = ys + 3; f->hy = (f->by - f->ay) / (double)(qy - 1);
    hipLaunchKernelGGL(k_sample, dim3((qx + 255) / 256, qy), dim3(256), 0, f->stream, scenario, f->dZ, qx, qy, f->ax,
                       f->hx, f->bx, f->ay, f->hy, f->by);
    rc = field_finish(who, f, delta);
    if (rc) { rtmi_field_destroy(f); return rc; }
    *out = f;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_field_from_samples(const double* x, int qx, const double* y, int qy, const double* Z, double delta,
                                        int dtype, void* stream, rtmi_field** out) {
    const char* who = "rtmi_field_from_samples";
    RTMI_ARG(x && y && Z, "null input");
    RTMI_ARG(delta > 0, "delta must be > 0");
    RTMI_ARG(qx >= 8 && qy >= 8, "grid must be at least 8x8");
    try {
        const std::vector<double> lx = linspace(x[0], x[qx - 1], qx), ly = linspace(y[0], y[qy - 1], qy);
        if (memcmp(lx.data(), x, qx * sizeof(double)) || memcmp(ly.data(), y, qy * sizeof(double)))
            return rtmi_internal_fail(RTMI_ERR_UNSUPPORTED, "rtmi_field_from_samples: axes must be numpy.linspace grids (genZ, RT_bench.py:429)");
    } catch (const std::exception& e) {
        return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + e.what()).c_str());
    }
    rtmi_field* f = nullptr;
    int rc = field_alloc(dtype, qx, qy, stream, &f);
    if (rc) { rtmi_field_destroy(f); return rc; }
    f->ax = x[0]; f->bx = x[qx - 1]; f->hx = (f->bx - f->ax) / (double)(qx - 1);
    f->ay = y[0]; f->by = y[qy - 1]; f->hy = (f->by - f->ay) / (double)(qy - 1);
    const hipError_t e = hipMemcpyAsync(f->dZ, Z, (size_t)qx * qy * sizeof(double), hipMemcpyHostToDevice, f->stream);
    rc = e == hipSuccess ? field_finish(who, f, delta)
                         : rtmi_internal_fail(RTMI_ERR_HIP, (std::string(who) + ": hipMemcpyAsync: " + hipGetErrorString(e)).c_str());
    if (rc) { rtmi_field_destroy(f); return rc; }
    *out = f;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_field_dims(const rtmi_field* f, int* qx, int* qy) {
    const char* who = "rtmi_field_dims";
    RTMI_ARG(f && qx && qy, "null");
    *qx = f->qx; *qy = f->qy;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_field_layered(const rtmi_field* f) { return f ? f->layered : 0; }

RTMI_EXPORT int rtmi_field_read(const rtmi_field* f, double* x, double* y, double* Z, double* cdy, double* cdx) {
    const char* who = "rtmi_field_read";
    RTMI_ARG(f, "null field");
    DEVICE_TRY(f, who);
    const size_t nz = (size_t)f->qx * f->qy * sizeof(double);
    RTMI_HIP(hipStreamSynchronize(f->stream));
    try {
        if (x) { auto v = linspace(f->ax, f->bx, f->qx); memcpy(x, v.data(), v.size() * sizeof(double)); }
        if (y) { auto v = linspace(f->ay, f->by, f->qy); memcpy(y, v.data(), v.size() * sizeof(double)); }
    } catch (const std::exception& e) {
        return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + e.what()).c_str());
    }
    if (Z) RTMI_HIP(hipMemcpy(Z, f->dZ, nz, hipMemcpyDeviceToHost));
    if (cdy) RTMI_HIP(hipMemcpy(cdy, f->dCdy, nz, hipMemcpyDeviceToHost));
    if (cdx) RTMI_HIP(hipMemcpy(cdx, f->dCdx, nz, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ------------------------------------------------------------------ diagnostic: numpy's array exp (np_exp) on the device
__global__ void k_debug_exp(long n, const double* x, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = np_exp(x[i]);
}

RTMI_EXPORT int rtmi_debug_exp(int64_t n, const double* x, double* out) {
    ARG_TRY(x && out, "rtmi_debug_exp: null");
    ARG_TRY(n >= 0, "rtmi_debug_exp: n < 0");
    if (n == 0) return RTMI_OK;
    const char* who = "rtmi_debug_exp";
    DevMem mem;
    double* d = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    RTMI_HIP(mem.get(&d, 2 * nb));
    RTMI_HIP(hipMemcpy(d, x, nb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_exp, blocks(n), dim3(256), 0, nullptr, (long)n, d, d + n);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(out, d + n, nb, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
