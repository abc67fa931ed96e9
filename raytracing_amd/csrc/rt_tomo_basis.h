// rt_tomo_basis.h -- the axis bases of a tomography model basis (tomo.hip, rtmi_tomo_basis_*), as host
// arithmetic with no HIP in it, so that a host program can include it (tests/native/tomo_basis_check.cpp): the rules of an axis,
// the ranges the transposed operator walks, the uniform B-spline axes of rtmi_bspline_axis, and the operator pair as plain loops.
//
// An axis basis of a fine axis of q samples onto m coefficients with bandwidth B (1 .. 4) is first [q] and wgt [q][B]: fine index j
// carries weight wgt[j][b] on coefficient first[j] + b.  0 <= first[j] <= m - B, first is non-decreasing, every weight is finite;
// zero weights and a coefficient that no fine index reaches are allowed.  Because first is non-decreasing the fine indices that
// reach coefficient l form one range [lo[l], hi[l]): lo[l] the first j with first[j] >= l - B + 1, hi[l] one past the last j with
// first[j] <= l; lo and hi are non-decreasing too, and for j in the range 0 <= l - first[j] < B.
// Build with -ffp-contract=off, as the library is.
#pragma once
#include <cmath>
#include <cstdint>

namespace rt {

constexpr int kBasisMaxBand = 4;

// nullptr for an axis that keeps the rules, else what is wrong; *at: the fine index it is wrong at (-1: the sizes)
inline const char* basis_axis_check(int64_t q, int64_t m, int64_t B, const int32_t* first, const double* wgt, int64_t* at) {
    *at = -1;
    if (B < 1 || B > kBasisMaxBand) return "the bandwidth must be in 1 .. 4";
    if (q < 1) return "the fine axis has no samples";
    if (m < B) return "fewer coefficients than the bandwidth";
    for (int64_t j = 0; j < q; j++) {
        *at = j;
        if (first[j] < 0 || (int64_t)first[j] > m - B) return "first is outside 0 .. m - B";
        if (j > 0 && first[j] < first[j - 1]) return "first decreases";
        for (int64_t b = 0; b < B; b++)
            if (!std::isfinite(wgt[j * B + b])) return "a weight is not finite";
    }
    *at = -1;
    return nullptr;
}

// lo [m], hi [m] of an axis that keeps the rules; an unreached coefficient gets lo == hi
inline void basis_ranges(int64_t q, int64_t m, int64_t B, const int32_t* first, int32_t* lo, int32_t* hi) {
    int64_t a = 0, b = 0;
    for (int64_t l = 0; l < m; l++) {
        while (a < q && (int64_t)first[a] < l - B + 1) a++;
        while (b < q && (int64_t)first[b] <= l) b++;
        lo[l] = (int32_t)a;
        hi[l] = (int32_t)(b > a ? b : a);
    }
}

// Uniform B-splines of degree 0, 1 or 3 (B = degree + 1) on n = m - degree intervals (degree 0: n = m) over q >= 2 samples, the
// first and the last sample on the ends of the knot span: e = min(floor(j n / (q - 1)), n - 1) in integers, first[j] = e,
// t = (j n - e (q - 1)) / (q - 1) in long double, the weights in long double, each rounded once to fp64.  false: sizes it cannot do.
inline bool bspline_axis(int64_t q, int64_t m, int degree, int32_t* first, double* wgt) {
    if (!(degree == 0 || degree == 1 || degree == 3) || q < 2 || m < degree + 1) return false;
    const int64_t n = degree == 0 ? m : m - degree, B = degree + 1;
    for (int64_t j = 0; j < q; j++) {
        int64_t e = j * n / (q - 1);
        if (e > n - 1) e = n - 1;
        first[j] = (int32_t)e;
        const long double t = (long double)(j * n - e * (q - 1)) / (long double)(q - 1);
        double* w = wgt + j * B;
        if (degree == 0) {
            w[0] = 1.0;
        } else if (degree == 1) {
            w[0] = (double)(1.0L - t);
            w[1] = (double)t;
        } else {
            const long double u = 1.0L - t;
            w[0] = (double)(u * u * u / 6.0L);
            w[1] = (double)(((3.0L * t - 6.0L) * t * t + 4.0L) / 6.0L);
            w[2] = (double)((((-3.0L * t + 3.0L) * t + 3.0L) * t + 1.0L) / 6.0L);
            w[3] = (double)(t * t * t / 6.0L);
        }
    }
    return true;
}

// One axis as the operator reads it
struct BasisAxis {
    int64_t q, m, B;
    const int32_t* first;
    const double* wgt;
};

// x [qy][qx] = P c, c [my][mx]: the definition the kernel follows, every product and every add a separate fp64 operation
inline void basis_prolong_host(const BasisAxis& X, const BasisAxis& Y, const double* c, double* x) {
    for (int64_t i = 0; i < Y.q; i++)
        for (int64_t j = 0; j < X.q; j++) {
            double acc = 0.0;
            for (int64_t a = 0; a < Y.B; a++) {
                double r = 0.0;
                for (int64_t b = 0; b < X.B; b++) {
                    const double p = X.wgt[j * X.B + b] * c[(Y.first[i] + a) * X.m + X.first[j] + b];
                    r = r + p;
                }
                const double p = Y.wgt[i * Y.B + a] * r;
                acc = acc + p;
            }
            x[i * X.q + j] = acc;
        }
}

// g [my][mx] = P^T x in two passes over the ranges, t [qy][mx] between them
inline void basis_restrict_host(const BasisAxis& X, const BasisAxis& Y, const int32_t* lox, const int32_t* hix, const int32_t* loy,
                                const int32_t* hiy, const double* x, double* t, double* g) {
    for (int64_t i = 0; i < Y.q; i++)
        for (int64_t l = 0; l < X.m; l++) {
            double s = 0.0;
            for (int64_t j = lox[l]; j < hix[l]; j++) {
                const double p = X.wgt[j * X.B + (l - X.first[j])] * x[i * X.q + j];
                s = s + p;
            }
            t[i * X.m + l] = s;
        }
    for (int64_t k = 0; k < Y.m; k++)
        for (int64_t l = 0; l < X.m; l++) {
            double s = 0.0;
            for (int64_t i = loy[k]; i < hiy[k]; i++) {
                const double p = Y.wgt[i * Y.B + (k - Y.first[i])] * t[i * X.m + l];
                s = s + p;
            }
            g[k * X.m + l] = s;
        }
}

}  // namespace rt
