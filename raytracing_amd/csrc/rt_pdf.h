// rt_pdf.h -- the arithmetic of a location pdf on a locator's map (pdf.hip, rtmi_locate_pdf, rtmi_locate_edt_pdf; include/rtmi.h,
// DESIGN.md section 33), with no HIP in it, so that a host program can include it (tests/native/pdf_levels.cpp): the density and
// the mass of a node, which the kernels call once per node, the histogram bin of a mass, and the per-event results, which the C
// entry computes on the host from the integer sums.  tests/pdf_ref.py restates all of it.
//
// Everything real is fp64 and every product, sum, quotient and square root below is one rounded operation: build with
// -ffp-contract=off, as the library is.  The only fused operations are those of rt_np_exp.h, which are part of its definition.
//
// * marks the best node of the search;  di = ix - ix*,  dj = iy - iy*
// Density   least squares   s2 = sigma sigma;  c = 0.5 / s2;  b = sw* c          once per event
//                           a = obj - obj*;  z = -(a b);  rho = z >= -700 ? exp(z) : +0.0     (a NaN z: +0.0; exp: rt_np_exp.h)
//           EDT             r = value / value*;  rho = r^p by square and multiply from the most significant bit of p:
//                           acc = r; for every lower bit, high to low: acc = acc acc; if the bit is set: acc = acc r
//                           p = power, or the best node's n where power is 0;  rho = +0.0 unless value >= 0 and value* > 0
// Mass      m = (uint64)trunc(rho 2^30): the product is exact, m* = 2^30, and every sum below is a sum of integers
// Bin       of m >= 1: b = the index of the leading one of m (0 .. 30), sub = the five bits below it (shifted up where b < 5),
//           bin = 32 b + sub, 0 .. 991, monotone in m; the least mass of a bin is edge(bin)
// Sums      Z = sum m;  Sx = sum m di;  Sy = sum m dj;  Sxx = sum m di di;  Sxy = sum m di dj;  Syy = sum m dj dj;
//           rim = sum m over ix in {0, nx - 1} or iy in {0, ny - 1};  nz = #{m > 0};  count[bin], mass[bin]
// Results   D(v) is the nearest double of an integer v (ties to even), Zd = D(Z); an event with Z = 0 has none
//           ax = D(Sx) / Zd;  ay = D(Sy) / Zd
//           mean_x = (gx0 + (double)ix* gdx) + ax gdx;  mean_y alike
//           cxx = (D(Sxx) / Zd - ax ax) (gdx gdx);  cxy = (D(Sxy) / Zd - ax ay) (gdx gdy);  cyy = (D(Syy) / Zd - ay ay) (gdy gdy)
//           h = (cxx + cyy) 0.5;  d = (cxx - cyy) 0.5;  r = sqrt(d d + cxy cxy);  l1 = h + r;  l2 = h - r
//           ellipse = {sqrt(l1), sqrt(l2 > 0 ? l2 : 0), 0.5 atan2(cxy, d)}: the semi-axes of the one-sigma ellipse and the angle
//               of the major one from +x, in (-pi/2, pi/2]
//           area = (Zd / 2^30) (gdx gdy);  rim_fraction = D(rim) / Zd
//           level c:  tq = (uint64)ceil(c Zd), at most Z;  from bin 991 down, C = sum count, M = sum mass, to the first bin B with
//               M >= tq:  level_count = C,  level_area = (double)C (gdx gdy),  level_fraction = D(M) / Zd,
//               level_rho = (double)edge(B) / 2^30
// Sample    q = (uint64)(u Zd), at most Z - 1 (u <= 0 or NaN: 0): the least node, in node order, whose inclusive cumulative mass
//           exceeds q
#pragma once
#include <cmath>
#include <cstdint>

#include "rt_fix128.h"
#include "rt_locate.h"
#include "rt_np_exp.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_PDF_HD __host__ __device__ __forceinline__
#else
#define RT_PDF_HD inline
#endif

namespace rt {

constexpr double kPdfCut = -700.0;                      // rt_edt.h's: below it the density is +0.0
constexpr double kPdfOne = 1073741824.0;                // 2^30: the mass of the best node
constexpr int kPdfBins = 992;                           // 31 leading-one positions of 32 bins
constexpr int kPdfMaxLevels = 8;
constexpr int64_t kPdfMaxAxis = 65536;                  // with it m di dj and m di di stay below 2^62

// b of an event of the least-squares kind
inline double pdf_l2_scale(double sw, double sigma) {
    const double s2 = sigma * sigma;
    const double c = 0.5 / s2;
    return sw * c;
}

RT_PDF_HD double pdf_rho_l2(double obj, double obj0, double b, const double* tab) {
    const double a = obj - obj0;
    const double z = -(a * b);
    return z >= kPdfCut ? np_exp_main(z, tab) : 0.0;
}

RT_PDF_HD double pdf_rho_edt(double value, double value0, int p) {
    if (!(value >= 0.0 && value0 > 0.0)) return 0.0;
    const double r = value / value0;
    int bit = 30;
    while (!(p >> bit & 1)) bit--;                      // p >= 1
    double acc = r;
    for (bit--; bit >= 0; bit--) {
        acc = acc * acc;
        if (p >> bit & 1) acc = acc * r;
    }
    return acc;
}

RT_PDF_HD unsigned long long pdf_mass(double rho) { return (unsigned long long)(rho * kPdfOne); }

RT_PDF_HD int pdf_bin(unsigned long long m) {           // m >= 1
#if defined(__HIP_DEVICE_COMPILE__)
    const int b = 63 - __clzll((long long)m);
#else
    const int b = 63 - __builtin_clzll(m);
#endif
    const unsigned long long sub = (b >= 5 ? m >> (b - 5) : m << (5 - b)) & 31ull;
    return 32 * b + (int)sub;
}

inline unsigned long long pdf_bin_edge(int bin) {
    const int b = bin / 32;
    const unsigned long long top = 32ull + (unsigned long long)(bin % 32);
    return b >= 5 ? top << (b - 5) : top >> (5 - b);
}

RT_PDF_HD unsigned long long pdf_sample_quantum(double u, unsigned long long Z) {      // Z >= 1
    const double v = (u > 0.0 ? u : 0.0) * (double)Z;
    if (v >= (double)Z) return Z - 1;
    const unsigned long long q = (unsigned long long)v;
    return q < Z ? q : Z - 1;
}

// the nearest double of the two's complement integer hi 2^64 + lo, through rt_fix128.h's biased form
inline double pdf_int_to_double(unsigned long long lo, unsigned long long hi) {
    const unsigned long long bl = lo + kFixBias;
    return fix_to_double(bl, hi + (bl < lo ? 1ull : 0ull));
}

// an event's integer sums: the second and first moments as two's complement (lo, hi)
struct PdfSums {
    unsigned long long Z, rim, nz;
    unsigned long long Sx[2], Sy[2], Sxx[2], Sxy[2], Syy[2];
};

struct PdfStats {
    double mean_x, mean_y, cov[3], ellipse[3], area, rim_fraction;
    int64_t nz, mass;
    int64_t level_count[kPdfMaxLevels];
    double level_area[kPdfMaxLevels], level_fraction[kPdfMaxLevels], level_rho[kPdfMaxLevels];
};

// an event without a candidate or without a pdf: counts 0, every real NaN
inline PdfStats pdf_none() {
    const double nan = std::nan("");
    PdfStats o{};
    o.mean_x = o.mean_y = o.area = o.rim_fraction = nan;
    for (int k = 0; k < 3; k++) o.cov[k] = o.ellipse[k] = nan;
    for (int k = 0; k < kPdfMaxLevels; k++) o.level_area[k] = o.level_fraction[k] = o.level_rho[k] = nan;
    return o;
}

// count, mass: the histogram [kPdfBins]; (ix, iy): the best node
inline PdfStats pdf_finalize(const PdfSums& s, const unsigned long long* count, const unsigned long long* mass, int ix, int iy,
                             const LocateGrid& g, int nlevels, const double* levels) {
    PdfStats o = pdf_none();
    if (s.Z == 0) return o;
    const double Zd = (double)s.Z;
    const double ax = pdf_int_to_double(s.Sx[0], s.Sx[1]) / Zd, ay = pdf_int_to_double(s.Sy[0], s.Sy[1]) / Zd;
    o.mean_x = (g.gx0 + (double)ix * g.gdx) + ax * g.gdx;
    o.mean_y = (g.gy0 + (double)iy * g.gdy) + ay * g.gdy;
    o.cov[0] = (pdf_int_to_double(s.Sxx[0], s.Sxx[1]) / Zd - ax * ax) * (g.gdx * g.gdx);
    o.cov[1] = (pdf_int_to_double(s.Sxy[0], s.Sxy[1]) / Zd - ax * ay) * (g.gdx * g.gdy);
    o.cov[2] = (pdf_int_to_double(s.Syy[0], s.Syy[1]) / Zd - ay * ay) * (g.gdy * g.gdy);
    const double h = (o.cov[0] + o.cov[2]) * 0.5, d = (o.cov[0] - o.cov[2]) * 0.5;
    const double r = std::sqrt(d * d + o.cov[1] * o.cov[1]);
    const double l1 = h + r, l2 = h - r;
    o.ellipse[0] = std::sqrt(l1);
    o.ellipse[1] = std::sqrt(l2 > 0.0 ? l2 : 0.0);
    o.ellipse[2] = 0.5 * std::atan2(o.cov[1], d);
    const double cell = g.gdx * g.gdy;
    o.area = (Zd / kPdfOne) * cell;
    o.rim_fraction = (double)s.rim / Zd;
    o.nz = (int64_t)s.nz;
    o.mass = (int64_t)s.Z;
    for (int k = 0; k < nlevels; k++) {
        const double want = std::ceil(levels[k] * Zd);
        const unsigned long long tq = want >= Zd ? s.Z : (unsigned long long)want;
        unsigned long long C = 0, M = 0;
        int B = kPdfBins - 1;
        for (; B >= 0; B--) {
            C += count[B];
            M += mass[B];
            if (M >= tq) break;
        }
        if (B < 0) B = 0;                               // a histogram that does not hold Z: not the kernels'
        o.level_count[k] = (int64_t)C;
        o.level_area[k] = (double)C * cell;
        o.level_fraction[k] = (double)M / Zd;
        o.level_rho[k] = (double)pdf_bin_edge(B) / kPdfOne;
    }
    return o;
}

}  // namespace rt
