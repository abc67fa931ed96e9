// beams.hip -- Gaussian beam summation (rtmi_gaussian_beams): the frequency-domain wavefield of each source on a regular grid,
// summed over the beams of its recorded fan.  DESIGN.md section 13; the formulas and rules are in include/rtmi.h.
//
// Three passes.  (1) Prep: rtmi_paraxial's kernel stores Q1 P1 Q2 P2 and n after every row (rtmi_internal_paraxial_tube); one
// lane per ray derives each row's values -- position, tangent, T, n, Re M, Im M, the unwrapped phase, the weighted amplitude and
// |Q|^2 -- into compact arrays indexed by a global row number (rays in the caller's order, then rows).  (2) Binning: one lane per
// step counts the 16 x 16 node tiles its footprint can touch, an exclusive scan places its entries, the fill writes (tile, row)
// pairs in step order and a stable radix sort by tile leaves every tile's steps in (m, i) order.  (3) Gather: one block per tile,
// one lane per node.  The tile's steps are staged through LDS in chunks; each lane tests every step of a chunk for ownership and
// notes the ones it owns, then adds their beams in that order, one complex exponential per frequency, into fp64 registers.
// The ownership test and the interpolation run in one fixed order (-ffp-contract=off), so that tests/beam_ref.py follows them.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_crossing.h"
#include "rt_rows.h"
#include "rtmi_host.h"

namespace {

constexpr int kTile = 16;                   // nodes per tile side: one 256-lane block per tile
constexpr int kBlock = kTile * kTile;
constexpr int kChunk = 64;                  // steps staged in LDS at a time
constexpr int kNwb = 8;                     // frequencies per gather launch (accumulators in registers)
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;
constexpr double kCutoff = 18.0;            // the defaults of rtmi_beam_params (include/rtmi.h says why)
constexpr double kWidthCells = 64.0;
constexpr double kCosTurn = 0.5403023058681398;   // cos(1): a step that turns more than 1 rad owns no node

// per-row values, [kRowCols][G] fp64
enum { V_X, V_Y, V_C, V_S, V_T, V_N, V_REM, V_IMM, V_PHI, V_AMP, V_QQ, kRowCols };
// a staged step, [kSegCols][kChunk] in LDS
enum { S_XA, S_YA, S_CA, S_SA, S_XB, S_YB, S_CB, S_SB, S_TA, S_TB, S_LNA, S_LNB, S_REA, S_REB, S_IMA, S_IMB, S_PHA, S_PHB,
       S_AMA, S_AMB, S_QM2, kSegCols };
// stats counters (device, uint64)
enum { C_CAPPED, C_TESTED, C_INSIDE, C_N };

__device__ __forceinline__ double wrap(double d) { return d - kTwoPi * rint(d / kTwoPi); }

struct Beam {
    double gx0, gdx, gy0, gdy;
    int nx, ny, ntx, nty;
    long ntiles;                // tiles per source
    double eps, cutoff, maxw, omin;
};

// q_max of a step from its rows' |Q|^2, capped at max_width
__device__ __forceinline__ double step_qmax(const Beam& B, double qqa, double qqb, bool& capped) {
    const double qq = qqa > qqb ? qqa : qqb;
    const double q = sqrt(2.0 * B.cutoff * qq / (B.omin * B.eps));
    capped = q > B.maxw;
    return capped ? B.maxw : q;
}

// ------------------------------------------------------------------------------------------------------------ (1) prep
struct PrepArgs {
    const int32_t* slot;        // [R] or NULL: slot of the caller's ray o
    const double* tube;         // [rec_rows][5][R] slot order: Q1 P1 Q2 P2 n
    const long long* rowbase;   // [R + 1] caller order: the ray's first global row
    const double* w;            // [R] caller order: quadrature weight (trapezoid, taper)
    long G;
    double eps;
    double* rv;                 // [kRowCols][G]
    int32_t* row_ray;           // [G]: the caller's ray of each row
    uint32_t* seg_row;          // [G - R]: the first row of each step, in (ray, step) order
};

// nrows[o] = the recorded rows of the caller's ray o, nrows[R] = 0
template <typename T> __global__ void k_rows(Rows<T> rec, const int32_t* slot, long long* nrows) {
    const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o < rec.R) nrows[o] = rec.last_recorded(slot ? (long)slot[o] : o) + 1;
    else if (o == rec.R) nrows[rec.R] = 0;
}

template <typename T> __global__ void k_prep(Rows<T> rec, PrepArgs A) {
    const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= rec.R) return;
    const long R = rec.R, G = A.G;
    const long k = A.slot ? (long)A.slot[o] : o;
    const long nr = rec.last_recorded(k) + 1;
    const long g0 = (long)A.rowbase[o];
    const T* col = rec.row(0, k);
    const double eps = A.eps;
    const double W = A.w[o] * sqrt(eps * A.tube[4 * R + k]) / (4.0 * kPi);
    double phi = -0.5 * kPi, aprev = -0.5 * kPi;
    for (long j = 0; j < nr; j++) {
        const T* r = col + (size_t)j * rec.pitch();
        const double x = (double)r[COL_X * R], y = (double)r[COL_Y * R], t = (double)r[COL_T * R], th = (double)r[COL_TH * R];
        const double* q = A.tube + (size_t)j * 5 * R + k;
        const double q1 = q[0], p1 = q[R], q2 = q[2 * R], p2 = q[3 * R], n = q[4 * R];
        const double eq1 = eps * q1, ep1 = eps * p1;
        const double qq = q2 * q2 + eq1 * eq1;
        const double re = (p2 * q2 + ep1 * eq1) / qq;
        const double im = (eps * (p2 * q1 - p1 * q2)) / qq;
        const double a = atan2(-eq1, q2);
        if (j > 0) phi = phi + wrap(a - aprev);
        aprev = a;
        const long g = g0 + j;
        double* v = A.rv + g;
        v[V_X * G] = x; v[V_Y * G] = y; v[V_C * G] = cos_g(th); v[V_S * G] = sin_g(th); v[V_T * G] = t; v[V_N * G] = n;
        v[V_REM * G] = re; v[V_IMM * G] = im; v[V_PHI * G] = phi; v[V_AMP * G] = W / sqrt(n * sqrt(qq)); v[V_QQ * G] = qq;
        A.row_ray[g] = (int32_t)o;
        if (j > 0) A.seg_row[g0 - o + j - 1] = (uint32_t)(g - 1);
    }
}

// ------------------------------------------------------------------------------------------------------------ (2) binning
struct BinArgs {
    const double* rv;
    long G, nseg;
    const uint32_t* seg_row;
    const int32_t* row_ray;
    int M;                      // fan size
    unsigned long long* count;  // [nseg + 1] (count pass)
    const unsigned long long* offs;   // [nseg + 1] (fill)
    uint32_t* keys;             // [E]: source * ntiles + tile
    uint32_t* vals;             // [E]: the step's first row
    unsigned long long* ctr;
};

// The tiles a step's footprint can touch, conservatively: the box of the chord grown by q_max plus the chord (the blended normal
// moves the interpolated point along the tangent by less than L / 4 per rad of turn), then the wedge between the two normals --
// some node of the tile with d_{i-1} >= 0 and some with d_i < 0, within a tolerance far above the rounding of d.
template <typename F> __device__ __forceinline__ void for_tiles(const Beam& B, const double* rv, long G, long a, long s, bool& capped, F fn) {
    capped = false;
    const long b = a + 1;
    const double xa = rv[V_X * G + a], ya = rv[V_Y * G + a], ca = rv[V_C * G + a], sa = rv[V_S * G + a];
    const double xb = rv[V_X * G + b], yb = rv[V_Y * G + b], cb = rv[V_C * G + b], sb = rv[V_S * G + b];
    if (ca * cb + sa * sb < kCosTurn) return;
    const double qm = step_qmax(B, rv[V_QQ * G + a], rv[V_QQ * G + b], capped);
    const double dx = xb - xa, dy = yb - ya;
    const double rad = qm + sqrt(dx * dx + dy * dy);
    const double tw = B.gdx * kTile, th = B.gdy * kTile;
    const double fx0 = floor((fmin(xa, xb) - rad - B.gx0) / tw), fx1 = floor((fmax(xa, xb) + rad - B.gx0) / tw);
    const double fy0 = floor((fmin(ya, yb) - rad - B.gy0) / th), fy1 = floor((fmax(ya, yb) + rad - B.gy0) / th);
    if (!(fx1 >= 0.0 && fy1 >= 0.0 && fx0 <= (double)(B.ntx - 1) && fy0 <= (double)(B.nty - 1))) return;
    const int tx0 = fx0 < 0.0 ? 0 : (int)fx0, tx1 = fx1 > (double)(B.ntx - 1) ? B.ntx - 1 : (int)fx1;
    const int ty0 = fy0 < 0.0 ? 0 : (int)fy0, ty1 = fy1 > (double)(B.nty - 1) ? B.nty - 1 : (int)fy1;
    const double tol = 1e-9 * (1.0 + fabs(xa) + fabs(ya) + tw + th);
    for (int ty = ty0; ty <= ty1; ty++) {
        const int iy1 = ty * kTile + kTile - 1 < B.ny - 1 ? ty * kTile + kTile - 1 : B.ny - 1;
        const double Y0 = B.gy0 + (double)(ty * kTile) * B.gdy, Y1 = B.gy0 + (double)iy1 * B.gdy;
        for (int tx = tx0; tx <= tx1; tx++) {
            const int ix1 = tx * kTile + kTile - 1 < B.nx - 1 ? tx * kTile + kTile - 1 : B.nx - 1;
            const double X0 = B.gx0 + (double)(tx * kTile) * B.gdx, X1 = B.gx0 + (double)ix1 * B.gdx;
            const double amax = fmax((X0 - xa) * ca, (X1 - xa) * ca) + fmax((Y0 - ya) * sa, (Y1 - ya) * sa);
            const double bmin = fmin((X0 - xb) * cb, (X1 - xb) * cb) + fmin((Y0 - yb) * sb, (Y1 - yb) * sb);
            if (amax >= -tol && bmin < tol) fn((uint32_t)(s * B.ntiles + (long)ty * B.ntx + tx));
        }
    }
}

__global__ void k_count(Beam B, BinArgs A) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > A.nseg) return;
    if (e == A.nseg) { A.count[e] = 0ull; return; }
    const long a = (long)A.seg_row[e];
    unsigned long long c = 0;
    bool capped;
    for_tiles(B, A.rv, A.G, a, (long)A.row_ray[a] / A.M, capped, [&](uint32_t) { c++; });
    A.count[e] = c;
    if (capped) atomicAdd(&A.ctr[C_CAPPED], 1ull);
}

__global__ void k_fill(Beam B, BinArgs A) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= A.nseg) return;
    const long a = (long)A.seg_row[e];
    unsigned long long at = A.offs[e];
    bool capped;
    for_tiles(B, A.rv, A.G, a, (long)A.row_ray[a] / A.M, capped, [&](uint32_t key) {
        A.keys[at] = key;
        A.vals[at] = (uint32_t)a;
        at++;
    });
}

// [begin, end) of every tile's run in the sorted keys (tiles without steps keep 0, 0)
__global__ void k_ranges(const uint32_t* keys, long E, uint32_t* begin, uint32_t* end) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint32_t k = keys[e];
    if (e == 0 || keys[e - 1] != k) begin[k] = (uint32_t)e;
    if (e == E - 1 || keys[e + 1] != k) end[k] = (uint32_t)(e + 1);
}

// ------------------------------------------------------------------------------------------------------------ (3) gather
struct GatherArgs {
    const double* rv;
    long G;
    const uint32_t* vals;
    const uint32_t* begin;
    const uint32_t* end;
    double om[kNwb];            // this launch's frequencies
    int nwg, w0, nw;            // how many of om are in use, the first one's index, all frequencies
    double* u;                  // [S][nw][ny][nx][2]
    unsigned long long* ctr;
    int count_pairs;            // add to C_TESTED / C_INSIDE (the first launch only)
};

__device__ __forceinline__ void stage(const Beam& B, const GatherArgs& A, long a, int j, double (*sg)[kChunk]) {
    const double* rv = A.rv;
    const long G = A.G, b = a + 1;
    const double xa = rv[V_X * G + a], ya = rv[V_Y * G + a], xb = rv[V_X * G + b], yb = rv[V_Y * G + b];
    const double dx = xb - xa, dy = yb - ya;
    const double L = sqrt(dx * dx + dy * dy);
    bool capped;
    const double qm = step_qmax(B, rv[V_QQ * G + a], rv[V_QQ * G + b], capped);
    sg[S_XA][j] = xa; sg[S_YA][j] = ya; sg[S_CA][j] = rv[V_C * G + a]; sg[S_SA][j] = rv[V_S * G + a];
    sg[S_XB][j] = xb; sg[S_YB][j] = yb; sg[S_CB][j] = rv[V_C * G + b]; sg[S_SB][j] = rv[V_S * G + b];
    sg[S_TA][j] = rv[V_T * G + a]; sg[S_TB][j] = rv[V_T * G + b];
    sg[S_LNA][j] = L * rv[V_N * G + a]; sg[S_LNB][j] = L * rv[V_N * G + b];
    sg[S_REA][j] = rv[V_REM * G + a]; sg[S_REB][j] = rv[V_REM * G + b];
    sg[S_IMA][j] = rv[V_IMM * G + a]; sg[S_IMB][j] = rv[V_IMM * G + b];
    sg[S_PHA][j] = rv[V_PHI * G + a]; sg[S_PHB][j] = rv[V_PHI * G + b];
    sg[S_AMA][j] = rv[V_AMP * G + a]; sg[S_AMB][j] = rv[V_AMP * G + b];
    sg[S_QM2][j] = qm * qm;
}

__global__ __launch_bounds__(kBlock) void k_gather(Beam B, GatherArgs A) {
    __shared__ double sg[kSegCols][kChunk];
    __shared__ unsigned char owned[kChunk][kBlock];      // per lane: the chunk's steps it owns, in order
    __shared__ unsigned long long tot[2];
    const int tid = threadIdx.x;
    if (tid < 2) tot[tid] = 0ull;
    const long key = blockIdx.x;
    const long s = key / B.ntiles, t = key - s * B.ntiles;
    const int ty = (int)(t / B.ntx), tx = (int)(t - (long)ty * B.ntx);
    const int ix = tx * kTile + (tid & (kTile - 1)), iy = ty * kTile + tid / kTile;
    const bool valid = ix < B.nx && iy < B.ny;
    const double X = B.gx0 + (double)ix * B.gdx, Y = B.gy0 + (double)iy * B.gdy;
    double ar[kNwb], ai[kNwb];
#pragma unroll
    for (int q = 0; q < kNwb; q++) { ar[q] = 0.0; ai[q] = 0.0; }
    unsigned long long tested = 0, inside = 0;
    const uint32_t e0 = A.begin[key], e1 = A.end[key];
    for (uint32_t c0 = e0; c0 < e1; c0 += kChunk) {
        const int nch = e1 - c0 < (uint32_t)kChunk ? (int)(e1 - c0) : kChunk;
        __syncthreads();
        if (tid < nch) stage(B, A, (long)A.vals[c0 + tid], tid, sg);
        __syncthreads();
        int cnt = 0;
        if (valid) {
            for (int j = 0; j < nch; j++) {
                const double da = (X - sg[S_XA][j]) * sg[S_CA][j] + (Y - sg[S_YA][j]) * sg[S_SA][j];
                const double db = (X - sg[S_XB][j]) * sg[S_CB][j] + (Y - sg[S_YB][j]) * sg[S_SB][j];
                if (da >= 0.0 && db < 0.0) owned[cnt++][tid] = (unsigned char)j;
            }
            tested += (unsigned long long)nch;
        }
        for (int r = 0; r < cnt; r++) {
            const int j = owned[r][tid];
            const double xa = sg[S_XA][j], ya = sg[S_YA][j], ca = sg[S_CA][j], sa = sg[S_SA][j];
            const double xb = sg[S_XB][j], yb = sg[S_YB][j], cb = sg[S_CB][j], sb = sg[S_SB][j];
            const double da = (X - xa) * ca + (Y - ya) * sa;
            const double db = (X - xb) * cb + (Y - yb) * sb;
            const double lam = da / (da - db);
            const double px = xa + lam * (xb - xa), py = ya + lam * (yb - ya);
            const double tcx = ca + lam * (cb - ca), tcy = sa + lam * (sb - sa);
            const double qn = (X - px) * (-tcy) + (Y - py) * tcx;
            const double q2 = (qn * qn) / (tcx * tcx + tcy * tcy);
            if (!(q2 <= sg[S_QM2][j])) continue;
            const double ima = sg[S_IMA][j];
            const double im = ima + lam * (sg[S_IMB][j] - ima);
            const double g = 0.5 * im * q2;
            if (B.omin * g > B.cutoff) continue;
            inside++;
            const double rea = sg[S_REA][j], pha = sg[S_PHA][j], ama = sg[S_AMA][j];
            const double re = rea + lam * (sg[S_REB][j] - rea);
            const double ph = pha + lam * (sg[S_PHB][j] - pha);
            const double am = ama + lam * (sg[S_AMB][j] - ama);
            const double T = herm(basis(lam), sg[S_TA][j], sg[S_LNA][j], sg[S_TB][j], sg[S_LNB][j]);
            const double h = T + 0.5 * re * q2;
            const double hp = 0.5 * ph;
#pragma unroll
            for (int q = 0; q < kNwb; q++) {
                if (q < A.nwg) {
                    const double w = A.om[q];
                    const double wg = w * g;
                    if (wg <= B.cutoff) {
                        const double amp = am * exp(-wg);
                        double sn, cs;
                        sincos(w * h - hp, &sn, &cs);
                        ar[q] += amp * cs;
                        ai[q] += amp * sn;
                    }
                }
            }
        }
    }
    if (valid) {
        const double c = 0.7071067811865476;     // e^{i pi/4} = (1 + i) / sqrt(2)
#pragma unroll
        for (int q = 0; q < kNwb; q++) {
            if (q < A.nwg) {
                const size_t o = ((((size_t)s * A.nw + A.w0 + q) * B.ny + iy) * B.nx + ix) * 2;
                A.u[o] = c * (ar[q] - ai[q]);
                A.u[o + 1] = c * (ar[q] + ai[q]);
            }
        }
    }
    if (A.count_pairs) {
        if (tested) atomicAdd(&tot[0], tested);
        if (inside) atomicAdd(&tot[1], inside);
        __syncthreads();
        if (tid == 0) {
            if (tot[0]) atomicAdd(&A.ctr[C_TESTED], tot[0]);
            if (tot[1]) atomicAdd(&A.ctr[C_INSIDE], tot[1]);
        }
    }
}

}  // namespace

RTMI_EXPORT int rtmi_gaussian_beams(rtmi_batch* b, int32_t fan_size, const rtmi_beam_params* bp, int32_t nw, const double* omega,
                                    double* u, rtmi_beam_stats* st) {
    const char* who = "rtmi_gaussian_beams";
    // ---- arguments, on the host
    RTMI_ARG(bp && omega && u, "null");
    RTMI_RC(check_grid_axes(who, *bp));
    RTMI_ARG(bp->eps > 0.0 && std::isfinite(bp->eps), "eps must be finite and > 0");
    RTMI_ARG(bp->cutoff >= 0.0 && std::isfinite(bp->cutoff) && bp->max_width >= 0.0 && std::isfinite(bp->max_width) &&
                 bp->edge_taper >= 0.0 && std::isfinite(bp->edge_taper),
             "cutoff, max_width and edge_taper must be finite and >= 0");
    RTMI_ARG(nw >= 1, "nw must be >= 1");
    double omin = INFINITY;
    for (int32_t q = 0; q < nw; q++) {
        RTMI_ARG(omega[q] > 0.0 && std::isfinite(omega[q]), "every omega must be finite and > 0");
        omin = omega[q] < omin ? omega[q] : omin;
    }
    RTMI_ARG(b, "null batch");
    RTMI_ARG(fan_size >= 2, "fan_size must be >= 2");
    Recorded rec;
    RTMI_RC(recorded(who, b, kRecIsotropic | kRecFromLaunch, fan_size, &rec));
    const rtmi_device_view& v = rec.v;
    const long R = (long)v.R, M = fan_size, S = R / M;
    std::vector<double> th0(R), w(R);
    RTMI_RC(rtmi_internal_batch_theta0(b, th0.data()));
    for (long s = 0; s < S; s++) {
        const double* t = th0.data() + s * M;
        const double dir = t[1] > t[0] ? 1.0 : -1.0;
        for (long m = 1; m < M; m++)
            RTMI_ARG(dir * (t[m] - t[m - 1]) > 0.0, "launch angles must be strictly monotone within a fan");
        for (long m = 0; m < M; m++) {
            double q = 0.5 * fabs(t[m < M - 1 ? m + 1 : m] - t[m > 0 ? m - 1 : m]);
            const double d = fmin(fabs(t[m] - t[0]), fabs(t[m] - t[M - 1]));
            if (bp->edge_taper > 0.0 && d < bp->edge_taper) q = q * (0.5 * (1.0 - cos(kPi * d / bp->edge_taper)));
            w[s * M + m] = q;
        }
    }
    Beam B{bp->gx0, bp->gdx, bp->gy0, bp->gdy, (int)bp->nx, (int)bp->ny, (int)((bp->nx + kTile - 1) / kTile),
           (int)((bp->ny + kTile - 1) / kTile), 0, bp->eps, bp->cutoff > 0.0 ? bp->cutoff : kCutoff,
           bp->max_width > 0.0 ? bp->max_width : kWidthCells * (bp->gdx > bp->gdy ? bp->gdx : bp->gdy), omin};
    B.ntiles = (long)B.ntx * B.nty;
    RTMI_ARG((double)S * (double)B.ntiles < 2147483648.0, "more than 2^31 tiles");

    // ---- (1) prep
    DevMem mem;
    EventMarks<4> ev;
    RTMI_HIP(ev.create());
    unsigned long long* ctr = nullptr;
    RTMI_HIP(mem.get(&ctr, C_N * sizeof(unsigned long long)));
    RTMI_HIP(hipMemset(ctr, 0, C_N * sizeof(unsigned long long)));
    double *tube = nullptr, *dw = nullptr;
    int32_t* slot = nullptr;
    long long *nrows = nullptr, *rowbase = nullptr;
    RTMI_HIP(mem.get(&tube, (size_t)v.rec_rows * 5 * R * sizeof(double)));
    RTMI_HIP(mem.get(&dw, (size_t)R * sizeof(double)));
    RTMI_HIP(mem.get(&nrows, (size_t)(R + 1) * sizeof(long long)));
    RTMI_HIP(mem.get(&rowbase, (size_t)(R + 1) * sizeof(long long)));
    RTMI_HIP(hipMemcpy(dw, w.data(), (size_t)R * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(ev.mark(0));
    RTMI_RC(rtmi_internal_paraxial_tube(who, b, tube));
    if (v.perm) {
        RTMI_HIP(mem.get(&slot, (size_t)R * sizeof(int32_t)));
        hipLaunchKernelGGL(k_inverse<int32_t>, blocks(R), dim3(256), 0, nullptr, v.perm, slot, R);
        RTMI_HIP(hipGetLastError());
    }
    by_dtype(v.dtype, [&](auto t) { hipLaunchKernelGGL(k_rows<decltype(t)>, blocks(R + 1), dim3(256), 0, nullptr, rows_of<decltype(t)>(v), slot, nrows); });
    RTMI_HIP(hipGetLastError());
    size_t scan_bytes = 0;
    void* scan_tmp = nullptr;
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nrows, rowbase, (int)(R + 1)));
    RTMI_HIP(mem.get(&scan_tmp, scan_bytes));
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, nrows, rowbase, (int)(R + 1)));
    long long Gll = 0;
    RTMI_HIP(hipMemcpy(&Gll, rowbase + R, sizeof(long long), hipMemcpyDeviceToHost));
    const long G = (long)Gll, nseg = G - R;
    RTMI_ARG(G < 2147483647L, "more than 2^31 recorded rows in the batch");
    double* rv = nullptr;
    int32_t* row_ray = nullptr;
    uint32_t* seg_row = nullptr;
    RTMI_HIP(mem.get(&rv, (size_t)kRowCols * G * sizeof(double)));
    RTMI_HIP(mem.get(&row_ray, (size_t)G * sizeof(int32_t)));
    RTMI_HIP(mem.get(&seg_row, (size_t)nseg * sizeof(uint32_t)));
    const PrepArgs pa{slot, tube, rowbase, dw, G, bp->eps, rv, row_ray, seg_row};
    by_dtype(v.dtype, [&](auto t) { hipLaunchKernelGGL(k_prep<decltype(t)>, blocks(R), dim3(256), 0, nullptr, rows_of<decltype(t)>(v), pa); });
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));

    // ---- (2) binning
    const long tiles = S * B.ntiles;
    uint32_t *begin = nullptr, *end = nullptr;
    RTMI_HIP(mem.get(&begin, (size_t)tiles * sizeof(uint32_t)));
    RTMI_HIP(mem.get(&end, (size_t)tiles * sizeof(uint32_t)));
    RTMI_HIP(hipMemset(begin, 0, (size_t)tiles * sizeof(uint32_t)));
    RTMI_HIP(hipMemset(end, 0, (size_t)tiles * sizeof(uint32_t)));
    unsigned long long *cnt = nullptr, *offs = nullptr;
    RTMI_HIP(mem.get(&cnt, (size_t)(nseg + 1) * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&offs, (size_t)(nseg + 1) * sizeof(unsigned long long)));
    BinArgs ba{rv, G, nseg, seg_row, row_ray, (int)M, cnt, offs, nullptr, nullptr, ctr};
    hipLaunchKernelGGL(k_count, blocks(nseg + 1), dim3(256), 0, nullptr, B, ba);
    RTMI_HIP(hipGetLastError());
    size_t cnt_bytes = 0;
    void* cnt_tmp = nullptr;
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cnt_bytes, cnt, offs, (int)(nseg + 1)));
    RTMI_HIP(mem.get(&cnt_tmp, cnt_bytes));
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(cnt_tmp, cnt_bytes, cnt, offs, (int)(nseg + 1)));
    unsigned long long E = 0;
    RTMI_HIP(hipMemcpy(&E, offs + nseg, sizeof(E), hipMemcpyDeviceToHost));
    RTMI_ARG(E < 2147483648ull, "more than 2^31 tile entries (a smaller grid or fewer sources per call)");
    const uint32_t* sorted = nullptr;
    if (E > 0) {
        uint32_t *keys = nullptr, *keys2 = nullptr, *vals = nullptr, *vals2 = nullptr;
        RTMI_HIP(mem.get(&keys, E * sizeof(uint32_t)));
        RTMI_HIP(mem.get(&keys2, E * sizeof(uint32_t)));
        RTMI_HIP(mem.get(&vals, E * sizeof(uint32_t)));
        RTMI_HIP(mem.get(&vals2, E * sizeof(uint32_t)));
        ba.keys = keys; ba.vals = vals;
        hipLaunchKernelGGL(k_fill, blocks(nseg), dim3(256), 0, nullptr, B, ba);
        RTMI_HIP(hipGetLastError());
        int bits = 1;
        while (bits < 32 && ((unsigned long long)tiles >> bits) != 0ull) bits++;
        size_t sort_bytes = 0;
        void* sort_tmp = nullptr;
        RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, keys2, vals, vals2, (int)E, 0, bits));
        RTMI_HIP(mem.get(&sort_tmp, sort_bytes));
        RTMI_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, keys, keys2, vals, vals2, (int)E, 0, bits));
        hipLaunchKernelGGL(k_ranges, blocks((long)E), dim3(256), 0, nullptr, keys2, (long)E, begin, end);
        RTMI_HIP(hipGetLastError());
        sorted = vals2;
    }
    RTMI_HIP(ev.mark(2));

    // ---- (3) gather, kNwb frequencies per launch
    double* du = nullptr;
    const size_t un = (size_t)S * nw * bp->ny * bp->nx * 2;
    RTMI_HIP(mem.get(&du, un * sizeof(double)));
    for (int32_t w0 = 0; w0 < nw; w0 += kNwb) {
        GatherArgs ga{};
        ga.rv = rv; ga.G = G; ga.vals = sorted; ga.begin = begin; ga.end = end;
        ga.nwg = nw - w0 < kNwb ? nw - w0 : kNwb;
        for (int q = 0; q < kNwb; q++) ga.om[q] = q < ga.nwg ? omega[w0 + q] : 0.0;
        ga.w0 = w0; ga.nw = nw; ga.u = du; ga.ctr = ctr; ga.count_pairs = w0 == 0;
        hipLaunchKernelGGL(k_gather, dim3((unsigned)tiles), dim3(kBlock), 0, nullptr, B, ga);
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(3));
    RTMI_HIP(ev.wait(3));
    RTMI_HIP(hipMemcpy(u, du, un * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        unsigned long long c[C_N];
        RTMI_HIP(hipMemcpy(c, ctr, sizeof(c), hipMemcpyDeviceToHost));
        *st = rtmi_beam_stats{};
        st->segments = nseg; st->tile_entries = (int64_t)E;
        st->pairs_tested = (int64_t)c[C_TESTED]; st->pairs_inside = (int64_t)c[C_INSIDE]; st->capped = (int64_t)c[C_CAPPED];
        st->cutoff = B.cutoff; st->max_width = B.maxw;
        double* ms[3] = {&st->prep_ms, &st->bin_ms, &st->gather_ms};
        for (int q = 0; q < 3; q++) RTMI_HIP(ev.ms(q, q + 1, ms[q]));
    }
    return RTMI_OK;
}
