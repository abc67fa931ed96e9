// ttgrid.hip -- traveltime (and amplitude) tables on a regular grid from recorded fans of rays: the ray-cell method.  First arrivals
// (rtmi_first_arrival_grid, rtmi_debug_grid_rows) and the karr earliest or most energetic arrivals
// (rtmi_arrival_grid, rtmi_debug_arrival_rows; section 18, and the kernels' own comment below).
//
// Adjacent rays m, m+1 of one fan and rows i, i+1 span the cell (m, i) with corners A = (m, i), B = (m+1, i), C = (m, i+1),
// D = (m+1, i+1); it is split into the triangles ABD (half 0) and ADC (half 1), over which T, the launch angle, the direction
// and the spread are linear.  Every grid node keeps the smallest T of the triangles that cover it, in three passes that give
// the same bits in every schedule: (1) rasterize, atomicMin on the bits of T (T >= 0: the IEEE order is the integer order) and
// count the covering triangles; (2) rasterize again, and where a triangle's T bits equal the node's minimum, atomicMin on the
// triangle's key (m rec_rows + i) 2 + half; (3) one lane per node decodes the winning key and evaluates the columns with the
// function that gave T in pass 1.  Each atomicMin is preceded by a plain load and skipped when it cannot win.
//
// One lane per cell column (source s, ray pair m, m+1) walks the rows of both rays, each row's x, y, T, theta read once per
// lane (the neighbouring lane reads the same lines).  Arithmetic is fp64 in one fixed order (-ffp-contract=off), so that
// tests/ttgrid_ref.py, a numpy restatement, follows it operation for operation.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_rows.h"
#include "rtmi_host.h"

namespace {

constexpr int kColsT = 5;                   // T theta0 theta ray step
constexpr int kColsA = 8;                   // ... J G kmah
constexpr double kTwoPi = 6.283185307179586;
constexpr unsigned long long kEmpty = ~0ull;
// the defaults of rtmi_grid_params (include/rtmi.h says why)
constexpr double kGapCells = 8.0;
constexpr double kDtheta = 0.25;

// stats counters (device, uint64): cells, skipped, triangles, folded, pass-1 adds, pass-1 mins, pass-2 mins
enum { C_CELLS, C_SKIP, C_TRI, C_FOLD, C_ADD1, C_MIN1, C_MIN2, C_N };

struct Grid {
    double gx0, gdx, gy0, gdy;
    int nx, ny;
    double max_gap, max_dtheta;
    double inv_gdx, inv_gdy;    // for the cell pre-test only (cell_has_node); every node test is exact
};

// what the passes read beside the rows, and the fans: S sources of M rays each
struct Rec {
    const int32_t* slot;        // [R] or NULL: slot of the caller's ray o (the inverse of rtmi_device_view.perm)
    const double* theta0;       // [R] caller order, or NULL: row 0's theta
    const double* row_J;        // [rec_rows][R] slot order, or NULL (no amplitude)
    const int32_t* row_kmah;
    int M, S;
};

struct Nodes {
    unsigned long long* tmin;   // [S][ny][nx]
    unsigned long long* key;
    int32_t* count;
    unsigned long long* ctr;    // [C_N]
};

struct V2 { double x, y; };
struct Corner { double x, y, t, th; };

template <typename T> __device__ __forceinline__ Corner corner(const Rows<T>& rec, long k, long i) {
    const T* p = rec.row(i, k);
    return Corner{(double)p[COL_X * rec.R], (double)p[COL_Y * rec.R], (double)p[COL_T * rec.R], (double)p[COL_TH * rec.R]};
}

__device__ __forceinline__ double wrap(double d) { return d - kTwoPi * rint(d / kTwoPi); }

// cross(b - a, p - a), anchored at the lexicographically smaller endpoint: edge(b, a, p) == -edge(a, b, p) bit for bit, so
// that two triangles sharing an edge see one value with opposite signs
__device__ __forceinline__ double edge(V2 a, V2 b, V2 p) {
    if (a.x < b.x || (a.x == b.x && a.y < b.y)) return (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x);
    return -((a.x - b.x) * (p.y - b.y) - (a.y - b.y) * (p.x - b.x));
}
// the top-left rule of a counter-clockwise triangle (y up): an edge whose direction points down, or left when horizontal
__device__ __forceinline__ bool top_left(V2 a, V2 b) {
    const double dy = b.y - a.y;
    return dy < 0.0 || (dy == 0.0 && b.x - a.x < 0.0);
}

// One triangle of a cell: its vertices v[0..2] counter-clockwise and which cell corner (0 A, 1 B, 2 C, 3 D) each one is.
struct Tri {
    V2 v[3];
    int c[3];
    double xmin, xmax, ymin, ymax;
    int folded;
};
// half 0: triangle ABD taken as A D B, half 1: ADC taken as A C D -- counter-clockwise in a fan whose rays are ordered by
// increasing launch angle.  false: zero signed area (skipped); a negative area (a fold) is re-oriented
__device__ __forceinline__ bool tri_setup(const V2 q[4], int half, Tri& t) {
    t.c[0] = 0; t.c[1] = half ? 2 : 3; t.c[2] = half ? 3 : 1;
    t.v[0] = q[t.c[0]]; t.v[1] = q[t.c[1]]; t.v[2] = q[t.c[2]];
    const double a = edge(t.v[0], t.v[1], t.v[2]);
    if (a == 0.0 || !(a == a)) return false;
    t.folded = a < 0.0;
    if (t.folded) {
        const V2 v = t.v[1]; t.v[1] = t.v[2]; t.v[2] = v;
        const int c = t.c[1]; t.c[1] = t.c[2]; t.c[2] = c;
    }
    t.xmin = fmin(fmin(t.v[0].x, t.v[1].x), t.v[2].x); t.xmax = fmax(fmax(t.v[0].x, t.v[1].x), t.v[2].x);
    t.ymin = fmin(fmin(t.v[0].y, t.v[1].y), t.v[2].y); t.ymax = fmax(fmax(t.v[0].y, t.v[1].y), t.v[2].y);
    return true;
}
// Barycentric weights (unnormalised) of p; true when p is inside the closed bounding box and inside the triangle by the
// top-left rule: w_k >= 0 for the edge opposite vertex k, with equality only on a top or left edge
__device__ __forceinline__ bool tri_weights(const Tri& t, V2 p, double w[3]) {
    if (p.x < t.xmin || p.x > t.xmax || p.y < t.ymin || p.y > t.ymax) return false;
    w[0] = edge(t.v[1], t.v[2], p);
    w[1] = edge(t.v[2], t.v[0], p);
    w[2] = edge(t.v[0], t.v[1], p);
    const bool i0 = w[0] > 0.0 || (w[0] == 0.0 && top_left(t.v[1], t.v[2]));
    const bool i1 = w[1] > 0.0 || (w[1] == 0.0 && top_left(t.v[2], t.v[0]));
    const bool i2 = w[2] > 0.0 || (w[2] == 0.0 && top_left(t.v[0], t.v[1]));
    return i0 && i1 && i2;
}
// the linear interpolant: ((w0 f0 + w1 f1) + w2 f2) / ((w0 + w1) + w2)
__device__ __forceinline__ double interp(const double w[3], double f0, double f1, double f2) {
    return ((w[0] * f0 + w[1] * f1) + w[2] * f2) / ((w[0] + w[1]) + w[2]);
}

__device__ __forceinline__ V2 node_xy(const Grid& g, int ix, int iy) { return V2{g.gx0 + (double)ix * g.gdx, g.gy0 + (double)iy * g.gdy}; }
// the node index range that can hold [lo, hi] (one node of margin; the exact test is tri_weights' bounding box)
__device__ __forceinline__ void node_range(double lo, double hi, double o, double h, int n, int& a, int& b) {
    double fa = floor((lo - o) / h) - 1.0, fb = ceil((hi - o) / h) + 1.0;
    fa = fa < 0.0 ? 0.0 : (fa > (double)n ? (double)n : fa);
    fb = fb > (double)(n - 1) ? (double)(n - 1) : (fb < -1.0 ? -1.0 : fb);
    a = (int)fa; b = (int)fb;
}

// the cell rule: both rays present at rows i and i+1 (the caller's loop), neighbours no further apart than max_gap at either
// row, and turned against each other by no more than max_dtheta
__device__ __forceinline__ bool cell_ok(const Grid& g, const Corner& a, const Corner& b, const Corner& c, const Corner& d) {
    const double dx0 = b.x - a.x, dy0 = b.y - a.y, dx1 = d.x - c.x, dy1 = d.y - c.y;
    if (!(sqrt(dx0 * dx0 + dy0 * dy0) <= g.max_gap) || !(sqrt(dx1 * dx1 + dy1 * dy1) <= g.max_gap)) return false;
    return fabs(wrap(b.th - a.th)) <= g.max_dtheta && fabs(wrap(d.th - c.th)) <= g.max_dtheta;
}

// Can [lo, hi] hold a node coordinate o + i h, 0 <= i < n?  Conservative by 1e-6 of a spacing (far above the rounding of o + i h):
// a false answer is exact, so skipping the cell's node loops changes no result.  No division: most cells of a dense fan hold no node.
__device__ __forceinline__ bool axis_has_node(double lo, double hi, double o, double inv, int n) {
    const double a = ceil((lo - o) * inv - 1e-6), b = floor((hi - o) * inv + 1e-6);
    return a <= b && b >= 0.0 && a <= (double)(n - 1);
}
__device__ __forceinline__ bool cell_has_node(const Grid& g, const V2 q[4]) {
    const double xl = fmin(fmin(q[0].x, q[1].x), fmin(q[2].x, q[3].x)), xh = fmax(fmax(q[0].x, q[1].x), fmax(q[2].x, q[3].x));
    if (!axis_has_node(xl, xh, g.gx0, g.inv_gdx, g.nx)) return false;
    const double yl = fmin(fmin(q[0].y, q[1].y), fmin(q[2].y, q[3].y)), yh = fmax(fmax(q[0].y, q[1].y), fmax(q[2].y, q[3].y));
    return axis_has_node(yl, yh, g.gy0, g.inv_gdy, g.ny);
}

__device__ __forceinline__ long slot_of(const Rec& r, long o) { return r.slot ? (long)r.slot[o] : o; }

__device__ __forceinline__ void block_add(unsigned long long* acc, int q, unsigned long long v) {
    if (v) atomicAdd(&acc[q], v);
}

// The raster walk of one lane, (source s, ray pair m, m+1), down the rows of both rays: visit(at, bits, key, t, w, k, i) for
// every candidate -- node `at` of [S][ny][nx] that triangle `key` of cell (m, i) covers with 0 <= T < inf, bits those of T, t and w
// the triangle and the node's weights in it, k the slots of rays m and m+1.
struct Walk { unsigned long long cells, skipped, tri, folded; };
template <typename T, typename F> __device__ __forceinline__ void walk(const Grid& g, const Rows<T>& rec, const Rec& r, long lane, Walk& n,
                                                                      F&& visit) {
    const long pairs = (long)r.M - 1;
    if (lane >= (long)r.S * pairs) return;
    const long s = lane / pairs, m = lane - s * pairs;
    const long o = s * r.M + m;
    const long k[2] = {slot_of(r, o), slot_of(r, o + 1)};
    const long l0 = rec.last_recorded(k[0]), l1 = rec.last_recorded(k[1]);
    const long L = l0 < l1 ? l0 : l1;
    const size_t base = (size_t)s * g.ny * g.nx;
    Corner A = corner(rec, k[0], 0), B = corner(rec, k[1], 0);
    for (long i = 0; i < L; i++) {
        const Corner C = corner(rec, k[0], i + 1), D = corner(rec, k[1], i + 1);
        n.cells++;
        if (!cell_ok(g, A, B, C, D)) {
            n.skipped++;
        } else {
            const V2 q[4] = {{A.x, A.y}, {B.x, B.y}, {C.x, C.y}, {D.x, D.y}};
            const double tq[4] = {A.t, B.t, C.t, D.t};
            const bool nodes = cell_has_node(g, q);
            for (int half = 0; half < 2; half++) {
                Tri t;
                if (!tri_setup(q, half, t)) continue;
                n.tri++;
                n.folded += t.folded;
                if (!nodes) continue;
                const unsigned long long key = ((unsigned long long)(m * rec.rec_rows + i) << 1) | (unsigned long long)half;
                int x0, x1, y0, y1;
                node_range(t.xmin, t.xmax, g.gx0, g.gdx, g.nx, x0, x1);
                node_range(t.ymin, t.ymax, g.gy0, g.gdy, g.ny, y0, y1);
                for (int iy = y0; iy <= y1; iy++)
                    for (int ix = x0; ix <= x1; ix++) {
                        double w[3];
                        if (!tri_weights(t, node_xy(g, ix, iy), w)) continue;
                        const double tv = interp(w, tq[t.c[0]], tq[t.c[1]], tq[t.c[2]]);
                        if (!(tv >= 0.0 && tv < INFINITY)) continue;
                        visit(base + (size_t)iy * g.nx + ix, (unsigned long long)__double_as_longlong(tv), key, t, w, k, i);
                    }
            }
        }
        A = C; B = D;
    }
}

// Passes 1 and 2: one lane per (source, ray pair).  pass 1: T minimum and count; pass 2: the key of the winner.
template <typename T> __global__ void k_raster(Grid g, Rows<T> rec, Rec r, Nodes nd, int pass) {
    __shared__ unsigned long long acc[C_N];
    if (threadIdx.x < C_N) acc[threadIdx.x] = 0ull;
    __syncthreads();
    Walk n{};
    unsigned long long n_add = 0, n_min = 0;
    walk(g, rec, r, (long)blockIdx.x * blockDim.x + threadIdx.x, n,
         [&](size_t at, unsigned long long bits, unsigned long long key, const Tri&, const double*, const long*, long) {
             if (pass == 1) {
                 atomicAdd(&nd.count[at], 1);
                 n_add++;
                 if (bits < __hip_atomic_load(&nd.tmin[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                     atomicMin(&nd.tmin[at], bits);
                     n_min++;
                 }
             } else if (bits == __hip_atomic_load(&nd.tmin[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &&
                        key < __hip_atomic_load(&nd.key[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                 atomicMin(&nd.key[at], key);
                 n_min++;
             }
         });
    if (pass == 1) {
        block_add(acc, C_CELLS, n.cells); block_add(acc, C_SKIP, n.skipped); block_add(acc, C_TRI, n.tri);
        block_add(acc, C_FOLD, n.folded); block_add(acc, C_ADD1, n_add); block_add(acc, C_MIN1, n_min);
    } else {
        block_add(acc, C_MIN2, n_min);
    }
    __syncthreads();
    if (threadIdx.x < C_N && acc[threadIdx.x]) atomicAdd(&nd.ctr[threadIdx.x], acc[threadIdx.x]);
}

// n |J| at a node: J and n = |(p_x, p_y)| of the triangle's corners interpolated -- the product under G's square root, and the
// criterion of RTMI_ARRIVAL_BY_AMPLITUDE.  k, row: slot and row of the cell's corners A B C D.
template <typename T> __device__ __forceinline__ double spread(const Rows<T>& rec, const Rec& r, const long k[4], const long row[4],
                                                               const Tri& t, const double w[3], double* Jn) {
    double J[3], n[3];
    for (int v = 0; v < 3; v++) {
        const int q = t.c[v];
        J[v] = r.row_J[(size_t)row[q] * rec.R + k[q]];
        const T* p = rec.row(row[q], k[q]);
        const double px = (double)p[COL_PX * rec.R], py = (double)p[COL_PY * rec.R];
        n[v] = sqrt(px * px + py * py);
    }
    *Jn = interp(w, J[0], J[1], J[2]);
    return interp(w, n[0], n[1], n[2]) * fabs(*Jn);
}

// The columns of node (ix, iy) of source s in the triangle `key`: o[q per], q < ncols.
template <typename T> __device__ __forceinline__ void node_columns(const Grid& g, const Rows<T>& rec, const Rec& r, long s, int ix, int iy,
                                                                   unsigned long long key, double* o, size_t per, int ncols) {
    const int half = (int)(key & 1ull);
    const long m = (long)((key >> 1) / (unsigned long long)rec.rec_rows), i = (long)((key >> 1) - (unsigned long long)m * rec.rec_rows);
    const long oa = s * r.M + m;
    const long k[4] = {slot_of(r, oa), slot_of(r, oa + 1), slot_of(r, oa), slot_of(r, oa + 1)};
    const long row[4] = {i, i, i + 1, i + 1};
    Corner c4[4];
    for (int q = 0; q < 4; q++) c4[q] = corner(rec, k[q], row[q]);
    const V2 q4[4] = {{c4[0].x, c4[0].y}, {c4[1].x, c4[1].y}, {c4[2].x, c4[2].y}, {c4[3].x, c4[3].y}};
    Tri t;
    tri_setup(q4, half, t);
    double w[3];
    tri_weights(t, node_xy(g, ix, iy), w);
    const int a = t.c[0], b = t.c[1], c = t.c[2];
    double th0[4];
    for (int q = 0; q < 4; q++)
        th0[q] = r.theta0 ? r.theta0[oa + (q & 1)] : (double)rec.row(0, k[q])[COL_TH * rec.R];
    double thu[4];
    for (int q = 0; q < 4; q++) thu[q] = c4[0].th + wrap(c4[q].th - c4[0].th);
    const double fr[4] = {0.0, 1.0, 0.0, 1.0}, fs[4] = {0.0, 0.0, 1.0, 1.0};
    o[0] = interp(w, c4[a].t, c4[b].t, c4[c].t);
    o[per] = interp(w, th0[a], th0[b], th0[c]);
    o[2 * per] = interp(w, thu[a], thu[b], thu[c]);
    o[3 * per] = (double)m + interp(w, fr[a], fr[b], fr[c]);
    o[4 * per] = (double)i + interp(w, fs[a], fs[b], fs[c]);
    if (ncols == kColsA) {
        double Jn;
        const double nJ = spread(rec, r, k, row, t, w, &Jn);
        // kmah: the corner of the largest weight (the first in a, b, c on a tie)
        const int kk = w[0] >= w[1] ? (w[0] >= w[2] ? a : c) : (w[1] >= w[2] ? b : c);
        o[5 * per] = Jn;
        o[6 * per] = 1.0 / sqrt(nJ);
        o[7 * per] = (double)r.row_kmah[(size_t)row[kk] * rec.R + k[kk]];
    }
}

// Pass 3: one lane per node.  out[s][col][ny][nx]; NaN where no triangle covers the node.
template <typename T> __global__ void k_columns(Grid g, Rows<T> rec, Rec r, Nodes nd, double* out, int ncols) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)g.nx * g.ny;
    if (id >= (long)r.S * per) return;
    const long s = id / per, at = id - s * per;
    const int iy = (int)(at / g.nx), ix = (int)(at - (long)iy * g.nx);
    double* o = out + (size_t)s * ncols * per + at;
    const unsigned long long key = nd.key[id];
    if (nd.count[id] == 0 || key == kEmpty) {
        for (int q = 0; q < ncols; q++) o[(size_t)q * per] = NAN;
        return;
    }
    node_columns(g, rec, r, s, ix, iy, key, o, (size_t)per, ncols);
}

// ---- later arrivals (rtmi_arrival_grid): every candidate kept in a list, no minimum atomics.  (a) the walk counts per node;
// (b) an exclusive scan of the counts gives each node its range of the list; (c) the walk again, each candidate taking the next
// place of its node's range (a returning atomicAdd on the node's cursor) and storing (bits of c, key) with one 16-byte store;
// (d) one lane per node selects its karr least entries by (bits, key) and writes their columns.  Which place a candidate takes
// depends on the schedule, which entries a node holds does not: the selection is by value.
struct List {
    int32_t* count;                 // [nodes]
    unsigned long long* cursor;     // [nodes + 1]: the scan's offsets; after pass (c) the end of each node's range
    ulonglong2* entry;              // [total]: x the bits of c, y the key
    unsigned long long total;
    unsigned long long* ctr;        // [C_N]
};

// passes (a) and (c), one lane per (source, ray pair).  A template argument, so that the count pass and the fill by time carry
// none of the amplitude's loads and registers.
enum { kCount, kFillByTime, kFillByAmplitude };
template <typename T, int MODE> __global__ void k_gather(Grid g, Rows<T> rec, Rec r, List ls) {
    constexpr bool fill = MODE != kCount;
    __shared__ unsigned long long acc[C_N];
    if (threadIdx.x < C_N) acc[threadIdx.x] = 0ull;
    __syncthreads();
    Walk n{};
    unsigned long long n_add = 0;
    walk(g, rec, r, (long)blockIdx.x * blockDim.x + threadIdx.x, n,
         [&](size_t at, unsigned long long bits, unsigned long long key, const Tri& t, const double* w, const long* k, long i) {
             n_add++;
             if (!fill) {
                 atomicAdd(&ls.count[at], 1);
                 return;
             }
             if (MODE == kFillByAmplitude) {
                 const long k4[4] = {k[0], k[1], k[0], k[1]}, row[4] = {i, i, i + 1, i + 1};
                 double Jn;
                 const double c = spread(rec, r, k4, row, t, w, &Jn);
                 bits = (unsigned long long)__double_as_longlong(c >= 0.0 && c < INFINITY ? c : INFINITY);
             }
             const unsigned long long e = atomicAdd(&ls.cursor[at], 1ull);
             if (e < ls.total) ls.entry[e] = make_ulonglong2(bits, key);
         });
    if (!fill) {
        block_add(acc, C_CELLS, n.cells); block_add(acc, C_SKIP, n.skipped); block_add(acc, C_TRI, n.tri);
        block_add(acc, C_FOLD, n.folded); block_add(acc, C_ADD1, n_add);
    } else {
        block_add(acc, C_MIN1, n_add);
    }
    __syncthreads();
    if (threadIdx.x < C_N && acc[threadIdx.x]) atomicAdd(&ls.ctr[threadIdx.x], acc[threadIdx.x]);
}

// the counts widened for the scan; cursor[nodes] = 0, so that the exclusive sum leaves the total there
__global__ void k_widen(const int32_t* count, unsigned long long* cursor, long nodes) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id <= nodes) cursor[id] = id < nodes ? (unsigned long long)count[id] : 0ull;
}

// Pass (d): one lane per node.  out[s][k][col][ny][nx]: arrival k is the k-th of the node's entries by (bits, key), found by
// repeated selection of the least entry above the one before (keys differ within a node); NaN for k >= count.
template <typename T> __global__ void k_select(Grid g, Rows<T> rec, Rec r, List ls, double* out, int ncols, int karr) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)g.nx * g.ny;
    if (id >= (long)r.S * per) return;
    const long s = id / per, at = id - s * per;
    const int iy = (int)(at / g.nx), ix = (int)(at - (long)iy * g.nx);
    const unsigned long long end = ls.cursor[id] <= ls.total ? ls.cursor[id] : ls.total;
    const unsigned long long cnt = (unsigned long long)ls.count[id], begin = end >= cnt ? end - cnt : end;
    ulonglong2 prev = make_ulonglong2(0ull, 0ull);
    for (int a = 0; a < karr; a++) {
        double* o = out + ((size_t)s * karr + a) * ncols * per + at;
        ulonglong2 best = make_ulonglong2(kEmpty, kEmpty);
        for (unsigned long long e = begin; e < end; e++) {
            const ulonglong2 v = ls.entry[e];
            const bool above = a == 0 || v.x > prev.x || (v.x == prev.x && v.y > prev.y);
            if (above && (v.x < best.x || (v.x == best.x && v.y < best.y))) best = v;
        }
        if (best.y == kEmpty) {
            for (int q = 0; q < ncols; q++) o[(size_t)q * per] = NAN;
        } else {
            node_columns(g, rec, r, s, ix, iy, best.y, o, (size_t)per, ncols);
            prev = best;
        }
    }
}

// the grid parameters checked and the defaults filled in (host)
int grid_of(const rtmi_grid_params* gp, const char* who, Grid* g) {
    RTMI_ARG(gp, "null grid parameters");
    RTMI_RC(check_grid_axes(who, *gp));
    RTMI_ARG(gp->max_gap >= 0.0 && std::isfinite(gp->max_gap) && gp->max_dtheta >= 0.0 && std::isfinite(gp->max_dtheta),
             "max_gap and max_dtheta must be finite and >= 0");
    RTMI_ARG(gp->amplitude == 0 || gp->amplitude == 1, "amplitude must be 0 or 1");
    *g = Grid{gp->gx0, gp->gdx, gp->gy0, gp->gdy, (int)gp->nx, (int)gp->ny,
              gp->max_gap > 0.0 ? gp->max_gap : kGapCells * (gp->gdx > gp->gdy ? gp->gdx : gp->gdy),
              gp->max_dtheta > 0.0 ? gp->max_dtheta : kDtheta, 1.0 / gp->gdx, 1.0 / gp->gdy};
    return RTMI_OK;
}

// The three passes on a record already on the device, results to the host.
template <typename T> int run_grid(const char* who, const Grid& g, const Rows<T>& rec, const Rec& r, int32_t* count, double* out,
                                   rtmi_grid_stats* st) {
    const size_t per = (size_t)g.nx * g.ny, nodes = per * (size_t)r.S;
    const int ncols = r.row_J ? kColsA : kColsT;
    DevMem mem;
    Nodes nd{};
    double* dout = nullptr;
    RTMI_HIP(mem.get(&nd.tmin, nodes * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&nd.key, nodes * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&nd.count, nodes * sizeof(int32_t)));
    RTMI_HIP(mem.get(&nd.ctr, C_N * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&dout, nodes * ncols * sizeof(double)));
    RTMI_HIP(hipMemset(nd.tmin, 0xff, nodes * sizeof(unsigned long long)));
    RTMI_HIP(hipMemset(nd.key, 0xff, nodes * sizeof(unsigned long long)));
    RTMI_HIP(hipMemset(nd.count, 0, nodes * sizeof(int32_t)));
    RTMI_HIP(hipMemset(nd.ctr, 0, C_N * sizeof(unsigned long long)));
    EventMarks<4> ev;
    RTMI_HIP(ev.create());
    const long lanes = (long)r.S * (r.M - 1);
    const dim3 blk(256), gl = blocks(lanes), gn = blocks((long)nodes);
    RTMI_HIP(ev.mark(0));
    for (int pass = 1; pass <= 2; pass++) {
        if (lanes > 0) {
            hipLaunchKernelGGL(k_raster<T>, gl, blk, 0, nullptr, g, rec, r, nd, pass);
            RTMI_HIP(hipGetLastError());
        }
        RTMI_HIP(ev.mark(pass));
    }
    hipLaunchKernelGGL(k_columns<T>, gn, blk, 0, nullptr, g, rec, r, nd, dout, ncols);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(3));
    RTMI_HIP(ev.wait(3));
    RTMI_HIP(hipMemcpy(count, nd.count, nodes * sizeof(int32_t), hipMemcpyDeviceToHost));
    RTMI_HIP(hipMemcpy(out, dout, nodes * ncols * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        unsigned long long c[C_N];
        RTMI_HIP(hipMemcpy(c, nd.ctr, sizeof(c), hipMemcpyDeviceToHost));
        *st = rtmi_grid_stats{};
        st->cells = (int64_t)c[C_CELLS]; st->skipped_cells = (int64_t)c[C_SKIP];
        st->triangles = (int64_t)c[C_TRI]; st->folded = (int64_t)c[C_FOLD];
        st->atomics[0] = c[C_ADD1]; st->atomics[1] = c[C_MIN1]; st->atomics[2] = c[C_MIN2];
        st->max_gap = g.max_gap; st->max_dtheta = g.max_dtheta;
        for (int q = 0; q < 3; q++) RTMI_HIP(ev.ms(q, q + 1, &st->pass_ms[q]));
    }
    return RTMI_OK;
}

// The four passes of rtmi_arrival_grid on a record already on the device, results to the host.  out NULL: passes (a) and (b) only.
template <typename T> int run_arrivals(const char* who, const Grid& g, const Rows<T>& rec, const Rec& r, int ncols,
                                       const rtmi_arrival_params& ap, int32_t* count, double* out, rtmi_arrival_stats* st) {
    const size_t per = (size_t)g.nx * g.ny, nodes = per * (size_t)r.S;
    RTMI_ARG(nodes < (size_t)2147483647, "more than 2^31 - 2 nodes in one call (fewer sources per call)");
    DevMem mem;
    List ls{};
    RTMI_HIP(mem.get(&ls.count, nodes * sizeof(int32_t)));
    RTMI_HIP(mem.get(&ls.cursor, (nodes + 1) * sizeof(unsigned long long)));
    RTMI_HIP(mem.get(&ls.ctr, C_N * sizeof(unsigned long long)));
    size_t scan_bytes = 0;
    void* scan_tmp = nullptr;
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, ls.cursor, (int)(nodes + 1)));
    RTMI_HIP(mem.get(&scan_tmp, scan_bytes));
    RTMI_HIP(hipMemset(ls.count, 0, nodes * sizeof(int32_t)));
    RTMI_HIP(hipMemset(ls.ctr, 0, C_N * sizeof(unsigned long long)));
    EventMarks<6> ev;
    RTMI_HIP(ev.create());
    const long lanes = (long)r.S * (r.M - 1);
    const dim3 blk(256), gl = blocks(lanes), gn = blocks((long)nodes);
    RTMI_HIP(ev.mark(0));
    if (lanes > 0) {
        hipLaunchKernelGGL((k_gather<T, kCount>), gl, blk, 0, nullptr, g, rec, r, ls);
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(1));
    hipLaunchKernelGGL(k_widen, blocks((long)nodes + 1), blk, 0, nullptr, ls.count, ls.cursor, (long)nodes);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, ls.cursor, (int)(nodes + 1)));
    RTMI_HIP(ev.mark(2));
    RTMI_HIP(hipMemcpy(&ls.total, ls.cursor + nodes, sizeof(ls.total), hipMemcpyDeviceToHost));
    double* dout = nullptr;
    const size_t nout = nodes * (size_t)ap.karr * ncols;
    if (out) {
        RTMI_HIP(mem.get(&ls.entry, (size_t)ls.total * sizeof(ulonglong2)));
        RTMI_HIP(mem.get(&dout, nout * sizeof(double)));
    }
    RTMI_HIP(ev.mark(3));
    if (out && lanes > 0) {
        if (ap.order == RTMI_ARRIVAL_BY_AMPLITUDE)
            hipLaunchKernelGGL((k_gather<T, kFillByAmplitude>), gl, blk, 0, nullptr, g, rec, r, ls);
        else
            hipLaunchKernelGGL((k_gather<T, kFillByTime>), gl, blk, 0, nullptr, g, rec, r, ls);
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(4));
    if (out) {
        hipLaunchKernelGGL(k_select<T>, gn, blk, 0, nullptr, g, rec, r, ls, dout, ncols, (int)ap.karr);
        RTMI_HIP(hipGetLastError());
    }
    RTMI_HIP(ev.mark(5));
    RTMI_HIP(ev.wait(5));
    RTMI_HIP(hipMemcpy(count, ls.count, nodes * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out) RTMI_HIP(hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost));
    if (st) {
        unsigned long long c[C_N];
        RTMI_HIP(hipMemcpy(c, ls.ctr, sizeof(c), hipMemcpyDeviceToHost));
        *st = rtmi_arrival_stats{};
        st->cells = (int64_t)c[C_CELLS]; st->skipped_cells = (int64_t)c[C_SKIP];
        st->triangles = (int64_t)c[C_TRI]; st->folded = (int64_t)c[C_FOLD];
        st->atomics[0] = c[C_ADD1]; st->atomics[1] = c[C_MIN1];
        st->max_gap = g.max_gap; st->max_dtheta = g.max_dtheta;
        st->candidates = (int64_t)ls.total;
        RTMI_HIP(ev.ms(0, 1, &st->pass_ms[0])); RTMI_HIP(ev.ms(3, 4, &st->pass_ms[1])); RTMI_HIP(ev.ms(4, 5, &st->pass_ms[2]));
        RTMI_HIP(ev.ms(1, 2, &st->scan_ms));
    }
    return RTMI_OK;
}

// rtmi_arrival_params checked (host): before any device work
int arrivals_of(const rtmi_arrival_params* ap, const char* who) {
    RTMI_ARG(ap, "null arrival parameters");
    RTMI_ARG(ap->karr >= 1 && ap->karr <= RTMI_MAX_ARRIVALS, "karr must be 1 .. 16");
    RTMI_ARG(ap->order == RTMI_ARRIVAL_BY_TIME || ap->order == RTMI_ARRIVAL_BY_AMPLITUDE,
             "order must be RTMI_ARRIVAL_BY_TIME or RTMI_ARRIVAL_BY_AMPLITUDE");
    return RTMI_OK;
}

// What both batch entries prepare on the device: the inverse of the view's permutation, and with amplitude the per-row J, kmah.
struct FanRec {
    DevMem mem;
    Recorded rec;
    Rec r{};
};
int fan_rec(const char* who, rtmi_batch* b, int32_t fan_size, bool amplitude, FanRec* f) {
    RTMI_ARG(fan_size >= 2, "fan_size must be >= 2");
    RTMI_RC(recorded(who, b, (amplitude ? kRecIsotropic : 0u) | kRecFromLaunch, fan_size, &f->rec));
    const rtmi_device_view& v = f->rec.v;
    const size_t R = (size_t)v.R;
    int32_t* slot = nullptr;
    double* rj = nullptr;
    int32_t* rk = nullptr;
    if (v.perm) {
        RTMI_HIP(f->mem.get(&slot, R * sizeof(int32_t)));
        hipLaunchKernelGGL(k_inverse<int32_t>, blocks((long)R), dim3(256), 0, nullptr, v.perm, slot, (long)R);
        RTMI_HIP(hipGetLastError());
    }
    if (amplitude) {
        const size_t cells = (size_t)v.rec_rows * R;
        RTMI_HIP(f->mem.get(&rj, cells * sizeof(double)));
        RTMI_HIP(f->mem.get(&rk, cells * sizeof(int32_t)));
        RTMI_HIP(hipMemset(rj, 0xff, cells * sizeof(double)));         // NaN (and kmah -1) on rows no ray reaches
        RTMI_HIP(hipMemset(rk, 0xff, cells * sizeof(int32_t)));
        RTMI_RC(rtmi_internal_paraxial_rows(who, b, rj, rk));
    }
    f->r = Rec{slot, nullptr, rj, rk, (int)fan_size, (int)(v.R / fan_size)};
    return RTMI_OK;
}

// caller-supplied rows as a record on the device: x, y, T, theta and, where given, n as (p_x, p_y) = (n, 0), whose length
// sqrt(n n + 0) is n again bit for bit
struct DebugRec {
    DevMem mem;
    Rows<double> rows{};
    Rec r{};
};
int debug_rec(const char* who, int32_t rows, int32_t R, int32_t fan_size, const double* x, const double* y, const double* T,
              const double* theta, const int32_t* last, const double* theta0, const double* J, const int32_t* kmah, const double* n,
              DebugRec* d) {
    RTMI_ARG(rows >= 1 && R >= 2, "rows >= 1 and R >= 2");
    RTMI_ARG(fan_size >= 2 && R % fan_size == 0, "R must be a multiple of fan_size >= 2");
    for (int32_t k = 0; k < R; k++) RTMI_ARG(last[k] >= 0 && last[k] < rows, "last must lie in [0, rows)");
    const size_t cells = (size_t)rows * R;
    std::vector<double> rec(6 * cells, 0.0);
    for (size_t i = 0; i < (size_t)rows; i++)
        for (size_t k = 0; k < (size_t)R; k++) {
            const size_t a = i * R + k, o = i * 6 * R + k;
            rec[o] = x[a]; rec[o + R] = y[a]; rec[o + 4 * R] = T[a]; rec[o + 5 * R] = theta[a];
            if (n) rec[o + 2 * R] = n[a];
        }
    double *drec = nullptr, *dth0 = nullptr, *dj = nullptr;
    int32_t *dlast = nullptr, *dk = nullptr;
    RTMI_HIP(d->mem.get(&drec, rec.size() * sizeof(double)));
    RTMI_HIP(d->mem.get(&dth0, (size_t)R * sizeof(double)));
    RTMI_HIP(d->mem.get(&dlast, (size_t)R * sizeof(int32_t)));
    RTMI_HIP(hipMemcpy(drec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(dth0, theta0, (size_t)R * sizeof(double), hipMemcpyHostToDevice));
    RTMI_HIP(hipMemcpy(dlast, last, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice));
    if (J) {
        RTMI_HIP(d->mem.get(&dj, cells * sizeof(double)));
        RTMI_HIP(d->mem.get(&dk, cells * sizeof(int32_t)));
        RTMI_HIP(hipMemcpy(dj, J, cells * sizeof(double), hipMemcpyHostToDevice));
        RTMI_HIP(hipMemcpy(dk, kmah, cells * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    d->rows = Rows<double>{drec, dlast, nullptr, (long)R, (long)rows};
    d->r = Rec{nullptr, dth0, dj, dk, (int)fan_size, (int)(R / fan_size)};
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_first_arrival_grid(rtmi_batch* b, int32_t fan_size, const rtmi_grid_params* gp, int32_t* count, double* out,
                                        rtmi_grid_stats* st) {
    const char* who = "rtmi_first_arrival_grid";
    RTMI_ARG(b && count && out, "null");
    Grid g;
    RTMI_RC(grid_of(gp, who, &g));
    FanRec f;
    RTMI_RC(fan_rec(who, b, fan_size, gp->amplitude != 0, &f));
    const rtmi_device_view& v = f.rec.v;
    return by_dtype(v.dtype, [&](auto t) { return run_grid(who, g, rows_of<decltype(t)>(v), f.r, count, out, st); });
}

RTMI_EXPORT int rtmi_arrival_grid(rtmi_batch* b, int32_t fan_size, const rtmi_grid_params* gp, const rtmi_arrival_params* ap,
                                  int32_t* count, double* out, rtmi_arrival_stats* st) {
    const char* who = "rtmi_arrival_grid";
    RTMI_ARG(b && count, "null");
    Grid g;
    RTMI_RC(grid_of(gp, who, &g));
    RTMI_RC(arrivals_of(ap, who));
    FanRec f;
    RTMI_RC(fan_rec(who, b, fan_size, gp->amplitude || ap->order == RTMI_ARRIVAL_BY_AMPLITUDE, &f));
    const rtmi_device_view& v = f.rec.v;
    const int ncols = gp->amplitude ? kColsA : kColsT;
    return by_dtype(v.dtype, [&](auto t) { return run_arrivals(who, g, rows_of<decltype(t)>(v), f.r, ncols, *ap, count, out, st); });
}

RTMI_EXPORT int rtmi_debug_grid_rows(int32_t rows, int32_t R, int32_t fan_size, const double* x, const double* y, const double* T,
                                     const double* theta, const int32_t* last, const double* theta0, const rtmi_grid_params* gp,
                                     int32_t* count, double* out, rtmi_grid_stats* st) {
    const char* who = "rtmi_debug_grid_rows";
    RTMI_ARG(x && y && T && theta && last && theta0 && count && out, "null");
    Grid g;
    RTMI_RC(grid_of(gp, who, &g));
    RTMI_ARG(!gp->amplitude, "no amplitude on caller-supplied rows");
    DebugRec d;
    RTMI_RC(debug_rec(who, rows, R, fan_size, x, y, T, theta, last, theta0, nullptr, nullptr, nullptr, &d));
    return run_grid(who, g, d.rows, d.r, count, out, st);
}

RTMI_EXPORT int rtmi_debug_arrival_rows(int32_t rows, int32_t R, int32_t fan_size, const double* x, const double* y, const double* T,
                                        const double* theta, const int32_t* last, const double* theta0, const double* J,
                                        const int32_t* kmah, const double* n, const rtmi_grid_params* gp,
                                        const rtmi_arrival_params* ap, int32_t* count, double* out, rtmi_arrival_stats* st) {
    const char* who = "rtmi_debug_arrival_rows";
    RTMI_ARG(x && y && T && theta && last && theta0 && count, "null");
    Grid g;
    RTMI_RC(grid_of(gp, who, &g));
    RTMI_RC(arrivals_of(ap, who));
    const bool amp = gp->amplitude || ap->order == RTMI_ARRIVAL_BY_AMPLITUDE;
    RTMI_ARG(!amp || (J && kmah && n), "the amplitude columns and RTMI_ARRIVAL_BY_AMPLITUDE need the J, kmah and n rows");
    DebugRec d;
    RTMI_RC(debug_rec(who, rows, R, fan_size, x, y, T, theta, last, theta0, amp ? J : nullptr, amp ? kmah : nullptr, amp ? n : nullptr, &d));
    return run_arrivals(who, g, d.rows, d.r, gp->amplitude ? kColsA : kColsT, *ap, count, out, st);
}
