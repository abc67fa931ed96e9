// rt_lsqr_device.h -- LSQR with every vector on the device, for any operator pair on device pointers (kirchhoff_lsqr.hip: the
// Kirchhoff pair; tomo.hip: the compiled ray-tomography matrix): the vector passes, the order-independent norm and the one loop
// every solver runs, for S = 1 .. 64 right-hand sides in lock-step.  include/rtmi.h (rtmi_kirchhoff_lsqr, rtmi_tomo_lsqr_multi)
// states the contract; DESIGN.md sections 21, 26 and 28 the definitions, section 32 how the single and the batched code became
// one; rt_lsqr.h the scalar recurrence (host, scipy's operation order).  Anonymous namespace: each unit gets its own copy, as with
// rtmi_host.h.
// Column c of every vector is a plane of its own: u, Av [S][per]; v, w, x, Atu [S][nm]; a single solve is S = 1.  Every pass has
// the column in blockIdx.y and takes the columns' scalars and a mask of the columns it may touch as one kernel argument
// (ColArgs), so that a pass is one launch and a reduction one read-back whatever S is.  A column outside the mask is not read
// and not written.  The passes are memory-bound: 256 lanes per block, grid-stride along x, at most 4 blocks per CU, 16-byte loads
// and stores when every pointer of the pass is 16-byte aligned and, for S > 1, every plane stride is even (`wide`, decided on the
// host for the whole launch; the solvers' own allocations always are aligned).  `wide` changes no bit.
//   k_absmax       max |y_i| over the finite y_i (block_max_to)
//   k_axmy_absmax  y_i = t_i - fl(a y_i), or <true> with a diagonal f: y_i = fl(f_i t_i) - fl(a y_i); max |y_i| of the new y in the same pass
//   k_scale        y_i = fl(a y_i); <true>: z_i = fl(f_i y_i) written beside it, the copy the next operator call reads
//   k_sub_mul, k_result, k_copy   what runs outside the iteration: y = fl(f fl(y - t)), x = fl(x0 + fl(dc x)), w = v
//   k_xw           x_i = x_i + fl(a w_i) and w_i = v_i - fl(b w_i)
//   k_sumsq        the norm's integer sum: S += rint(ldexp(fl(x_i x_i), -e)), a two-word sum with an explicit carry per lane, per
//                  wave and per block, then one two-word atomic add per block into the column's global pair.  Integer sums
//                  commute: the same bits in every schedule.
// Every product and every add or subtract is a separate fp64 operation: the kernels spell them __dmul_rn / __dadd_rn, and the
// units are built with -ffp-contract=off like the rest of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_fix128.h"
#include "rt_lsqr.h"
#include "rtmi_host.h"

static_assert(RTMI_LSQR_RANGE == rt::kLsqrRange, "rtmi.h and rt_lsqr.h name one istop");
static_assert(RTMI_LSQR_MULTI_MAX == 64, "a mask of columns is one 64-bit word");

namespace {

constexpr int kMultiMax = RTMI_LSQR_MULTI_MAX;
// The reduction words of one column: [0] a maximum, [2], [3] k_sumsq's pair.  A caller with one column may pass any handle's `red`
// (kRedWords): words [4] and up are not touched.
constexpr size_t kRedM = 4;
static_assert(kRedM <= kRedWords, "one column's words fit a handle's");

// Per column: two scalars, the exponent of its sum of squares, and the columns the pass touches
struct ColArgs {
    double a[kMultiMax], b[kMultiMax];
    int e[kMultiMax];
    unsigned long long live;
};

__device__ __forceinline__ bool col_live(unsigned long long live, int c) { return (live >> c) & 1ull; }
inline unsigned long long col_bit(int c) { return 1ull << c; }
inline unsigned long long all_cols(int S) { return S == 64 ? ~0ull : (col_bit(S) - 1ull); }

// one pass's items of lane gid in its column: f2(i) for the pairs (2 i, 2 i + 1) when wide, f1(i) for single items
template <typename F2, typename F1>
__device__ __forceinline__ void sweep(long n, bool wide, F2&& f2, F1&& f1) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x, gsz = (long)gridDim.x * 256;
    if (wide) {
        for (long i = gid; i < n / 2; i += gsz) f2(i);
        if ((n & 1) && gid == 0) f1(n - 1);
    } else {
        for (long i = gid; i < n; i += gsz) f1(i);
    }
}

__device__ __forceinline__ double axmy(double t, double a, double y) { return __dadd_rn(t, -__dmul_rn(a, y)); }

// into the column's red[c][0]; k_absmax_finite (kirchhoff.hip) per column
__global__ void __launch_bounds__(256) k_absmax(const double* __restrict__ x, size_t s, long n, bool wide, unsigned long long live,
                                                unsigned long long* __restrict__ red) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    x += (size_t)c * s;
    double m = 0.0;
    auto take = [&](double v) {
        const double a = fabs(v);
        m = a < INFINITY ? fmax(m, a) : m;                    // NaN fails the compare
    };
    sweep(n, wide,
          [&](long i) {
              const double2 v = ((const double2*)x)[i];
              take(v.x);
              take(v.y);
          },
          [&](long i) { take(x[i]); });
    block_max_to(red + (size_t)c * kRedM, m);
}

// F: f is the diagonal the operator's result is multiplied by: the row weights on A's side (fs values per column, 0: one
// weighting for all), the column scale on A^T's
template <bool F>
__global__ void __launch_bounds__(256) k_axmy_absmax(double* __restrict__ y, const double* __restrict__ t, size_t s, const double* __restrict__ f,
                                                     size_t fs, ColArgs K, long n, bool wide, unsigned long long* __restrict__ red) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    y += (size_t)c * s;
    t += (size_t)c * s;
    if (F) f += (size_t)c * fs;
    const double a = K.a[c];
    double m = 0.0;
    sweep(n, wide,
          [&](long i) {
              double2 tv = ((const double2*)t)[i];
              const double2 yv = ((const double2*)y)[i];
              if (F) {
                  const double2 fv = ((const double2*)f)[i];
                  tv = make_double2(__dmul_rn(fv.x, tv.x), __dmul_rn(fv.y, tv.y));
              }
              const double2 r = make_double2(axmy(tv.x, a, yv.x), axmy(tv.y, a, yv.y));
              ((double2*)y)[i] = r;
              m = fmax(m, fmax(fabs(r.x), fabs(r.y)));
          },
          [&](long i) {
              const double r = axmy(F ? __dmul_rn(f[i], t[i]) : t[i], a, y[i]);
              y[i] = r;
              m = fmax(m, fabs(r));
          });
    block_max_to(red + (size_t)c * kRedM, m);
}

// y_i = fl(a y_i), and with F: z_i = fl(f_i y_i) of the new y
template <bool F>
__global__ void __launch_bounds__(256) k_scale(double* __restrict__ y, double* __restrict__ z, size_t s, const double* __restrict__ f, size_t fs,
                                               ColArgs K, long n, bool wide) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    y += (size_t)c * s;
    if (F) {
        z += (size_t)c * s;
        f += (size_t)c * fs;
    }
    const double a = K.a[c];
    sweep(n, wide,
          [&](long i) {
              const double2 v = ((const double2*)y)[i];
              const double2 r = make_double2(__dmul_rn(a, v.x), __dmul_rn(a, v.y));
              ((double2*)y)[i] = r;
              if (F) {
                  const double2 fv = ((const double2*)f)[i];
                  ((double2*)z)[i] = make_double2(__dmul_rn(fv.x, r.x), __dmul_rn(fv.y, r.y));
              }
          },
          [&](long i) {
              const double r = __dmul_rn(a, y[i]);
              y[i] = r;
              if (F) z[i] = __dmul_rn(f[i], r);
          });
}

// What runs once, outside the iteration: y_i = fl(y_i - t_i) (t given), then y_i = fl(f_i y_i) (f given); ts, fs 0: one t, one f
// for all columns ...
__global__ void __launch_bounds__(256) k_sub_mul(double* __restrict__ y, size_t s, const double* __restrict__ t, size_t ts,
                                                 const double* __restrict__ f, size_t fs, long n, unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    y += (size_t)c * s;
    if (t) t += (size_t)c * ts;
    if (f) f += (size_t)c * fs;
    sweep(n, false, [](long) {},
          [&](long i) {
              double r = y[i];
              if (t) r = __dadd_rn(r, -t[i]);
              if (f) r = __dmul_rn(f[i], r);
              y[i] = r;
          });
}

// ... and the result: x_i = fl(x0_i + fl(dc_i x_i)), an absent factor left out; dc and x0 are one vector for all columns
__global__ void __launch_bounds__(256) k_result(double* __restrict__ x, size_t s, const double* __restrict__ dc, const double* __restrict__ x0,
                                                long n, unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    x += (size_t)c * s;
    sweep(n, false, [](long) {},
          [&](long i) {
              double r = x[i];
              if (dc) r = __dmul_rn(dc[i], r);
              if (x0) r = __dadd_rn(x0[i], r);
              x[i] = r;
          });
}

__global__ void __launch_bounds__(256) k_xw(double* __restrict__ x, double* __restrict__ w, const double* __restrict__ v, size_t s, ColArgs K,
                                            long n, bool wide) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    x += (size_t)c * s;
    w += (size_t)c * s;
    v += (size_t)c * s;
    const double c1 = K.a[c], c2 = K.b[c];
    sweep(n, wide,
          [&](long i) {
              const double2 xv = ((const double2*)x)[i], wv = ((const double2*)w)[i], vv = ((const double2*)v)[i];
              ((double2*)x)[i] = make_double2(__dadd_rn(xv.x, __dmul_rn(c1, wv.x)), __dadd_rn(xv.y, __dmul_rn(c1, wv.y)));
              ((double2*)w)[i] = make_double2(axmy(vv.x, c2, wv.x), axmy(vv.y, c2, wv.y));
          },
          [&](long i) {
              const double wi = w[i];
              x[i] = __dadd_rn(x[i], __dmul_rn(c1, wi));
              w[i] = axmy(v[i], c2, wi);
          });
}

__global__ void __launch_bounds__(256) k_copy(double* __restrict__ w, const double* __restrict__ v, size_t s, long n, bool wide,
                                              unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    w += (size_t)c * s;
    v += (size_t)c * s;
    sweep(n, wide, [&](long i) { ((double2*)w)[i] = ((const double2*)v)[i]; }, [&](long i) { w[i] = v[i]; });
}

// With the column's exponent K.e[c], into the column's pair red[c][2], [3] = (lo, hi), an unsigned two-word integer that starts
// from 0.  A term is at most 2^57 quanta (rt_fix128.h).
__global__ void __launch_bounds__(256) k_sumsq(const double* __restrict__ x, size_t s, long n, ColArgs K, bool wide,
                                               unsigned long long* __restrict__ red) {
    __shared__ unsigned long long wlo[4], whi[4];
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    x += (size_t)c * s;
    unsigned long long* const acc = red + (size_t)c * kRedM + 2;
    const int e = K.e[c];
    unsigned long long lo = 0ull, hi = 0ull;
    auto term = [&](double v) {
        const unsigned long long q = (unsigned long long)(long long)rint(ldexp(__dmul_rn(v, v), -e));
        lo += q;
        hi += lo < q ? 1ull : 0ull;
    };
    sweep(n, wide,
          [&](long i) {
              const double2 v = ((const double2*)x)[i];
              term(v.x);
              term(v.y);
          },
          [&](long i) { term(x[i]); });
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long olo = __shfl_xor(lo, off), ohi = __shfl_xor(hi, off);
        lo += olo;
        hi += ohi + (lo < olo ? 1ull : 0ull);
    }
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) { wlo[tid >> 6] = lo; whi[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        lo = wlo[0];
        hi = whi[0];
        for (int q = 1; q < 4; q++) {
            lo += wlo[q];
            hi += whi[q] + (lo < wlo[q] ? 1ull : 0ull);
        }
        // rt::add128 with a two-word addend: the low word's carry is read off the value the add returned
        if (lo | hi) {
            const unsigned long long old = lo ? atomicAdd(acc, lo) : 0ull;
            const unsigned long long h = hi + ((old + lo) < old ? 1ull : 0ull);
            if (h) atomicAdd(acc + 1, h);
        }
    }
}

// The device words of the reductions, kRedM per column, and the launch shape of a pass over S columns of n values
struct Vec {
    unsigned long long* red;
    int cus, S;
    dim3 grid(size_t n, size_t per) const { return dim3(stride_blocks(cus, n, per).x, (unsigned)S); }
    size_t red_bytes() const { return (size_t)S * kRedM * sizeof(unsigned long long); }
    // the one `wide` of a launch: every plane stride even (one column has no second plane) and every pointer 16-byte aligned
    bool wide(std::initializer_list<size_t> strides, std::initializer_list<const void*> ptrs) const {
        for (const size_t s : strides)
            if (S > 1 && (s & 1)) return false;
        for (const void* p : ptrs)
            if ((uintptr_t)p & 15) return false;
        return true;
    }
};

// max |x| over the finite values of the columns in `live`, one launch and one read-back: M [S], 0 for a column outside
int absmax(const char* who, const Vec& V, const double* d, size_t s, size_t n, unsigned long long live, double* M) {
    unsigned long long h[kMultiMax * kRedM];
    RTMI_HIP(hipMemsetAsync(V.red, 0, V.red_bytes(), nullptr));
    hipLaunchKernelGGL(k_absmax, V.grid(n, 2), dim3(256), 0, nullptr, d, s, (long)n, V.wide({s}, {d}), live, V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) std::memcpy(&M[c], &h[(size_t)c * kRedM], sizeof(double));
    return RTMI_OK;
}

// The norms of the columns in `live`, each of n finite doubles with max |x_i| = M [c]: nrm [S]; range [S] = true,
// and no norm, when fl(M M) is not a normal number; exps [S] (or NULL) the exponents.  One launch, one read-back.
int norms(const char* who, const Vec& V, const double* d, size_t s, size_t n, unsigned long long live, const double* M, double* nrm,
          bool* range, int* exps = nullptr) {
    ColArgs K{};
    for (int c = 0; c < V.S; c++) {
        if (!(live & col_bit(c))) continue;
        range[c] = false;
        nrm[c] = 0.0;
        if (exps) exps[c] = 0;
        if (M[c] == 0.0) continue;
        const double bound = M[c] * M[c];
        if (!std::isnormal(bound)) {
            range[c] = true;
            continue;
        }
        K.e[c] = rt::fix_exponent(bound);
        K.live |= col_bit(c);
    }
    if (!K.live) return RTMI_OK;
    unsigned long long h[kMultiMax * kRedM];
    RTMI_HIP(hipMemsetAsync(V.red, 0, V.red_bytes(), nullptr));
    hipLaunchKernelGGL(k_sumsq, V.grid(n, 2), dim3(256), 0, nullptr, d, s, (long)n, K, V.wide({s}, {d}), V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) {
        if (!(K.live & col_bit(c))) continue;
        const unsigned long long s0 = h[(size_t)c * kRedM + 2], s1 = h[(size_t)c * kRedM + 3];
        const unsigned long long lo = s0 + rt::kFixBias;      // the accumulator of rt_fix128.h: the low word carries the bias
        const unsigned long long hi = s1 + (lo < s0 ? 1ull : 0ull);
        // sqrt(S 2^e) with the even part of e taken out of the root: the same bits, and S 2^e itself may exceed fp64's range
        const int e = K.e[c], odd = e & 1;
        nrm[c] = std::ldexp(std::sqrt(std::ldexp(rt::fix_to_double(lo, hi), odd)), (e - odd) / 2);
        if (exps) exps[c] = e;
    }
    return RTMI_OK;
}

// y = t - a y, or with f: y = f t - a y, for the columns in K.live with a = K.a, then the norms of the new y
int axmy_norm(const char* who, const Vec& V, double* y, const double* t, size_t s, const double* f, size_t fs, const ColArgs& K, size_t n,
              double* nrm, bool* range) {
    unsigned long long h[kMultiMax * kRedM];
    double M[kMultiMax];
    RTMI_HIP(hipMemsetAsync(V.red, 0, V.red_bytes(), nullptr));
    if (f)
        hipLaunchKernelGGL(k_axmy_absmax<true>, V.grid(n, 2), dim3(256), 0, nullptr, y, t, s, f, fs, K, (long)n, V.wide({s, fs}, {y, t, f}), V.red);
    else
        hipLaunchKernelGGL(k_axmy_absmax<false>, V.grid(n, 2), dim3(256), 0, nullptr, y, t, s, f, fs, K, (long)n, V.wide({s}, {y, t}), V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) std::memcpy(&M[c], &h[(size_t)c * kRedM], sizeof(double));
    return norms(who, V, y, s, n, K.live, M, nrm, range);
}

// y = a y for the columns in K.live; with f also z = f y of the new y
int scale(const char* who, const Vec& V, double* y, double* z, size_t s, const double* f, size_t fs, const ColArgs& K, size_t n) {
    if (f)
        hipLaunchKernelGGL(k_scale<true>, V.grid(n, 2), dim3(256), 0, nullptr, y, z, s, f, fs, K, (long)n, V.wide({s, fs}, {y, z, f}));
    else
        hipLaunchKernelGGL(k_scale<false>, V.grid(n, 2), dim3(256), 0, nullptr, y, z, s, f, fs, K, (long)n, V.wide({s}, {y}));
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

int sub_mul(const char* who, const Vec& V, double* y, size_t s, const double* t, size_t ts, const double* f, size_t fs, size_t n,
            unsigned long long live) {
    hipLaunchKernelGGL(k_sub_mul, V.grid(n, 1), dim3(256), 0, nullptr, y, s, t, ts, f, fs, (long)n, live);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

int result(const char* who, const Vec& V, double* x, size_t s, const double* dc, const double* x0, size_t n, unsigned long long live) {
    hipLaunchKernelGGL(k_result, V.grid(n, 1), dim3(256), 0, nullptr, x, s, dc, x0, (long)n, live);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

// A start model x0 is the caller's business, around the loop: the right-hand side of every column becomes u = fl(u - t) over its
// n leading rows, the data's, with t = A x0 computed once (rows after them, a regulariser's, keep a right-hand side of 0).  With
// the row weights f (fs per column; only where n is all of u) the same pass goes on to u = fl(f u), the loop's first pass, and
// the caller sets LsqrOptions::rhs_weighted ...
int lsqr_sub_start(const char* who, const Vec& V, double* u, size_t per, const double* t, size_t n, const double* f = nullptr, size_t fs = 0) {
    return sub_mul(who, V, u, per, t, 0, f, fs, n, all_cols(V.S));
}

// ... and after the loop, and after whatever maps its x to x0's grid, x = fl(x0 + x) in every column
int lsqr_add_start(const char* who, const Vec& V, double* x, size_t s, const double* x0, size_t n) {
    return result(who, V, x, s, nullptr, x0, n, all_cols(V.S));
}

// The rules every solver has for its parameters
int lsqr_check_params(const char* who, const rtmi_lsqr_params* lp) {
    RTMI_ARG(lp, "null params");
    RTMI_ARG(lp->iter_lim >= 1, "iter_lim must be >= 1");
    RTMI_ARG(std::isfinite(lp->damp) && lp->damp >= 0.0, "damp must be finite and >= 0");
    RTMI_ARG(std::isfinite(lp->atol) && lp->atol >= 0.0, "atol must be finite and >= 0");
    RTMI_ARG(std::isfinite(lp->btol) && lp->btol >= 0.0, "btol must be finite and >= 0");
    return RTMI_OK;
}

// The solver's device vectors, S planes each: u, Av of the data's length `per`; v, w, x, Atu of the model's length `nm`
struct LsqrVectors {
    double *u, *Av, *v, *w, *x, *Atu;
};

// The options of a weighted solve, on the device (include/rtmi.h, rtmi_lsqr_options): the row weights wr,
// wrs values per column (0: one weighting [per] for all), and the column scale dc [nm], one for all, either of them NULL, and
// beside them the planes the weighting costs: uw = wr u [S][per] with wr, vd = dc v [S][nm] with dc, which the fused passes write
// and the operator calls read.
struct LsqrOptions {
    const double *wr = nullptr, *dc = nullptr;
    size_t wrs = 0;
    double *uw = nullptr, *vd = nullptr;
    bool rhs_weighted = false;                                // u is wr b already (lsqr_sub_start with f)
};

// The rule for the caller's options, before any device work: finite values.  nwr: the values row_weight has.
int lsqr_check_options(const char* who, const rtmi_lsqr_options* lo, size_t nwr, size_t nm) {
    if (!lo) return RTMI_OK;
    if (lo->row_weight)
        for (size_t i = 0; i < nwr; i++) RTMI_ARG(std::isfinite(lo->row_weight[i]), "row_weight has a value that is not finite");
    if (lo->col_scale)
        for (size_t i = 0; i < nm; i++) RTMI_ARG(std::isfinite(lo->col_scale[i]), "col_scale has a value that is not finite");
    if (lo->x0)
        for (size_t i = 0; i < nm; i++) RTMI_ARG(std::isfinite(lo->x0[i]), "x0 has a value that is not finite");
    return RTMI_OK;
}

// The one upload of row_weight and col_scale into memory of `mem`, and the planes beside them, for S columns.  row_weight has nwr
// values, per column when wr_cols; rows nwr .. per - 1 carry no weight: their factor is 1.0, and a product with 1.0 changes no
// bit.  *doubles: what was allocated, for bytes_device.
int lsqr_upload_options(const char* who, DevMem& mem, const rtmi_lsqr_options* lo, int S, bool wr_cols, size_t nwr, size_t per, size_t nm,
                        LsqrOptions* O, size_t* doubles) {
    *O = LsqrOptions{};
    *doubles = 0;
    if (!lo) return RTMI_OK;
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    auto get = [&](double** d, size_t n) {
        *doubles += n;
        return mem.get(d, n * sizeof(double)) == hipSuccess;
    };
    if (lo->row_weight) {
        const size_t nw = wr_cols ? (size_t)S : 1;
        std::vector<double> h(nw * per, 1.0);
        for (size_t c = 0; c < nw; c++) std::memcpy(h.data() + c * per, lo->row_weight + c * nwr, nwr * sizeof(double));
        double* d = nullptr;
        if (!get(&d, nw * per) || !get(&O->uw, (size_t)S * per)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(d, h.data(), nw * per * sizeof(double), hipMemcpyHostToDevice));
        O->wr = d;
        O->wrs = wr_cols ? per : 0;
    }
    if (lo->col_scale) {
        double* d = nullptr;
        if (!get(&d, nm) || !get(&O->vd, (size_t)S * nm)) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(d, lo->col_scale, nm * sizeof(double), hipMemcpyHostToDevice));
        O->dc = d;
    }
    return RTMI_OK;
}

// The loop of every solver, for V.S columns in lock-step: B's vectors are planes of `per` and `nm` values per column, u holds the
// right-hand sides, x is zero, both on the device already; x is left on the device.
//   Ax(s, y, mask)          y = A s for the columns in mask (others may be computed, none is read back)
//   At(s, g, mask, range)   g = A^T s for the columns in mask, range [S]: a bound of the column's product left fp64's normal range
//                           (it is treated as a norm out of range), g not written
// Both return an RTMI_ code.  out [S]: istop, itn, the four norms and vector_ms; history [S][iter_lim][4] (host) or NULL.
// With options O the loop is that of the operator W A D on the right-hand side W b, and x = D y at the end:
//   before   u = fl(wr u), one pass (unless the caller's start-model pass did it: rhs_weighted)
//   A        reads vd = fl(dc v), which the pass that scales v wrote beside it; its result enters u = fl(wr t) - fl(alfa u)
//   A^T      reads uw = fl(wr u), which the pass that scales u wrote beside it; its result enters v = fl(dc t) - fl(beta v)
//   after    x = fl(dc x), one pass
// so an iteration has the passes it had, each reading one vector more (the diagonal) or writing one more (the copy).  An absent
// option is left out, not multiplied by 1: with none of them the loop launches exactly the kernels it launches without options.
// One rt::LsqrState per column.  A column leaves at lsqr_done, at a zero right-hand side or first alfa, or at a norm or an A^T
// bound out of range; in the last case its iteration is abandoned (S = S0): itn, the scalars, the history and x are those of the
// last iteration that was completed.  From then on no pass has the column in its mask.
template <typename AX, typename AT>
int lsqr_loop(const char* who, const Vec& V, const rtmi_lsqr_params* lp, size_t per, size_t nm, const LsqrVectors& B, AX&& Ax, AT&& At,
              double* history, rtmi_lsqr_stats* out, const LsqrOptions& O = LsqrOptions{}) {
    const int S = V.S;
    const size_t wrs = O.wrs;
    double *const u = B.u, *const Av = B.Av, *const v = B.v, *const w = B.w, *const xd = B.x, *const Atu = B.Atu;
    const double *const uin = O.wr ? O.uw : u, *const vin = O.dc ? O.vd : v;          // what A^T and A read
    const unsigned long long all = all_cols(S);
    // the time of a vector section: its passes and read-backs, to the point where the device is idle
    double vector_ms = 0.0, t_sec = 0.0;
    auto sec_begin = [&]() { t_sec = now_ms(); };
    auto sec_end = [&]() {
        const hipError_t r = hipStreamSynchronize(nullptr);
        vector_ms += now_ms() - t_sec;
        return r;
    };
    std::vector<rt::LsqrState> St((size_t)S), St0((size_t)S);
    for (rt::LsqrState& s : St) rt::lsqr_begin(s, lp->damp, lp->atol, lp->btol, lp->iter_lim);
    bool range[kMultiMax] = {}, rr[kMultiMax] = {};
    double M[kMultiMax] = {}, nrm[kMultiMax] = {};
    auto each = [&](unsigned long long mask, auto&& f) {
        for (int c = 0; c < S; c++)
            if (mask & col_bit(c)) f(c);
    };
    ColArgs K{};

    sec_begin();
    if (O.wr && !O.rhs_weighted) RTMI_RC(sub_mul(who, V, u, per, nullptr, 0, O.wr, wrs, per, all));
    RTMI_RC(absmax(who, V, u, per, per, all, M));
    RTMI_RC(norms(who, V, u, per, per, all, M, nrm, rr));
    unsigned long long live = 0ull;                           // the columns whose loop goes on
    each(all, [&](int c) {
        range[c] = rr[c];
        if (!rr[c] && rt::lsqr_first_beta(St[c], nrm[c])) live |= col_bit(c);
    });
    if (live) {
        K.live = live;
        each(live, [&](int c) { K.a[c] = 1.0 / St[c].beta; });
        RTMI_RC(scale(who, V, u, O.uw, per, O.wr, wrs, K, per));
    }
    RTMI_HIP(sec_end());
    if (live) {
        RTMI_RC(At(uin, v, live, rr));
        each(live, [&](int c) {
            if (rr[c]) { range[c] = true; live &= ~col_bit(c); }
        });
    }
    if (live) {
        sec_begin();
        if (O.dc) RTMI_RC(sub_mul(who, V, v, nm, nullptr, 0, O.dc, 0, nm, live));
        RTMI_RC(absmax(who, V, v, nm, nm, live, M));
        RTMI_RC(norms(who, V, v, nm, nm, live, M, nrm, rr));
        unsigned long long next = 0ull;
        each(live, [&](int c) {
            if (rr[c]) range[c] = true;
            else if (rt::lsqr_first_alfa(St[c], nrm[c])) next |= col_bit(c);
        });
        live = next;
        if (live) {
            K.live = live;
            each(live, [&](int c) { K.a[c] = 1.0 / St[c].alfa; });
            RTMI_RC(scale(who, V, v, O.vd, nm, O.dc, 0, K, nm));
            hipLaunchKernelGGL(k_copy, V.grid(nm, 2), dim3(256), 0, nullptr, w, v, nm, (long)nm, V.wide({nm}, {w, v}), live);
            RTMI_HIP(hipGetLastError());
        }
        RTMI_HIP(sec_end());
    }
    for (;;) {
        unsigned long long act = 0ull;
        each(live, [&](int c) {
            if (!rt::lsqr_done(St[c])) act |= col_bit(c);
        });
        live = act;
        if (!act) break;
        each(act, [&](int c) { St0[c] = St[c]; });
        RTMI_RC(Ax(vin, Av, act));
        sec_begin();
        K.live = act;
        each(act, [&](int c) { K.a[c] = St[c].alfa; });
        RTMI_RC(axmy_norm(who, V, u, Av, per, O.wr, wrs, K, per, nrm, rr));          // u = A v - alfa u
        unsigned long long stepped = 0ull, cont = 0ull;       // cont: the columns that finish this iteration
        each(act, [&](int c) {
            if (rr[c]) {
                range[c] = true;
                live &= ~col_bit(c);
                return;
            }
            cont |= col_bit(c);
            if (rt::lsqr_beta(St[c], nrm[c])) stepped |= col_bit(c);
        });
        if (stepped) {
            K.live = stepped;
            each(stepped, [&](int c) { K.a[c] = 1.0 / St[c].beta; });
            RTMI_RC(scale(who, V, u, O.uw, per, O.wr, wrs, K, per));
        }
        RTMI_HIP(sec_end());
        auto abandon = [&](int c) {
            St[c] = St0[c];
            range[c] = true;
            live &= ~col_bit(c);
            cont &= ~col_bit(c);
            stepped &= ~col_bit(c);
        };
        if (stepped) {
            RTMI_RC(At(uin, Atu, stepped, rr));
            each(stepped, [&](int c) {
                if (rr[c]) abandon(c);
            });
        }
        if (stepped) {
            sec_begin();
            K.live = stepped;
            each(stepped, [&](int c) { K.a[c] = St[c].beta; });
            RTMI_RC(axmy_norm(who, V, v, Atu, nm, O.dc, 0, K, nm, nrm, rr));         // v = A^T u - beta v
            ColArgs Ks{};
            each(stepped, [&](int c) {
                if (rr[c]) {
                    abandon(c);
                    return;
                }
                // a v that is not scaled (alfa = 0: v is zero) still needs its copy: a factor 1.0 changes no bit of v
                if (rt::lsqr_alfa(St[c], nrm[c])) { Ks.a[c] = 1.0 / St[c].alfa; Ks.live |= col_bit(c); }
                else if (O.dc) { Ks.a[c] = 1.0; Ks.live |= col_bit(c); }
            });
            if (Ks.live) RTMI_RC(scale(who, V, v, O.vd, nm, O.dc, 0, Ks, nm));
            RTMI_HIP(sec_end());
        }
        if (cont) {
            K.live = cont;
            each(cont, [&](int c) {
                rt::lsqr_rotate(St[c]);
                K.a[c] = St[c].c1;
                K.b[c] = St[c].c2;
            });
            sec_begin();
            hipLaunchKernelGGL(k_xw, V.grid(nm, 2), dim3(256), 0, nullptr, xd, w, v, nm, K, (long)nm, V.wide({nm}, {xd, w, v}));
            RTMI_HIP(hipGetLastError());
            RTMI_HIP(sec_end());
            if (history)
                each(cont, [&](int c) {
                    double* row = history + ((size_t)c * (size_t)lp->iter_lim + (size_t)(St[c].itn - 1)) * 4;
                    row[0] = St[c].alfa; row[1] = St[c].beta; row[2] = St[c].r1norm; row[3] = St[c].arnorm;
                });
        }
    }
    if (O.dc) {
        sec_begin();
        RTMI_RC(result(who, V, xd, nm, O.dc, nullptr, nm, all));
        RTMI_HIP(sec_end());
    }
    for (int c = 0; c < S; c++) {
        out[c].istop = range[c] ? rt::kLsqrRange : St[c].istop;
        out[c].itn = St[c].itn;
        out[c].r1norm = St[c].r1norm; out[c].r2norm = St[c].r2norm; out[c].anorm = St[c].anorm; out[c].arnorm = St[c].arnorm;
        out[c].vector_ms = vector_ms;
    }
    return RTMI_OK;
}

}  // namespace
