// rt_lsqr_device.h -- LSQR with every vector on the device, for any operator pair on device pointers (kirchhoff_lsqr.hip: the
// Kirchhoff pair; tomo.hip: the compiled ray-tomography matrix): the vector passes, the order-independent norm and the one loop
// both solvers run.  include/rtmi.h (rtmi_kirchhoff_lsqr) states the contract; DESIGN.md section 21 the definitions; rt_lsqr.h the
// scalar recurrence (host, scipy's operation order).  Anonymous namespace: each unit gets its own copy, as with rtmi_host.h.
// The vector passes are memory-bound: 256 lanes per block, grid-stride, at most 4 blocks per CU, 16-byte loads and stores when
// every pointer of the pass is 16-byte aligned (`wide`; the solvers' own allocations always are).
//   k_axmy_absmax  y_i = t_i - fl(a y_i), and max |y_i| of the new y in the same pass (block_max_to)
//   k_scale        y_i = fl(s y_i)
//   k_axmy_absmax_f, k_scale_copy   the same two passes of the weighted loop (LsqrOptions): y_i = fl(f_i t_i) - fl(a y_i), and
//                  y_i = fl(s y_i) with z_i = fl(f_i y_i) written beside it, the copy the next operator call reads
//   k_xw           x_i = x_i + fl(c1 w_i) and w_i = v_i - fl(c2 w_i)
//   k_sumsq        the norm's integer sum: S += rint(ldexp(fl(x_i x_i), -e)), a two-word sum with an explicit carry per lane, per
//                  wave and per block, then one two-word atomic add per block into one global pair.  Integer sums commute: the
//                  same bits in every schedule.
// Every product and every add or subtract is a separate fp64 operation: the kernels spell them __dmul_rn / __dadd_rn, and the
// units are built with -ffp-contract=off like the rest of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rt_fix128.h"
#include "rt_lsqr.h"
#include "rtmi_host.h"

static_assert(RTMI_LSQR_RANGE == rt::kLsqrRange, "rtmi.h and rt_lsqr.h name one istop");

namespace {

// one pass's items of lane gid: f2(i) for the pairs (2 i, 2 i + 1) when wide, f1(i) for single items
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

__global__ void __launch_bounds__(256) k_axmy_absmax(double* __restrict__ y, const double* __restrict__ t, double a, long n, bool wide,
                                                     unsigned long long* __restrict__ out) {
    double m = 0.0;
    sweep(n, wide,
          [&](long i) {
              const double2 yv = ((const double2*)y)[i], tv = ((const double2*)t)[i];
              const double2 r = make_double2(axmy(tv.x, a, yv.x), axmy(tv.y, a, yv.y));
              ((double2*)y)[i] = r;
              m = fmax(m, fmax(fabs(r.x), fabs(r.y)));
          },
          [&](long i) {
              const double r = axmy(t[i], a, y[i]);
              y[i] = r;
              m = fmax(m, fabs(r));
          });
    block_max_to(out, m);
}

__global__ void __launch_bounds__(256) k_scale(double* __restrict__ y, double s, long n, bool wide) {
    sweep(n, wide,
          [&](long i) {
              const double2 v = ((const double2*)y)[i];
              ((double2*)y)[i] = make_double2(__dmul_rn(s, v.x), __dmul_rn(s, v.y));
          },
          [&](long i) { y[i] = __dmul_rn(s, y[i]); });
}

// The two passes of the weighted loop (LsqrOptions below).  f is the diagonal the operator's result is multiplied by: the row
// weights on A's side, the column scale on A^T's.
__global__ void __launch_bounds__(256) k_axmy_absmax_f(double* __restrict__ y, const double* __restrict__ t, const double* __restrict__ f,
                                                       double a, long n, bool wide, unsigned long long* __restrict__ out) {
    double m = 0.0;
    sweep(n, wide,
          [&](long i) {
              const double2 yv = ((const double2*)y)[i], tv = ((const double2*)t)[i], fv = ((const double2*)f)[i];
              const double2 r = make_double2(axmy(__dmul_rn(fv.x, tv.x), a, yv.x), axmy(__dmul_rn(fv.y, tv.y), a, yv.y));
              ((double2*)y)[i] = r;
              m = fmax(m, fmax(fabs(r.x), fabs(r.y)));
          },
          [&](long i) {
              const double r = axmy(__dmul_rn(f[i], t[i]), a, y[i]);
              y[i] = r;
              m = fmax(m, fabs(r));
          });
    block_max_to(out, m);
}

// y_i = fl(s y_i) and z_i = fl(f_i y_i) of the new y
__global__ void __launch_bounds__(256) k_scale_copy(double* __restrict__ y, double* __restrict__ z, const double* __restrict__ f, double s,
                                                    long n, bool wide) {
    sweep(n, wide,
          [&](long i) {
              const double2 v = ((const double2*)y)[i], fv = ((const double2*)f)[i];
              const double2 r = make_double2(__dmul_rn(s, v.x), __dmul_rn(s, v.y));
              ((double2*)y)[i] = r;
              ((double2*)z)[i] = make_double2(__dmul_rn(fv.x, r.x), __dmul_rn(fv.y, r.y));
          },
          [&](long i) {
              const double r = __dmul_rn(s, y[i]);
              y[i] = r;
              z[i] = __dmul_rn(f[i], r);
          });
}

// What the weighted loop runs once, outside the iteration: y_i = fl(y_i - t_i) (t given), then y_i = fl(f_i y_i) (f given) ...
__global__ void __launch_bounds__(256) k_sub_mul(double* __restrict__ y, const double* __restrict__ t, const double* __restrict__ f, long n) {
    sweep(n, false, [](long) {},
          [&](long i) {
              double r = y[i];
              if (t) r = __dadd_rn(r, -t[i]);
              if (f) r = __dmul_rn(f[i], r);
              y[i] = r;
          });
}

// ... and the result: x_i = fl(x0_i + fl(dc_i x_i)), an absent factor left out
__global__ void __launch_bounds__(256) k_result(double* __restrict__ x, const double* __restrict__ dc, const double* __restrict__ x0, long n) {
    sweep(n, false, [](long) {},
          [&](long i) {
              double r = x[i];
              if (dc) r = __dmul_rn(dc[i], r);
              if (x0) r = __dadd_rn(x0[i], r);
              x[i] = r;
          });
}

__global__ void __launch_bounds__(256) k_xw(double* __restrict__ x, double* __restrict__ w, const double* __restrict__ v, double c1,
                                            double c2, long n, bool wide) {
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

// acc = (lo, hi), an unsigned two-word integer that starts from 0.  A term is at most 2^57 quanta (rt_fix128.h).
__global__ void __launch_bounds__(256) k_sumsq(const double* __restrict__ x, long n, int e, bool wide, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long wlo[4], whi[4];
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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The words of a handle's `red` (kRedWords of them) the solver uses: [0] rtmi_internal_absmax_finite, [1] k_axmy_absmax, [2], [3]
// k_sumsq.
struct Vec {
    unsigned long long* red;
    int cus;
};

// The norm of n finite doubles with max |x_i| = M: range = true, and no norm, when fl(M M) is not a normal number
int norm_of(const char* who, const Vec& V, const double* d, size_t n, double M, double* norm, int* e_out, bool* range) {
    *range = false;
    *e_out = 0;
    *norm = 0.0;
    if (M == 0.0) return RTMI_OK;
    const double bound = M * M;
    if (!std::isnormal(bound)) {
        *range = true;
        return RTMI_OK;
    }
    const int e = rt::fix_exponent(bound);
    RTMI_HIP(hipMemsetAsync(V.red + 2, 0, 2 * sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(k_sumsq, stride_blocks(V.cus, n, 2), dim3(256), 0, nullptr, d, (long)n, e, aligned16(d), V.red + 2);
    RTMI_HIP(hipGetLastError());
    unsigned long long s[2] = {0, 0};
    RTMI_HIP(hipMemcpy(s, V.red + 2, sizeof(s), hipMemcpyDeviceToHost));
    const unsigned long long lo = s[0] + rt::kFixBias;         // the accumulator of rt_fix128.h: the low word carries the bias
    const unsigned long long hi = s[1] + (lo < s[0] ? 1ull : 0ull);
    // sqrt(S 2^e) with the even part of e taken out of the root: the same bits, and S 2^e itself may exceed fp64's range
    const int odd = e & 1;
    *norm = std::ldexp(std::sqrt(std::ldexp(rt::fix_to_double(lo, hi), odd)), (e - odd) / 2);
    *e_out = e;
    return RTMI_OK;
}

// y = t - a y, or with f: y = f t - a y, then the norm of the new y
int axmy_norm(const char* who, const Vec& V, double* y, const double* t, const double* f, double a, size_t n, double* norm, bool* range) {
    RTMI_HIP(hipMemsetAsync(V.red + 1, 0, sizeof(unsigned long long), nullptr));
    if (f)
        hipLaunchKernelGGL(k_axmy_absmax_f, stride_blocks(V.cus, n, 2), dim3(256), 0, nullptr, y, t, f, a, (long)n,
                           aligned16(y) && aligned16(t) && aligned16(f), V.red + 1);
    else
        hipLaunchKernelGGL(k_axmy_absmax, stride_blocks(V.cus, n, 2), dim3(256), 0, nullptr, y, t, a, (long)n, aligned16(y) && aligned16(t), V.red + 1);
    RTMI_HIP(hipGetLastError());
    double M = 0.0;
    RTMI_HIP(hipMemcpy(&M, V.red + 1, sizeof(double), hipMemcpyDeviceToHost));
    int e = 0;
    return norm_of(who, V, y, n, M, norm, &e, range);
}

// y = s y; with f also z = f y of the new y
int scale(const char* who, const Vec& V, double* y, double s, size_t n, double* z = nullptr, const double* f = nullptr) {
    if (f)
        hipLaunchKernelGGL(k_scale_copy, stride_blocks(V.cus, n, 2), dim3(256), 0, nullptr, y, z, f, s, (long)n,
                           aligned16(y) && aligned16(z) && aligned16(f));
    else
        hipLaunchKernelGGL(k_scale, stride_blocks(V.cus, n, 2), dim3(256), 0, nullptr, y, s, (long)n, aligned16(y));
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
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

// The solver's device vectors: u, Av of the data's length `per`; v, w, x, Atu of the model's length `nm`
struct LsqrVectors {
    double *u, *Av, *v, *w, *x, *Atu;
};

// The options of a weighted solve, on the device (include/rtmi.h, rtmi_lsqr_options): the row weights wr
// [per], the column scale dc [nm] and the start model x0 [nm], any of them NULL, and beside them the two vectors the weighting
// costs: uw = wr u [per] with wr, vd = dc v [nm] with dc, which the fused passes write and the operator calls read.  nrhs: the
// leading values of u that are data (A x0 is subtracted from them; rows after them, a regulariser's, keep a right-hand side of 0).
struct LsqrOptions {
    const double *wr = nullptr, *dc = nullptr, *x0 = nullptr;
    double *uw = nullptr, *vd = nullptr;
    size_t nrhs = 0;
    bool any() const { return wr || dc || x0; }
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

// The one upload of the options into memory of `mem`, and the vectors beside them.  Rows nwr .. per - 1 carry no weight: their
// factor is 1.0, and a product with 1.0 changes no bit.  *doubles: what was allocated, for bytes_device.
int lsqr_upload_options(const char* who, DevMem& mem, const rtmi_lsqr_options* lo, size_t nwr, size_t per, size_t nm, LsqrOptions* O,
                        size_t* doubles) {
    *O = LsqrOptions{};
    *doubles = 0;
    O->nrhs = nwr;
    if (!lo) return RTMI_OK;
    const std::string no_mem = std::string(who) + ": hipMalloc failed";
    auto up = [&](const double* src, size_t n, size_t total, const double** dst) {
        double* d = nullptr;
        if (mem.get(&d, total * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        RTMI_HIP(hipMemcpy(d, src, n * sizeof(double), hipMemcpyHostToDevice));
        if (total > n) {
            const std::vector<double> ones(total - n, 1.0);
            RTMI_HIP(hipMemcpy(d + n, ones.data(), (total - n) * sizeof(double), hipMemcpyHostToDevice));
        }
        *dst = d;
        *doubles += total;
        return (int)RTMI_OK;
    };
    if (lo->row_weight) {
        RTMI_RC(up(lo->row_weight, nwr, per, &O->wr));
        if (mem.get(&O->uw, per * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        *doubles += per;
    }
    if (lo->col_scale) {
        RTMI_RC(up(lo->col_scale, nm, nm, &O->dc));
        if (mem.get(&O->vd, nm * sizeof(double)) != hipSuccess) return rtmi_internal_fail(RTMI_ERR_ALLOC, no_mem.c_str());
        *doubles += nm;
    }
    if (lo->x0) RTMI_RC(up(lo->x0, nm, nm, &O->x0));
    return RTMI_OK;
}

// The loop of both solvers, from u = the right-hand side and x = 0, both on the device already, to x on the device.
// Ax(s, t): t = A s, s of nm and t of per values; At(s, t, &range): t = A^T s, which may report that a bound of its own left
// fp64's normal range (range = true: it is treated as a norm out of range).  Both return an RTMI_ code.  Fills out's istop, itn,
// the four norms and vector_ms; history [iter_lim][4] may be NULL.
// With options O the loop is that of the operator W A D on the right-hand side W (b - A x0), and x = x0 + D y at the end:
//   before   u = fl(wr fl(u - A x0)) over the data rows, one forward product and one pass
//   A        reads vd = fl(dc v), which the pass that scales v wrote beside it; its result enters u = fl(wr t) - fl(alfa u)
//   A^T      reads uw = fl(wr u), which the pass that scales u wrote beside it; its result enters v = fl(dc t) - fl(beta v)
//   after    x = fl(x0 + fl(dc x)), one pass
// so an iteration has the passes it had, each reading one vector more (the diagonal) or writing one more (the copy).  An absent
// option is left out, not multiplied by 1: with none of them the loop launches exactly the kernels it launched without options.
template <typename AX, typename AT>
int lsqr_loop(const char* who, const Vec& V, const rtmi_lsqr_params* lp, size_t per, size_t nm, const LsqrVectors& B, AX&& Ax, AT&& At,
              double* history, rtmi_lsqr_stats* out, const LsqrOptions& O = LsqrOptions{}) {
    double *const u = B.u, *const Av = B.Av, *const v = B.v, *const w = B.w, *const xd = B.x, *const Atu = B.Atu;
    const double *const uin = O.wr ? O.uw : u, *const vin = O.dc ? O.vd : v;          // what A^T and A read
    double vector_ms = 0.0;
    rt::LsqrState S;
    rt::lsqr_begin(S, lp->damp, lp->atol, lp->btol, lp->iter_lim);
    bool range = false;
    double nrm = 0.0, M = 0.0;
    int e = 0;
    // the time of a vector section: its passes and read-backs, to the point where the device is idle
    double t_sec = 0.0;
    auto sec_begin = [&]() { t_sec = now_ms(); };
    auto sec_end = [&]() {
        const hipError_t r = hipStreamSynchronize(nullptr);
        vector_ms += now_ms() - t_sec;
        return r;
    };
    auto sub_mul = [&](double* y, const double* t, const double* f, size_t n) {
        hipLaunchKernelGGL(k_sub_mul, stride_blocks(V.cus, n, 1), dim3(256), 0, nullptr, y, t, f, (long)n);
        RTMI_HIP(hipGetLastError());
        return (int)RTMI_OK;
    };

    if (O.x0) RTMI_RC(Ax(O.x0, Av));                                                 // the residual of the start model
    sec_begin();
    if (O.x0 && O.wr && O.nrhs == per) {
        RTMI_RC(sub_mul(u, Av, O.wr, per));                                          // both in one pass: the same two roundings
    } else {
        if (O.x0) RTMI_RC(sub_mul(u, Av, nullptr, O.nrhs));
        if (O.wr) RTMI_RC(sub_mul(u, nullptr, O.wr, per));
    }
    RTMI_RC(rtmi_internal_absmax_finite(who, V.red, V.cus, u, per, &M));
    RTMI_RC(norm_of(who, V, u, per, M, &nrm, &e, &range));
    bool go = !range && rt::lsqr_first_beta(S, nrm);
    if (go) RTMI_RC(scale(who, V, u, 1.0 / S.beta, per, O.uw, O.wr));
    RTMI_HIP(sec_end());
    if (go) {
        RTMI_RC(At(uin, v, &range));
        go = !range;
    }
    if (go) {
        sec_begin();
        if (O.dc) RTMI_RC(sub_mul(v, nullptr, O.dc, nm));
        RTMI_RC(rtmi_internal_absmax_finite(who, V.red, V.cus, v, nm, &M));
        RTMI_RC(norm_of(who, V, v, nm, M, &nrm, &e, &range));
        go = !range && rt::lsqr_first_alfa(S, nrm);
        if (go) {
            RTMI_RC(scale(who, V, v, 1.0 / S.alfa, nm, O.vd, O.dc));
            RTMI_HIP(hipMemcpyAsync(w, v, nm * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
        }
        RTMI_HIP(sec_end());
    }
    // A norm that leaves the range inside the loop abandons its iteration: itn, the scalars, the history and x are those of
    // the last iteration that was completed.
    while (go && !rt::lsqr_done(S)) {
        const rt::LsqrState S0 = S;
        RTMI_RC(Ax(vin, Av));
        sec_begin();
        RTMI_RC(axmy_norm(who, V, u, Av, O.wr, S.alfa, per, &nrm, &range));          // u = A v - alfa u
        if (range) {
            RTMI_HIP(sec_end());
            break;
        }
        const bool stepped = rt::lsqr_beta(S, nrm);
        if (stepped) RTMI_RC(scale(who, V, u, 1.0 / S.beta, per, O.uw, O.wr));
        RTMI_HIP(sec_end());
        if (stepped) {
            RTMI_RC(At(uin, Atu, &range));
            if (range) {
                S = S0;
                break;
            }
            sec_begin();
            RTMI_RC(axmy_norm(who, V, v, Atu, O.dc, S.beta, nm, &nrm, &range));      // v = A^T u - beta v
            if (range) {
                RTMI_HIP(sec_end());
                S = S0;
                break;
            }
            // a v that is not scaled (alfa = 0: v is zero) still needs its copy: a factor 1.0 changes no bit of v
            if (rt::lsqr_alfa(S, nrm)) RTMI_RC(scale(who, V, v, 1.0 / S.alfa, nm, O.vd, O.dc));
            else if (O.dc) RTMI_RC(scale(who, V, v, 1.0, nm, O.vd, O.dc));
            RTMI_HIP(sec_end());
        }
        rt::lsqr_rotate(S);
        sec_begin();
        hipLaunchKernelGGL(k_xw, stride_blocks(V.cus, nm, 2), dim3(256), 0, nullptr, xd, w, v, S.c1, S.c2, (long)nm,
                           aligned16(xd) && aligned16(w) && aligned16(v));
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(sec_end());
        if (history) {
            double* row = history + (size_t)(S.itn - 1) * 4;
            row[0] = S.alfa; row[1] = S.beta; row[2] = S.r1norm; row[3] = S.arnorm;
        }
    }
    if (O.dc || O.x0) {
        sec_begin();
        hipLaunchKernelGGL(k_result, stride_blocks(V.cus, nm, 1), dim3(256), 0, nullptr, xd, O.dc, O.x0, (long)nm);
        RTMI_HIP(hipGetLastError());
        RTMI_HIP(sec_end());
    }
    out->istop = range ? rt::kLsqrRange : S.istop;
    out->itn = S.itn;
    out->r1norm = S.r1norm; out->r2norm = S.r2norm; out->anorm = S.anorm; out->arnorm = S.arnorm;
    out->vector_ms = vector_ms;
    return RTMI_OK;
}

}  // namespace
