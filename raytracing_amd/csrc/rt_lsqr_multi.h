// rt_lsqr_multi.h -- the loop of rt_lsqr_device.h for S right-hand sides in lock-step (tomo.hip: rtmi_tomo_lsqr_multi; DESIGN.md
// section 28).  Column s of every vector is a plane of its own: u, Av [S][per]; v, w, x, Atu [S][nm].  Every pass is the pass of
// rt_lsqr_device.h with the column in blockIdx.y: it takes the columns' scalars and a mask of the columns it may touch as one
// kernel argument (ColArgs), so that a pass is one launch and a reduction one read-back whatever S is.  A column outside the mask
// is not read and not written.  The arithmetic per element is that of the single passes, spelled the same way; the maxima and the
// integer sums do not depend on the order, so a column has the bits the single loop gives it (the single passes' 16-byte form
// changes no bit either, and is left out here).
#pragma once
#include <cstring>
#include <vector>

#include "rt_lsqr_device.h"

static_assert(RTMI_LSQR_MULTI_MAX == 64, "a mask of columns is one 64-bit word");

namespace {

constexpr int kMultiMax = RTMI_LSQR_MULTI_MAX;
// The reduction words of one column, as Vec's: [0] a maximum, [2], [3] k_sumsq_m's pair
constexpr size_t kRedM = 4;

// Per column: two scalars, the exponent of its sum of squares, and the columns the pass touches
struct ColArgs {
    double a[kMultiMax], b[kMultiMax];
    int e[kMultiMax];
    unsigned long long live;
};

__device__ __forceinline__ bool col_live(unsigned long long live, int c) { return (live >> c) & 1ull; }

// f(i) for the items of one column: grid-stride along x
template <typename F> __device__ __forceinline__ void sweep_m(long n, F&& f) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x, gsz = (long)gridDim.x * 256;
    for (long i = gid; i < n; i += gsz) f(i);
}

// k_absmax_finite (kirchhoff.hip) per column
__global__ void __launch_bounds__(256) k_absmax_finite_m(const double* __restrict__ x, size_t xs, long n, unsigned long long live,
                                                         unsigned long long* __restrict__ red) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    x += (size_t)c * xs;
    double m = 0.0;
    sweep_m(n, [&](long i) {
        const double a = fabs(x[i]);
        m = a < INFINITY ? fmax(m, a) : m;                    // NaN fails the compare
    });
    block_max_to(red + (size_t)c * kRedM, m);
}

// k_axmy_absmax and k_axmy_absmax_f: y = t - a y, or with f: y = f t - a y; fs 0: one f for all columns
__global__ void __launch_bounds__(256) k_axmy_absmax_m(double* __restrict__ y, const double* __restrict__ t, size_t s,
                                                       const double* __restrict__ f, size_t fs, ColArgs K, long n,
                                                       unsigned long long* __restrict__ red) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    y += (size_t)c * s;
    t += (size_t)c * s;
    if (f) f += (size_t)c * fs;
    const double a = K.a[c];
    double m = 0.0;
    sweep_m(n, [&](long i) {
        const double r = axmy(f ? __dmul_rn(f[i], t[i]) : t[i], a, y[i]);
        y[i] = r;
        m = fmax(m, fabs(r));
    });
    block_max_to(red + (size_t)c * kRedM, m);
}

// k_scale and k_scale_copy: y = fl(a y), and with f also z = fl(f y) of the new y
__global__ void __launch_bounds__(256) k_scale_m(double* __restrict__ y, double* __restrict__ z, size_t s, const double* __restrict__ f,
                                                 size_t fs, ColArgs K, long n) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    y += (size_t)c * s;
    if (f) {
        z += (size_t)c * s;
        f += (size_t)c * fs;
    }
    const double a = K.a[c];
    sweep_m(n, [&](long i) {
        const double r = __dmul_rn(a, y[i]);
        y[i] = r;
        if (f) z[i] = __dmul_rn(f[i], r);
    });
}

// k_sub_mul: y = fl(y - t) (t given), then y = fl(f y) (f given); ts, fs 0: one t, one f for all columns
__global__ void __launch_bounds__(256) k_sub_mul_m(double* __restrict__ y, size_t s, const double* __restrict__ t, size_t ts,
                                                   const double* __restrict__ f, size_t fs, long n, unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    y += (size_t)c * s;
    if (t) t += (size_t)c * ts;
    if (f) f += (size_t)c * fs;
    sweep_m(n, [&](long i) {
        double r = y[i];
        if (t) r = __dadd_rn(r, -t[i]);
        if (f) r = __dmul_rn(f[i], r);
        y[i] = r;
    });
}

// k_result: x = fl(x0 + fl(dc x)), an absent factor left out; dc and x0 are one vector for all columns
__global__ void __launch_bounds__(256) k_result_m(double* __restrict__ x, size_t s, const double* __restrict__ dc,
                                                  const double* __restrict__ x0, long n, unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    x += (size_t)c * s;
    sweep_m(n, [&](long i) {
        double r = x[i];
        if (dc) r = __dmul_rn(dc[i], r);
        if (x0) r = __dadd_rn(x0[i], r);
        x[i] = r;
    });
}

// k_xw: x = x + fl(a w), w = v - fl(b w)
__global__ void __launch_bounds__(256) k_xw_m(double* __restrict__ x, double* __restrict__ w, const double* __restrict__ v, size_t s,
                                              ColArgs K, long n) {
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    x += (size_t)c * s;
    w += (size_t)c * s;
    v += (size_t)c * s;
    const double c1 = K.a[c], c2 = K.b[c];
    sweep_m(n, [&](long i) {
        const double wi = w[i];
        x[i] = __dadd_rn(x[i], __dmul_rn(c1, wi));
        w[i] = axmy(v[i], c2, wi);
    });
}

// w = v, the copy the single loop makes with hipMemcpyAsync
__global__ void __launch_bounds__(256) k_copy_m(double* __restrict__ w, const double* __restrict__ v, size_t s, long n,
                                                unsigned long long live) {
    const int c = (int)blockIdx.y;
    if (!col_live(live, c)) return;
    w += (size_t)c * s;
    v += (size_t)c * s;
    sweep_m(n, [&](long i) { w[i] = v[i]; });
}

// k_sumsq per column, with the column's exponent K.e[c], into the column's pair red[c][2], [3]
__global__ void __launch_bounds__(256) k_sumsq_m(const double* __restrict__ x, size_t s, long n, ColArgs K,
                                                 unsigned long long* __restrict__ red) {
    __shared__ unsigned long long wlo[4], whi[4];
    const int c = (int)blockIdx.y;
    if (!col_live(K.live, c)) return;
    x += (size_t)c * s;
    unsigned long long* const acc = red + (size_t)c * kRedM + 2;
    const int e = K.e[c];
    unsigned long long lo = 0ull, hi = 0ull;
    sweep_m(n, [&](long i) {
        const double v = x[i];
        const unsigned long long q = (unsigned long long)(long long)rint(ldexp(__dmul_rn(v, v), -e));
        lo += q;
        hi += lo < q ? 1ull : 0ull;
    });
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
        if (lo | hi) {
            const unsigned long long old = lo ? atomicAdd(acc, lo) : 0ull;
            const unsigned long long h = hi + ((old + lo) < old ? 1ull : 0ull);
            if (h) atomicAdd(acc + 1, h);
        }
    }
}

// The device words of the batched reductions, kRedM per column, and the grid's second dimension
struct VecM {
    unsigned long long* red;
    int cus, S;
    dim3 grid(size_t n) const { return dim3(stride_blocks(cus, n, 1).x, (unsigned)S); }
    size_t red_bytes() const { return (size_t)S * kRedM * sizeof(unsigned long long); }
};

inline unsigned long long col_bit(int c) { return 1ull << c; }

// max |x| over the finite values of the columns in `live`, one launch and one read-back: M [S], 0 for a column outside
int absmax_m(const char* who, const VecM& V, const double* d, size_t s, size_t n, unsigned long long live, double* M) {
    unsigned long long h[kMultiMax * kRedM];
    RTMI_HIP(hipMemsetAsync(V.red, 0, V.red_bytes(), nullptr));
    hipLaunchKernelGGL(k_absmax_finite_m, V.grid(n), dim3(256), 0, nullptr, d, s, (long)n, live, V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) std::memcpy(&M[c], &h[(size_t)c * kRedM], sizeof(double));
    return RTMI_OK;
}

// norm_of for the columns in `live`, from their maxima M: nrm [S] and range [S]; one launch, one read-back
int norms_m(const char* who, const VecM& V, const double* d, size_t s, size_t n, unsigned long long live, const double* M, double* nrm,
            bool* range) {
    ColArgs K{};
    for (int c = 0; c < V.S; c++) {
        if (!(live & col_bit(c))) continue;
        range[c] = false;
        nrm[c] = 0.0;
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
    hipLaunchKernelGGL(k_sumsq_m, V.grid(n), dim3(256), 0, nullptr, d, s, (long)n, K, V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) {
        if (!(K.live & col_bit(c))) continue;
        const unsigned long long s0 = h[(size_t)c * kRedM + 2], s1 = h[(size_t)c * kRedM + 3];
        const unsigned long long lo = s0 + rt::kFixBias, hi = s1 + (lo < s0 ? 1ull : 0ull);
        const int e = K.e[c], odd = e & 1;
        nrm[c] = std::ldexp(std::sqrt(std::ldexp(rt::fix_to_double(lo, hi), odd)), (e - odd) / 2);
    }
    return RTMI_OK;
}

// axmy_norm for the columns in K.live with a = K.a: two launches, two read-backs
int axmy_norm_m(const char* who, const VecM& V, double* y, const double* t, size_t s, const double* f, size_t fs, const ColArgs& K, size_t n,
                double* nrm, bool* range) {
    unsigned long long h[kMultiMax * kRedM];
    double M[kMultiMax];
    RTMI_HIP(hipMemsetAsync(V.red, 0, V.red_bytes(), nullptr));
    hipLaunchKernelGGL(k_axmy_absmax_m, V.grid(n), dim3(256), 0, nullptr, y, t, s, f, fs, K, (long)n, V.red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(h, V.red, V.red_bytes(), hipMemcpyDeviceToHost));
    for (int c = 0; c < V.S; c++) std::memcpy(&M[c], &h[(size_t)c * kRedM], sizeof(double));
    return norms_m(who, V, y, s, n, K.live, M, nrm, range);
}

int scale_m(const char* who, const VecM& V, double* y, double* z, size_t s, const double* f, size_t fs, const ColArgs& K, size_t n) {
    hipLaunchKernelGGL(k_scale_m, V.grid(n), dim3(256), 0, nullptr, y, z, s, f, fs, K, (long)n);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

int sub_mul_m(const char* who, const VecM& V, double* y, size_t s, const double* t, size_t ts, const double* f, size_t fs, size_t n,
              unsigned long long live) {
    hipLaunchKernelGGL(k_sub_mul_m, V.grid(n), dim3(256), 0, nullptr, y, s, t, ts, f, fs, (long)n, live);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

int result_m(const char* who, const VecM& V, double* x, size_t s, const double* dc, const double* x0, size_t n, unsigned long long live) {
    hipLaunchKernelGGL(k_result_m, V.grid(n), dim3(256), 0, nullptr, x, s, dc, x0, (long)n, live);
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}

// lsqr_loop for V.S columns in lock-step: B's vectors are planes of `per` and `nm` values per column, u holds the right-hand
// sides, x is zero.  O.wr has wrs values per column (0: one weighting for all), O.dc is one vector for all, O.uw and O.vd are
// planes like u and v; O.x0 is the caller's business, as in tomo_lsqr_basis_run.
//   Ax(s, y, mask)          y = A s for the columns in mask (others may be computed, none is read back)
//   At(s, g, mask, range)   g = A^T s for the columns in mask, range [S]: the column's bound left the normal range, g not written
// One rt::LsqrState per column.  A column leaves where the single loop leaves -- lsqr_done, a zero right-hand side or first alfa,
// a norm or an A^T bound out of range (its iteration abandoned: S = S0) -- and from then on no pass has it in its mask.
// history [S][iter_lim][4] (host, zeroed by the caller) or NULL; out [S].
template <typename AX, typename AT>
int lsqr_loop_multi(const char* who, const VecM& V, const rtmi_lsqr_params* lp, size_t per, size_t nm, const LsqrVectors& B, AX&& Ax, AT&& At,
                    double* history, rtmi_lsqr_stats* out, const LsqrOptions& O, size_t wrs) {
    const int S = V.S;
    double *const u = B.u, *const Av = B.Av, *const v = B.v, *const w = B.w, *const xd = B.x, *const Atu = B.Atu;
    const double *const uin = O.wr ? O.uw : u, *const vin = O.dc ? O.vd : v;
    const unsigned long long all = S == 64 ? ~0ull : (col_bit(S) - 1ull);
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
    if (O.wr) RTMI_RC(sub_mul_m(who, V, u, per, nullptr, 0, O.wr, wrs, per, all));
    RTMI_RC(absmax_m(who, V, u, per, per, all, M));
    RTMI_RC(norms_m(who, V, u, per, per, all, M, nrm, rr));
    unsigned long long live = 0ull;                           // the columns whose loop goes on
    each(all, [&](int c) {
        range[c] = rr[c];
        if (!rr[c] && rt::lsqr_first_beta(St[c], nrm[c])) live |= col_bit(c);
    });
    if (live) {
        K.live = live;
        each(live, [&](int c) { K.a[c] = 1.0 / St[c].beta; });
        RTMI_RC(scale_m(who, V, u, O.uw, per, O.wr, wrs, K, per));
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
        if (O.dc) RTMI_RC(sub_mul_m(who, V, v, nm, nullptr, 0, O.dc, 0, nm, live));
        RTMI_RC(absmax_m(who, V, v, nm, nm, live, M));
        RTMI_RC(norms_m(who, V, v, nm, nm, live, M, nrm, rr));
        unsigned long long next = 0ull;
        each(live, [&](int c) {
            if (rr[c]) range[c] = true;
            else if (rt::lsqr_first_alfa(St[c], nrm[c])) next |= col_bit(c);
        });
        live = next;
        if (live) {
            K.live = live;
            each(live, [&](int c) { K.a[c] = 1.0 / St[c].alfa; });
            RTMI_RC(scale_m(who, V, v, O.vd, nm, O.dc, 0, K, nm));
            hipLaunchKernelGGL(k_copy_m, V.grid(nm), dim3(256), 0, nullptr, w, v, nm, (long)nm, live);
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
        RTMI_RC(axmy_norm_m(who, V, u, Av, per, O.wr, wrs, K, per, nrm, rr));        // u = A v - alfa u
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
            RTMI_RC(scale_m(who, V, u, O.uw, per, O.wr, wrs, K, per));
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
            RTMI_RC(axmy_norm_m(who, V, v, Atu, nm, O.dc, 0, K, nm, nrm, rr));       // v = A^T u - beta v
            ColArgs Ks{};
            each(stepped, [&](int c) {
                if (rr[c]) {
                    abandon(c);
                    return;
                }
                // a v that is not scaled (alfa = 0) still needs its copy: a factor 1.0 changes no bit of v
                if (rt::lsqr_alfa(St[c], nrm[c])) { Ks.a[c] = 1.0 / St[c].alfa; Ks.live |= col_bit(c); }
                else if (O.dc) { Ks.a[c] = 1.0; Ks.live |= col_bit(c); }
            });
            if (Ks.live) RTMI_RC(scale_m(who, V, v, O.vd, nm, O.dc, 0, Ks, nm));
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
            hipLaunchKernelGGL(k_xw_m, V.grid(nm), dim3(256), 0, nullptr, xd, w, v, nm, K, (long)nm);
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
        RTMI_RC(result_m(who, V, xd, nm, O.dc, nullptr, nm, all));
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
