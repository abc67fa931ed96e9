// kirchhoff.hip -- Kirchhoff migration and modelling from traveltime tables (rtmi_kirchhoff_create / _migrate / _model /
// _destroy): the diffraction-stack operator pair L^T (traces -> image, optionally split into opening-angle bins) and L
// (reflectivity model -> traces), exact transposes of each other up to rounding.  include/rtmi.h states the operator; DESIGN.md
// section 14 the kernels and the fixed-point derivation.
//   L^T  one lane per image node, x fastest (table reads are coalesced).  The lane walks the traces in the caller's order and
//        adds into an fp64 register (no bins) or into its own column of an LDS array [bin][lane]: no atomics, one fixed order.
//        T, amp and theta of the source are kept while the source index does not change (a wave-uniform test).
//   L    one block per trace.  The trace's samples are two-word (128-bit) fixed-point accumulators in LDS; the lanes sweep the
//        nodes, round each contribution once to an integer number of quanta 2^scale_exp and add it with a returning 64-bit LDS
//        atomic (the carry into the high word is read off the returned old value: rt_fix128.h).  Integer sums
//        commute, so the result has the same bits in every schedule and trace order.  The block converts and stores its trace.
// Several arrivals per node (rtmi_kirchhoff_create_multi / _migrate2 / _model2): tables [P][K][nn], a trace
// meets a node in K^2 pairs of a source and a receiver arrival, each rotated by the phase of its caustic count -- a choice of
// one of two trace channels and a sign.  k_migrate_multi and k_model_multi are the two kernels above with the pair loops
// unrolled over the template parameter K: the 2 K table values of a (trace, node) are loaded once and serve its K^2 pairs.
// The tables and the geometry live on the device in the handle.  Every kernel has one launch path, on device pointers
// (rtmi_kirchhoff_migrate_dev / _model_dev); the host-pointer entries upload into the handle's staging buffers,
// run that path on them and download.  The model's quantum comes from k_absmax_finite, a reduction over the model on the device.
// What the pair's arithmetic, the handle and its creation share with the anti-aliased pair (kirchhoff_aa.hip): rt_kirchhoff.h.
#include "rt_kirchhoff.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ L^T
// image [nb][nn]; counts [gridDim.x]: the block's contributing pairs (plain stores, summed by the host).
template <bool AMP, bool BINS>
__global__ void k_migrate(KArgs A, const double* __restrict__ data, double* __restrict__ image, unsigned long long* __restrict__ counts) {
    extern __shared__ double acc[];                           // BINS: [nb][blockDim.x]
    __shared__ unsigned long long wcnt[4];
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long x0 = (long)blockIdx.x * BS + tid;
    const bool in = x0 < A.nn;
    const long x = in ? x0 : A.nn - 1;                        // lanes past the image read its last node and store nothing
    double sum = 0.0;
    if (BINS)
        for (int b = 0; b < A.nb; b++) acc[b * BS + tid] = 0.0;
    unsigned long long cnt = 0;
    int sprev = -1;
    double Ts = 0.0, As = 0.0, Hs = 0.0;
#pragma unroll 4
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform: a shot-ordered list re-reads the source rarely
            Ts = A.T[(size_t)s * A.nn + x];
            if (AMP) As = A.amp[(size_t)s * A.nn + x];
            if (BINS) Hs = A.theta[(size_t)s * A.nn + x];
            sprev = s;
        }
        const double Tr = A.T[(size_t)r * A.nn + x];
        const double Ar = AMP ? A.amp[(size_t)r * A.nn + x] : 0.0;
        const double Hr = BINS ? A.theta[(size_t)r * A.nn + x] : 0.0;
        const Pair p = pair_of<AMP, BINS>(A, Ts, Tr, As, Ar, Hs, Hr, wk);
        const double* d = data + (size_t)k * A.nt + p.j;      // j = 0 when the pair does not contribute: always in bounds
        const double d0 = d[0], d1 = d[1];
        const double v = p.c * (d0 + p.a * (d1 - d0));
        if (BINS) {
            if (p.ok) acc[p.b * BS + tid] += v;
        } else {
            sum += p.ok ? v : 0.0;                            // sum is never -0: adding +0 changes no bit
        }
        cnt += (p.ok && in) ? 1ull : 0ull;
    }
    if (in) {
        if (BINS)
            for (int b = 0; b < A.nb; b++) image[(size_t)b * A.nn + x] = acc[b * BS + tid];
        else
            image[x] = sum;
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------ L
// Sample i's accumulator is (lo[i], hi[i]) of rt_fix128.h.
// One block per trace; data [N][nt]; counts [N].  The trace is processed in windows of at most kWindow samples.
template <bool AMP, bool BINS>
__global__ void k_model(KArgs A, const double* __restrict__ m, int e, int W, double* __restrict__ data,
                        unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned long long fix[];               // lo [W], hi [W]
    __shared__ unsigned long long wcnt[4];
    unsigned long long* lo = fix;
    unsigned long long* hi = fix + W;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long k = blockIdx.x;
    const int s = A.isrc[k], r = A.irec[k];
    const double wk = A.w[k];
    const double* Tsp = A.T + (size_t)s * A.nn;
    const double* Trp = A.T + (size_t)r * A.nn;
    const double* Asp = AMP ? A.amp + (size_t)s * A.nn : nullptr;
    const double* Arp = AMP ? A.amp + (size_t)r * A.nn : nullptr;
    const double* Hsp = BINS ? A.theta + (size_t)s * A.nn : nullptr;
    const double* Hrp = BINS ? A.theta + (size_t)r * A.nn : nullptr;
    unsigned long long cnt = 0;
    for (long j0 = 0; j0 < A.nt; j0 += W) {
        const long j1 = (j0 + W < A.nt) ? j0 + W : A.nt;      // the window [j0, j1)
        for (int i = tid; i < W; i += BS) { lo[i] = rt::kFixBias; hi[i] = 0ull; }
        __syncthreads();
#pragma unroll 2
        for (long x = tid; x < A.nn; x += BS) {
            const Pair p = pair_of<AMP, BINS>(A, Tsp[x], Trp[x], AMP ? Asp[x] : 0.0, AMP ? Arp[x] : 0.0, BINS ? Hsp[x] : 0.0,
                                              BINS ? Hrp[x] : 0.0, wk);
            if (!p.ok) continue;
            if (j0 == 0) cnt++;
            if (p.j + 1 < j0 || p.j >= j1) continue;
            const double cm = p.c * m[(size_t)p.b * A.nn + x];
            if (!(fabs(cm) < INFINITY)) continue;             // a non-finite model value contributes nothing
            const double v0 = cm * (1.0 - p.a), v1 = cm * p.a;
            if (p.j >= j0) (void)rt::add128(lo, hi, (int)(p.j - j0), (long long)rint(ldexp(v0, -e)));
            if (p.j + 1 < j1) (void)rt::add128(lo, hi, (int)(p.j + 1 - j0), (long long)rint(ldexp(v1, -e)));
        }
        __syncthreads();
        for (long i = tid; i < j1 - j0; i += BS) data[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(lo[i], hi[i]), e);
        __syncthreads();
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[k] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------ several arrivals
// L^T.  data0, data1 [N][nt] (data1 is read only with PHASE); image [nb][nn]; counts [gridDim.x].  The sum runs over k, then ks,
// then kr, as rtmi.h defines it.  All K^2 gathers of a trace are issued before the first add, outside the `contributes` test.
template <int K, bool AMP, bool BINS, bool PHASE>
__global__ void __launch_bounds__(256) k_migrate_multi(KArgs A, const int8_t* __restrict__ kmah, const double* __restrict__ data0,
                                const double* __restrict__ data1, double* __restrict__ image, unsigned long long* __restrict__ counts) {
    extern __shared__ double acc[];                           // BINS: [nb][blockDim.x]
    __shared__ unsigned long long wcnt[4];
    constexpr int KK = K * K;
    constexpr int kUnroll = K == 1 ? 4 : K == 2 ? 2 : 1;      // pairs in flight: 4, 8, 9, 16
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long x0 = (long)blockIdx.x * BS + tid;
    const bool in = x0 < A.nn;
    const long x = in ? x0 : A.nn - 1;
    double sum = 0.0;
    if (BINS)
        for (int b = 0; b < A.nb; b++) acc[b * BS + tid] = 0.0;
    unsigned long long cnt = 0;
    int sprev = -1;
    Arr<K> S;
#pragma unroll
    for (int i = 0; i < K; i++) { S.T[i] = 0.0; S.A[i] = 0.0; S.H[i] = 0.0; S.m[i] = 0; }
#pragma unroll kUnroll
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform, as in k_migrate
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)s * K * A.nn + x, S);
            sprev = s;
        }
        Arr<K> R;
        load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)r * K * A.nn + x, R);
        Pair p[KK];
        bool neg[KK];
        double d0[KK], d1[KK];
#pragma unroll
        for (int i = 0; i < KK; i++) {
            const int ks = i / K, kr = i % K;
            p[i] = pair_of<AMP, BINS>(A, S.T[ks], R.T[kr], S.A[ks], R.A[kr], S.H[ks], R.H[kr], wk);
            const double* ch = data0;
            neg[i] = false;
            if (PHASE) {
                const Phase ph = phase_of(S.m[ks], R.m[kr]);
                p[i].ok = p[i].ok && ph.valid;
                neg[i] = ph.neg;
                ch = ph.odd ? data1 : data0;
            }
            const double* d = ch + (size_t)k * A.nt + p[i].j; // j = 0 when the range test failed: always in bounds
            d0[i] = d[0];
            d1[i] = d[1];
        }
#pragma unroll
        for (int i = 0; i < KK; i++) {
            const double cv = p[i].c * (d0[i] + p[i].a * (d1[i] - d0[i]));
            const double v = neg[i] ? -cv : cv;
            if (BINS) {
                if (p[i].ok) acc[p[i].b * BS + tid] += v;
            } else {
                sum += p[i].ok ? v : 0.0;                     // sum is never -0: adding +0 changes no bit
            }
            cnt += (p[i].ok && in) ? 1ull : 0ull;
        }
    }
    if (in) {
        if (BINS)
            for (int b = 0; b < A.nb; b++) image[(size_t)b * A.nn + x] = acc[b * BS + tid];
        else
            image[x] = sum;
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[blockIdx.x] = t;
    }
}

// L.  One block per trace; data0, data1 [N][nt] (data1 is written only with PHASE); counts [N].  Channel c's accumulators are
// lo = fix + 2 c W, hi = lo + W; windows of W samples as in k_model.  Two channels double a block's LDS, which halves the blocks
// a CU holds: the host launches 512 lanes with PHASE, so that the waves per CU stay what they were (any block size gives the
// same bits).
template <int K, bool AMP, bool BINS, bool PHASE>
__global__ void __launch_bounds__(512) k_model_multi(KArgs A, const int8_t* __restrict__ kmah, const double* __restrict__ m, int e, int W,
                              double* __restrict__ data0, double* __restrict__ data1, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned long long fix[];               // lo0 [W], hi0 [W] and, PHASE, lo1 [W], hi1 [W]
    __shared__ unsigned long long wcnt[8];
    constexpr int KK = K * K;
    constexpr int kChannels = PHASE ? 2 : 1;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long k = blockIdx.x;
    const int s = A.isrc[k], r = A.irec[k];
    const double wk = A.w[k];
    unsigned long long cnt = 0;
    for (long j0 = 0; j0 < A.nt; j0 += W) {
        const long j1 = (j0 + W < A.nt) ? j0 + W : A.nt;      // the window [j0, j1)
        for (int i = tid; i < 2 * kChannels * W; i += BS) fix[i] = ((i / W) & 1) ? 0ull : rt::kFixBias;
        __syncthreads();
        for (long x = tid; x < A.nn; x += BS) {
            Arr<K> S, R;
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)s * K * A.nn + x, S);
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)r * K * A.nn + x, R);
            const double mx = BINS ? 0.0 : m[x];
#pragma unroll
            for (int i = 0; i < KK; i++) {
                const int ks = i / K, kr = i % K;
                Pair p = pair_of<AMP, BINS>(A, S.T[ks], R.T[kr], S.A[ks], R.A[kr], S.H[ks], R.H[kr], wk);
                Phase ph{true, false, false};
                if (PHASE) ph = phase_of(S.m[ks], R.m[kr]);
                if (!(p.ok && ph.valid)) continue;
                if (j0 == 0) cnt++;
                if (p.j + 1 < j0 || p.j >= j1) continue;
                const double cm = p.c * (BINS ? m[(size_t)p.b * A.nn + x] : mx);
                if (!(fabs(cm) < INFINITY)) continue;         // a non-finite model value contributes nothing
                const double u0 = cm * (1.0 - p.a), u1 = cm * p.a;
                const double v0 = ph.neg ? -u0 : u0, v1 = ph.neg ? -u1 : u1;
                unsigned long long* lo = fix + (ph.odd ? 2 * W : 0);
                unsigned long long* hi = lo + W;
                if (p.j >= j0) (void)rt::add128(lo, hi, (int)(p.j - j0), (long long)rint(ldexp(v0, -e)));
                if (p.j + 1 < j1) (void)rt::add128(lo, hi, (int)(p.j + 1 - j0), (long long)rint(ldexp(v1, -e)));
            }
        }
        __syncthreads();
        for (long i = tid; i < j1 - j0; i += BS) {
            data0[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(fix[i], fix[W + i]), e);
            if (PHASE) data1[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(fix[2 * W + i], fix[3 * W + i]), e);
        }
        __syncthreads();
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int q = 0; q < (BS + 63) / 64; q++) t += wcnt[q];
        counts[k] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------ max |x|
// *out = the bits of max |x_i| over the finite x_i of n doubles, 0 when there is none; *out starts from 0.  A grid-stride pass,
// 16-byte loads when x is 16-byte aligned (wide), a wave and a block reduction, one integer atomic max per block (block_max_to).
// fmax is exact: any order gives the same bits.  The model's quantum (model_exponent) and the solver's norms read it.
__global__ void __launch_bounds__(256) k_absmax_finite(const double* __restrict__ x, long n, bool wide, unsigned long long* __restrict__ out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x, gsz = (long)gridDim.x * 256;
    double m = 0.0;
    auto take = [&](double v) {
        const double a = fabs(v);
        m = a < INFINITY ? fmax(m, a) : m;                    // NaN fails the compare
    };
    if (wide) {
        const double2* x2 = (const double2*)x;
        for (long i = gid; i < n / 2; i += gsz) {
            const double2 v = x2[i];
            take(v.x);
            take(v.y);
        }
        if ((n & 1) && gid == 0) take(x[n - 1]);
    } else {
        for (long i = gid; i < n; i += gsz) take(x[i]);
    }
    block_max_to(out, m);
}

// The kernel of (karr, amp, bins, phase): the flags become template arguments one at a time.
struct MultiLaunch {
    dim3 grid, blk;
    size_t lds;
    KArgs A;
    const int8_t* kmah;
    const double* in0;      // migrate: data0; model: the model
    const double* in1;      // migrate: data1
    double *out0, *out1;    // migrate: image, -; model: data0, data1
    int e, W;
    unsigned long long* counts;
};
template <bool MODEL, int K, bool... F>
void launch_multi(const bool* f, const MultiLaunch& L) {
    if constexpr (sizeof...(F) == 3) {
        if constexpr (MODEL)
            hipLaunchKernelGGL((k_model_multi<K, F...>), L.grid, L.blk, L.lds, nullptr, L.A, L.kmah, L.in0, L.e, L.W, L.out0, L.out1, L.counts);
        else
            hipLaunchKernelGGL((k_migrate_multi<K, F...>), L.grid, L.blk, L.lds, nullptr, L.A, L.kmah, L.in0, L.in1, L.out0, L.counts);
    } else {
        if (*f) launch_multi<MODEL, K, F..., true>(f + 1, L);
        else launch_multi<MODEL, K, F..., false>(f + 1, L);
    }
}
template <bool MODEL>
void launch_multi(int karr, bool amp, bool bins, bool phase, const MultiLaunch& L) {
    const bool f[3] = {amp, bins, phase};
    switch (karr) {
        case 1: launch_multi<MODEL, 1>(f, L); break;
        case 2: launch_multi<MODEL, 2>(f, L); break;
        case 3: launch_multi<MODEL, 3>(f, L); break;
        default: launch_multi<MODEL, 4>(f, L); break;
    }
}

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_create(const rtmi_kirchhoff_params* kp, const double* T, const double* amp, const double* theta,
                                      const int32_t* isrc, const int32_t* irec, const double* w, rtmi_kirchhoff** out) {
    const char* who = "rtmi_kirchhoff_create";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_ARG(kp, "null kp");
    return create_impl(who, kp, 0, T, amp, theta, nullptr, isrc, irec, w, out);
}

RTMI_EXPORT int rtmi_kirchhoff_create_multi(const rtmi_kirchhoff_multi_params* mp, const double* T, const double* amp,
                                            const double* theta, const double* kmah, const int32_t* isrc, const int32_t* irec,
                                            const double* w, rtmi_kirchhoff** out) {
    const char* who = "rtmi_kirchhoff_create_multi";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_ARG(mp, "null kp");
    rtmi_kirchhoff_params kp{};
    RTMI_RC(multi_params(who, mp, &kp));
    return create_impl(who, &kp, mp->karr, T, amp, theta, kmah, isrc, irec, w, out);
}

// ------------------------------------------------------------------------------------------------------------ device pointers
int rtmi_internal_absmax_finite(const char* who, unsigned long long* red, int cus, const double* d_x, size_t n, double* out) {
    RTMI_HIP(hipMemsetAsync(red, 0, sizeof(unsigned long long), nullptr));
    const bool wide = ((uintptr_t)d_x & 15) == 0;
    hipLaunchKernelGGL(k_absmax_finite, stride_blocks(cus, n, 2), dim3(256), 0, nullptr, d_x, (long)n, wide, red);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(hipMemcpy(out, red, sizeof(double), hipMemcpyDeviceToHost));         // the bits of a double
    return RTMI_OK;
}

int rtmi_internal_kirchhoff_migrate_dev(rtmi_kirchhoff* k, const char* who, const double* d0, const double* d1, double* d_image,
                                        rtmi_kirchhoff_stats* st, bool counts) {
    if (k->nlev) return rtmi_internal_kirchhoff_aa_migrate_dev(k, who, d0, d1, d_image, st, counts);
    const size_t N = (size_t)k->kp.N, nn = k->nn;
    const bool phase = k->kmah != nullptr;
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const int BS = migrate_block(k->nb);
    const dim3 grid((unsigned)((nn + BS - 1) / BS)), blk(BS);
    const bool bins = k->kp.nbin > 0, has_amp = k->amp != nullptr;
    const size_t lds = bins ? (size_t)k->nb * BS * sizeof(double) : 0;
    const KArgs A = k->args();
    MultiLaunch L{};
    L.grid = grid;
    L.blk = blk;
    L.lds = lds;
    L.A = A;
    L.kmah = k->kmah;
    L.in0 = d0;
    L.in1 = phase ? d1 : nullptr;
    L.out0 = d_image;
    L.counts = k->counts;
    RTMI_HIP(ev.mark(0));
    if (k->karr) launch_multi<false>(k->karr, has_amp, bins, phase, L);
    else if (has_amp && bins) hipLaunchKernelGGL((k_migrate<true, true>), grid, blk, lds, nullptr, A, d0, d_image, k->counts);
    else if (has_amp) hipLaunchKernelGGL((k_migrate<true, false>), grid, blk, lds, nullptr, A, d0, d_image, k->counts);
    else if (bins) hipLaunchKernelGGL((k_migrate<false, true>), grid, blk, lds, nullptr, A, d0, d_image, k->counts);
    else hipLaunchKernelGGL((k_migrate<false, false>), grid, blk, lds, nullptr, A, d0, d_image, k->counts);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    if (st) {
        const int kk = k->karr ? k->karr * k->karr : 1;
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->pairs = (int64_t)(N * nn) * kk;
        if (counts) RTMI_RC(read_counts(k, grid.x, &st->contributing, who));
    }
    return RTMI_OK;
}

int rtmi_internal_kirchhoff_model_dev(rtmi_kirchhoff* k, const char* who, const double* d_model, double* d0, double* d1,
                                      rtmi_kirchhoff_stats* st, bool counts) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn, nm = (size_t)k->nb * nn;
    // the quantum: one bound on one contribution for every kind of handle (DESIGN.md 19 on the number of contributions)
    double max_m = 0.0;
    RTMI_RC(rtmi_internal_absmax_finite(who, k->red, k->cus, d_model, nm, &max_m));
    const int e = model_exponent(k, max_m);
    if (k->nlev) return rtmi_internal_kirchhoff_aa_model_dev(k, who, d_model, e, d0, d1, st, counts);
    const bool phase = k->kmah != nullptr;
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    const size_t window = phase ? kWindow / 2 : kWindow;      // two channels share the 64 KiB
    const int W = (int)(nt < window ? nt : window);
    const dim3 grid((unsigned)N), blk(phase ? 512 : 256);
    const size_t lds = (size_t)W * (phase ? 4 : 2) * sizeof(unsigned long long);
    const bool bins = k->kp.nbin > 0, has_amp = k->amp != nullptr;
    const KArgs A = k->args();
    MultiLaunch L{};
    L.W = W;
    L.e = e;
    L.grid = grid;
    L.blk = blk;
    L.lds = lds;
    L.A = A;
    L.kmah = k->kmah;
    L.in0 = d_model;
    L.out0 = d0;
    L.out1 = phase ? d1 : nullptr;
    L.counts = k->counts;
    RTMI_HIP(ev.mark(0));
    if (k->karr) launch_multi<true>(k->karr, has_amp, bins, phase, L);
    else if (has_amp && bins) hipLaunchKernelGGL((k_model<true, true>), grid, blk, lds, nullptr, A, d_model, e, W, d0, k->counts);
    else if (has_amp) hipLaunchKernelGGL((k_model<true, false>), grid, blk, lds, nullptr, A, d_model, e, W, d0, k->counts);
    else if (bins) hipLaunchKernelGGL((k_model<false, true>), grid, blk, lds, nullptr, A, d_model, e, W, d0, k->counts);
    else hipLaunchKernelGGL((k_model<false, false>), grid, blk, lds, nullptr, A, d_model, e, W, d0, k->counts);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    if (st) {
        const int kk = k->karr ? k->karr * k->karr : 1;
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->pairs = (int64_t)(N * nn) * kk;
        st->scale_exp = e;
        if (counts) RTMI_RC(read_counts(k, N, &st->contributing, who));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_kirchhoff_migrate_dev(rtmi_kirchhoff* k, const double* d_data0, const double* d_data1, double* d_image,
                                           rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_migrate_dev";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(d_data0, "null d_data0");
    RTMI_ARG(d_image, "null d_image");
    RTMI_ARG(d_data1 || !k->kmah, "null d_data1 on a handle that has kmah");
    RTMI_RC(check_device(k, who));
    const size_t per = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    RTMI_RC(check_device_pointer(k, who, d_data0, per, "d_data0"));
    if (k->kmah) RTMI_RC(check_device_pointer(k, who, d_data1, per, "d_data1"));
    RTMI_RC(check_device_pointer(k, who, d_image, (size_t)k->nb * k->nn * sizeof(double), "d_image"));
    return rtmi_internal_kirchhoff_migrate_dev(k, who, d_data0, d_data1, d_image, st, true);
}

RTMI_EXPORT int rtmi_kirchhoff_model_dev(rtmi_kirchhoff* k, const double* d_model, double* d_data0, double* d_data1,
                                         rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_model_dev";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(d_model, "null d_model");
    RTMI_ARG(d_data0, "null d_data0");
    RTMI_ARG(d_data1 || !k->kmah, "null d_data1 on a handle that has kmah");
    RTMI_RC(check_device(k, who));
    const size_t per = (size_t)k->kp.N * (size_t)k->kp.nt * sizeof(double);
    const bool two = k->karr >= 1 && d_data1;                 // on a handle of rtmi_kirchhoff_create d_data1 is ignored
    RTMI_RC(check_device_pointer(k, who, d_model, (size_t)k->nb * k->nn * sizeof(double), "d_model"));
    RTMI_RC(check_device_pointer(k, who, d_data0, per, "d_data0"));
    if (two) RTMI_RC(check_device_pointer(k, who, d_data1, per, "d_data1"));
    RTMI_RC(rtmi_internal_kirchhoff_model_dev(k, who, d_model, d_data0, d_data1, st, true));
    if (two && !k->kmah) RTMI_HIP(hipMemset(d_data1, 0, per)); // without kmah every pair is of channel 0
    return RTMI_OK;
}

// ------------------------------------------------------------------------------------------------------------ host pointers
// upload into the handle's staging buffers, the body above on them, download
namespace {

int migrate_host(rtmi_kirchhoff* k, const char* who, const double* data0, const double* data1, double* image, rtmi_kirchhoff_stats* st) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn;
    const bool phase = k->kmah != nullptr;
    const double t_up = now_ms();
    RTMI_HIP(hipMemcpy(k->data, data0, N * nt * sizeof(double), hipMemcpyHostToDevice));
    if (phase) RTMI_HIP(hipMemcpy(k->data + N * nt, data1, N * nt * sizeof(double), hipMemcpyHostToDevice));
    const double upload_ms = now_ms() - t_up;
    RTMI_RC(rtmi_internal_kirchhoff_migrate_dev(k, who, k->data, phase ? k->data + N * nt : nullptr, k->image, st, true));
    RTMI_HIP(hipMemcpy(image, k->image, (size_t)k->nb * nn * sizeof(double), hipMemcpyDeviceToHost));
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}

int model_host(rtmi_kirchhoff* k, const char* who, const double* model, double* data0, double* data1, rtmi_kirchhoff_stats* st) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nm = (size_t)k->nb * k->nn;
    const bool phase = k->kmah != nullptr;
    const double t_up = now_ms();
    RTMI_HIP(hipMemcpy(k->image, model, nm * sizeof(double), hipMemcpyHostToDevice));
    const double upload_ms = now_ms() - t_up;
    RTMI_RC(rtmi_internal_kirchhoff_model_dev(k, who, k->image, k->data, phase ? k->data + N * nt : nullptr, st, true));
    RTMI_HIP(hipMemcpy(data0, k->data, N * nt * sizeof(double), hipMemcpyDeviceToHost));
    if (data1) {
        if (phase) RTMI_HIP(hipMemcpy(data1, k->data + N * nt, N * nt * sizeof(double), hipMemcpyDeviceToHost));
        else std::memset(data1, 0, N * nt * sizeof(double));  // without kmah every pair is of channel 0
    }
    if (st) st->upload_ms = upload_ms;
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_migrate(rtmi_kirchhoff* k, const double* data, double* image, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_migrate";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(data, "null data");
    RTMI_ARG(image, "null image");
    RTMI_ARG(k->karr == 0, "the handle is rtmi_kirchhoff_create_multi's: call rtmi_kirchhoff_migrate2");
    RTMI_RC(check_device(k, who));
    return migrate_host(k, who, data, nullptr, image, st);
}

RTMI_EXPORT int rtmi_kirchhoff_model(rtmi_kirchhoff* k, const double* model, double* data, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_model";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(model, "null model");
    RTMI_ARG(data, "null data");
    RTMI_ARG(k->karr == 0, "the handle is rtmi_kirchhoff_create_multi's: call rtmi_kirchhoff_model2");
    RTMI_RC(check_device(k, who));
    return model_host(k, who, model, data, nullptr, st);
}

RTMI_EXPORT int rtmi_kirchhoff_migrate2(rtmi_kirchhoff* k, const double* data0, const double* data1, double* image,
                                        rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_migrate2";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(data0, "null data0");
    RTMI_ARG(image, "null image");
    RTMI_ARG(k->karr >= 1, "the handle is rtmi_kirchhoff_create's: call rtmi_kirchhoff_migrate");
    RTMI_ARG(data1 || !k->kmah, "null data1 on a handle that has kmah");
    RTMI_RC(check_device(k, who));
    return migrate_host(k, who, data0, data1, image, st);
}

RTMI_EXPORT int rtmi_kirchhoff_model2(rtmi_kirchhoff* k, const double* model, double* data0, double* data1, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_model2";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(model, "null model");
    RTMI_ARG(data0, "null data0");
    RTMI_ARG(k->karr >= 1, "the handle is rtmi_kirchhoff_create's: call rtmi_kirchhoff_model");
    RTMI_ARG(data1 || !k->kmah, "null data1 on a handle that has kmah");
    RTMI_RC(check_device(k, who));
    return model_host(k, who, model, data0, data1, st);
}

RTMI_EXPORT void rtmi_kirchhoff_destroy(rtmi_kirchhoff* k) { delete k; }
