// kirchhoff.hip -- Kirchhoff migration and modelling from traveltime tables (rtmi_kirchhoff_create / _create_multi, _migrate /
// _model / _migrate2 / _model2 and their _dev forms, _illumination / _illumination_dev, _destroy): the diffraction-stack operator
// pair L^T (traces -> image, optionally split into opening-angle bins) and L (reflectivity model -> traces), exact transposes of
// each other up to rounding.
// include/rtmi.h states the operator; DESIGN.md section 14 the kernels and the fixed-point derivation; section 26 the illumination
// map, k_illumination: the sum of the squared weights of L^T's contributing pairs per image value, k_migrate without its traces.
//   L^T  one lane per image node, x fastest (table reads are coalesced).  The lane walks the traces in the caller's order and
//        adds into an fp64 register (no bins) or into its own column of an LDS array [bin][lane]: no atomics, one fixed order.
//        T, amp and theta of the source are kept while the source index does not change (a wave-uniform test).
//   L    one block per trace.  The trace's samples are two-word (128-bit) fixed-point accumulators in LDS; the lanes sweep the
//        nodes, round each contribution once to an integer number of quanta 2^scale_exp and add it with a returning 64-bit LDS
//        atomic (the carry into the high word is read off the returned old value: rt_fix128.h).  Integer sums
//        commute, so the result has the same bits in every schedule and trace order.  The block converts and stores its trace.
// One kernel text each, k_migrate and k_model <K, AMP, BINS, PHASE, AA>, serves every kind of handle:
//   K      arrivals per node: tables [P][K][nn], a trace meets a node in K^2 pairs of a source and a receiver
//          arrival; the pair loops are unrolled over K, the 2 K table values of a (trace, node) are loaded once and serve its K^2
//          pairs.  A handle of rtmi_kirchhoff_create runs K = 1: its tables [P][nn] are that layout.
//   PHASE  with kmah, each pair is rotated by the phase of its caustic count: a choice of one of two trace channels and a sign.
//   AA     anti-aliased by operator slope (rtmi_kirchhoff_create_aa): one more table value per slot, pt, and
//          per pair the choice of one level of a bank of filtered traces (L^T), or of per-level accumulators (L).  The bank's
//          filter and the sum over the levels are kirchhoff_aa.hip's.
// The tables and the geometry live on the device in the handle.  The kernels have one launch path, on device pointers
// (rtmi_kirchhoff_migrate_dev / _model_dev); the host-pointer entries upload into the handle's staging buffers,
// run that path on them and download.  The model's quantum comes from k_absmax_finite, a reduction over the model on the device.
#include <type_traits>

#include "rt_kirchhoff.h"

namespace {

// What the kernels of a handle that is not anti-aliased take in AAArgs' place: nothing.
struct NoAA {
    NoAA() = default;
    __host__ __device__ NoAA(const AAArgs&) {}
};
template <bool AA> using AAOf = std::conditional_t<AA, AAArgs, NoAA>;

// The level of a pair (rtmi.h): wave-uniform thresholds, 7 compares, no branch.  A NaN slope selects level 0; such a pair does not
// contribute.
__device__ __forceinline__ unsigned level_of(const AAArgs& Q, double inv_dt, double ps, double pr) {
    const double q1 = fabs(ps) * Q.asrc;
    const double q2 = fabs(pr) * Q.arec;
    const double q3 = fabs(ps + pr) * Q.amid;
    const double sl = fmax(fmax(q1, q2), q3) * inv_dt;
    unsigned l = 0;
#pragma unroll
    for (int i = 0; i < kMaxLev - 1; i++) l += sl > Q.thr[i] ? 1u : 0u;
    return l;
}

// pt of the K arrivals of one table at one node; without anti-aliasing there is none
template <int K> __device__ __forceinline__ void load_pt(const AAArgs& Q, long nn, size_t at, double (&o)[K]) {
#pragma unroll
    for (int i = 0; i < K; i++) o[i] = Q.pt[at + (size_t)i * nn];
}
template <int K> __device__ __forceinline__ void load_pt(const NoAA&, long, size_t, double (&)[K]) {}

// ------------------------------------------------------------------------------------------------------------ L^T
// data0, data1 [N][nt] (data1 is read only with PHASE); AA: data0 is the bank [nlev][channels][N][nt]; image [nb][nn]; counts
// [gridDim.x]: the block's contributing pairs (plain stores, summed by the host).  The sum runs over k, then ks, then kr, as rtmi.h
// defines it.  All K^2 gathers of a trace are issued before the first add, outside the `contributes` test; the level and, AA, the
// channel move the gather's base address by selects and a multiply, never by a branch.
template <int K, bool AMP, bool BINS, bool PHASE, bool AA>
__global__ void __launch_bounds__(256) k_migrate(KArgs A, const int8_t* __restrict__ kmah, const double* __restrict__ data0,
                                                 const double* __restrict__ data1, double* __restrict__ image,
                                                 unsigned long long* __restrict__ counts, AAOf<AA> Q) {
    extern __shared__ double acc[];                           // BINS: [nb][blockDim.x]
    constexpr int KK = K * K;
    constexpr int kUnroll = K == 1 ? 4 : K == 2 ? 2 : 1;      // pairs in flight: 4, 8, 9, 16
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long x0 = (long)blockIdx.x * BS + tid;
    const bool in = x0 < A.nn;
    const long x = in ? x0 : A.nn - 1;                        // lanes past the image read its last node and store nothing
    double sum = 0.0;
    if (BINS)
        for (int b = 0; b < A.nb; b++) acc[b * BS + tid] = 0.0;
    unsigned long long cnt = 0;
    int sprev = -1;
    Arr<K> S;
    double Sp[K];
#pragma unroll
    for (int i = 0; i < K; i++) { S.T[i] = 0.0; S.A[i] = 0.0; S.H[i] = 0.0; S.m[i] = 0; Sp[i] = 0.0; }
#pragma unroll kUnroll
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform: a shot-ordered list re-reads the source rarely
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)s * K * A.nn + x, S);
            load_pt<K>(Q, A.nn, (size_t)s * K * A.nn + x, Sp);
            sprev = s;
        }
        Arr<K> R;
        double Rp[K];
        load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)r * K * A.nn + x, R);
        load_pt<K>(Q, A.nn, (size_t)r * K * A.nn + x, Rp);
        Pair p[KK];
        bool neg[KK];
        double d0[KK], d1[KK];
#pragma unroll
        for (int i = 0; i < KK; i++) {
            const int ks = i / K, kr = i % K;
            p[i] = pair_of<AMP, BINS>(A, S.T[ks], R.T[kr], S.A[ks], R.A[kr], S.H[ks], R.H[kr], wk);
            const double* ch = data0;
            size_t at = 0;
            if constexpr (AA) {
                p[i].ok = p[i].ok && fabs(Sp[ks]) < INFINITY && fabs(Rp[kr]) < INFINITY;
                at = (size_t)level_of(Q, A.inv_dt, Sp[ks], Rp[kr]) * (size_t)Q.lstride;
            }
            neg[i] = false;
            if (PHASE) {
                const Phase ph = phase_of(S.m[ks], R.m[kr]);
                p[i].ok = p[i].ok && ph.valid;
                neg[i] = ph.neg;
                if constexpr (AA) at += ph.odd ? (size_t)Q.cstride : 0;     // an offset here, a pointer there: DESIGN.md section 20
                else ch = ph.odd ? data1 : data0;
            }
            const double* d = ch + at + (size_t)k * A.nt + p[i].j;          // j = 0 when the range test failed: always in bounds
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
    block_count_to(counts, blockIdx.x, cnt);
}

// ------------------------------------------------------------------------------------------------------------ illumination
// illum [nb][nn]: per (b, x) the sum over migrate's contributing pairs, in migrate's order, of (c c) ((1 - a)(1 - a) + a a): the
// squared weights a pair puts on its two samples (rtmi.h).  k_migrate's lane layout, table reads and shot-ordered reuse of the
// source's values, with no trace read: what is left is the table traffic.  kmah and pt only decide whether a pair contributes,
// so they are wave-uniform pointer tests here, not template arguments: NULL on a handle without them.
template <int K, bool AMP, bool BINS>
__global__ void __launch_bounds__(256) k_illumination(KArgs A, const int8_t* __restrict__ kmah, const double* __restrict__ pt,
                                                      double* __restrict__ illum, unsigned long long* __restrict__ counts) {
    extern __shared__ double acc[];                           // BINS: [nb][blockDim.x]
    constexpr int KK = K * K;
    constexpr int kUnroll = K == 1 ? 4 : K == 2 ? 2 : 1;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const long x0 = (long)blockIdx.x * BS + tid;
    const bool in = x0 < A.nn;
    const long x = in ? x0 : A.nn - 1;                        // lanes past the image read its last node and store nothing
    double sum = 0.0;
    if (BINS)
        for (int b = 0; b < A.nb; b++) acc[b * BS + tid] = 0.0;
    unsigned long long cnt = 0;
    int sprev = -1;
    Arr<K> S;
    double Sp[K];
    // the values that only gate a pair: the caustic count (0 without kmah: valid) and pt (0.0 without pt: finite)
    auto load_gates = [&](size_t at, Arr<K>& o, double (&p)[K]) {
#pragma unroll
        for (int i = 0; i < K; i++) {
            const size_t q = at + (size_t)i * A.nn;
            o.m[i] = kmah ? (int)kmah[q] : 0;
            p[i] = pt ? pt[q] : 0.0;
        }
    };
#pragma unroll
    for (int i = 0; i < K; i++) { S.T[i] = 0.0; S.A[i] = 0.0; S.H[i] = 0.0; S.m[i] = 0; Sp[i] = 0.0; }
#pragma unroll kUnroll
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform, as in k_migrate
            load_arr<K, AMP, BINS, false>(A, nullptr, (size_t)s * K * A.nn + x, S);
            load_gates((size_t)s * K * A.nn + x, S, Sp);
            sprev = s;
        }
        Arr<K> R;
        double Rp[K];
        load_arr<K, AMP, BINS, false>(A, nullptr, (size_t)r * K * A.nn + x, R);
        load_gates((size_t)r * K * A.nn + x, R, Rp);
#pragma unroll
        for (int i = 0; i < KK; i++) {
            const int ks = i / K, kr = i % K;
            const Pair p = pair_of<AMP, BINS>(A, S.T[ks], R.T[kr], S.A[ks], R.A[kr], S.H[ks], R.H[kr], wk);
            const bool ok = p.ok && (S.m[ks] | R.m[kr]) >= 0 && fabs(Sp[ks]) < INFINITY && fabs(Rp[kr]) < INFINITY;
            const double om = 1.0 - p.a;
            const double v = (p.c * p.c) * (om * om + p.a * p.a);
            if (BINS) {
                if (ok) acc[p.b * BS + tid] += v;
            } else {
                sum += ok ? v : 0.0;
            }
            cnt += (ok && in) ? 1ull : 0ull;
        }
    }
    if (in) {
        if (BINS)
            for (int b = 0; b < A.nb; b++) illum[(size_t)b * A.nn + x] = acc[b * BS + tid];
        else
            illum[x] = sum;
    }
    block_count_to(counts, blockIdx.x, cnt);
}

template <int K> void launch_illumination(bool amp, bool bins, dim3 grid, dim3 blk, size_t lds, const KArgs& A, const int8_t* kmah,
                                          const double* pt, double* illum, unsigned long long* counts) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, blk, lds, nullptr, A, kmah, pt, illum, counts); };
    if (amp) { if (bins) go(k_illumination<K, true, true>); else go(k_illumination<K, true, false>); }
    else     { if (bins) go(k_illumination<K, false, true>); else go(k_illumination<K, false, false>); }
}

// ------------------------------------------------------------------------------------------------------------ L
// One block per trace; data0, data1 [N][nt] (data1 is written only with PHASE); AA: data0 is the spreads [nlev][channels][N][nt];
// counts [N].  Sample i's accumulator is (lo[i], hi[i]) of rt_fix128.h; accumulator q = level * channels + channel has
// lo = fix + 2 q W, hi = lo + W.  The trace is processed in windows of W samples, at most kWindow over the accumulators: more
// accumulators shrink the window, and two channels double a block's LDS, which halves the blocks a CU holds: the host launches 512
// lanes with PHASE, so that the waves per CU stay what they were (any block size gives the same bits).
template <int K, bool AMP, bool BINS, bool PHASE, bool AA>
__global__ void __launch_bounds__(512) k_model(KArgs A, const int8_t* __restrict__ kmah, const double* __restrict__ m, int e, int W,
                                               double* __restrict__ data0, double* __restrict__ data1,
                                               unsigned long long* __restrict__ counts, AAOf<AA> Q) {
    extern __shared__ unsigned long long fix[];               // [nlev (AA)][channels][lo | hi][W]
    constexpr int KK = K * K;
    constexpr int kChannels = PHASE ? 2 : 1;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const int nacc = [&] { if constexpr (AA) return Q.nlev * kChannels; else return kChannels; }();
    const long k = blockIdx.x;
    const int s = A.isrc[k], r = A.irec[k];
    const double wk = A.w[k];
    unsigned long long cnt = 0;
    for (long j0 = 0; j0 < A.nt; j0 += W) {
        const long j1 = (j0 + W < A.nt) ? j0 + W : A.nt;      // the window [j0, j1)
        for (int i = tid; i < 2 * nacc * W; i += BS) fix[i] = ((i / W) & 1) ? 0ull : rt::kFixBias;
        __syncthreads();
        for (long x = tid; x < A.nn; x += BS) {
            Arr<K> S, R;
            double Sp[K], Rp[K];
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)s * K * A.nn + x, S);
            load_arr<K, AMP, BINS, PHASE>(A, kmah, (size_t)r * K * A.nn + x, R);
            load_pt<K>(Q, A.nn, (size_t)s * K * A.nn + x, Sp);
            load_pt<K>(Q, A.nn, (size_t)r * K * A.nn + x, Rp);
            const double mx = BINS ? 0.0 : m[x];
#pragma unroll
            for (int i = 0; i < KK; i++) {
                const int ks = i / K, kr = i % K;
                Pair p = pair_of<AMP, BINS>(A, S.T[ks], R.T[kr], S.A[ks], R.A[kr], S.H[ks], R.H[kr], wk);
                if constexpr (AA) p.ok = p.ok && fabs(Sp[ks]) < INFINITY && fabs(Rp[kr]) < INFINITY;
                Phase ph{true, false, false};
                if (PHASE) ph = phase_of(S.m[ks], R.m[kr]);
                if (!(p.ok && ph.valid)) continue;
                if (j0 == 0) cnt++;
                if (p.j + 1 < j0 || p.j >= j1) continue;
                const double cm = p.c * (BINS ? m[(size_t)p.b * A.nn + x] : mx);
                if (!(fabs(cm) < INFINITY)) continue;         // a non-finite model value contributes nothing
                const double u0 = cm * (1.0 - p.a), u1 = cm * p.a;
                const double v0 = ph.neg ? -u0 : u0, v1 = ph.neg ? -u1 : u1;
                unsigned long long* lo;
                if constexpr (AA) {
                    const int q = (int)level_of(Q, A.inv_dt, Sp[ks], Rp[kr]) * kChannels + (ph.odd ? 1 : 0);
                    lo = fix + (size_t)2 * q * W;
                } else {
                    lo = fix + (ph.odd ? 2 * W : 0);
                }
                unsigned long long* hi = lo + W;
                if (p.j >= j0) (void)rt::add128(lo, hi, (int)(p.j - j0), (long long)rint(ldexp(v0, -e)));
                if (p.j + 1 < j1) (void)rt::add128(lo, hi, (int)(p.j + 1 - j0), (long long)rint(ldexp(v1, -e)));
            }
        }
        __syncthreads();
        if constexpr (AA) {                                   // each window's spreads, one rounding each
            for (int q = 0; q < nacc; q++) {
                const unsigned long long* lo = fix + (size_t)2 * q * W;
                double* out = data0 + (size_t)q * Q.cstride + (size_t)k * A.nt + j0;
                for (long i = tid; i < j1 - j0; i += BS) out[i] = ldexp(rt::fix_to_double(lo[i], lo[W + i]), e);
            }
        } else {
            for (long i = tid; i < j1 - j0; i += BS) {
                data0[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(fix[i], fix[W + i]), e);
                if (PHASE) data1[(size_t)k * A.nt + j0 + i] = ldexp(rt::fix_to_double(fix[2 * W + i], fix[3 * W + i]), e);
            }
        }
        __syncthreads();
    }
    block_count_to(counts, k, cnt);
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

// One launch of either kernel.  migrate: in0, in1 the channels (AA: in0 the bank), out0 the image; model: in0 the model, out0, out1
// the channels (AA: out0 the spreads).
struct PairLaunch {
    dim3 grid, blk;
    size_t lds;
    KArgs A;
    AAArgs Q;
    const int8_t* kmah;
    const double *in0, *in1;
    double *out0, *out1;
    int e, W;
    unsigned long long* counts;
};
// The kernel of (model, aa, amp, bins, phase) and K: the flags become template arguments one at a time.
template <int K, bool... F>
void launch_pair(const bool* f, const PairLaunch& L) {
    if constexpr (sizeof...(F) == 5) {
        constexpr bool v[5] = {F...};
        if constexpr (v[0])
            hipLaunchKernelGGL((k_model<K, v[2], v[3], v[4], v[1]>), L.grid, L.blk, L.lds, nullptr, L.A, L.kmah, L.in0, L.e, L.W, L.out0, L.out1,
                               L.counts, AAOf<v[1]>(L.Q));
        else
            hipLaunchKernelGGL((k_migrate<K, v[2], v[3], v[4], v[1]>), L.grid, L.blk, L.lds, nullptr, L.A, L.kmah, L.in0, L.in1, L.out0, L.counts,
                               AAOf<v[1]>(L.Q));
    } else {
        if (*f) launch_pair<K, F..., true>(f + 1, L);
        else launch_pair<K, F..., false>(f + 1, L);
    }
}
// karr = 0, a handle of rtmi_kirchhoff_create: its tables [P][nn] are [P][1][nn]
void launch_pair(int karr, bool model, bool aa, bool amp, bool bins, bool phase, const PairLaunch& L) {
    const bool f[5] = {model, aa, amp, bins, phase};
    switch (karr) {
        case 0:
        case 1: launch_pair<1>(f, L); break;
        case 2: launch_pair<2>(f, L); break;
        case 3: launch_pair<3>(f, L); break;
        default: launch_pair<4>(f, L); break;
    }
}

int64_t to_ns(double ms) { return (int64_t)std::llround(ms * 1e6); }

// The one bracket of a launch, for both kernels and every kind of handle: the caller has set L's grid, block, LDS and pointers.
// On an anti-aliased handle of more than one level the bank's filter runs before migrate's kernel and the sum over the levels after
// model's; kernel_ms covers both and reserved[0] is that part of it in nanoseconds.
int run_pair(rtmi_kirchhoff* k, const char* who, bool model, PairLaunch& L, rtmi_kirchhoff_stats* st, bool counts) {
    const bool aa = k->nlev > 0, sweep = k->nlev > 1;
    L.A = k->args();
    if (aa) L.Q = k->aa_args();
    L.kmah = k->kmah;
    L.counts = k->counts;
    EventMarks<4> ev;
    RTMI_HIP(ev.create());
    RTMI_HIP(ev.mark(0));
    if (sweep && !model) RTMI_RC(rtmi_internal_kirchhoff_aa_sweep(k, who, false));
    RTMI_HIP(ev.mark(1));
    launch_pair(k->karr, model, aa, k->amp != nullptr, k->kp.nbin > 0, k->kmah != nullptr, L);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(2));
    if (sweep && model) RTMI_RC(rtmi_internal_kirchhoff_aa_sweep(k, who, true));
    RTMI_HIP(ev.mark(3));
    RTMI_HIP(ev.wait(3));
    if (st) {
        const int kk = k->karr ? k->karr * k->karr : 1;
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(aa && !model ? 0 : 1, aa && model ? 3 : 2, &st->kernel_ms));
        if (aa) {
            double aux_ms = 0.0;
            RTMI_HIP(model ? ev.ms(2, 3, &aux_ms) : ev.ms(0, 1, &aux_ms));
            st->reserved[0] = to_ns(aux_ms);
        }
        st->pairs = (int64_t)((size_t)k->kp.N * k->nn) * kk;
        st->scale_exp = L.e;
        if (counts) RTMI_RC(read_counts(k, L.grid.x, &st->contributing, who));
    }
    return RTMI_OK;
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

// On an anti-aliased handle, level 0 of `data` is where the bank's filter reads the caller's channels and the sum over the levels
// leaves the traces: device pointers other than the handle's own staging are copied to and from it on the device.
int rtmi_internal_kirchhoff_migrate_dev(rtmi_kirchhoff* k, const char* who, const double* d0, const double* d1, double* d_image,
                                        rtmi_kirchhoff_stats* st, bool counts) {
    const size_t per = (size_t)k->kp.N * (size_t)k->kp.nt;
    const bool phase = k->kmah != nullptr, aa = k->nlev > 0;
    if (aa && d0 != k->data) RTMI_HIP(hipMemcpyAsync(k->data, d0, per * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    if (aa && phase && d1 != k->data + per) RTMI_HIP(hipMemcpyAsync(k->data + per, d1, per * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    const int BS = migrate_block(k->nb);
    PairLaunch L{};
    L.grid = dim3((unsigned)((k->nn + BS - 1) / BS));
    L.blk = dim3(BS);
    L.lds = k->kp.nbin > 0 ? (size_t)k->nb * BS * sizeof(double) : 0;
    L.in0 = aa ? k->data : d0;
    L.in1 = phase && !aa ? d1 : nullptr;
    L.out0 = d_image;
    return run_pair(k, who, false, L, st, counts);
}

int rtmi_internal_kirchhoff_model_dev(rtmi_kirchhoff* k, const char* who, const double* d_model, double* d0, double* d1,
                                      rtmi_kirchhoff_stats* st, bool counts) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nm = (size_t)k->nb * k->nn;
    const bool phase = k->kmah != nullptr, aa = k->nlev > 0;
    // the quantum: one bound on one contribution for every kind of handle (DESIGN.md 19 on the number of contributions)
    double max_m = 0.0;
    RTMI_RC(rtmi_internal_absmax_finite(who, k->red, k->cus, d_model, nm, &max_m));
    const size_t nacc = (size_t)(aa ? k->nlev : 1) * (phase ? 2 : 1);     // every level and channel shares the 64 KiB
    const size_t window = (size_t)kWindow / nacc;
    PairLaunch L{};
    L.W = (int)(nt < window ? nt : window);
    L.e = model_exponent(k, max_m);
    L.grid = dim3((unsigned)N);
    L.blk = dim3(phase ? 512 : 256);
    L.lds = (size_t)L.W * 2 * nacc * sizeof(unsigned long long);
    L.in0 = d_model;
    L.out0 = aa ? k->data : d0;
    L.out1 = phase && !aa ? d1 : nullptr;
    RTMI_RC(run_pair(k, who, true, L, st, counts));
    if (aa && d0 != k->data) RTMI_HIP(hipMemcpy(d0, k->data, N * nt * sizeof(double), hipMemcpyDeviceToDevice));
    if (aa && phase && d1 != k->data + N * nt) RTMI_HIP(hipMemcpy(d1, k->data + N * nt, N * nt * sizeof(double), hipMemcpyDeviceToDevice));
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

// ------------------------------------------------------------------------------------------------------------ illumination
namespace {

// the kernel into d_illum [nb][nn], memory of the handle's device; st may be NULL
int illumination_dev(rtmi_kirchhoff* k, const char* who, double* d_illum, rtmi_kirchhoff_stats* st) {
    const int BS = migrate_block(k->nb);
    const dim3 grid((unsigned)((k->nn + BS - 1) / BS)), blk(BS);
    const bool amp = k->amp != nullptr, bins = k->kp.nbin > 0;
    const size_t lds = bins ? (size_t)k->nb * BS * sizeof(double) : 0;
    const KArgs A = k->args();
    EventMarks<2> ev;
    RTMI_HIP(ev.create());
    RTMI_HIP(ev.mark(0));
    switch (k->karr) {
        case 0:
        case 1: launch_illumination<1>(amp, bins, grid, blk, lds, A, k->kmah, k->pt, d_illum, k->counts); break;
        case 2: launch_illumination<2>(amp, bins, grid, blk, lds, A, k->kmah, k->pt, d_illum, k->counts); break;
        case 3: launch_illumination<3>(amp, bins, grid, blk, lds, A, k->kmah, k->pt, d_illum, k->counts); break;
        default: launch_illumination<4>(amp, bins, grid, blk, lds, A, k->kmah, k->pt, d_illum, k->counts); break;
    }
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    RTMI_HIP(ev.wait(1));
    if (st) {
        *st = rtmi_kirchhoff_stats{};
        RTMI_HIP(ev.ms(0, 1, &st->kernel_ms));
        st->pairs = (int64_t)((size_t)k->kp.N * k->nn) * (k->karr ? k->karr * k->karr : 1);
        RTMI_RC(read_counts(k, grid.x, &st->contributing, who));
    }
    return RTMI_OK;
}

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_illumination_dev(rtmi_kirchhoff* k, double* d_illum, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_illumination_dev";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(d_illum, "null d_illum");
    RTMI_RC(check_device(k, who));
    RTMI_RC(check_device_pointer(k, who, d_illum, (size_t)k->nb * k->nn * sizeof(double), "d_illum"));
    return illumination_dev(k, who, d_illum, st);
}

RTMI_EXPORT int rtmi_kirchhoff_illumination(rtmi_kirchhoff* k, double* illum, rtmi_kirchhoff_stats* st) {
    const char* who = "rtmi_kirchhoff_illumination";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(illum, "null illum");
    RTMI_RC(check_device(k, who));
    RTMI_RC(illumination_dev(k, who, k->image, st));
    RTMI_HIP(hipMemcpy(illum, k->image, (size_t)k->nb * k->nn * sizeof(double), hipMemcpyDeviceToHost));
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
