// kirchhoff_aa.hip -- the Kirchhoff pair anti-aliased by operator slope (rtmi_kirchhoff_create_aa / rtmi_kirchhoff_aa_filter, and
// rtmi_kirchhoff_migrate2 / _model2 on such a handle): a bank of triangle-filtered copies of the traces, and per (trace, node)
// pair the choice of one of them by the slope of the summation curve across neighbouring traces.  include/rtmi.h states the
// operator; DESIGN.md section 20 the kernels, the memory and what was measured.
//   k_aa_filter   one lane per output sample, j fastest: level l's copy of every trace, the 2 hw[l] + 1 taps in the defined order.
//   k_migrate_aa  k_migrate_multi (kirchhoff.hip) with one more table value per slot, pt, and the level select: at most 7
//                 compares against wave-uniform thresholds; the level and the channel move the gather's base address by selects
//                 and a multiply, never by a branch, and all K^2 gathers are issued before the first add.
//   k_model_aa    k_model_multi with accumulators [level][channel][lo|hi][W] in LDS; each window's spreads go to the handle's
//                 [nlev][channels][N][nt] buffer, one rounding each.
//   k_aa_gather   one lane per sample: ch = S_0 + sum over l >= 1 of F_hw[l] S_l, l ascending, in place over level 0.
// The handle's one buffer `data` [nlev][channels][N][nt] is the bank in migrate2 and the spreads in model2.  One launch path, on
// device pointers (kirchhoff.hip's rtmi_internal_kirchhoff_migrate_dev / _model_dev lead here).
#include "rt_kirchhoff.h"

namespace {

constexpr int kMaxLev = RTMI_KIRCHHOFF_MAX_LEVELS;

// Levels 1 .. nlev - 1 of the bank: entry l - 1.
struct Taps { int hw[kMaxLev - 1]; double inv[kMaxLev - 1]; };

// (F_k x)[j] of one trace x of nt samples: i ascending from 0.0, every product and add a separate fp64 operation
__device__ __forceinline__ double tri_at(const double* __restrict__ x, long j, long nt, int k, double inv) {
    const long lo = j < (long)k ? -j : -(long)k;
    const long hi = nt - 1 - j < (long)k ? nt - 1 - j : (long)k;
    double sum = 0.0;
    for (long i = lo; i <= hi; i++) {
        const long ai = i < 0 ? -i : i;
        sum = sum + (double)((long)k + 1 - ai) * x[j + i];
    }
    return sum * inv;
}

// buf [nlev][per], per = rows nt: level blockIdx.y + 1 of the first `per` samples from level 0.
__global__ void __launch_bounds__(256) k_aa_filter(double* buf, long per, long lstride, long nt, Taps F) {
    const int l = (int)blockIdx.y;
    const int k = F.hw[l];
    const double inv = F.inv[l];
    const double* src = buf;
    double* dst = buf + (size_t)(l + 1) * lstride;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const long j = i % nt;
        dst[i] = tri_at(src + (i - j), j, nt, k, inv);
    }
}

// buf [nlev][per]: level 0 becomes S_0 + sum over l of F_hw[l] S_l, l ascending.  A lane reads level 0 at its own sample only.
__global__ void __launch_bounds__(256) k_aa_gather(double* buf, long per, long lstride, long nt, int nlev, Taps F) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const long j = i % nt;
        double acc = buf[i];
        for (int l = 1; l < nlev; l++) acc = acc + tri_at(buf + (size_t)l * lstride + (i - j), j, nt, F.hw[l - 1], F.inv[l - 1]);
        buf[i] = acc;
    }
}

struct AAArgs {
    const double* pt;              // [P][K][nn]
    double asrc, arec, amid;
    double thr[kMaxLev - 1];       // (double)hw[l] for l < nlev - 1, +inf from there on: the level is the number of thresholds below sl
    long lstride, cstride;         // doubles from one level to the next (channels N nt) and from channel 0 to channel 1 (N nt)
};

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

template <int K> __device__ __forceinline__ void load_pt(const AAArgs& Q, long nn, size_t at, double (&o)[K]) {
#pragma unroll
    for (int i = 0; i < K; i++) o[i] = Q.pt[at + (size_t)i * nn];
}

// L^T.  bank [nlev][channels][N][nt]; image [nb][nn]; counts [gridDim.x].  k_migrate_multi's loop and order.
template <int K, bool AMP, bool BINS, bool PHASE>
__global__ void __launch_bounds__(256) k_migrate_aa(KArgs A, AAArgs Q, const int8_t* __restrict__ kmah, const double* __restrict__ bank,
                                                    double* __restrict__ image, unsigned long long* __restrict__ counts) {
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
    double Sp[K];
#pragma unroll
    for (int i = 0; i < K; i++) { S.T[i] = 0.0; S.A[i] = 0.0; S.H[i] = 0.0; S.m[i] = 0; Sp[i] = 0.0; }
#pragma unroll kUnroll
    for (long k = 0; k < A.N; k++) {
        const int s = A.isrc[k], r = A.irec[k];
        const double wk = A.w[k];
        if (s != sprev) {                                     // wave-uniform, as in k_migrate
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
            p[i].ok = p[i].ok && fabs(Sp[ks]) < INFINITY && fabs(Rp[kr]) < INFINITY;
            size_t at = (size_t)level_of(Q, A.inv_dt, Sp[ks], Rp[kr]) * (size_t)Q.lstride;
            neg[i] = false;
            if (PHASE) {
                const Phase ph = phase_of(S.m[ks], R.m[kr]);
                p[i].ok = p[i].ok && ph.valid;
                neg[i] = ph.neg;
                at += ph.odd ? (size_t)Q.cstride : 0;
            }
            const double* d = bank + at + (size_t)k * A.nt + p[i].j;    // j = 0 when the range test failed: always in bounds
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

// L.  One block per trace; spread [nlev][channels][N][nt]; counts [N].  Accumulator q = level * channels + channel has
// lo = fix + 2 q W, hi = lo + W; windows of W samples as in k_model_multi.
template <int K, bool AMP, bool BINS, bool PHASE>
__global__ void __launch_bounds__(512) k_model_aa(KArgs A, AAArgs Q, const int8_t* __restrict__ kmah, const double* __restrict__ m, int e,
                                                  int W, int nlev, double* __restrict__ spread, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned long long fix[];               // [nlev][channels][lo | hi][W]
    __shared__ unsigned long long wcnt[8];
    constexpr int KK = K * K;
    constexpr int kChannels = PHASE ? 2 : 1;
    const int tid = (int)threadIdx.x, BS = (int)blockDim.x;
    const int nacc = nlev * kChannels;
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
                p.ok = p.ok && fabs(Sp[ks]) < INFINITY && fabs(Rp[kr]) < INFINITY;
                Phase ph{true, false, false};
                if (PHASE) ph = phase_of(S.m[ks], R.m[kr]);
                if (!(p.ok && ph.valid)) continue;
                if (j0 == 0) cnt++;
                if (p.j + 1 < j0 || p.j >= j1) continue;
                const double cm = p.c * (BINS ? m[(size_t)p.b * A.nn + x] : mx);
                if (!(fabs(cm) < INFINITY)) continue;         // a non-finite model value contributes nothing
                const double u0 = cm * (1.0 - p.a), u1 = cm * p.a;
                const double v0 = ph.neg ? -u0 : u0, v1 = ph.neg ? -u1 : u1;
                const int q = (int)level_of(Q, A.inv_dt, Sp[ks], Rp[kr]) * kChannels + (ph.odd ? 1 : 0);
                unsigned long long* lo = fix + (size_t)2 * q * W;
                unsigned long long* hi = lo + W;
                if (p.j >= j0) (void)rt::add128(lo, hi, (int)(p.j - j0), (long long)rint(ldexp(v0, -e)));
                if (p.j + 1 < j1) (void)rt::add128(lo, hi, (int)(p.j + 1 - j0), (long long)rint(ldexp(v1, -e)));
            }
        }
        __syncthreads();
        for (int q = 0; q < nacc; q++) {
            const unsigned long long* lo = fix + (size_t)2 * q * W;
            double* out = spread + (size_t)q * Q.cstride + (size_t)k * A.nt + j0;
            for (long i = tid; i < j1 - j0; i += BS) out[i] = ldexp(rt::fix_to_double(lo[i], lo[W + i]), e);
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

// The kernel of (karr, amp, bins, phase): the flags become template arguments one at a time.
struct AALaunch {
    dim3 grid, blk;
    size_t lds;
    KArgs A;
    AAArgs Q;
    const int8_t* kmah;
    const double* model;    // model: the model
    double* buf;            // migrate: the bank; model: the spreads
    double* image;          // migrate
    int e, W, nlev;
    unsigned long long* counts;
};
template <bool MODEL, int K, bool... F>
void launch_aa(const bool* f, const AALaunch& L) {
    if constexpr (sizeof...(F) == 3) {
        if constexpr (MODEL)
            hipLaunchKernelGGL((k_model_aa<K, F...>), L.grid, L.blk, L.lds, nullptr, L.A, L.Q, L.kmah, L.model, L.e, L.W, L.nlev, L.buf, L.counts);
        else
            hipLaunchKernelGGL((k_migrate_aa<K, F...>), L.grid, L.blk, L.lds, nullptr, L.A, L.Q, L.kmah, L.buf, L.image, L.counts);
    } else {
        if (*f) launch_aa<MODEL, K, F..., true>(f + 1, L);
        else launch_aa<MODEL, K, F..., false>(f + 1, L);
    }
}
template <bool MODEL>
void launch_aa(int karr, bool amp, bool bins, bool phase, const AALaunch& L) {
    const bool f[3] = {amp, bins, phase};
    switch (karr) {
        case 1: launch_aa<MODEL, 1>(f, L); break;
        case 2: launch_aa<MODEL, 2>(f, L); break;
        case 3: launch_aa<MODEL, 3>(f, L); break;
        default: launch_aa<MODEL, 4>(f, L); break;
    }
}

size_t channels(const rtmi_kirchhoff* k) { return k->kmah ? 2 : 1; }

Taps taps_of(const rtmi_kirchhoff* k) {
    Taps F{};
    for (int l = 1; l < k->nlev; l++) {
        const double n = (double)(k->hw[l] + 1);
        F.hw[l - 1] = k->hw[l];
        F.inv[l - 1] = 1.0 / (n * n);
    }
    return F;
}

AAArgs aa_args(const rtmi_kirchhoff* k) {
    AAArgs Q{};
    Q.pt = k->pt;
    Q.asrc = k->asrc; Q.arec = k->arec; Q.amid = k->amid;
    for (int l = 0; l < kMaxLev - 1; l++) Q.thr[l] = l < k->nlev - 1 ? (double)k->hw[l] : INFINITY;
    Q.cstride = (long)((size_t)k->kp.N * (size_t)k->kp.nt);
    Q.lstride = (long)channels(k) * Q.cstride;
    return Q;
}

// one lane per sample, at most 2^20 blocks (the kernels stride over the rest)
dim3 sample_blocks(size_t per, int levels) {
    const size_t b = (per + 255) / 256;
    return dim3((unsigned)(b < (1u << 20) ? b : (1u << 20)), (unsigned)levels);
}

int64_t to_ns(double ms) { return (int64_t)std::llround(ms * 1e6); }

}  // namespace

RTMI_EXPORT int rtmi_kirchhoff_create_aa(const rtmi_kirchhoff_aa_params* ap, const double* T, const double* amp, const double* theta,
                                         const double* kmah, const double* pt, const int32_t* isrc, const int32_t* irec,
                                         const double* w, rtmi_kirchhoff** out) {
    const char* who = "rtmi_kirchhoff_create_aa";
    RTMI_ARG(out, "null out");
    *out = nullptr;
    RTMI_ARG(ap, "null kp");
    rtmi_kirchhoff_params kp{};
    RTMI_RC(multi_params(who, ap, &kp));
    return create_impl(who, &kp, ap->karr, T, amp, theta, kmah, isrc, irec, w, out, ap, pt);
}

RTMI_EXPORT int rtmi_kirchhoff_aa_filter(rtmi_kirchhoff* k, const double* data, double* bank) {
    const char* who = "rtmi_kirchhoff_aa_filter";
    RTMI_ARG(k, "null handle");
    RTMI_ARG(data, "null data");
    RTMI_ARG(bank, "null bank");
    RTMI_ARG(k->nlev >= 1, "the handle is not rtmi_kirchhoff_create_aa's");
    RTMI_RC(check_device(k, who));
    const size_t per = (size_t)k->kp.N * (size_t)k->kp.nt;
    const AAArgs Q = aa_args(k);
    std::memcpy(bank, data, per * sizeof(double));            // level 0: the trace as given
    if (k->nlev == 1) return RTMI_OK;
    RTMI_HIP(hipMemcpy(k->data, data, per * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_aa_filter, sample_blocks(per, k->nlev - 1), dim3(256), 0, nullptr, k->data, (long)per, Q.lstride, (long)k->kp.nt,
                       taps_of(k));
    RTMI_HIP(hipGetLastError());
    for (int l = 1; l < k->nlev; l++)
        RTMI_HIP(hipMemcpy(bank + (size_t)l * per, k->data + (size_t)l * Q.lstride, per * sizeof(double), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// The handle's level 0 is where k_aa_filter reads the caller's channels and k_aa_gather leaves the traces: device pointers other
// than the handle's own staging are copied to and from it on the device.
int rtmi_internal_kirchhoff_aa_migrate_dev(rtmi_kirchhoff* k, const char* who, const double* d0, const double* d1, double* d_image,
                                           rtmi_kirchhoff_stats* st, bool counts) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn;
    const bool phase = k->kmah != nullptr;
    if (d0 != k->data) RTMI_HIP(hipMemcpyAsync(k->data, d0, N * nt * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    if (phase && d1 != k->data + N * nt)
        RTMI_HIP(hipMemcpyAsync(k->data + N * nt, d1, N * nt * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
    EventMarks<3> ev;
    RTMI_HIP(ev.create());
    const int BS = migrate_block(k->nb);
    const bool bins = k->kp.nbin > 0;
    AALaunch L{};
    L.grid = dim3((unsigned)((nn + BS - 1) / BS));
    L.blk = dim3(BS);
    L.lds = bins ? (size_t)k->nb * BS * sizeof(double) : 0;
    L.A = k->args();
    L.Q = aa_args(k);
    L.kmah = k->kmah;
    L.buf = k->data;
    L.image = d_image;
    L.counts = k->counts;
    RTMI_HIP(ev.mark(0));
    if (k->nlev > 1)
        hipLaunchKernelGGL(k_aa_filter, sample_blocks((size_t)L.Q.lstride, k->nlev - 1), dim3(256), 0, nullptr, k->data, L.Q.lstride,
                           L.Q.lstride, (long)nt, taps_of(k));
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    launch_aa<false>(k->karr, k->amp != nullptr, bins, phase, L);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(2));
    RTMI_HIP(ev.wait(2));
    if (st) {
        *st = rtmi_kirchhoff_stats{};
        double filter_ms = 0.0;
        RTMI_HIP(ev.ms(0, 2, &st->kernel_ms));
        RTMI_HIP(ev.ms(0, 1, &filter_ms));
        st->reserved[0] = to_ns(filter_ms);
        st->pairs = (int64_t)(N * nn) * k->karr * k->karr;
        if (counts) RTMI_RC(read_counts(k, L.grid.x, &st->contributing, who));
    }
    return RTMI_OK;
}

int rtmi_internal_kirchhoff_aa_model_dev(rtmi_kirchhoff* k, const char* who, const double* d_model, int e, double* d0, double* d1,
                                         rtmi_kirchhoff_stats* st, bool counts) {
    const size_t N = (size_t)k->kp.N, nt = (size_t)k->kp.nt, nn = k->nn;
    const bool phase = k->kmah != nullptr;
    EventMarks<3> ev;
    RTMI_HIP(ev.create());
    const size_t window = (size_t)kWindow / ((size_t)k->nlev * channels(k));        // every level and channel shares the 64 KiB
    AALaunch L{};
    L.W = (int)(nt < window ? nt : window);
    L.e = e;
    L.nlev = k->nlev;
    L.grid = dim3((unsigned)N);
    L.blk = dim3(phase ? 512 : 256);
    L.lds = (size_t)L.W * 2 * (size_t)k->nlev * channels(k) * sizeof(unsigned long long);
    L.A = k->args();
    L.Q = aa_args(k);
    L.kmah = k->kmah;
    L.model = d_model;
    L.buf = k->data;
    L.counts = k->counts;
    RTMI_HIP(ev.mark(0));
    launch_aa<true>(k->karr, k->amp != nullptr, k->kp.nbin > 0, phase, L);
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(1));
    if (k->nlev > 1)
        hipLaunchKernelGGL(k_aa_gather, sample_blocks((size_t)L.Q.lstride, 1), dim3(256), 0, nullptr, k->data, L.Q.lstride, L.Q.lstride,
                           (long)nt, k->nlev, taps_of(k));
    RTMI_HIP(hipGetLastError());
    RTMI_HIP(ev.mark(2));
    RTMI_HIP(ev.wait(2));
    if (d0 != k->data) RTMI_HIP(hipMemcpy(d0, k->data, N * nt * sizeof(double), hipMemcpyDeviceToDevice));
    if (phase && d1 != k->data + N * nt) RTMI_HIP(hipMemcpy(d1, k->data + N * nt, N * nt * sizeof(double), hipMemcpyDeviceToDevice));
    if (st) {
        *st = rtmi_kirchhoff_stats{};
        double gather_ms = 0.0;
        RTMI_HIP(ev.ms(0, 2, &st->kernel_ms));
        RTMI_HIP(ev.ms(1, 2, &gather_ms));
        st->reserved[0] = to_ns(gather_ms);
        st->pairs = (int64_t)(N * nn) * k->karr * k->karr;
        st->scale_exp = e;
        if (counts) RTMI_RC(read_counts(k, N, &st->contributing, who));
    }
    return RTMI_OK;
}
