// kirchhoff_aa.hip -- what a Kirchhoff handle anti-aliased by operator slope adds to the pair (rtmi_kirchhoff_create_aa /
// rtmi_kirchhoff_aa_filter): a bank of triangle-filtered copies of the traces, of which the pair kernels choose one per (trace,
// node) pair by the slope of the summation curve across neighbouring traces.  include/rtmi.h states the operator; DESIGN.md section
// 20 the kernels, the memory and what was measured.
//   k_aa_filter   one lane per output sample, j fastest: level l's copy of every trace, the 2 hw[l] + 1 taps in the defined order.
//   k_aa_gather   one lane per sample: ch = S_0 + sum over l >= 1 of F_hw[l] S_l, l ascending, in place over level 0.
// The handle's one buffer `data` [nlev][channels][N][nt] is the bank in migrate2 and the spreads in model2.  The pair kernels and
// their launch path are kirchhoff.hip's, which calls rtmi_internal_kirchhoff_aa_sweep for the filter before migrate and the sum
// after model.
#include "rt_kirchhoff.h"

namespace {

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

Taps taps_of(const rtmi_kirchhoff* k) {
    Taps F{};
    for (int l = 1; l < k->nlev; l++) {
        const double n = (double)(k->hw[l] + 1);
        F.hw[l - 1] = k->hw[l];
        F.inv[l - 1] = 1.0 / (n * n);
    }
    return F;
}

// one lane per sample, at most 2^20 blocks (the kernels stride over the rest)
dim3 sample_blocks(size_t per, int levels) {
    const size_t b = (per + 255) / 256;
    return dim3((unsigned)(b < (1u << 20) ? b : (1u << 20)), (unsigned)levels);
}

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
    const AAArgs Q = k->aa_args();
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

int rtmi_internal_kirchhoff_aa_sweep(rtmi_kirchhoff* k, const char* who, bool gather) {
    const long per = k->aa_args().lstride, nt = (long)k->kp.nt;            // every channel of one level
    if (gather) hipLaunchKernelGGL(k_aa_gather, sample_blocks((size_t)per, 1), dim3(256), 0, nullptr, k->data, per, per, nt, k->nlev, taps_of(k));
    else hipLaunchKernelGGL(k_aa_filter, sample_blocks((size_t)per, k->nlev - 1), dim3(256), 0, nullptr, k->data, per, per, nt, taps_of(k));
    RTMI_HIP(hipGetLastError());
    return RTMI_OK;
}
