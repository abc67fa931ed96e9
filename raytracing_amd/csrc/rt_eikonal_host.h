// rt_eikonal_host.h -- what the host sides of eikonal.hip and eikonal_lin.hip share: the way out of an entry on a failed
// allocation, the argument checks of rtmi_eikonal_params, the size of a block and a block's sum.  After rtmi_host.h; in an anonymous namespace, as that header is.
#pragma once

#define RTMI_ALLOC(expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            (void)hipGetLastError();                                                                              \
            return rtmi_internal_fail(RTMI_ERR_ALLOC, (std::string(who) + ": " + #expr + ": " + hipGetErrorString(e_)).c_str()); \
        }                                                                                                         \
    } while (0)

namespace {

constexpr int kMaxBlock = 256;                          // lanes of a block: one wave per SIMD; a barrier costs more with more waves

// the block's sum of v, the same in every lane; `slot` alternates between two calls in a row
__device__ __forceinline__ unsigned long long block_sum(unsigned long long (*red)[kMaxBlock / 64], int slot, unsigned long long v) {
    for (int off = 1; off < 64; off <<= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    const int tid = (int)threadIdx.x, waves = (int)(blockDim.x >> 6);
    if ((tid & 63) == 0) red[slot][tid >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int k = 0; k < waves; k++) s += red[slot][k];
    return s;
}

// what every form of the call refuses before it touches the device
int check_eikonal(const char* who, const rtmi_eikonal_params* ep, const void* n, int64_t S, const void* src, const void* n_src) {
    RTMI_ARG(ep, "null ep");
    RTMI_ARG(ep->nx >= 1 && ep->ny >= 1, "nx and ny must be >= 1");
    RTMI_ARG((double)ep->nx * (double)ep->ny <= (double)(1L << 31), "more than 2^31 nodes per source");
    RTMI_ARG(ep->gdx > 0.0 && ep->gdy > 0.0 && std::isfinite(ep->gdx) && std::isfinite(ep->gdy), "gdx and gdy must be finite and > 0");
    RTMI_ARG(std::isfinite(ep->gx0) && std::isfinite(ep->gy0), "gx0 and gy0 must be finite");
    RTMI_ARG(S >= 0, "S must be >= 0");
    RTMI_ARG(S == 0 || n, "null n");
    RTMI_ARG(S == 0 || src, "null src");
    RTMI_ARG(S == 0 || n_src, "null n_src");
    RTMI_ARG(ep->max_rounds >= 0, "max_rounds must be >= 0");
    RTMI_ARG(std::isfinite(ep->ball), "ball must be finite");
    RTMI_ARG(ep->reserved[0] == 0 || ep->reserved[0] == 1, "reserved[0] must be 0 or 1");
    return RTMI_OK;
}

// what the fills, which read ep->scheme as a scheme of theirs, refuse on top of that
int check_eikonal_scheme(const char* who, const rtmi_eikonal_params* ep) {
    RTMI_ARG(ep->scheme == RTMI_EIKONAL_PLAIN || ep->scheme == RTMI_EIKONAL_FACTORED || ep->scheme == RTMI_EIKONAL_FACTORED_LIN,
             "scheme must be RTMI_EIKONAL_PLAIN, RTMI_EIKONAL_FACTORED or RTMI_EIKONAL_FACTORED_LIN");
    return RTMI_OK;
}

// the fill's scheme: RTMI_EIKONAL_FACTORED_LIN fills as RTMI_EIKONAL_FACTORED does
bool eikonal_fills_factored(const rtmi_eikonal_params* ep) {
    return ep->scheme == RTMI_EIKONAL_FACTORED || ep->scheme == RTMI_EIKONAL_FACTORED_LIN;
}

}  // namespace
