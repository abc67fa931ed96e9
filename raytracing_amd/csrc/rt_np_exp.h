// rt_np_exp.h -- the main path of numpy's array exp on float64 (Intel SVML's __svml_exp8_ha, numpy/_core/src/umath/svml, BSD-3),
// one text for the host and the device: field.hip's np_exp evaluates a scenario with it (and keeps the fall-back for large
// arguments to itself), rt_edt.h's kernel of a station pair is it on [-700, 0], and rtmi_edt_exp hands it out on the host, so that
// a numpy restatement needs no fma of its own.  No HIP in it.
//
// |x| < 0x1.61da04cbafe44p+9 (707.7):  N = floor(x * log2(e) * 16) / 16 -- the floor of the exact product, an fma away from the
// rounded one -- r = x - N ln2 in two pieces, a degree-6 polynomial in three interleaved pairs, 2^(j/16) from a 16-entry table
// with its correction term, scaled by 2^floor(N).  Every fma below is one; build with -ffp-contract=off so that nothing else is.
// The tables are passed in, 32 doubles (2^(j/16) rounded, then its rounding error): a kernel that calls this per lane may keep
// them where its lanes read them best.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_NP_EXP_HD __host__ __device__ __forceinline__
#else
#define RT_NP_EXP_HD inline
#endif

namespace rt {

constexpr int kExpTableLen = 32;

// entry i of the tables: 2^(i/16) for i < 16, its correction term for 16 <= i < 32
RT_NP_EXP_HD const double* np_exp_tables() {
    static const double tab[kExpTableLen] = {0x1.0000000000000p+0, 0x1.0b5586cf9890fp+0, 0x1.172b83c7d517bp+0, 0x1.2387a6e756238p+0,
        0x1.306fe0a31b715p+0, 0x1.3dea64c123422p+0, 0x1.4bfdad5362a27p+0, 0x1.5ab07dd485429p+0, 0x1.6a09e667f3bcdp+0,
        0x1.7a11473eb0187p+0, 0x1.8ace5422aa0dbp+0, 0x1.9c49182a3f090p+0, 0x1.ae89f995ad3adp+0, 0x1.c199bdd85529cp+0,
        0x1.d5818dcfba487p+0, 0x1.ea4afa2a490dap+0,
        0x0.0p+0, 0x1.79aa65d837b6dp-54, -0x1.01b15eaa59348p-55, 0x1.68efde3a8a894p-54,
        0x1.34d754db0abb6p-55, 0x1.59f48a72a4c6dp-55, 0x1.690cebb7aafb0p-56, 0x1.063e1e21c5409p-54, -0x1.3b3efbf5e2228p-54,
        -0x1.b32dcb94da51dp-56, 0x1.db72fc1f0eab4p-55, 0x1.1affc2b91ce27p-56, 0x1.c1a7792cb3387p-55, 0x1.36eae30af0cb3p-56,
        0x1.4a385a63d07a7p-56, -0x1.ff7128fd391f0p-55};
    return tab;
}

// x with |x| < 707.7 (the caller's to see to); tab: the 32 entries above, wherever they are kept
RT_NP_EXP_HD double np_exp_main(double x, const double* tab) {
    const double L2E = 0x1.71547652b82fep+0, LN2H = 0x1.62e42fefa39efp-1, LN2L = 0x1.abc9e3b39803fp-56;
    const double A = 0x1.7411836940c04p-10, B = 0x1.1101cbbc265c0p-7, C = 0x1.55557242d68fep-5, D = 0x1.5555553939732p-3,
                 E = 0x1.000000000d008p-1, F = 0x1.fffffffffff70p-1;
    // floor of the EXACT product x*L2E on the 1/16 grid (== the toward-zero fma onto the shifter 1.5*2^48 + 1023)
    const double p = x * L2E, e = __builtin_fma(x, L2E, -p);
    double f16 = floor(p * 16.0);
    if (f16 == p * 16.0 && e < 0) f16 -= 1.0;
    const double N = f16 * 0.0625;
    const int j = (int)((long long)f16 & 15);
    double r = __builtin_fma(-N, LN2H, x);
    r = __builtin_fma(-N, LN2L, r);
    const double r2 = r * r;
    const double P1 = __builtin_fma(A, r, B), P2 = __builtin_fma(C, r, D), P3 = __builtin_fma(E, r, F);
    double q = __builtin_fma(r2, P1, P2);
    q = __builtin_fma(r2, q, P3);
    double t = __builtin_fma(q, r, tab[16 + j]);
    t = __builtin_fma(tab[j], t, tab[j]);
    return ldexp(t, (int)floor(N));
}

}  // namespace rt
