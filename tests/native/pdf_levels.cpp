// rt_pdf.h as a program of its own (tests/test_pdf_native.py builds it plain and with -fsanitize=address,undefined): the host
// finalisation of an event's integer sums, and the density, mass, bin and sample quantum of single values.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared; the integer
// sums are signed decimals of up to 128 bits:
//     final <Z> <rim> <nz> <Sx> <Sy> <Sxx> <Sxy> <Syy> <ix> <iy> <gx0> <gdx> <gy0> <gdy> <nlevels> <levels ...> <n> then n times <bin> <count> <mass>
//         -> "final <mean_x> <mean_y> <cxx> <cxy> <cyy> <a> <b> <azimuth> <area> <rim_fraction> <nz> <mass>" then per level
//            " <count> <area> <fraction> <rho>"
//     l2 <obj> <obj0> <sw> <sigma>  -> "l2 <rho> <mass>"         edt <value> <value0> <p>  -> "edt <rho> <mass>"
//     bin <m>  -> "bin <bin> <edge>"                              quantum <u> <Z>  -> "quantum <q>"
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

static unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {      // rt_fix128.h's add128 wants one: not called
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}

#include "../../raytracing_amd/csrc/rt_pdf.h"

static bool read_words(unsigned long long* w) {          // a signed decimal -> two's complement (lo, hi)
    char s[64];
    if (std::scanf("%63s", s) != 1) return false;
    const bool neg = s[0] == '-';
    unsigned __int128 v = 0;
    for (const char* c = s + (neg ? 1 : 0); *c; c++) {
        if (*c < '0' || *c > '9') return false;
        v = v * 10 + (unsigned)(*c - '0');
    }
    if (neg) v = ~v + 1;
    w[0] = (unsigned long long)v;
    w[1] = (unsigned long long)(v >> 64);
    return true;
}

int main() {
    (void)&atomicAdd;
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "final")) {
            rt::PdfSums s{};
            int ix = 0, iy = 0, nlevels = 0;
            long n = 0;
            rt::LocateGrid g{};
            double levels[rt::kPdfMaxLevels] = {};
            if (std::scanf("%llu %llu %llu", &s.Z, &s.rim, &s.nz) != 3) return 2;
            if (!read_words(s.Sx) || !read_words(s.Sy) || !read_words(s.Sxx) || !read_words(s.Sxy) || !read_words(s.Syy)) return 2;
            if (std::scanf("%d %d %la %la %la %la %d", &ix, &iy, &g.gx0, &g.gdx, &g.gy0, &g.gdy, &nlevels) != 7) return 2;
            if (nlevels < 0 || nlevels > rt::kPdfMaxLevels) return 2;
            for (int k = 0; k < nlevels; k++)
                if (std::scanf("%la", &levels[k]) != 1) return 2;
            if (std::scanf("%ld", &n) != 1 || n < 0 || n > rt::kPdfBins) return 2;
            std::vector<unsigned long long> count(rt::kPdfBins, 0ull), mass(rt::kPdfBins, 0ull);
            for (long i = 0; i < n; i++) {
                int bin = 0;
                unsigned long long c = 0, m = 0;
                if (std::scanf("%d %llu %llu", &bin, &c, &m) != 3 || bin < 0 || bin >= rt::kPdfBins) return 2;
                count[(size_t)bin] = c;
                mass[(size_t)bin] = m;
            }
            const rt::PdfStats o = rt::pdf_finalize(s, count.data(), mass.data(), ix, iy, g, nlevels, levels);
            std::printf("final %a %a %a %a %a %a %a %a %a %a %lld %lld", o.mean_x, o.mean_y, o.cov[0], o.cov[1], o.cov[2], o.ellipse[0],
                        o.ellipse[1], o.ellipse[2], o.area, o.rim_fraction, (long long)o.nz, (long long)o.mass);
            for (int k = 0; k < nlevels; k++)
                std::printf(" %lld %a %a %a", (long long)o.level_count[k], o.level_area[k], o.level_fraction[k], o.level_rho[k]);
            std::printf("\n");
        } else if (!std::strcmp(cmd, "l2")) {
            double obj = 0.0, obj0 = 0.0, sw = 0.0, sigma = 0.0;
            if (std::scanf("%la %la %la %la", &obj, &obj0, &sw, &sigma) != 4) return 2;
            const double rho = rt::pdf_rho_l2(obj, obj0, rt::pdf_l2_scale(sw, sigma), rt::np_exp_tables());
            std::printf("l2 %a %llu\n", rho, rt::pdf_mass(rho));
        } else if (!std::strcmp(cmd, "edt")) {
            double v = 0.0, v0 = 0.0;
            int p = 0;
            if (std::scanf("%la %la %d", &v, &v0, &p) != 3 || p < 1 || p > 4096) return 2;
            const double rho = rt::pdf_rho_edt(v, v0, p);
            std::printf("edt %a %llu\n", rho, rt::pdf_mass(rho));
        } else if (!std::strcmp(cmd, "bin")) {
            unsigned long long m = 0;
            if (std::scanf("%llu", &m) != 1 || m < 1) return 2;
            const int bin = rt::pdf_bin(m);
            std::printf("bin %d %llu\n", bin, rt::pdf_bin_edge(bin));
        } else if (!std::strcmp(cmd, "quantum")) {
            double u = 0.0;
            unsigned long long Z = 0;
            if (std::scanf("%la %llu", &u, &Z) != 2 || Z < 1) return 2;
            std::printf("quantum %llu\n", rt::pdf_sample_quantum(u, Z));
        } else {
            return 2;
        }
    }
    return 0;
}
