// Test helper (CPU, g++, a program of its own): raytracing_amd/csrc/rt_filter.h, the half-derivative taps of the device's trace
// filter and the definition of F and F^T as a host loop.  stdin: a count, then that many "L dt" (dt a hex float); a count, then
// that many cases "nt L origin", the L taps and the nt samples of one trace (hex floats).  stdout: per (L, dt) a line "taps" with
// the L half-derivative taps; per case a line "y" with F x and a line "yt" with F^T x, all as hex floats.
// tests/test_filter_ref.py builds it twice, plain and with -fsanitize=address,undefined, and compares every bit with the library's
// taps and with tests/filter_ref.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_amd/csrc/rt_filter.h"

static bool read_double(double* v) {
    char buf[128];
    if (std::scanf("%127s", buf) != 1) return false;
    *v = std::strtod(buf, nullptr);
    return true;
}

static void print_line(const char* tag, const std::vector<double>& v) {
    std::printf("%s", tag);
    for (double a : v) std::printf(" %a", a);
    std::printf("\n");
}

int main() {
    long count = 0;
    if (std::scanf("%ld", &count) != 1 || count < 0) return 2;
    for (long c = 0; c < count; c++) {
        long L = 0;
        double dt = 0.0;
        if (std::scanf("%ld", &L) != 1 || L < 1 || !read_double(&dt) || !(dt > 0.0)) return 2;
        std::vector<double> taps((size_t)L);
        rt::half_derivative_taps(L, dt, taps.data());
        print_line("taps", taps);
    }
    if (std::scanf("%ld", &count) != 1 || count < 0) return 2;
    for (long c = 0; c < count; c++) {
        long nt = 0, L = 0, o = 0;
        if (std::scanf("%ld %ld %ld", &nt, &L, &o) != 3 || nt < 1 || L < 1 || o < 0 || o >= L) return 2;
        std::vector<double> f((size_t)L), x((size_t)nt), y((size_t)nt);
        for (double& v : f)
            if (!read_double(&v)) return 2;
        for (double& v : x)
            if (!read_double(&v)) return 2;
        rt::filter_host(f.data(), L, o, false, nt, x.data(), y.data());
        print_line("y", y);
        rt::filter_host(f.data(), L, o, true, nt, x.data(), y.data());
        print_line("yt", y);
    }
    return 0;
}
