// Test helper (CPU, g++, a program of its own): raytracing_amd/csrc/rt_hilbert.h, the taps of the device's Hilbert transform and
// its definition as a host loop.  stdin: n, then the n samples of one trace (hex floats).  stdout: "taps" and the
// floor((n - 1) / 2) taps, then "y" and the n values of H x, all as hex floats.  tests/test_hilbert_ref.py builds it twice, plain
// and with -fsanitize=address,undefined, and compares every bit with the library's taps and with tests/hilbert_ref.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_amd/csrc/rt_hilbert.h"

int main() {
    long n = 0;
    if (std::scanf("%ld", &n) != 1 || n < 1) return 2;
    std::vector<double> x((size_t)n), y((size_t)n), taps((size_t)rt::hilbert_ntaps(n));
    for (double& v : x) {
        char buf[128];
        if (std::scanf("%127s", buf) != 1) return 2;
        v = std::strtod(buf, nullptr);
    }
    rt::hilbert_taps(n, taps.data());
    rt::hilbert_host(taps.data(), n, x.data(), y.data());
    std::printf("taps");
    for (double v : taps) std::printf(" %a", v);
    std::printf("\ny");
    for (double v : y) std::printf(" %a", v);
    std::printf("\n");
    return 0;
}
