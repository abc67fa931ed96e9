// rt_eikonal_tomo.h as a program of its own (tests/test_eikonal_tomo_host.py builds it plain and with -fsanitize=address,undefined):
// the cell weights of a point, the sample, the lists of the transposed product and the live-row rule.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     cell <nx> <ny> <gx0> <gdx> <gy0> <gdy> <x> <y> <source 0|1>   -> "cell <inside> <ok> <i0> <i1> <i2> <i3> <w0> <w1> <w2> <w3>"
//     sample <w0> <w1> <w2> <w3> <v0> <v1> <v2> <v3>                 -> "sample <value>"
//     lists <P> <use take 0|1>  then 4 P node indices and, with take, P flags
//                                                                  -> "node ...", "off ...", "pair ..."
//     live <nn> <R>  then nn values each of n and T and 4 R node indices        -> "live <R flags>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_eikonal_tomo.h"

static bool read(double* v) { return std::scanf("%la", v) == 1; }

static void print_ints(const char* name, const std::vector<int32_t>& a) {
    std::printf("%s", name);
    for (int32_t v : a) std::printf(" %d", (int)v);
    std::printf("\n");
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "cell")) {
            long nx = 0, ny = 0;
            double gx0, gdx, gy0, gdy, x, y;
            int source = 0;
            if (std::scanf("%ld %ld", &nx, &ny) != 2 || nx < 1 || ny < 1) return 2;
            if (!(read(&gx0) && read(&gdx) && read(&gy0) && read(&gdy) && read(&x) && read(&y)) || std::scanf("%d", &source) != 1) return 2;
            const rt::EikGrid g = rt::eik_grid(gx0, gdx, gy0, gdy);
            const rt::EtomoCell c = rt::etomo_cell(g, nx, ny, x, y, source != 0);
            std::printf("cell %d %d %ld %ld %ld %ld %a %a %a %a\n", (int)c.inside, (int)rt::etomo_receiver_ok(g, nx, ny, x, y), c.idx[0], c.idx[1],
                        c.idx[2], c.idx[3], c.w[0], c.w[1], c.w[2], c.w[3]);
        } else if (!std::strcmp(cmd, "sample")) {
            double w[4], v[4];
            for (double& a : w)
                if (!read(&a)) return 2;
            for (double& a : v)
                if (!read(&a)) return 2;
            std::printf("sample %a\n", rt::etomo_sample(v[0], v[1], v[2], v[3], w));
        } else if (!std::strcmp(cmd, "lists")) {
            long P = 0;
            int use = 0;
            if (std::scanf("%ld %d", &P, &use) != 2 || P < 0 || P > (1L << 20)) return 2;
            std::vector<long> idx(4 * (size_t)P);
            std::vector<uint8_t> take((size_t)P);
            for (long& v : idx)
                if (std::scanf("%ld", &v) != 1) return 2;
            if (use)
                for (uint8_t& t : take) {
                    int v = 0;
                    if (std::scanf("%d", &v) != 1) return 2;
                    t = (uint8_t)v;
                }
            const rt::EtomoLists L = rt::etomo_lists(idx.data(), P, use ? take.data() : nullptr);
            print_ints("node", L.node);
            print_ints("off", L.off);
            print_ints("pair", L.pair);
        } else if (!std::strcmp(cmd, "live")) {
            long nn = 0, R = 0;
            if (std::scanf("%ld %ld", &nn, &R) != 2 || nn < 1 || R < 0 || nn > (1L << 22) || R > (1L << 20)) return 2;
            std::vector<double> n((size_t)nn), T((size_t)nn);
            std::vector<long> idx(4 * (size_t)R);
            for (double& v : n)
                if (!read(&v)) return 2;
            for (double& v : T)
                if (!read(&v)) return 2;
            for (long& v : idx)
                if (std::scanf("%ld", &v) != 1 || v < 0 || v >= nn) return 2;
            std::printf("live");
            for (long k = 0; k < R; k++) std::printf(" %d", (int)rt::etomo_live(n.data(), T.data(), idx.data() + 4 * k));
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
