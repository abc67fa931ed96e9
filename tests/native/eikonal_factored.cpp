// rt_eikonal.h's source-factored scheme as a program of its own (tests/test_eikonal_factored_host.py builds it plain and with
// -fsanitize=address,undefined): the corrected update of a free node and the serial solve of one source under either scheme.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     update <gx0> <gdx> <gy0> <gdy> <i> <j> <xs> <ys> <n_src> <l> <r> <dn> <up> <s>   -> "update <t>"
//     solve <scheme> <nx> <ny> <gx0> <gdx> <gy0> <gdy> <xs> <ys> <n_src> <ball> <max_rounds> <has T 0|1>  then nx ny values of n
//         and, with T, nx ny values of T
//         -> "solve <rounds> <clean> <free> <filled> <changes>", then (with T) "T" and nx ny values, then "filled" and nx ny digits
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_eikonal.h"

static bool read(double* v) { return std::scanf("%la", v) == 1; }

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "update")) {
            double gx0, gdx, gy0, gdy, xs, ys, n_src, l, r, dn, up, s;
            long i = 0, j = 0;
            if (!(read(&gx0) && read(&gdx) && read(&gy0) && read(&gdy)) || std::scanf("%ld %ld", &i, &j) != 2) return 2;
            if (!(read(&xs) && read(&ys) && read(&n_src) && read(&l) && read(&r) && read(&dn) && read(&up) && read(&s))) return 2;
            std::printf("update %a\n", rt::eik_update_factored(rt::eik_grid(gx0, gdx, gy0, gdy), i, j, xs, ys, n_src, l, r, dn, up, s));
        } else if (!std::strcmp(cmd, "solve")) {
            long nx = 0, ny = 0;
            double gx0, gdx, gy0, gdy, xs, ys, n_src, ball;
            int scheme = 0, max_rounds = 0, has_t = 0;
            if (std::scanf("%d %ld %ld", &scheme, &nx, &ny) != 3 || nx < 1 || ny < 1 || nx * ny > (1L << 22)) return 2;
            if (scheme != rt::kEikPlain && scheme != rt::kEikFactored) return 2;
            if (!(read(&gx0) && read(&gdx) && read(&gy0) && read(&gdy) && read(&xs) && read(&ys) && read(&n_src) && read(&ball))) return 2;
            if (std::scanf("%d %d", &max_rounds, &has_t) != 2) return 2;
            const size_t nn = (size_t)(nx * ny);
            std::vector<double> n(nn), T(has_t ? nn : 0), w(nn);
            std::vector<uint8_t> st(nn), filled(nn);
            for (double& v : n)
                if (!read(&v)) return 2;
            for (double& v : T)
                if (!read(&v)) return 2;
            const rt::EikResult r = rt::eik_solve(rt::eik_grid(gx0, gdx, gy0, gdy), nx, ny, n.data(), xs, ys, n_src, ball, max_rounds,
                                                  has_t ? T.data() : nullptr, w.data(), st.data(), filled.data(), scheme);
            std::printf("solve %d %d %ld %ld %ld\n", r.rounds, r.clean, (long)r.free_nodes, (long)r.filled, (long)r.changes);
            if (has_t) {
                std::printf("T");
                for (double v : T) std::printf(" %a", v);
                std::printf("\n");
            }
            std::printf("filled ");
            for (uint8_t v : filled) std::printf("%d", (int)v);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
