// The factored linearisation of rt_eikonal_lin.h as a program of its own (tests/test_eikonal_factored_lin_host.py builds it plain
// and with -fsanitize=address,undefined): the coefficients of a free node and the serial tangent and adjoint solves of one source.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     coef <gx0> <gdx> <gy0> <gdy> <i> <j> <xs> <ys> <n_src> <l> <r> <dn> <up> <s> <t>   -> "coef <ca> <cb> <cs> <csrc> <parents>"
//     tangent <nx> <ny> <gx0> <gdx> <gy0> <gdy> <xs> <ys> <n_src> <ball> <max_rounds> <dn_src> <has seed 0|1>  then nx ny values
//         each of n, T, filled (0 or 1), dn and, with a seed, dT_seed
//         -> "tangent <rounds> <clean> <nodes> <changes>", then "dT" and nx ny values
//     adjoint <nx> ... <max_rounds>  then nx ny values each of n, T, filled and r
//         -> "adjoint <rounds> <clean> <nodes> <changes> <g_src>", then "lam" and nx ny values, then "g" and nx ny values
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_eikonal_lin.h"

static bool read(double* v) { return std::scanf("%la", v) == 1; }

static bool read_all(std::vector<double>& a) {
    for (double& v : a)
        if (!read(&v)) return false;
    return true;
}

static void print_all(const char* name, const std::vector<double>& a) {
    std::printf("%s", name);
    for (double v : a) std::printf(" %a", v);
    std::printf("\n");
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "coef")) {
            double gx0, gdx, gy0, gdy, xs, ys, n_src, l, r, dn, up, s, t;
            long i = 0, j = 0;
            if (!(read(&gx0) && read(&gdx) && read(&gy0) && read(&gdy)) || std::scanf("%ld %ld", &i, &j) != 2) return 2;
            if (!(read(&xs) && read(&ys) && read(&n_src) && read(&l) && read(&r) && read(&dn) && read(&up) && read(&s) && read(&t))) return 2;
            const rt::EikLinNode c = rt::eik_flin_coef(rt::eik_grid(gx0, gdx, gy0, gdy), i, j, xs, ys, n_src, l, r, dn, up, s, t);
            std::printf("coef %a %a %a %a %d\n", c.ca, c.cb, c.cs, c.csrc, (int)c.code);
        } else if (!std::strcmp(cmd, "tangent") || !std::strcmp(cmd, "adjoint")) {
            const bool adj = cmd[0] == 'a';
            long nx = 0, ny = 0;
            double gx0, gdx, gy0, gdy, xs, ys, n_src, ball, dn_src = 0.0;
            int max_rounds = 0, has_seed = 0;
            if (std::scanf("%ld %ld", &nx, &ny) != 2 || nx < 1 || ny < 1 || nx * ny > (1L << 22)) return 2;
            if (!(read(&gx0) && read(&gdx) && read(&gy0) && read(&gdy) && read(&xs) && read(&ys) && read(&n_src) && read(&ball))) return 2;
            if (std::scanf("%d", &max_rounds) != 1) return 2;
            if (!adj && (!read(&dn_src) || std::scanf("%d", &has_seed) != 1)) return 2;
            const size_t nn = (size_t)(nx * ny);
            std::vector<double> n(nn), T(nn), in(nn), seed(has_seed ? nn : 0), out(nn), g(nn), ca(nn), cb(nn), k(nn);
            std::vector<uint8_t> filled(nn), code(nn), kids(nn);
            if (!read_all(n) || !read_all(T)) return 2;
            for (uint8_t& f : filled) {
                int v = 0;
                if (std::scanf("%d", &v) != 1) return 2;
                f = (uint8_t)v;
            }
            if (!read_all(in) || !read_all(seed)) return 2;
            const rt::EikGrid gr = rt::eik_grid(gx0, gdx, gy0, gdy);
            if (adj) {
                double g_src = 0.0;
                const rt::EikLinResult r = rt::eik_lin_adjoint(gr, nx, ny, n.data(), T.data(), filled.data(), xs, ys, n_src, ball, max_rounds,
                                                               in.data(), out.data(), g.data(), &g_src, ca.data(), cb.data(), code.data(),
                                                               kids.data(), true);
                std::printf("adjoint %d %d %ld %ld %a\n", r.rounds, r.clean, (long)r.nodes, (long)r.changes, g_src);
                print_all("lam", out);
                print_all("g", g);
            } else {
                const rt::EikLinResult r = rt::eik_lin_tangent(gr, nx, ny, n.data(), T.data(), filled.data(), xs, ys, n_src, ball, max_rounds,
                                                               in.data(), dn_src, has_seed ? seed.data() : nullptr, out.data(), ca.data(),
                                                               cb.data(), k.data(), code.data(), true);
                std::printf("tangent %d %d %ld %ld\n", r.rounds, r.clean, (long)r.nodes, (long)r.changes);
                print_all("dT", out);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
