// rt_locate.h as a program of its own (tests/test_locate_host.py builds it plain and with -fsanitize=address,undefined): the
// refinement of a located node on its 3 x 3 window, and the two steps of a node's objective as a plain loop.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     refine <9 values of win_obj> <9 values of win_tau> <ref> <sw> <ix> <iy> <gx0> <gdx> <gy0> <gdy>
//         -> "refine <x> <y> <t0> <dx> <dy> <cxx> <cxy> <cyy> <refined>"
//     node <P> <weighted 0|1> <need>  then P times: <tr> <w> <T>   (tr: t - ref, nan for a pick that is not valid)
//         -> "node <n> <sw> <tau> <obj>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_locate.h"

template <bool W> static void node(const std::vector<double>& tr, const std::vector<double>& w, const std::vector<double>& T, int need) {
    rt::LocateSums a{0, 0.0, 0.0};
    for (size_t r = 0; r < tr.size(); r++)
        if (!std::isnan(tr[r]) && std::isfinite(T[r])) rt::locate_pass1<W>(a, tr[r], w[r], T[r]);
    const double sw = W ? a.sw : (double)a.n;
    const bool cand = a.n >= (need > 1 ? need : 1);
    const double tau = cand ? a.sd / sw : std::nan("");
    double q = 0.0;
    for (size_t r = 0; r < tr.size(); r++)
        if (!std::isnan(tr[r]) && std::isfinite(T[r])) rt::locate_pass2<W>(q, tau, tr[r], w[r], T[r]);
    std::printf("node %d %a %a %a\n", a.n, sw, tau, cand ? q / sw : INFINITY);
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "refine")) {
            std::vector<double> f(9), tau(9);
            double ref = 0.0, sw = 0.0;
            int ix = 0, iy = 0;
            rt::LocateGrid g{};
            for (double& v : f)
                if (std::scanf("%la", &v) != 1) return 2;
            for (double& v : tau)
                if (std::scanf("%la", &v) != 1) return 2;
            if (std::scanf("%la %la %d %d %la %la %la %la", &ref, &sw, &ix, &iy, &g.gx0, &g.gdx, &g.gy0, &g.gdy) != 8) return 2;
            const rt::LocateRefined o = rt::locate_refine(f.data(), tau.data(), ref, sw, ix, iy, g);
            std::printf("refine %a %a %a %a %a %a %a %a %d\n", o.x, o.y, o.t0, o.dx, o.dy, o.cov[0], o.cov[1], o.cov[2], o.refined);
        } else if (!std::strcmp(cmd, "node")) {
            long P = 0;
            int weighted = 0, need = 0;
            if (std::scanf("%ld %d %d", &P, &weighted, &need) != 3 || P < 0 || P > 4096) return 2;
            std::vector<double> tr((size_t)P), w((size_t)P), T((size_t)P);
            for (long r = 0; r < P; r++)
                if (std::scanf("%la %la %la", &tr[(size_t)r], &w[(size_t)r], &T[(size_t)r]) != 3) return 2;
            if (weighted) node<true>(tr, w, T, need);
            else node<false>(tr, w, T, need);
        } else {
            return 2;
        }
    }
    return 0;
}
