// rt_stack.h as a program of its own (tests/test_stack_host.py builds it plain and with -fsanitize=address,undefined): the
// selection of events from a detection series and the two refinements of an event on its 3 x 3 x 3 window.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     select <M> <threshold> <min_sep> <max_events>  then M times: <peak> <peak_node>
//         -> "select <K> <remained> <m of event 0> ... <m of event K - 1>"
//     refine <27 values of win> <o> <od> <ix> <iy> <gx0> <gdx> <gy0> <gdy>
//         -> "refine <x> <y> <t0> <dx> <dy> <dm> <refined>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_stack.h"

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "select")) {
            long M = 0, min_sep = 0, max_events = 0;
            double threshold = 0.0;
            if (std::scanf("%ld %la %ld %ld", &M, &threshold, &min_sep, &max_events) != 4 || M < 0 || M > (1 << 20)) return 2;
            std::vector<double> peak((size_t)M);
            std::vector<int32_t> node((size_t)M);
            for (long m = 0; m < M; m++)
                if (std::scanf("%la %d", &peak[(size_t)m], &node[(size_t)m]) != 2) return 2;
            int remained = 0;
            const std::vector<int64_t> taken = rt::stack_select(peak.data(), node.data(), M, threshold, min_sep, max_events, &remained);
            std::printf("select %zu %d", taken.size(), remained);
            for (int64_t m : taken) std::printf(" %lld", (long long)m);
            std::printf("\n");
        } else if (!std::strcmp(cmd, "refine")) {
            std::vector<double> win(27);
            double o = 0.0, od = 0.0;
            int ix = 0, iy = 0;
            rt::LocateGrid g{};
            for (double& v : win)
                if (std::scanf("%la", &v) != 1) return 2;
            if (std::scanf("%la %la %d %d %la %la %la %la", &o, &od, &ix, &iy, &g.gx0, &g.gdx, &g.gy0, &g.gdy) != 8) return 2;
            const rt::StackRefined r = rt::stack_refine(win.data(), o, od, ix, iy, g);
            std::printf("refine %a %a %a %a %a %a %d\n", r.x, r.y, r.t0, r.dx, r.dy, r.dm, r.refined);
        } else {
            return 2;
        }
    }
    return 0;
}
