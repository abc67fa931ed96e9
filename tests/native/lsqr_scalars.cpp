// Test helper (CPU, g++, a program of its own): raytracing_amd/csrc/rt_lsqr.h, the scalar recurrence of rtmi_kirchhoff_lsqr, fed a
// recorded sequence of norms.  stdin: damp atol btol iter_lim, then beta and alfa of the start, then beta and alfa of every
// iteration (hex floats).  stdout: one line per iteration, the state as hex floats, in the order of
// tests/kirchhoff_lsqr_ref.py's Scalars.record().  tests/test_kirchhoff_lsqr_ref.py builds it twice, plain and with
// -fsanitize=address,undefined, and compares every bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../raytracing_amd/csrc/rt_lsqr.h"

static bool next(double* v) {
    char buf[128];
    if (std::scanf("%127s", buf) != 1) return false;
    *v = std::strtod(buf, nullptr);
    return true;
}

int main() {
    double damp, atol, btol, lim, beta, alfa;
    if (!next(&damp) || !next(&atol) || !next(&btol) || !next(&lim)) return 2;
    rt::LsqrState S;
    rt::lsqr_begin(S, damp, atol, btol, (int)lim);
    if (!next(&beta) || !next(&alfa)) return 2;
    std::vector<std::string> lines;
    bool go = rt::lsqr_first_beta(S, beta) && rt::lsqr_first_alfa(S, alfa);
    while (go && !rt::lsqr_done(S)) {
        if (!next(&beta) || !next(&alfa)) return 3;
        if (rt::lsqr_beta(S, beta)) (void)rt::lsqr_alfa(S, alfa);
        rt::lsqr_rotate(S);
        const double rec[12] = {S.alfa, S.beta, S.anorm, S.rhobar, S.phibar, S.c1, S.c2, S.r1norm, S.r2norm, S.arnorm, S.xnorm,
                                (double)S.istop};
        std::string line;
        for (double v : rec) {
            char buf[64];
            std::snprintf(buf, sizeof buf, "%a ", v);
            line += buf;
        }
        lines.push_back(line);
    }
    for (const std::string& l : lines) std::printf("%s\n", l.c_str());
    std::printf("end %d %d\n", S.itn, S.istop);
    return 0;
}
