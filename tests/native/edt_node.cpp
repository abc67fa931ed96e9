// rt_edt.h as a program of its own (tests/test_edt_host.py builds it plain and with -fsanitize=address,undefined): one node of
// one event by the loops the window kernel runs, and exp itself.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     node <P> <weighted 0|1> <need> <sigma>  then P times: <tr> <w> <T>   (tr: t - ref, nan for a pick that is not valid)
//         -> "node <n> <npairs> <value> <tau> <sum of omega> <P values of omega>"
//     exp <z>   -> "exp <exp(z)>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_edt.h"

template <bool W> static void node(const std::vector<double>& tr, const std::vector<double>& w, const std::vector<double>& T, int need,
                                   double sigma) {
    const int P = (int)tr.size();
    const double s2 = sigma * sigma;
    const rt::EdtView v{P, tr.data(), w.data(), 1, T.data(), 1, s2, rt::edt_g(s2, s2), rt::np_exp_tables()};
    const rt::EdtNode q = rt::edt_node<W>(v, need > 2 ? need : 2);
    std::vector<double> omega((size_t)P + 1);
    double den = 0.0;
    const double tau = rt::edt_tau<W>(v, &den, omega.data());
    std::printf("node %d %lld %a %a %a", q.n, (long long)q.n * (q.n - 1) / 2, q.value, tau, den);
    for (int r = 0; r < P; r++) std::printf(" %a", omega[(size_t)r]);
    std::printf("\n");
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "node")) {
            long P = 0;
            int weighted = 0, need = 0;
            double sigma = 0.0;
            if (std::scanf("%ld %d %d %la", &P, &weighted, &need, &sigma) != 4 || P < 0 || P > 4096) return 2;
            std::vector<double> tr((size_t)P), w((size_t)P), T((size_t)P);
            for (long r = 0; r < P; r++)
                if (std::scanf("%la %la %la", &tr[(size_t)r], &w[(size_t)r], &T[(size_t)r]) != 3) return 2;
            if (weighted) node<true>(tr, w, T, need, sigma);
            else node<false>(tr, w, T, need, sigma);
        } else if (!std::strcmp(cmd, "exp")) {
            double z = 0.0;
            if (std::scanf("%la", &z) != 1 || !(z >= rt::kEdtCut && z <= 0.0)) return 2;
            std::printf("exp %a\n", rt::edt_exp(z, rt::np_exp_tables()));
        } else {
            return 2;
        }
    }
    return 0;
}
