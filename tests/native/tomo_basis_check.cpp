// rt_tomo_basis.h as a program of its own (tests/test_tomo_basis_ref.py builds it plain and with -fsanitize=address,undefined):
// the rules of an axis basis, the ranges of the transposed operator, the B-spline axes and the operator pair as host loops.
// stdin is a list of commands; doubles are read and printed as hexadecimal floats, so that every bit is compared:
//     axis <x|y> <q> <m> <B>  then q times: first w_0 .. w_(B-1)
//         -> "axis bad <index> <reason>" or "axis ok", "lo <m values>", "hi <m values>"; a good axis is kept in its slot
//     bspline <q> <m> <degree>
//         -> "bspline refused" or "bspline ok" and q lines "<first> <w_0> .. <w_degree>"
//     pair  then my mx values of c and qy qx values of x, for the axes in the two slots
//         -> "prolong <qy qx values>", "restrict <my mx values>"
// Every array is allocated at its exact size: an index outside it ends the program under the sanitizer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracing_amd/csrc/rt_tomo_basis.h"

struct Axis {
    int64_t q = 0, m = 0, B = 0;
    std::vector<int32_t> first, lo, hi;
    std::vector<double> wgt;
    rt::BasisAxis view() const { return rt::BasisAxis{q, m, B, first.data(), wgt.data()}; }
};

static void print_doubles(const char* name, const std::vector<double>& v) {
    std::printf("%s", name);
    for (double d : v) std::printf(" %a", d);
    std::printf("\n");
}

int main() {
    Axis slot[2];
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "axis")) {
            char which[4];
            long q = 0, m = 0, B = 0;
            if (std::scanf("%3s %ld %ld %ld", which, &q, &m, &B) != 4 || q < 0 || m < 0 || B < 0 || B > 16) return 2;
            Axis a;
            a.q = q; a.m = m; a.B = B;
            a.first.resize((size_t)q);
            a.wgt.resize((size_t)(q * B));
            for (long j = 0; j < q; j++) {
                int f = 0;
                if (std::scanf("%d", &f) != 1) return 2;
                a.first[(size_t)j] = f;
                for (long b = 0; b < B; b++)
                    if (std::scanf("%la", &a.wgt[(size_t)(j * B + b)]) != 1) return 2;
            }
            int64_t at = -1;
            const char* why = rt::basis_axis_check(a.q, a.m, a.B, a.first.data(), a.wgt.data(), &at);
            if (why) {
                std::printf("axis bad %lld %s\n", (long long)at, why);
                continue;
            }
            a.lo.resize((size_t)m);
            a.hi.resize((size_t)m);
            rt::basis_ranges(a.q, a.m, a.B, a.first.data(), a.lo.data(), a.hi.data());
            std::printf("axis ok\nlo");
            for (int32_t v : a.lo) std::printf(" %d", v);
            std::printf("\nhi");
            for (int32_t v : a.hi) std::printf(" %d", v);
            std::printf("\n");
            slot[which[0] == 'y'] = a;
        } else if (!std::strcmp(cmd, "bspline")) {
            long q = 0, m = 0, degree = 0;
            if (std::scanf("%ld %ld %ld", &q, &m, &degree) != 3) return 2;
            const bool sizes = q >= 0 && degree >= 0 && degree <= 3;
            std::vector<int32_t> first(sizes ? (size_t)q : 0);
            std::vector<double> wgt(sizes ? (size_t)(q * (degree + 1)) : 0);
            if (!sizes || !rt::bspline_axis(q, m, (int)degree, first.data(), wgt.data())) {
                std::printf("bspline refused\n");
                continue;
            }
            std::printf("bspline ok\n");
            for (long j = 0; j < q; j++) {
                std::printf("%d", first[(size_t)j]);
                for (long b = 0; b <= degree; b++) std::printf(" %a", wgt[(size_t)(j * (degree + 1) + b)]);
                std::printf("\n");
            }
        } else if (!std::strcmp(cmd, "pair")) {
            const Axis &X = slot[0], &Y = slot[1];
            if (X.q < 1 || Y.q < 1) return 2;
            std::vector<double> c((size_t)(Y.m * X.m)), x((size_t)(Y.q * X.q)), px((size_t)(Y.q * X.q)), t((size_t)(Y.q * X.m)), g((size_t)(Y.m * X.m));
            for (double& v : c)
                if (std::scanf("%la", &v) != 1) return 2;
            for (double& v : x)
                if (std::scanf("%la", &v) != 1) return 2;
            rt::basis_prolong_host(X.view(), Y.view(), c.data(), px.data());
            rt::basis_restrict_host(X.view(), Y.view(), X.lo.data(), X.hi.data(), Y.lo.data(), Y.hi.data(), x.data(), t.data(), g.data());
            print_doubles("prolong", px);
            print_doubles("restrict", g);
        } else {
            return 2;
        }
    }
    return 0;
}
