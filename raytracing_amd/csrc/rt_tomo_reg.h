// rt_tomo_reg.h -- the regulariser rows of the tomography solvers on a grid of gy x gx values: first differences, second
// differences, their transposed terms, and the check of rtmi_tomo_reg.  Shared by tomo.hip (rtmi_tomo_lsqr*, on the cell grid or a
// basis's coefficient grid) and eikonal_tomo.hip (rtmi_eikonal_tomo_lsqr, on the node grid); DESIGN.md sections 24 and 27 define
// the rows, tests/tomo_ref.py (diff_*) and tests/tomo_basis_ref.py (diff2_*) restate them.  After rtmi_host.h; in an anonymous
// namespace, as that header is: each unit gets its own copy.
#pragma once

namespace {

// The smoothing rows: ux [qy][qx - 1] = fl(lx fl(x[i][j + 1] - x[i][j])), uy [qy - 1][qx] = fl(ly fl(x[i + 1][j] - x[i][j]))
__global__ void __launch_bounds__(256) k_tomo_diff(const double* __restrict__ x, int qx, int qy, double lx, double ly, double* __restrict__ ux,
                                                   double* __restrict__ uy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)qx * qy) return;
    const int iy = (int)(i / qx), jx = (int)(i % qx);
    const double c = x[i];
    if (jx < qx - 1) ux[(size_t)iy * (qx - 1) + jx] = __dmul_rn(lx, __dadd_rn(x[i + 1], -c));
    if (iy < qy - 1) uy[i] = __dmul_rn(ly, __dadd_rn(x[i + qx], -c));
}

// The second-difference rows on a grid of gy x gx values: uxx [gy][gx - 2] = fl(mx fl(fl(s[k][l] + s[k][l + 2]) - fl(2 s[k][l + 1]))),
// uyy [gy - 2][gx] alike in y; an axis with fewer than 3 values has no rows
__global__ void __launch_bounds__(256) k_tomo_diff2(const double* __restrict__ s, int gx, int gy, double mx, double my, double* __restrict__ uxx,
                                                    double* __restrict__ uyy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)gx * gy) return;
    const int k = (int)(i / gx), l = (int)(i % gx);
    const double c = s[i];
    if (l < gx - 2) uxx[(size_t)k * (gx - 2) + l] = __dmul_rn(mx, __dadd_rn(__dadd_rn(c, s[i + 2]), -__dmul_rn(2.0, s[i + 1])));
    if (k < gy - 2) uyy[i] = __dmul_rn(my, __dadd_rn(__dadd_rn(c, s[i + 2 * (long)gx]), -__dmul_rn(2.0, s[i + gx])));
}

// The regulariser's transposed terms on the grid, added to g = gA in place.  First differences (ux given): k_tomo_finish's r and s.
// Second differences (uxx given): r2 = fl(mx fl(fl(uxx[k][l - 2] + uxx[k][l]) - fl(2 uxx[k][l - 1]))), s2 alike in y, a missing
// neighbour +0.0.  g = fl(gA + fl(r + s)), fl(gA + fl(r2 + s2)), or with both fl(gA + fl(fl(r + s) + fl(r2 + s2))).
__global__ void __launch_bounds__(256) k_tomo_reg_t(double* __restrict__ g, int gx, int gy, const double* __restrict__ ux,
                                                    const double* __restrict__ uy, double lx, double ly, const double* __restrict__ uxx,
                                                    const double* __restrict__ uyy, double mx, double my) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)gx * gy) return;
    const int k = (int)(i / gx), l = (int)(i % gx);
    double d1 = 0.0, d2 = 0.0;
    if (ux) {
        const double xa = l > 0 ? ux[(size_t)k * (gx - 1) + l - 1] : 0.0, xb = l < gx - 1 ? ux[(size_t)k * (gx - 1) + l] : 0.0;
        const double ya = k > 0 ? uy[i - gx] : 0.0, yb = k < gy - 1 ? uy[i] : 0.0;
        d1 = __dadd_rn(__dmul_rn(lx, __dadd_rn(xa, -xb)), __dmul_rn(ly, __dadd_rn(ya, -yb)));
    }
    if (uxx) {
        const size_t w = (size_t)(gx > 2 ? gx - 2 : 0), o = (size_t)k * w;
        const double xa = l >= 2 ? uxx[o + l - 2] : 0.0, xb = (l >= 1 && l < gx - 1) ? uxx[o + l - 1] : 0.0, xc = l < gx - 2 ? uxx[o + l] : 0.0;
        const double ya = k >= 2 ? uyy[i - 2 * (long)gx] : 0.0, yb = (k >= 1 && k < gy - 1) ? uyy[i - gx] : 0.0, yc = k < gy - 2 ? uyy[i] : 0.0;
        d2 = __dadd_rn(__dmul_rn(mx, __dadd_rn(__dadd_rn(xa, xc), -__dmul_rn(2.0, xb))),
                       __dmul_rn(my, __dadd_rn(__dadd_rn(ya, yc), -__dmul_rn(2.0, yb))));
    }
    g[i] = __dadd_rn(g[i], ux && uxx ? __dadd_rn(d1, d2) : ux ? d1 : d2);
}

// reg's weights, checked; *d1, *d2: the pair, or NULL when both of its weights are zero (the pair has no rows then)
int check_reg(const char* who, const rtmi_tomo_reg* reg, const double** d1, const double** d2) {
    *d1 = *d2 = nullptr;
    if (!reg) return RTMI_OK;
    for (const double v : {reg->d1[0], reg->d1[1]}) RTMI_ARG(std::isfinite(v) && v >= 0.0, "reg.d1 must be finite and >= 0");
    for (const double v : {reg->d2[0], reg->d2[1]}) RTMI_ARG(std::isfinite(v) && v >= 0.0, "reg.d2 must be finite and >= 0");
    if (reg->d1[0] != 0.0 || reg->d1[1] != 0.0) *d1 = reg->d1;
    if (reg->d2[0] != 0.0 || reg->d2[1] != 0.0) *d2 = reg->d2;
    return RTMI_OK;
}

}  // namespace
