// rt_lsqr.h -- the scalar recurrence of LSQR (Paige and Saunders 1982) for rtmi_kirchhoff_lsqr (kirchhoff_lsqr.hip; DESIGN.md
// section 21): the state and one function per half-step, in the operation order of scipy.sparse.linalg.lsqr, every operation a
// separate fp64 operation (build with -ffp-contract=off, as the library is).  Plain C++ with no HIP in it: a host program includes
// it (tests/native/lsqr_scalars.cpp), and the solver calls it between the vector passes, whose norms it is handed:
//     lsqr_begin(S, damp, atol, btol, iter_lim)
//     lsqr_first_beta(S, |b|)          false: b = 0, the solution is x = 0 (istop 0)
//     lsqr_first_alfa(S, |A^T u|)      false: A^T b = 0, likewise
//     until lsqr_done(S):
//         lsqr_beta(S, |A v - alfa u|)     true: u is scaled by 1 / beta and A^T u is formed
//         lsqr_alfa(S, |A^T u - beta v|)   only after a true lsqr_beta; true: v is scaled by 1 / alfa
//         lsqr_rotate(S)                   then x = x + c1 w, w = v - c2 w, with S.c1 = phi / rho, S.c2 = theta / rho
// Included: _sym_ortho, the damp rotation, rhobar, phibar, theta, phi, rho, the right rotation z, xxnorm that r1norm needs under
// damping, r1norm, r2norm, anorm, arnorm, the stop tests 1, 2 and 7 and the early returns.  xnorm enters test 1 as in scipy (it
// comes from scalars alone) but is not reported.  Left out: conlim / acond and var (a vector norm more per iteration), the tests
// 3 to 6 (acond, and the machine-precision guards), show.  Row weights, a column scale and x0 need no scalar of their own: the
// loop around these half-steps applies them to the vectors (rt_lsqr_device.h, LsqrOptions).
#pragma once
#include <cmath>

namespace rt {

// istop: 0, 1, 2 and 7 are scipy's; kLsqrRange is the solver's own: a norm's bound max|x|^2 left the normal range of fp64
enum { kLsqrZero = 0, kLsqrResidual = 1, kLsqrLeastSquares = 2, kLsqrIterLim = 7, kLsqrRange = 8 };

struct LsqrState {
    double damp, dampsq, atol, btol;
    int iter_lim, itn, istop;
    bool done;
    double alfa, beta, bnorm;
    double anorm, rhobar, phibar, rnorm, r1norm, r2norm, arnorm;
    double res2, xnorm, xxnorm, z, cs2, sn2;
    double c1, c2;                  // the vector update of this iteration
};

inline double lsqr_sign(double a) { return a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : 0.0; }

// scipy's _sym_ortho: a stable Givens rotation
inline void lsqr_sym_ortho(double a, double b, double* c, double* s, double* r) {
    if (b == 0.0) {
        *c = lsqr_sign(a); *s = 0.0; *r = std::fabs(a);
    } else if (a == 0.0) {
        *c = 0.0; *s = lsqr_sign(b); *r = std::fabs(b);
    } else if (std::fabs(b) > std::fabs(a)) {
        const double tau = a / b;
        *s = lsqr_sign(b) / std::sqrt(1.0 + tau * tau);
        *c = *s * tau;
        *r = b / *s;
    } else {
        const double tau = b / a;
        *c = lsqr_sign(a) / std::sqrt(1.0 + tau * tau);
        *s = *c * tau;
        *r = a / *c;
    }
}

inline void lsqr_begin(LsqrState& S, double damp, double atol, double btol, int iter_lim) {
    S = LsqrState{};
    S.damp = damp; S.dampsq = damp * damp; S.atol = atol; S.btol = btol; S.iter_lim = iter_lim;
    S.cs2 = -1.0;
}

inline bool lsqr_first_beta(LsqrState& S, double beta) {
    S.bnorm = beta;
    S.beta = beta;
    S.rnorm = S.r1norm = S.r2norm = beta;
    S.phibar = beta;
    if (!(beta > 0.0)) S.done = true;       // alfa = 0, arnorm = 0: x = 0
    return !S.done;
}

inline bool lsqr_first_alfa(LsqrState& S, double alfa) {
    S.alfa = alfa;
    S.rhobar = alfa;
    S.arnorm = alfa * S.beta;
    if (S.arnorm == 0.0) S.done = true;
    return !S.done;
}

inline bool lsqr_done(const LsqrState& S) { return S.done || S.itn >= S.iter_lim; }

inline bool lsqr_beta(LsqrState& S, double beta) {
    S.itn = S.itn + 1;
    S.beta = beta;
    if (beta > 0.0) {
        S.anorm = std::sqrt(S.anorm * S.anorm + S.alfa * S.alfa + beta * beta + S.dampsq);
        return true;
    }
    return false;
}

inline bool lsqr_alfa(LsqrState& S, double alfa) {
    S.alfa = alfa;
    return alfa > 0.0;
}

inline void lsqr_rotate(LsqrState& S) {
    const double eps = 2.220446049250313e-16;
    double rhobar1, psi;
    if (S.damp > 0.0) {
        rhobar1 = std::sqrt(S.rhobar * S.rhobar + S.dampsq);
        const double cs1 = S.rhobar / rhobar1;
        const double sn1 = S.damp / rhobar1;
        psi = sn1 * S.phibar;
        S.phibar = cs1 * S.phibar;
    } else {
        rhobar1 = S.rhobar;
        psi = 0.0;
    }
    double cs, sn, rho;
    lsqr_sym_ortho(rhobar1, S.beta, &cs, &sn, &rho);
    const double theta = sn * S.alfa;
    S.rhobar = -cs * S.alfa;
    const double phi = cs * S.phibar;
    S.phibar = sn * S.phibar;
    const double tau = sn * phi;
    S.c1 = phi / rho;
    S.c2 = theta / rho;
    // the rotation on the right, for the norm of x
    const double delta = S.sn2 * rho;
    const double gambar = -S.cs2 * rho;
    const double rhs = phi - delta * S.z;
    const double zbar = rhs / gambar;
    S.xnorm = std::sqrt(S.xxnorm + zbar * zbar);
    const double gamma = std::sqrt(gambar * gambar + theta * theta);
    S.cs2 = gambar / gamma;
    S.sn2 = theta / gamma;
    S.z = rhs / gamma;
    S.xxnorm = S.xxnorm + S.z * S.z;
    // the norms of rbar and Abar' rbar
    const double res1 = S.phibar * S.phibar;
    S.res2 = S.res2 + psi * psi;
    S.rnorm = std::sqrt(res1 + S.res2);
    S.arnorm = S.alfa * std::fabs(tau);
    if (S.damp > 0.0) {
        const double r1sq = S.rnorm * S.rnorm - S.dampsq * S.xxnorm;
        S.r1norm = std::sqrt(std::fabs(r1sq));
        if (r1sq < 0.0) S.r1norm = -S.r1norm;
    } else {
        S.r1norm = S.rnorm;
    }
    S.r2norm = S.rnorm;
    const double test1 = S.rnorm / S.bnorm;
    const double test2 = S.arnorm / (S.anorm * S.rnorm + eps);
    const double rtol = S.btol + S.atol * S.anorm * S.xnorm / S.bnorm;
    if (S.itn >= S.iter_lim) S.istop = kLsqrIterLim;
    if (test2 <= S.atol) S.istop = kLsqrLeastSquares;
    if (test1 <= rtol) S.istop = kLsqrResidual;
    if (S.istop != 0) S.done = true;
}

}  // namespace rt
