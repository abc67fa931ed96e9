"""Restatement of rtmi_kirchhoff_lsqr (include/rtmi.h): fix_norm, the order-independent norm, with Python
integers; lsqr_loop, LSQR in the operation order of scipy.sparse.linalg.lsqr with the elementwise updates in numpy (numpy forms
a * y as a temporary, so every product and every add or subtract is rounded on its own) and the scalar recurrence in Python
floats -- raytracing_amd/csrc/rt_lsqr.h line for line.  Test infrastructure."""
import copy
import math

import numpy as np

FIX_BITS = 57
LSQR_RANGE = 8                     # RTMI_LSQR_RANGE
EPS = float(np.finfo(np.float64).eps)
TINY = 2.0 ** -1022                # the smallest normal number


class NormRange(Exception):
    """max|x|^2 is not a normal number"""


def fix_exponent(bound):
    return math.frexp(bound)[1] - FIX_BITS


def fix_norm(x, with_exponent=False):
    """M = max|x|; 0 -> +0.  bound = fl(M M), e = fix_exponent(bound); q_i = rint(ldexp(fl(x_i x_i), -e)); S = sum q_i, exact;
    sqrt(ldexp(fl(S), e)), the even part of e taken out of the root."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    M = float(np.max(np.abs(x)))
    if M == 0.0:
        return (0.0, 0) if with_exponent else 0.0
    bound = M * M
    if not (TINY <= bound < math.inf):
        raise NormRange(f"max|x|^2 = {bound!r}")
    e = fix_exponent(bound)
    sq = x * x                                         # one rounding per product
    S = 0
    for p in sq.tolist():
        S += round(math.ldexp(p, -e))                  # round(): ties to even, an int
    odd = e & 1                                        # sqrt(S 2^e) with the even part of e taken out of the root: the same
    nrm = math.ldexp(math.sqrt(math.ldexp(float(S), odd)), (e - odd) // 2)    # bits, and S 2^e may exceed fp64's range
    return (nrm, e) if with_exponent else nrm


def _sign(a):
    return 1.0 if a > 0.0 else -1.0 if a < 0.0 else 0.0


def sym_ortho(a, b):
    if b == 0.0:
        return _sign(a), 0.0, abs(a)
    if a == 0.0:
        return 0.0, _sign(b), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = _sign(b) / math.sqrt(1.0 + tau * tau)
        c = s * tau
        r = b / s
    else:
        tau = b / a
        c = _sign(a) / math.sqrt(1.0 + tau * tau)
        s = c * tau
        r = a / c
    return c, s, r


class Scalars:
    """rt::LsqrState and its half-steps"""

    def __init__(self, damp, atol, btol, iter_lim):
        self.damp, self.dampsq, self.atol, self.btol, self.iter_lim = float(damp), float(damp) * float(damp), float(atol), float(btol), iter_lim
        self.itn = self.istop = 0
        self.done = False
        self.alfa = self.beta = self.bnorm = 0.0
        self.anorm = self.rhobar = self.phibar = self.rnorm = self.r1norm = self.r2norm = self.arnorm = 0.0
        self.res2 = self.xnorm = self.xxnorm = self.z = self.sn2 = 0.0
        self.cs2 = -1.0
        self.c1 = self.c2 = 0.0

    def first_beta(self, beta):
        self.bnorm = self.beta = self.rnorm = self.r1norm = self.r2norm = self.phibar = beta
        if not beta > 0.0:
            self.done = True
        return not self.done

    def first_alfa(self, alfa):
        self.alfa = self.rhobar = alfa
        self.arnorm = alfa * self.beta
        if self.arnorm == 0.0:
            self.done = True
        return not self.done

    def finished(self):
        return self.done or self.itn >= self.iter_lim

    def step_beta(self, beta):
        self.itn += 1
        self.beta = beta
        if beta > 0.0:
            self.anorm = math.sqrt(self.anorm * self.anorm + self.alfa * self.alfa + beta * beta + self.dampsq)
            return True
        return False

    def step_alfa(self, alfa):
        self.alfa = alfa
        return alfa > 0.0

    def rotate(self):
        if self.damp > 0.0:
            rhobar1 = math.sqrt(self.rhobar * self.rhobar + self.dampsq)
            cs1 = self.rhobar / rhobar1
            sn1 = self.damp / rhobar1
            psi = sn1 * self.phibar
            self.phibar = cs1 * self.phibar
        else:
            rhobar1 = self.rhobar
            psi = 0.0
        cs, sn, rho = sym_ortho(rhobar1, self.beta)
        theta = sn * self.alfa
        self.rhobar = -cs * self.alfa
        phi = cs * self.phibar
        self.phibar = sn * self.phibar
        tau = sn * phi
        self.c1 = phi / rho
        self.c2 = theta / rho
        delta = self.sn2 * rho
        gambar = -self.cs2 * rho
        rhs = phi - delta * self.z
        zbar = rhs / gambar
        self.xnorm = math.sqrt(self.xxnorm + zbar * zbar)
        gamma = math.sqrt(gambar * gambar + theta * theta)
        self.cs2 = gambar / gamma
        self.sn2 = theta / gamma
        self.z = rhs / gamma
        self.xxnorm = self.xxnorm + self.z * self.z
        res1 = self.phibar * self.phibar
        self.res2 = self.res2 + psi * psi
        self.rnorm = math.sqrt(res1 + self.res2)
        self.arnorm = self.alfa * abs(tau)
        if self.damp > 0.0:
            r1sq = self.rnorm * self.rnorm - self.dampsq * self.xxnorm
            self.r1norm = math.sqrt(abs(r1sq))
            if r1sq < 0.0:
                self.r1norm = -self.r1norm
        else:
            self.r1norm = self.rnorm
        self.r2norm = self.rnorm
        test1 = self.rnorm / self.bnorm
        test2 = self.arnorm / (self.anorm * self.rnorm + EPS)
        rtol = self.btol + self.atol * self.anorm * self.xnorm / self.bnorm
        if self.itn >= self.iter_lim:
            self.istop = 7
        if test2 <= self.atol:
            self.istop = 2
        if test1 <= rtol:
            self.istop = 1
        if self.istop != 0:
            self.done = True

    def record(self):
        """what tests/native/lsqr_scalars.cpp prints per iteration"""
        return (self.alfa, self.beta, self.anorm, self.rhobar, self.phibar, self.c1, self.c2, self.r1norm, self.r2norm, self.arnorm,
                self.xnorm, float(self.istop))


def lsqr_loop(matvec, rmatvec, b, iter_lim, damp=0.0, atol=0.0, btol=0.0, norm=fix_norm, scalars=None):
    """-> dict(x, istop, itn, r1norm, r2norm, anorm, arnorm, history [itn, 4]: alfa, beta, r1norm, arnorm).  matvec: x -> A x and
    rmatvec: y -> A^T y on flat fp64 arrays.  scalars: a list that receives Scalars.record() of every iteration."""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    S = Scalars(damp, atol, btol, iter_lim)
    hist = []
    x = S0 = None
    try:
        u = b.copy()
        go = S.first_beta(norm(u))
        if go:
            u = (1.0 / S.beta) * u
            v = np.asarray(rmatvec(u), dtype=np.float64).reshape(-1).copy()
            x = np.zeros(v.size)
            go = S.first_alfa(norm(v))
            if go:
                v = (1.0 / S.alfa) * v
                w = v.copy()
        while go and not S.finished():
            S0 = copy.copy(S)                          # a norm out of range abandons its iteration: the last completed one stands
            t = np.asarray(matvec(v), dtype=np.float64).reshape(-1)
            u = t - S.alfa * u
            if S.step_beta(norm(u)):
                u = (1.0 / S.beta) * u
                t = np.asarray(rmatvec(u), dtype=np.float64).reshape(-1)
                v = t - S.beta * v
                if S.step_alfa(norm(v)):
                    v = (1.0 / S.alfa) * v
            S.rotate()
            x = x + S.c1 * w
            w = v - S.c2 * w
            hist.append((S.alfa, S.beta, S.r1norm, S.arnorm))
            if scalars is not None:
                scalars.append(S.record())
        istop = S.istop
    except NormRange:
        istop = LSQR_RANGE
        if S0 is not None:
            S = S0
    if x is None:
        x = np.zeros(np.asarray(rmatvec(np.zeros(b.size))).size)
    return {"x": x, "istop": istop, "itn": S.itn, "r1norm": S.r1norm, "r2norm": S.r2norm, "anorm": S.anorm, "arnorm": S.arnorm,
            "history": np.array(hist, dtype=np.float64).reshape(-1, 4)}
