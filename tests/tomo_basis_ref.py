"""Restatement of the tomography model basis and its solver (include/rtmi.h, rtmi_tomo_basis_* and rtmi_tomo_lsqr_basis;
raytracing_amd/csrc/rt_tomo_basis.h): the uniform B-spline axes in np.longdouble, the ranges of the
transposed operator, prolong and restrict in the stated operation order (numpy forms every product as a temporary, so every
product and every add is rounded on its own), the second-difference pair, the stacked operator, and the solver on top of
kirchhoff_lsqr_ref.lsqr_loop, lsqr_weighted_ref.lsqr_weighted and tomo_ref.stacked.  Test infrastructure."""
import numpy as np

import lsqr_weighted_ref as LW
import tomo_ref as TR

LD = np.longdouble


def bspline_axis(q, m, degree):
    """(first [q] int32, wgt [q, degree + 1]): e = min(floor(j n / (q - 1)), n - 1), t = (j n - e (q - 1)) / (q - 1) in long double,
    the weights in long double and rounded once"""
    assert degree in (0, 1, 3) and q >= 2 and m >= degree + 1
    n = m if degree == 0 else m - degree
    first = np.zeros(q, dtype=np.int32)
    wgt = np.zeros((q, degree + 1))
    for j in range(q):
        e = min(j * n // (q - 1), n - 1)
        first[j] = e
        t = LD(j * n - e * (q - 1)) / LD(q - 1)
        if degree == 0:
            w = [LD(1)]
        elif degree == 1:
            w = [LD(1) - t, t]
        else:
            u = LD(1) - t
            w = [u * u * u / LD(6), ((LD(3) * t - LD(6)) * t * t + LD(4)) / LD(6),
                 (((LD(-3) * t + LD(3)) * t + LD(3)) * t + LD(1)) / LD(6), t * t * t / LD(6)]
        wgt[j] = [float(v) for v in w]
    return first, wgt


def ranges(first, m, B):
    """lo [m], hi [m]: lo[l] the first j with first[j] >= l - B + 1, hi[l] one past the last j with first[j] <= l"""
    first = np.asarray(first, dtype=np.int64)
    q = len(first)
    lo = np.zeros(m, dtype=np.int64)
    hi = np.zeros(m, dtype=np.int64)
    for l in range(m):
        j = 0
        while j < q and first[j] < l - B + 1:
            j += 1
        lo[l] = j
        k = q
        while k > 0 and first[k - 1] > l:
            k -= 1
        hi[l] = max(k, j)
    return lo, hi


class Basis:
    """P = Py (x) Px from c [my, mx] to x [qy, qx]"""

    def __init__(self, fx, wx, fy, wy, mx, my):
        self.fx, self.fy = np.asarray(fx, dtype=np.int64), np.asarray(fy, dtype=np.int64)
        self.wx = np.asarray(wx, dtype=np.float64).reshape(len(self.fx), -1)
        self.wy = np.asarray(wy, dtype=np.float64).reshape(len(self.fy), -1)
        self.qx, self.qy, self.mx, self.my = len(self.fx), len(self.fy), int(mx), int(my)
        self.bx, self.by = self.wx.shape[1], self.wy.shape[1]
        self.lox, self.hix = ranges(self.fx, self.mx, self.bx)
        self.loy, self.hiy = ranges(self.fy, self.my, self.by)

    @classmethod
    def bspline(cls, qx, qy, mx, my, degree=3):
        dx, dy = (degree, degree) if np.ndim(degree) == 0 else degree
        fx, wx = bspline_axis(qx, mx, dx)
        fy, wy = bspline_axis(qy, my, dy)
        return cls(fx, wx, fy, wy, mx, my)

    def prolong(self, c):
        """acc = +0; per a: r = +0, per b: r = r + wx[j][b] c[fy[i] + a][fx[j] + b]; acc = acc + wy[i][a] r"""
        c = np.asarray(c, dtype=np.float64).reshape(self.my, self.mx)
        acc = np.zeros((self.qy, self.qx))
        for a in range(self.by):
            r = np.zeros((self.qy, self.qx))
            for b in range(self.bx):
                r = r + self.wx[None, :, b] * c[(self.fy + a)[:, None], (self.fx + b)[None, :]]
            acc = acc + self.wy[:, a][:, None] * r
        return acc

    def restrict(self, x):
        """t[i][l]: j ascending over [lo_x[l], hi_x[l]); g[k][l]: i ascending over [lo_y[k], hi_y[k]); both from +0"""
        x = np.asarray(x, dtype=np.float64).reshape(self.qy, self.qx)
        t = np.zeros((self.qy, self.mx))
        for l in range(self.mx):
            for j in range(self.lox[l], self.hix[l]):
                t[:, l] = t[:, l] + self.wx[j, l - self.fx[j]] * x[:, j]
        g = np.zeros((self.my, self.mx))
        for k in range(self.my):
            for i in range(self.loy[k], self.hiy[k]):
                g[k, :] = g[k, :] + self.wy[i, k - self.fy[i]] * t[i, :]
        return g

    def axis_matrix(self, axis):
        f, w, m = (self.fx, self.wx, self.mx) if axis == "x" else (self.fy, self.wy, self.my)
        M = np.zeros((len(f), m))
        for j in range(len(f)):
            for b in range(w.shape[1]):
                M[j, f[j] + b] += w[j, b]
        return M

    def dense(self):
        """P as a dense [qy qx, my mx] matrix, from the weights"""
        return np.kron(self.axis_matrix("y"), self.axis_matrix("x"))


def diff2_forward(s, gx, gy, mx2, my2):
    """[Dxx s | Dyy s]: fl(mx2 fl(fl(s[k][l] + s[k][l+2]) - fl(2 s[k][l+1]))) [gy, gx-2], alike in y [gy-2, gx]; an axis with
    fewer than 3 values has no rows"""
    s = np.asarray(s, dtype=np.float64).reshape(gy, gx)
    ux = mx2 * ((s[:, :-2] + s[:, 2:]) - 2.0 * s[:, 1:-1]) if gx > 2 else np.zeros((gy, 0))
    uy = my2 * ((s[:-2, :] + s[2:, :]) - 2.0 * s[1:-1, :]) if gy > 2 else np.zeros((0, gx))
    return np.r_[ux.ravel(), uy.ravel()]


def n_diff2(gx, gy):
    return gy * max(gx - 2, 0), max(gy - 2, 0) * gx


def diff2_transpose(u, gx, gy, mx2, my2):
    """fl(r2 + s2) at every node: r2 = fl(mx2 fl(fl(uxx[k][l-2] + uxx[k][l]) - fl(2 uxx[k][l-1]))), s2 alike, missing neighbours +0"""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    nx, ny = n_diff2(gx, gy)
    xa = np.zeros((gy, gx)); xb = np.zeros((gy, gx)); xc = np.zeros((gy, gx))
    ya = np.zeros((gy, gx)); yb = np.zeros((gy, gx)); yc = np.zeros((gy, gx))
    if gx > 2:
        uxx = u[:nx].reshape(gy, gx - 2)
        xa[:, 2:] = uxx; xb[:, 1:-1] = uxx; xc[:, :-2] = uxx
    if gy > 2:
        uyy = u[nx:nx + ny].reshape(gy - 2, gx)
        ya[2:, :] = uyy; yb[1:-1, :] = uyy; yc[:-2, :] = uyy
    return (mx2 * ((xa + xc) - 2.0 * xb) + my2 * ((ya + yc) - 2.0 * yb)).ravel()


def n_reg(gx, gy, d1, d2):
    n1 = 0 if d1 is None else gy * (gx - 1) + (gy - 1) * gx
    return n1, n1 + (0 if d2 is None else sum(n_diff2(gx, gy)))


def _present(pair):
    """a pair equal to (0, 0), or None, is absent"""
    return None if pair is None or (pair[0] == 0.0 and pair[1] == 0.0) else (float(pair[0]), float(pair[1]))


def stacked(row_ptr, base, val, qx, qy, basis=None, d1=None, d2=None, vmax=None):
    """(matvec, rmatvec, rows of the regulariser) of u = [A P s | Dx s | Dy s | Dxx s | Dyy s] on the grid G of s"""
    d1, d2 = _present(d1), _present(d2)
    mvA, rmvA = TR.stacked(row_ptr, base, val, qx, qy, smooth=None, vmax=vmax)
    rows = len(row_ptr) - 1
    gx, gy = (qx, qy) if basis is None else (basis.mx, basis.my)
    n1, nr = n_reg(gx, gy, d1, d2)

    def mv(s):
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        parts = [mvA(s if basis is None else basis.prolong(s).ravel())]
        if d1 is not None:
            parts.append(TR.diff_forward(s, gx, gy, *d1))
        if d2 is not None:
            parts.append(diff2_forward(s, gx, gy, *d2))
        return np.concatenate(parts)

    def rmv(u):
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        g = rmvA(u[:rows])
        if basis is not None:
            g = basis.restrict(g).ravel()
        if d1 is not None and d2 is not None:
            return g + (TR.diff_transpose(u[rows:rows + n1], gx, gy, *d1) + diff2_transpose(u[rows + n1:], gx, gy, *d2))
        if d1 is not None:
            return g + TR.diff_transpose(u[rows:], gx, gy, *d1)
        if d2 is not None:
            return g + diff2_transpose(u[rows:], gx, gy, *d2)
        return g
    return mv, rmv, nr


def lsqr(row_ptr, base, val, qx, qy, rhs, iter_lim, basis=None, d1=None, d2=None, wr=None, dc=None, x0=None, vmax=None, **kw):
    """rtmi_tomo_lsqr_basis: min |W A P D y - W (b - A x0)|^2 + damp^2 |y|^2 + the regulariser rows of D y over y on G; c = D y,
    x = x0 + P c.  x0 is a fine model: its residual is taken with A alone.  -> lsqr_loop's dict with c [gy, gx] and x [qy, qx]."""
    mv, rmv, nr = stacked(row_ptr, base, val, qx, qy, basis=basis, d1=d1, d2=d2, vmax=vmax)
    rows = len(row_ptr) - 1
    r = np.asarray(rhs, dtype=np.float64).reshape(-1).copy()
    if x0 is not None:
        x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
        r = r - TR.apply(row_ptr, base, val, qx, x0)
    b = np.r_[r, np.zeros(nr)]
    out = LW.lsqr_weighted(mv, rmv, b, iter_lim, wr=wr, dc=dc, x0=None, ndata=rows, **kw)
    c = out["x"]
    x = c if basis is None else basis.prolong(c).ravel()
    if x0 is not None:
        x = x0 + x
    gx, gy = (qx, qy) if basis is None else (basis.mx, basis.my)
    out["c"], out["x"] = c.reshape(gy, gx), x.reshape(qy, qx)
    return out
