"""numpy restatement of rtmi_paraxial (include/rtmi.h; raytracing_amd/csrc/paraxial.hip): the same propagator, crossing rule
and operation order, element by element.  Test infrastructure.

Field values come from scipy: the reference's own fits rebuilt from their coefficients (the oracle's or Field.arrays()) --
n's bilinear spline, and the two bicubic gradient fits with their derivatives (BivariateSpline.ev(..., dx=1)) -- where the
device evaluates the same splines as cell polynomials (< 1e-15 of each quantity's scale apart).  sin and cos are np.sin /
np.cos (glibc's, which the kernel reproduces)."""
import numpy as np
from scipy.interpolate import BivariateSpline

from crossing_ref import _basis, _dbasis, _herm, normalise

FIELDS = ("Q1", "P1", "Q2", "P2", "J", "G", "kmah")


def _knots(a, k):
    """FITPACK's interpolating knot vector on a linspace axis: degree 1 through every sample, degree 3 not-a-knot"""
    a = np.asarray(a, dtype=np.float64)
    if k == 1:
        return np.r_[a[0], a, a[-1]]
    return np.r_[[a[0]] * 4, a[2:-2], [a[-1]] * 4]


class SplineField:
    """The field of (x, y, Z, coef_dy, coef_dx) as the reference fits it (RT_bench.py:455-457): RectBivariateSpline's argument
    order is (y, x), so scipy's dx is d/dy here and dy is d/dx.  Points outside the grid are clamped (FITPACK's quirk Q4)."""

    def __init__(self, x, y, Z, cdy, cdx):
        self.x, self.y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        tx1, ty1, tx3, ty3 = _knots(x, 1), _knots(y, 1), _knots(x, 3), _knots(y, 3)
        self.n = BivariateSpline._from_tck((ty1, tx1, np.ravel(Z), 1, 1))
        self.gx = BivariateSpline._from_tck((ty3, tx3, np.ravel(cdx), 3, 3))
        self.gy = BivariateSpline._from_tck((ty3, tx3, np.ravel(cdy), 3, 3))

    def _clamp(self, x, y):
        return np.clip(y, self.y[0], self.y[-1]), np.clip(x, self.x[0], self.x[-1])

    def __call__(self, x, y):
        """-> n, dn/dx, dn/dy, d(dn/dx)/dx, d(dn/dx)/dy, d(dn/dy)/dx, d(dn/dy)/dy"""
        yc, xc = self._clamp(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        return (self.n.ev(yc, xc), self.gx.ev(yc, xc), self.gy.ev(yc, xc),
                self.gx.ev(yc, xc, dy=1), self.gx.ev(yc, xc, dx=1), self.gy.ev(yc, xc, dy=1), self.gy.ev(yc, xc, dx=1))

    def dgrad(self, x, y):
        return self(x, y)[3:]


def kappa(f, c, s):
    """K = n_ee - 2 n_e^2 / n for the normal e = (-sin theta, cos theta)"""
    n, gx, gy, gxx, gxy, gyx, gyy = f
    ex, ey = -s, c
    ne = gx * ex + gy * ey
    nee = ex * (gxx * ex + gxy * ey) + ey * (gyx * ex + gyy * ey)
    return nee - 2.0 * ne * ne / n


def kdk(t, h, ka, kb, wm):
    """one kick-drift-kick step of length h on t = [q1, p1, q2, p2] (a new list)"""
    q1, p1, q2, p2 = t
    a, d, b = 0.5 * h * ka, h * wm, 0.5 * h * kb
    p1 = p1 + a * q1; p2 = p2 + a * q2
    q1 = q1 + d * p1; q2 = q2 + d * p2
    p1 = p1 + b * q1; p2 = p2 + b * q2
    return [q1, p1, q2, p2]


def sign_change(a, b):
    return ((a > 0.0) & (b <= 0.0)) | ((a < 0.0) & (b >= 0.0))


def cross_tau(f0, d0, f1, d1):
    """rt_crossing.h cross_tau, vectorised (crossing_ref's loop)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(f1 == 0.0, 1.0, f0 / np.where(f1 == 0.0, 1.0, f0 - f1))
        lo, hi = np.zeros_like(tau), np.ones_like(tau)
        act = f1 != 0.0
        for _ in range(64):
            if not act.any():
                break
            g = _herm(_basis(tau), f0, d0, f1, d1)
            act &= g != 0.0
            same = (g < 0.0) == (f0 < 0.0)
            lo = np.where(act & same, tau, lo)
            hi = np.where(act & ~same, tau, hi)
            act &= ~(hi - lo < 2.0 ** -52)
            gd = _herm(_dbasis(tau), f0, d0, f1, d1)
            tn = tau - g / gd
            tau = np.where(act, np.where((tn > lo) & (tn < hi), tn, 0.5 * (lo + hi)), tau)
    return tau


def _columns(t, n0, nr, kmah):
    q1, p1, q2, p2 = t
    J = n0 * q2
    with np.errstate(divide="ignore"):
        G = 1.0 / np.sqrt(nr * np.abs(J))
    return np.stack([q1, p1, q2, p2, J, G, kmah.astype(np.float64)])


def paraxial(s_ray, last, field, line=None, kmax=4, rec_rows=None):
    """s_ray [rows, 6, R] (fp64 or fp32), last [R] = each ray's last written row, field: a SplineField (or any callable of the
    same signature).  Returns (count [R] int32, at_line [kmax, 7, R] or None, at_end [7, R]) as rtmi_paraxial."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    rec_rows = rows if rec_rows is None else int(rec_rows)
    last = np.asarray(last, dtype=np.int64)
    trunc = last >= rec_rows
    x = s_ray[:, 0, :].astype(np.float64)
    y = s_ray[:, 1, :].astype(np.float64)
    th = s_ray[:, 5, :].astype(np.float64)
    c, s = np.cos(th), np.sin(th)
    live = (np.arange(rows)[:, None] <= last[None, :]) & ~trunc[None, :]
    f = [np.ones((rows, R))] + [np.zeros((rows, R)) for _ in range(6)]
    vals = field(x[live], y[live])
    for q in range(7):
        f[q][live] = vals[q]
    K = kappa(f, c, s)
    w = 1.0 / f[0]
    n0 = f[0][0]
    if line is not None:
        A, B, Cc = normalise(line)
        fl = (A * x + B * y) - Cc
        at_line = np.full((kmax, 7, R), np.nan)
    else:
        at_line = None
    count = np.zeros(R, dtype=np.int32)
    kmah = np.zeros(R, dtype=np.int64)
    t = [np.ones(R), np.zeros(R), np.zeros(R), np.ones(R)]
    nl = f[0][0].copy()
    for i in range(1, int(max(last[~trunc].max(initial=0), 0)) + 1):
        act = live[i]
        dx, dy = x[i] - x[i - 1], y[i] - y[i - 1]
        ln = np.sqrt(dx * dx + dy * dy)
        if line is not None:
            hit = act & sign_change(fl[i - 1], fl[i])
            keep = hit & (count < kmax)
            if keep.any():
                k = np.nonzero(keep)[0]
                d0 = ln[k] * (A * c[i - 1, k] + B * s[i - 1, k])
                d1 = ln[k] * (A * c[i, k] + B * s[i, k])
                tau = cross_tau(fl[i - 1, k], d0, fl[i, k], d1)
                kt = K[i - 1, k] + tau * (K[i, k] - K[i - 1, k])
                wt = w[i - 1, k] + tau * (w[i, k] - w[i - 1, k])
                u = kdk([v[k] for v in t], tau * ln[k], K[i - 1, k], kt, 0.5 * (w[i - 1, k] + wt))
                km = kmah[k] + sign_change(t[2][k], u[2])
                at_line[count[k], :, k] = _columns(u, n0[k], 1.0 / wt, km).T
            count += hit
        q2 = t[2]
        nt = kdk(t, ln, K[i - 1], K[i], 0.5 * (w[i - 1] + w[i]))
        t = [np.where(act, a, b) for a, b in zip(nt, t)]
        kmah += act & sign_change(q2, t[2])
        nl = np.where(act, f[0][i], nl)
    at_end = _columns(t, n0, nl, kmah)
    at_end[:, trunc] = np.nan
    count[trunc] = -1
    return count, at_line, at_end


def vert_closed_form(th0, x, y, xs=-2.0, ys=-2.0):
    """|J| on the arc of radius rho about (xc, -9) through the source, launched at th0 (v = 18 + 2 y: V_nn = 0)"""
    rho = (ys + 9) / np.cos(th0)
    xc = xs + (ys + 9) * np.tan(th0)
    phs = np.arctan2(ys + 9, xs - xc)
    ph = np.arctan2(y + 9, x - xc)
    return rho * np.abs(np.cos(phs) - np.cos(ph)) / np.sin(phs)


def as_dict(cols):
    return {k: cols[..., q, :] for q, k in enumerate(FIELDS)}
