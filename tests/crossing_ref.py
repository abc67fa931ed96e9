"""numpy restatement of rtmi_crossings (include/rtmi.h; raytracing_amd/csrc/twopoint.hip): the same rule and the same
operation order, element by element, so that it gives the device's bits from the same rows.  Test infrastructure.

sin and cos are np.sin / np.cos (glibc's, which the kernel reproduces through rt_libm.h); the receiver angle is np.arctan2,
which may differ from the device's atan2 in the last bit -- the tests compare that column to 2 ulp."""
import numpy as np

FIELDS = ("u", "x", "y", "T", "theta", "s")


def normalise(line):
    a, b, c = (float(v) for v in line)
    nrm = np.sqrt(a * a + b * b)
    if not (nrm > 0) or not np.isfinite(nrm) or not np.isfinite(c):
        raise ValueError("the line needs (a, b) != (0, 0) and finite coefficients")
    return a / nrm, b / nrm, c / nrm


def _basis(t):
    t2 = t * t
    t3 = t2 * t
    return (2.0 * t3 - 3.0 * t2) + 1.0, (t3 - 2.0 * t2) + t, 3.0 * t2 - 2.0 * t3, t3 - t2


def _dbasis(t):
    t2 = t * t
    return 6.0 * t2 - 6.0 * t, (3.0 * t2 - 4.0 * t) + 1.0, 6.0 * t - 6.0 * t2, 3.0 * t2 - 2.0 * t


def _herm(h, p0, m0, p1, m1):
    return ((p0 * h[0] + m0 * h[1]) + p1 * h[2]) + m1 * h[3]


def crossings(s_ray, last, line, kmax=4, rec_rows=None):
    """s_ray [rows, 6, R] (x, y, p_x, p_y, T, theta; fp64 or fp32), last [R] = each ray's last written row.  A ray whose last
    row is >= rec_rows (default: the rows given) has count -1.  Returns (count [R] int32, out [kmax, 6, R])."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    rec_rows = rows if rec_rows is None else int(rec_rows)
    last = np.asarray(last, dtype=np.int64)
    A, B, Cc = normalise(line)
    count = np.zeros(R, dtype=np.int32)
    out = np.full((kmax, 6, R), np.nan)
    col = lambda q: s_ray[:, q, :].astype(np.float64)          # noqa: E731
    x, y = col(0), col(1)
    f = (A * x + B * y) - Cc
    i = np.arange(rows)[:, None]
    f0, f1 = f[:-1], f[1:]
    hit = ((f0 < 0.0) & (f1 >= 0.0)) | ((f0 > 0.0) & (f1 <= 0.0))
    hit &= (i[1:] <= last[None, :])
    trunc = last >= rec_rows
    hit[:, trunc] = False
    ii, kk = np.nonzero(hit)                                    # step ii+1 of ray kk, in row order
    order = np.lexsort((ii, kk))
    ii, kk = ii[order], kk[order]
    idx = np.zeros(len(kk), dtype=np.int64)                     # crossing index of each hit within its ray
    if len(kk):
        start = np.r_[0, np.nonzero(np.diff(kk))[0] + 1]
        run = np.diff(np.r_[start, len(kk)])
        idx = np.arange(len(kk)) - np.repeat(start, run)
    np.add.at(count, kk, 1)
    count[trunc] = -1
    keep = idx < kmax
    ii, kk, idx = ii[keep], kk[keep], idx[keep]
    if len(kk) == 0:
        return count, out
    r0, r1 = ii, ii + 1
    g = lambda q, r: s_ray[r, q, kk].astype(np.float64)         # noqa: E731
    x0, y0, x1, y1 = g(0, r0), g(1, r0), g(0, r1), g(1, r1)
    fa, fb = f[r0, kk], f[r1, kk]
    th0, th1 = g(5, r0), g(5, r1)
    c0, s0, c1, s1 = np.cos(th0), np.sin(th0), np.cos(th1), np.sin(th1)
    dx, dy = x1 - x0, y1 - y0
    ln = np.sqrt(dx * dx + dy * dy)
    tx0, ty0, tx1, ty1 = ln * c0, ln * s0, ln * c1, ln * s1
    d0, d1 = ln * (A * c0 + B * s0), ln * (A * c1 + B * s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(fb == 0.0, 1.0, fa / np.where(fb == 0.0, 1.0, fa - fb))
        lo, hi = np.zeros_like(tau), np.ones_like(tau)
        act = fb != 0.0
        for _ in range(64):
            if not act.any():
                break
            gv = _herm(_basis(tau), fa, d0, fb, d1)
            act &= gv != 0.0
            same = (gv < 0.0) == (fa < 0.0)
            lo = np.where(act & same, tau, lo)
            hi = np.where(act & ~same, tau, hi)
            act &= ~(hi - lo < 2.0 ** -52)
            gd = _herm(_dbasis(tau), fa, d0, fb, d1)
            tn = tau - gv / gd
            tau = np.where(act, np.where((tn > lo) & (tn < hi), tn, 0.5 * (lo + hi)), tau)
    h, hd = _basis(tau), _dbasis(tau)
    xs, ys = _herm(h, x0, tx0, x1, tx1), _herm(h, y0, ty0, y1, ty1)
    m0 = g(2, r0) * c0 + g(3, r0) * s0
    m1 = g(2, r1) * c1 + g(3, r1) * s1
    tt = _herm(h, g(4, r0), ln * m0, g(4, r1), ln * m1)
    th = np.arctan2(_herm(hd, y0, ty0, y1, ty1), _herm(hd, x0, tx0, x1, tx1))
    vals = (A * ys - B * xs, xs, ys, tt, th, ii.astype(np.float64) + tau)
    for q, v in enumerate(vals):
        out[idx, q, kk] = v
    return count, out


def as_dict(count, out):
    d = {"count": count}
    for q, k in enumerate(FIELDS):
        d[k] = out[:, q]
    return d
