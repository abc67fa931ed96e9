"""Restatement of rtmi_tomo_* (include/rtmi.h; raytracing_amd/csrc/tomo.hip): the segments of a matrix row
from a ray's recorded rows, sequentially per ray in the kernel's operation order; the forward product as defined; the transposed
product with Python integers; the first-difference operators; the solver, by handing the stacked operator to
kirchhoff_lsqr_ref.lsqr_loop.  Test infrastructure.

The weights a_j follow rt_sens_walk.h's walk with weight 1 on the one observation; the cell and phi come from
sensitivity_ref.weights, whose u differs from the kernel's fused form in the last bit, and coef is not fused either: segment values
agree with the device to rounding, `base` and the segment counts exactly.  The products and the solver are defined
on given segments and are restated bit for bit."""
import math

import numpy as np

import crossing_ref as X
import kirchhoff_lsqr_ref as K
import sensitivity_ref as S

SKIP = -2                                  # RTMI_TOMO_SKIP


def _tau(fa, d0, fb, d1):
    """rt_crossing.h's cross_tau, elementwise (crossing_ref.crossings' loop)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(fb == 0.0, 1.0, fa / np.where(fb == 0.0, 1.0, fa - fb))
        lo, hi = np.zeros_like(tau), np.ones_like(tau)
        act = fb != 0.0
        for _ in range(64):
            if not act.any():
                break
            gv = X._herm(X._basis(tau), fa, d0, fb, d1)
            act &= gv != 0.0
            same = (gv < 0.0) == (fa < 0.0)
            lo = np.where(act & same, tau, lo)
            hi = np.where(act & ~same, tau, hi)
            act &= ~(hi - lo < 2.0 ** -52)
            gd = X._herm(X._dbasis(tau), fa, d0, fb, d1)
            tn = tau - gv / gd
            tau = np.where(act, np.where((tn > lo) & (tn < hi), tn, 0.5 * (lo + hi)), tau)
    return tau


def row_weights(s_ray, last, which, line=None, kmax=4, rec_rows=None):
    """a [rows, R]: the weight of every recorded row in ray m's observation which[m] (coef not applied), and end [R]: the last row
    that carries any (-1: an empty row or a skipped ray)."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    rec_rows = rows if rec_rows is None else int(rec_rows)
    last = np.asarray(last, dtype=np.int64)
    which = np.asarray(which, dtype=np.int64)
    x = s_ray[:, 0, :].astype(np.float64); y = s_ray[:, 1, :].astype(np.float64); th = s_ray[:, 5, :].astype(np.float64)
    dx = np.diff(x, axis=0); dy = np.diff(y, axis=0)
    ln = np.zeros((rows + 1, R))
    ln[1:rows] = np.sqrt(dx * dx + dy * dy)                 # ln[i]: step i (rows i-1 -> i)
    half = (1.0 * ln) * 0.5
    end = np.where((which == SKIP) | (last >= rec_rows), -1, last)
    hit_step = np.zeros(R, dtype=np.int64)
    cross = np.nonzero((which >= 0) & (end >= 0))[0]
    if len(cross):
        A, B, Cc = X.normalise(line)
        f = (A * x + B * y) - Cc
        hit = ((f[:-1] < 0.0) & (f[1:] >= 0.0)) | ((f[:-1] > 0.0) & (f[1:] <= 0.0))
        hit &= np.arange(1, rows)[:, None] <= last[None, :]
        nth = np.cumsum(hit, axis=0)                         # crossings up to and including step i + 1
        for m in cross:
            c = which[m]
            steps = np.nonzero(hit[:, m] & (nth[:, m] == c + 1))[0]
            if c >= kmax or len(steps) == 0:
                end[m] = -1
            else:
                hit_step[m] = steps[0] + 1
                end[m] = hit_step[m]
    # the trapezoid weights of a ray observed at its end; a crossing's ray has them on the rows before its step
    # row j: acur of step j (0 + half_j), then aprev += half_{j+1}; steps outside 1 .. lastw add +0.0, which changes no bit
    lastw = np.where(which >= 0, hit_step - 1, end)
    i_ = np.arange(rows + 1)[:, None]
    hm = np.where((i_ >= 1) & (i_ <= lastw[None, :]), half, 0.0)
    a = hm[:rows] + hm[1:rows + 1]
    j = np.arange(rows)[:, None]
    for m in cross:
        if end[m] < 0:
            continue
        i = hit_step[m]
        A, B, Cc = X.normalise(line)
        fa = (A * x[i - 1, m] + B * y[i - 1, m]) - Cc
        fb = (A * x[i, m] + B * y[i, m]) - Cc
        L = ln[i, m]
        d0 = L * (A * np.cos(th[i - 1, m]) + B * np.sin(th[i - 1, m]))
        d1 = L * (A * np.cos(th[i, m]) + B * np.sin(th[i, m]))
        tau = float(_tau(np.array([fa]), np.array([d0]), np.array([fb]), np.array([d1]))[0])
        _, h10, h01, h11 = X._basis(tau)
        aprev = hm[i - 1, m] + (1.0 * L) * (0.5 * h01 + h10)
        acur = (1.0 * L) * (0.5 * h01 + h11)
        zero = (0.0 * L) * 0.5                               # W = 0 from this step on
        a[i - 1, m] = aprev + zero
        a[i, m] = acur + zero
    a[j > end[None, :]] = 0.0
    return a, end


def segments(s_ray, last, ax, ay, which=None, line=None, kmax=4, method=6, gamma=1.0, rec_rows=None):
    """-> (nseg [R]: -1 for a skipped ray, row_ptr [rows + 1], base [n], val [n, 4]); the rows are the rays that are not
    skipped, in order."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    which = np.full(R, -1, dtype=np.int64) if which is None else np.asarray(which, dtype=np.int64)
    a, end = row_weights(s_ray, last, which, line=line, kmax=kmax, rec_rows=rec_rows)
    x = s_ray[:, 0, :].astype(np.float64); y = s_ray[:, 1, :].astype(np.float64); th = s_ray[:, 5, :].astype(np.float64)
    wr = a * S._coef(th, method, gamma) if method >= 10 else a
    cols, phi = S.weights(ax, ay, x, y)
    cell = cols[0].reshape(rows, R)
    phi = phi.reshape(4, rows, R)
    cur = np.full(R, -1, dtype=np.int64)
    p = np.zeros((R, 4))
    out_m, out_b, out_p = [], [], []

    def emit(mask):
        idx = np.nonzero(mask)[0]
        if len(idx):
            out_m.append(idx); out_b.append(cur[idx].copy()); out_p.append(p[idx].copy())

    for j in range(int(end.max()) + 1 if R else 0):
        act = j <= end
        b = cell[j]
        emit(act & (b != cur) & (cur >= 0))
        new = act & (b != cur)
        cur[new] = b[new]
        p[new] = 0.0
        for q in range(4):
            p[act, q] = p[act, q] + wr[j, act] * phi[q, j, act]
    emit(cur >= 0)
    m_all = np.concatenate(out_m) if out_m else np.zeros(0, dtype=np.int64)
    order = np.argsort(m_all, kind="stable")
    base = (np.concatenate(out_b) if out_b else np.zeros(0, dtype=np.int64))[order]
    val = (np.concatenate(out_p) if out_p else np.zeros((0, 4)))[order]
    count = np.bincount(m_all, minlength=R) if R else np.zeros(0, dtype=np.int64)
    keep = which != SKIP
    nseg = np.where(keep, count, -1).astype(np.int32)
    row_ptr = np.r_[0, np.cumsum(count[keep])].astype(np.int64)
    return nseg, row_ptr, base.astype(np.int32), val


def to_csr(row_ptr, base, val, qx, qy):
    import scipy.sparse as sp
    rows = len(row_ptr) - 1
    r = np.repeat(np.arange(rows), np.diff(row_ptr))
    b = np.asarray(base, dtype=np.int64)
    cols = np.stack([b, b + 1, b + qx, b + qx + 1], axis=1)
    return sp.coo_matrix((np.asarray(val).ravel(), (np.repeat(r, 4), cols.ravel())), shape=(rows, qx * qy)).tocsr()


def apply(row_ptr, base, val, qx, x):
    """y_r: acc = +0, then per segment in visit order acc = acc + (((p0 x0 + p1 x1) + p2 x2) + p3 x3)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = np.diff(row_ptr)
    y = np.zeros(len(n))
    b = np.asarray(base, dtype=np.int64)
    for k in range(int(n.max()) if len(n) else 0):
        r = np.nonzero(n > k)[0]
        s = row_ptr[r] + k
        c, pv = b[s], val[s]
        t = ((pv[:, 0] * x[c] + pv[:, 1] * x[c + 1]) + pv[:, 2] * x[c + qx]) + pv[:, 3] * x[c + qx + 1]
        y[r] = y[r] + t
    return y


def transpose(row_ptr, base, val, qx, qy, w, vmax=None):
    """g [qy qx]: every product rint(fl(p_q w_r) 2^-e) summed per sample as an integer, one rounding to fp64.  vmax: the handle's
    (max |p| over everything appended); None: that of val.  Raises kirchhoff_lsqr_ref.NormRange when fl(vmax W) is not normal."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    val = np.asarray(val, dtype=np.float64).reshape(-1, 4)
    g = np.zeros(qx * qy)
    vmax = float(np.max(np.abs(val))) if vmax is None and len(val) else (0.0 if vmax is None else float(vmax))
    W = float(np.max(np.abs(w))) if len(w) else 0.0
    if W == 0.0 or len(val) == 0 or vmax == 0.0:
        return g
    bound = vmax * W
    if not (K.TINY <= bound < math.inf):
        raise K.NormRange(f"Vmax max|w| = {bound!r}")
    e = K.fix_exponent(bound)
    r = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    prod = val * w[r][:, None]
    q = np.rint(np.ldexp(prod, -e))                          # integers below 2^57, exact in fp64
    b = np.asarray(base, dtype=np.int64)
    cols = np.stack([b, b + 1, b + qx, b + qx + 1], axis=1).ravel()
    qi = q.ravel().astype(np.int64)
    hi, lo = qi >> 32, qi & 0xFFFFFFFF                       # two int64 sums that cannot overflow
    sh = np.zeros(qx * qy, dtype=np.int64); sl = np.zeros(qx * qy, dtype=np.int64)
    np.add.at(sh, cols, hi)
    np.add.at(sl, cols, lo)
    for i in np.nonzero((sh != 0) | (sl != 0))[0]:
        g[i] = math.ldexp(float((int(sh[i]) << 32) + int(sl[i])), e)
    return g


def diff_forward(x, qx, qy, lx, ly):
    """[Dx x | Dy x]: fl(lx fl(x[i][j+1] - x[i][j])) [qy, qx-1], then fl(ly fl(x[i+1][j] - x[i][j])) [qy-1, qx]"""
    x = np.asarray(x, dtype=np.float64).reshape(qy, qx)
    return np.r_[(lx * (x[:, 1:] - x[:, :-1])).ravel(), (ly * (x[1:, :] - x[:-1, :])).ravel()]


def diff_transpose(u, qx, qy, lx, ly):
    """fl(r + s) at every node: r = fl(lx fl(ux[i][j-1] - ux[i][j])), s = fl(ly fl(uy[i-1][j] - uy[i][j])), missing neighbours +0"""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    ux = u[:qy * (qx - 1)].reshape(qy, qx - 1)
    uy = u[qy * (qx - 1):].reshape(qy - 1, qx)
    xa = np.zeros((qy, qx)); xb = np.zeros((qy, qx)); ya = np.zeros((qy, qx)); yb = np.zeros((qy, qx))
    xa[:, 1:] = ux; xb[:, :-1] = ux
    ya[1:, :] = uy; yb[:-1, :] = uy
    return (lx * (xa - xb) + ly * (ya - yb)).ravel()


def stacked(row_ptr, base, val, qx, qy, smooth=None, vmax=None):
    """(matvec, rmatvec) of u = [A x | Dx x | Dy x]"""
    rows = len(row_ptr) - 1

    def mv(x):
        y = apply(row_ptr, base, val, qx, x)
        return y if smooth is None else np.r_[y, diff_forward(x, qx, qy, *smooth)]

    def rmv(u):
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        g = transpose(row_ptr, base, val, qx, qy, u[:rows], vmax=vmax)
        return g if smooth is None else g + diff_transpose(u[rows:], qx, qy, *smooth)
    return mv, rmv


def lsqr(row_ptr, base, val, qx, qy, rhs, iter_lim, damp=0.0, smooth=None, atol=0.0, btol=0.0, vmax=None):
    """rtmi_tomo_lsqr: the loop of rtmi_kirchhoff_lsqr over the stacked operator, the right-hand side padded with zeros"""
    mv, rmv = stacked(row_ptr, base, val, qx, qy, smooth=smooth, vmax=vmax)
    nd = 0 if smooth is None else qy * (qx - 1) + (qy - 1) * qx
    b = np.r_[np.asarray(rhs, dtype=np.float64).reshape(-1), np.zeros(nd)]
    out = K.lsqr_loop(mv, rmv, b, iter_lim, damp=damp, atol=atol, btol=btol)
    out["x"] = out["x"].reshape(qy, qx)
    return out
