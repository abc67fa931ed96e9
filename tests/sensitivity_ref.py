"""numpy restatement of rtmi_traveltime_perturb / rtmi_traveltime_backproject (include/rtmi.h; raytracing_amd/csrc/sensitivity.hip):
the Frechet derivative A of the reported traveltimes with respect to the field's n samples, built from the rows as a scipy.sparse
CSR matrix, with crossing_ref's tau*.  Test infrastructure.

Each row i of a ray carries a weight on the four samples of its cell (the bilinear weights phi); the traveltime at the end of
a ray is the trapezoid sum of coef n over its rows, and at a crossing on step i the Hermite blend of rtmi_crossings with
h00 + h01 = 1 gives rows 0 .. i-2 their trapezoid weights, row i-1 L_{i-1}/2 + L_i (h01/2 + h10) and row i L_i (h01/2 + h11)."""
import numpy as np
import scipy.sparse as sp

import crossing_ref as X


def axes(x, y):
    """The field's map (rtmi_field_from_samples): origin, end and 1/h of each linspace axis."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    hx = (x[-1] - x[0]) / (len(x) - 1); hy = (y[-1] - y[0]) / (len(y) - 1)
    return (x[0], x[-1], 1.0 / hx, len(x)), (y[0], y[-1], 1.0 / hy, len(y))


def _axis(p, a, b, inv_h, q):
    ncell = q - 1
    pa = p - a
    with np.errstate(invalid="ignore"):
        j = np.floor(pa * inv_h)
    out = ~((j >= 0) & (j < ncell))
    if out.any():
        pc = np.clip(p[out], a, b)
        pa = pa.copy(); j = j.copy()
        pa[out] = pc - a
        j[out] = np.clip(np.floor(pa[out] * inv_h), 0, ncell - 1)
    u = pa * inv_h - j
    return j.astype(np.int64), u


def weights(ax, ay, x, y):
    """(cols [4, n], phi [4, n]) of points (x, y): the flat sample indices iy qx + ix and the bilinear weights."""
    x = np.asarray(x, dtype=np.float64).ravel(); y = np.asarray(y, dtype=np.float64).ravel()
    jx, u = _axis(x, *ax)
    jy, v = _axis(y, *ay)
    qx = ax[3]
    b = jy * qx + jx
    cols = np.stack([b, b + 1, b + qx, b + qx + 1])
    phi = np.stack([(1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v])
    return cols, phi


def _coef(th, method, gamma):
    if method < 10:
        return np.ones_like(th)
    gs = gamma * np.sin(th)
    c = np.cos(th)
    return np.sqrt(gs * gs + c * c)


def matrices(s_ray, last, ax, ay, line=None, kmax=4, method=6, gamma=1.0, rec_rows=None):
    """s_ray [rows, 6, R] (x, y, p_x, p_y, T, theta), last [R].  Returns dict: 'end' CSR [R, qy qx] (zero rows for rays past
    the record), and with a line 'line' CSR [kmax R, qy qx] (row c R + m: crossing c of ray m; zero past count) and 'count'."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    rec_rows = rows if rec_rows is None else int(rec_rows)
    last = np.asarray(last, dtype=np.int64)
    nz = ax[3] * ay[3]
    x = s_ray[:, 0, :].astype(np.float64); y = s_ray[:, 1, :].astype(np.float64); th = s_ray[:, 5, :].astype(np.float64)
    i = np.arange(rows)[:, None]
    ok = (i <= last[None, :]) & (last[None, :] < rec_rows)
    coef = _coef(th, method, gamma)
    dx = np.diff(x, axis=0); dy = np.diff(y, axis=0)
    L = np.zeros((rows + 1, R))
    L[1:rows] = np.sqrt(dx * dx + dy * dy)                  # L[i]: step i (rows i-1 -> i)
    L[1:rows][~ok[1:]] = 0.0
    cols, phi = weights(ax, ay, x, y)                        # [4, rows R]
    cols = cols.reshape(4, rows, R); phi = phi.reshape(4, rows, R)
    trap = np.where(ok, coef * (L[:rows] + L[1:]) * 0.5, 0.0)   # end weights (L past last is 0)

    def csr(rr, jj, ii, w, nrow):
        val = (phi[:, jj, ii] * w[None, :]).ravel()
        return sp.coo_matrix((val, (np.broadcast_to(rr, (4, len(rr))).ravel(), cols[:, jj, ii].ravel())),
                             shape=(nrow, nz)).tocsr()

    jj, ii = np.nonzero(ok)
    out = {"end": csr(ii, jj, ii, trap[jj, ii], R)}
    if line is None:
        return out
    count, cr = X.crossings(s_ray, last, line, kmax=kmax, rec_rows=rec_rows)
    out["count"] = count
    A, B, Cc = X.normalise(line)
    f = (A * x + B * y) - Cc
    hit = ((f[:-1] < 0.0) & (f[1:] >= 0.0)) | ((f[:-1] > 0.0) & (f[1:] <= 0.0))
    hit &= ok[1:]
    st, ray = np.nonzero(hit.T)                              # ray-major, steps in order
    ray, st = st, ray + 1
    idx = np.zeros(len(ray), dtype=np.int64)
    if len(ray):
        start = np.r_[0, np.nonzero(np.diff(ray))[0] + 1]
        idx = np.arange(len(ray)) - np.repeat(start, np.diff(np.r_[start, len(ray)]))
    keep = idx < kmax
    ray, st, idx = ray[keep], st[keep], idx[keep]
    tau = cr[idx, 5, ray] - (st - 1)
    t2 = tau * tau; t3 = t2 * tau
    h10 = (t3 - 2.0 * t2) + tau; h01 = 3.0 * t2 - 2.0 * t3; h11 = t3 - t2
    Li = L[st, ray]
    # rows 0 .. i-2: the trapezoid weights of the prefix
    n_pre = np.maximum(st - 1, 0)
    rr = np.repeat(idx * R + ray, n_pre)
    m_ = np.repeat(ray, n_pre)
    j_ = np.arange(n_pre.sum()) - np.repeat(np.cumsum(n_pre) - n_pre, n_pre)
    w_pre = coef[j_, m_] * (L[j_, m_] + L[j_ + 1, m_]) * 0.5
    w_a = coef[st - 1, ray] * (L[st - 1, ray] * 0.5 + Li * (0.5 * h01 + h10))
    w_b = coef[st, ray] * (Li * (0.5 * h01 + h11))
    r_all = np.r_[rr, idx * R + ray, idx * R + ray]
    j_all = np.r_[j_, st - 1, st]
    m_all = np.r_[m_, ray, ray]
    w_all = np.r_[w_pre, w_a, w_b]
    out["line"] = csr(r_all, j_all, m_all, w_all, kmax * R)
    out["crossings"] = cr
    return out


def perturb(M, dZ):
    """A dZ from matrices(): {'end': [R], 'line': [kmax, R] (NaN past count)}; rays past the record NaN at the end."""
    z = np.asarray(dZ, dtype=np.float64).ravel()
    R = M["end"].shape[0]
    d = {"end": M["end"] @ z}
    if "line" in M:
        ln = (M["line"] @ z).reshape(-1, R)
        c = M["count"]
        ln[np.arange(ln.shape[0])[:, None] >= np.maximum(c, 0)[None, :]] = np.nan
        d["line"] = ln
        d["end"][c < 0] = np.nan
    return d


def backproject(M, w_end=None, w_line=None):
    """A^T w from matrices(); NaN weights count as 0."""
    g = np.zeros(M["end"].shape[1])
    if w_end is not None:
        g += M["end"].T @ np.nan_to_num(np.asarray(w_end, dtype=np.float64), nan=0.0)
    if w_line is not None:
        g += M["line"].T @ np.nan_to_num(np.asarray(w_line, dtype=np.float64), nan=0.0).ravel()
    return g
