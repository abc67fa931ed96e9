"""numpy restatement of rtmi_arrival_grid (include/rtmi.h; raytracing_amd/csrc/ttgrid.hip): the candidates of
rtmi_first_arrival_grid -- every (triangle, node) pair its cell, gap and fill rules accept with 0 <= T < inf, gathered here once
more with tests/ttgrid_ref.py's element functions and in its operation order -- sorted per node by (bits of c, key), the first K
of them kept.  c = T by time; c = nn * |Jn|, the product under G's square root, by amplitude (+inf where that is not >= 0 and
< inf).  Test infrastructure.  Also the lens bed: the one field, fan and grid on which traced rays fold into a triplication."""
import numpy as np

from ttgrid_ref import AMPLITUDE_FIELDS, FIELDS, _node_hi, _node_lo, defaults, edge, interp, top_left, wrap

BY_TIME, BY_AMPLITUDE = "time", "amplitude"


def candidates(x, y, T, theta, last, grid, fan_size=None, theta0=None, max_gap=None, max_dtheta=None, rec_rows=None,
               amplitude=None, chunk=256):
    """Arguments as ttgrid_ref.first_arrival_grid.  -> (S, dict of flat arrays over all candidates: node (of [S, ny, nx]), key,
    the columns T theta0 theta ray step, and with amplitude = (J, kmah, n) also J G kmah and nJ = nn * |Jn|)."""
    x, y, T, th = (np.asarray(a).astype(np.float64) for a in (x, y, T, theta))
    rows, R = x.shape
    rec_rows = rows if rec_rows is None else int(rec_rows)
    M = R if fan_size is None else int(fan_size)
    S = R // M
    gx0, gdx, nx, gy0, gdy, ny = grid
    nx, ny = int(nx), int(ny)
    gap, dth = defaults(grid, max_gap, max_dtheta)
    th0 = th[0] if theta0 is None else np.asarray(theta0, dtype=np.float64)
    le = np.minimum(np.asarray(last, dtype=np.int64), rec_rows - 1)
    s_of = np.repeat(np.arange(S), M - 1)
    m_of = np.tile(np.arange(M - 1), S)
    o0 = s_of * M + m_of
    L = np.minimum(le[o0], le[o0 + 1])
    per = nx * ny
    names = FIELDS + (AMPLITUDE_FIELDS + ("nJ",) if amplitude is not None else ())
    cand = {k: [] for k in ("node", "key") + names}
    if amplitude is not None:
        Ja, Ka, Na = (np.asarray(a) for a in amplitude)
    for i0 in range(0, int(L.max(initial=0)), chunk):
        i1 = min(i0 + chunk, int(L.max()))
        ii, pp = np.nonzero(np.arange(i0, i1)[:, None] < L[None, :])
        i = ii + i0
        o, s, m = o0[pp], s_of[pp], m_of[pp]
        cr = [(i, o), (i, o + 1), (i + 1, o), (i + 1, o + 1)]          # A B C D
        X = [x[r, k] for r, k in cr]; Y = [y[r, k] for r, k in cr]
        Tc = [T[r, k] for r, k in cr]; Th = [th[r, k] for r, k in cr]
        with np.errstate(invalid="ignore"):
            d0 = np.sqrt((X[1] - X[0]) * (X[1] - X[0]) + (Y[1] - Y[0]) * (Y[1] - Y[0]))
            d1 = np.sqrt((X[3] - X[2]) * (X[3] - X[2]) + (Y[3] - Y[2]) * (Y[3] - Y[2]))
            ok = (d0 <= gap) & (d1 <= gap) & (np.abs(wrap(Th[1] - Th[0])) <= dth) & (np.abs(wrap(Th[3] - Th[2])) <= dth)
        thu = [Th[0] + wrap(Th[q] - Th[0]) for q in range(4)]
        t0c = [th0[o], th0[o + 1], th0[o], th0[o + 1]]
        fr, fs = [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]
        if amplitude is not None:
            Jc = [Ja[r, k].astype(np.float64) for r, k in cr]
            Kc = [Ka[r, k] for r, k in cr]
            Nc = [Na[r, k].astype(np.float64) for r, k in cr]
        for half in (0, 1):
            c = np.array([0, 2 if half else 3, 3 if half else 1])     # A D B, A C D
            a = edge(X[c[0]], Y[c[0]], X[c[1]], Y[c[1]], X[c[2]], Y[c[2]])
            keep = ok & (a != 0.0) & (a == a)
            fold = keep & (a < 0.0)
            sel = np.nonzero(keep)[0]
            ci = np.tile(c, (len(sel), 1))
            ci[fold[sel]] = ci[fold[sel]][:, [0, 2, 1]]                  # re-oriented counter-clockwise
            pick = lambda arrs: [np.choose(ci[:, q], [v[sel] for v in arrs]) for q in range(3)]   # noqa: E731
            vx, vy = pick(X), pick(Y)
            xmin = np.fmin(np.fmin(vx[0], vx[1]), vx[2]); xmax = np.fmax(np.fmax(vx[0], vx[1]), vx[2])
            ymin = np.fmin(np.fmin(vy[0], vy[1]), vy[2]); ymax = np.fmax(np.fmax(vy[0], vy[1]), vy[2])
            xa, xb = _node_lo(xmin, gx0, gdx, nx), _node_hi(xmax, gx0, gdx, nx)
            ya, yb = _node_lo(ymin, gy0, gdy, ny), _node_hi(ymax, gy0, gdy, ny)
            wx, wy = np.maximum(xb - xa + 1, 0), np.maximum(yb - ya + 1, 0)
            n = wx * wy
            if n.sum() == 0:
                continue
            t = np.repeat(np.arange(len(sel)), n)
            off = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
            ix = xa[t] + off % wx[t]; iy = ya[t] + off // wx[t]
            px = gx0 + ix.astype(np.float64) * gdx; py = gy0 + iy.astype(np.float64) * gdy
            V = [(vx[q][t], vy[q][t]) for q in range(3)]
            inb = (px >= xmin[t]) & (px <= xmax[t]) & (py >= ymin[t]) & (py <= ymax[t])
            w0 = edge(*V[1], *V[2], px, py); w1 = edge(*V[2], *V[0], px, py); w2 = edge(*V[0], *V[1], px, py)
            ins = inb & ((w0 > 0.0) | ((w0 == 0.0) & top_left(*V[1], *V[2])))
            ins &= (w1 > 0.0) | ((w1 == 0.0) & top_left(*V[2], *V[0]))
            ins &= (w2 > 0.0) | ((w2 == 0.0) & top_left(*V[0], *V[1]))
            t, w0, w1, w2, ix, iy = t[ins], w0[ins], w1[ins], w2[ins], ix[ins], iy[ins]
            cc = ci[t]
            g = lambda arrs: [np.choose(cc[:, q], [v[sel][t] if np.ndim(v) else np.full(len(t), v) for v in arrs])  # noqa: E731
                              for q in range(3)]
            with np.errstate(invalid="ignore", divide="ignore"):
                tv = interp(w0, w1, w2, *g(Tc))
            good = (tv >= 0.0) & (tv < np.inf)
            tt = sel[t]
            cand["node"].append((s[tt] * per + iy * nx + ix)[good])
            cand["key"].append(((m[tt] * rec_rows + i[tt]) * 2 + half)[good].astype(np.uint64))
            with np.errstate(invalid="ignore", divide="ignore"):
                vals = {"T": tv, "theta0": interp(w0, w1, w2, *g(t0c)), "theta": interp(w0, w1, w2, *g(thu)),
                        "ray": m[tt].astype(np.float64) + interp(w0, w1, w2, *g(fr)),
                        "step": i[tt].astype(np.float64) + interp(w0, w1, w2, *g(fs))}
                if amplitude is not None:
                    Jn = interp(w0, w1, w2, *g(Jc))
                    nn = interp(w0, w1, w2, *g(Nc))
                    kq = np.where(w0 >= w1, np.where(w0 >= w2, 0, 2), np.where(w1 >= w2, 1, 2))
                    nJ = nn * np.abs(Jn)
                    vals.update(J=Jn, G=1.0 / np.sqrt(nJ), nJ=nJ,
                                kmah=np.choose(np.choose(kq, cc.T), [k[sel][t] for k in Kc]).astype(np.float64))
            for k in names:
                cand[k].append(vals[k][good])
    cat = {k: (np.concatenate(v) if v else np.empty(0)) for k, v in cand.items()}
    cat["node"] = cat["node"].astype(np.int64)
    cat["key"] = cat["key"].astype(np.uint64)
    return S, cat


def arrival_grid(x, y, T, theta, last, grid, arrivals=1, order=BY_TIME, amplitude=None, columns=None, **kw):
    """The K = arrivals first candidates of every node by (bits of c, key).  amplitude = (J, kmah, n) [rows, R]: needed by
    order "amplitude"; the J G kmah columns are returned when columns is true (default: whenever amplitude is given).
    -> dict of [S, K, ny, nx] arrays (NaN past a node's count), 'key' (int64, -1 past the count), 'c' (the criterion), and count
    [S, ny, nx]."""
    K = int(arrivals)
    S, cat = candidates(x, y, T, theta, last, grid, amplitude=amplitude, **kw)
    nx, ny = int(grid[2]), int(grid[5])
    per = nx * ny
    node = cat["node"]
    if order == BY_AMPLITUDE:
        ok = (cat["nJ"] >= 0.0) & (cat["nJ"] < np.inf)
        c = np.where(ok, cat["nJ"], np.inf)
    else:
        c = cat["T"]
    names = FIELDS + (AMPLITUDE_FIELDS if (amplitude is not None if columns is None else columns) else ())
    count = np.bincount(node, minlength=S * per).astype(np.int32)
    res = {k: np.full((S * per, K), np.nan) for k in names + ("c",)}
    key = np.full((S * per, K), -1, dtype=np.int64)
    if len(node):
        order_ = np.lexsort((cat["key"], np.ascontiguousarray(c).view(np.uint64), node))
        sn = node[order_]
        rank = np.arange(len(sn)) - np.searchsorted(sn, sn, side="left")        # place within the node's sorted run
        keep = rank < K
        at, rk, src = sn[keep], rank[keep], order_[keep]
        for k in names:
            res[k][at, rk] = cat[k][src]
        res["c"][at, rk] = c[src]
        key[at, rk] = cat["key"][src].astype(np.int64)
    out = {k: v.reshape(S, ny, nx, K).transpose(0, 3, 1, 2).copy() for k, v in res.items()}
    out["key"] = key.reshape(S, ny, nx, K).transpose(0, 3, 1, 2).copy()
    out["count"] = count.reshape(S, ny, nx)
    return out


def from_record(s_ray, last, grid, **kw):
    """arrival_grid on a record s_ray [rows, 6, R] (columns x, y, p_x, p_y, T, theta) as Batch.rows() returns it"""
    s_ray = np.asarray(s_ray)
    return arrival_grid(s_ray[:, 0], s_ray[:, 1], s_ray[:, 4], s_ray[:, 5], last, grid, **kw)


# ---------------------------------------------------------------- the lens bed
# A slow Gaussian lens in front of a point source: behind it the fan folds, and between the two caustics three branches cover a
# node (count 3).  The first arrival there skirts the lens; the strongest is the branch through it (kmah 1).
LENS_H = 0.05
LENS_BOX = (0.0, 4.0, -1.5, 1.5)
LENS_SOURCE = (0.2, 0.0)
LENS_THETA = np.linspace(-0.6, 0.6, 256)
LENS_STEP, LENS_MAX_SIZE, LENS_METHOD = 0.01, 600, 6
LENS_GRID = (0.05, 0.05, 79, -1.45, 0.05, 59)


def lens_samples():
    """-> x, y, Z [len(y), len(x)], h: the field's samples (n = 1 + 0.5 exp(-r^2 / (2 0.3^2)) about (1.5, 0))"""
    x = np.arange(0, 4 + 1e-9, LENS_H)
    y = np.arange(-1.5, 1.5 + 1e-9, LENS_H)
    X, Y = np.meshgrid(x, y)
    return x, y, 1 + 0.5 * np.exp(-((X - 1.5) ** 2 + Y ** 2) / (2 * 0.3 ** 2)), LENS_H


# ---------------------------------------------------------------- synthetic rows
def cusp_rows(M=401, rows=101):
    """test_ttgrid_ref.fold_rows' cusp, restated: rays x = u (1 - 2 t) + t u^3, y = t, u in [-1.5, 1.5]; at x = 0, t > 1/2 the
    branches u = 0 and +-sqrt((2t - 1) / t).  T = t - 0.05 u; J = dx/du = (1 - 2t) + 3 t u^2; n = 1; kmah 1 where J < 0."""
    u = np.linspace(-1.5, 1.5, M)
    t = np.linspace(0.0, 1.0, rows)
    U, Tt = u[None, :], t[:, None]
    x = U * (1 - 2 * Tt) + Tt * U ** 3
    y = np.broadcast_to(Tt, x.shape).astype(np.float64)
    J = (1 - 2 * Tt) + 3 * Tt * U ** 2
    return dict(x=x, y=y, T=Tt - 0.05 * U, theta=np.full(x.shape, np.pi / 2), last=np.full(M, rows - 1), theta0=u,
                amplitude=(J, (J < 0).astype(np.int32), np.ones(x.shape)))


def accordion_rows(M=41, legs=9, per_leg=4):
    """9 sheets over one strip: rays x = u, y a zigzag of 9 legs in t between 0 and 1, T = t.  Every node with 0 < y < 1 inside the
    fan is covered once per leg.  The sheets alternate in orientation (every other leg is folded)."""
    u = np.linspace(0.0, 1.0, M)
    rows = legs * per_leg + 1
    t = np.arange(rows) / per_leg                                   # leg index + fraction
    z = np.where(np.floor(t) % 2 == 0, t - np.floor(t), 1.0 - (t - np.floor(t)))
    z[-1] = 1.0 if legs % 2 else 0.0
    x = np.broadcast_to(u[None, :], (rows, M)).astype(np.float64)
    y = np.broadcast_to(z[:, None], (rows, M)).astype(np.float64)
    T = np.broadcast_to(t[:, None], (rows, M)).astype(np.float64)
    return dict(x=x, y=y, T=T, theta=np.full(x.shape, np.pi / 2), last=np.full(M, rows - 1), theta0=u)
