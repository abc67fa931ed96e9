"""Event location by grid search over traveltime tables, restated in numpy (include/rtmi.h, rtmi_locate; DESIGN.md section 29;
raytracing_amd/csrc/rt_locate.h).  Every product, sum and quotient is one fp64 operation in the order of the header, so the
device's results are compared with these bit for bit: the nodes are vectorised, the stations are a loop, r ascending.

    locate(T, t, w=None, need=None, grid=None) -> dict of arrays over the E events
    refine(win_obj, win_tau, ref, sw, ix, iy, grid) -> (x, y, t0, dx, dy, cov [3], refined), rt::locate_refine's twin
"""
import numpy as np


def event_maps(T, t, w=None, need=None):
    """One event: (ref, n, sw, tau, obj, cand) with the last five [ny, nx]; ref None when the event has no valid pick (then no
    node is a candidate and the map is the +inf of a node that is none)."""
    P = T.shape[0]
    valid = np.isfinite(t)
    if w is not None:
        valid &= np.isfinite(w) & (w > 0)
    shape = T.shape[1:]
    if not valid.any():
        return (None, np.zeros(shape, dtype=np.int32), np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape, np.inf),
                np.zeros(shape, dtype=bool))
    ref = t[np.flatnonzero(valid)[0]]
    n = np.zeros(shape, dtype=np.int32)
    sw = np.zeros(shape)
    sd = np.zeros(shape)
    with np.errstate(all="ignore"):
        for r in range(P):
            if not valid[r]:
                continue
            fin = np.isfinite(T[r])
            d = (t[r] - ref) - T[r]
            n += fin
            if w is None:
                sw = np.where(fin, sw + 1.0, sw)
                sd = np.where(fin, sd + d, sd)
            else:
                sw = np.where(fin, sw + w[r], sw)
                sd = np.where(fin, sd + w[r] * d, sd)
        nd = int(valid.sum()) if need is None else int(need)
        cand = n >= max(nd, 1)
        tau = np.where(cand, sd / sw, np.nan)
        q = np.zeros(shape)
        for r in range(P):
            if not valid[r]:
                continue
            fin = np.isfinite(T[r])
            d = (t[r] - ref) - T[r]
            u = d - tau
            q = np.where(fin, q + (u * u if w is None else (w[r] * u) * u), q)
        obj = np.where(cand, q / sw, np.inf)
    return ref, n, sw, tau, obj, cand


def refine(f, tau, ref, sw, ix, iy, grid):
    """rt::locate_refine: f, tau [3, 3] (row j = y, column i = x); grid = (gx0, gdx, nx, gy0, gdy, ny)"""
    gx0, gdx, _, gy0, gdy, _ = grid
    f = np.asarray(f, dtype=np.float64).reshape(3, 3)
    tau = np.asarray(tau, dtype=np.float64).reshape(3, 3)
    ref, sw, gx0, gdx, gy0, gdy = (np.float64(v) for v in (ref, sw, gx0, gdx, gy0, gdy))
    node = (gx0 + (np.float64(ix) + 0.0) * gdx, gy0 + (np.float64(iy) + 0.0) * gdy, ref + tau[1, 1], 0.0, 0.0, np.full(3, np.nan), 0)
    if not np.isfinite(f).all():
        return node
    F = lambda j, i: f[j + 1, i + 1]                                            # noqa: E731
    with np.errstate(all="ignore"):
        gx = (((F(-1, 1) - F(-1, -1)) + (F(0, 1) - F(0, -1))) + (F(1, 1) - F(1, -1))) / 6.0
        gy = (((F(1, -1) - F(-1, -1)) + (F(1, 0) - F(-1, 0))) + (F(1, 1) - F(-1, 1))) / 6.0
        cx = lambda j: (F(j, 1) - 2.0 * F(j, 0)) + F(j, -1)                     # noqa: E731
        cy = lambda i: (F(1, i) - 2.0 * F(0, i)) + F(-1, i)                     # noqa: E731
        hxx = ((cx(-1) + cx(0)) + cx(1)) / 3.0
        hyy = ((cy(-1) + cy(0)) + cy(1)) / 3.0
        hxy = (((F(1, 1) - F(1, -1)) - F(-1, 1)) + F(-1, -1)) / 4.0
        det = hxx * hyy - hxy * hxy
        if not (hxx > 0.0 and det > 0.0):
            return node
        dx = -((hyy * gx - hxy * gy) / det)
        dy = -((hxx * gy - hxy * gx) / det)
        if not (abs(dx) <= 1.0 and abs(dy) <= 1.0):
            return node
        x = gx0 + (np.float64(ix) + dx) * gdx
        y = gy0 + (np.float64(iy) + dy) * gdy
        t0 = ((ref + tau[1, 1]) + dx * ((tau[1, 2] - tau[1, 0]) / 2.0)) + dy * ((tau[2, 1] - tau[0, 1]) / 2.0)
        s = 2.0 / sw
        cov = np.array([(s * (hyy / det)) * (gdx * gdx), (s * (-hxy / det)) * (gdx * gdy), (s * (hxx / det)) * (gdy * gdy)])
    return x, y, t0, dx, dy, cov, 1


def locate(T, t, w=None, need=None, grid=None):
    """T [P, ny, nx], t [E, P], w [E, P] or None, need [E] or None.  Returns node, ix, iy, count, sw, obj, ref, t0 [E], win_obj,
    win_tau [E, 3, 3], maps [E, ny, nx], and with a grid also x, y, t0_refined, dx, dy, cov [E, 3], refined."""
    T = np.asarray(T, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    E = t.shape[0]
    _, ny, nx = T.shape
    out = {k: np.full(E, np.nan) for k in ("sw", "obj", "ref", "t0")}
    out.update({k: np.full(E, -1, dtype=np.int32) for k in ("node", "ix", "iy")})
    out["count"] = np.zeros(E, dtype=np.int32)
    out["win_obj"] = np.full((E, 3, 3), np.nan)
    out["win_tau"] = np.full((E, 3, 3), np.nan)
    out["maps"] = np.empty((E, ny, nx))
    if grid is not None:
        out.update({k: np.full(E, np.nan) for k in ("x", "y", "t0_refined", "dx", "dy")})
        out["cov"] = np.full((E, 3), np.nan)
        out["refined"] = np.zeros(E, dtype=np.int32)
    for e in range(E):
        ref, n, sw, tau, obj, cand = event_maps(T, t[e], None if w is None else np.asarray(w, dtype=np.float64)[e],
                                          None if need is None else need[e])
        out["maps"][e] = obj
        cand = np.flatnonzero(cand.ravel())
        if len(cand) == 0:
            continue
        key = obj.ravel()[cand]
        key = np.where(np.isnan(key), np.inf, key)
        node = int(cand[np.argmin(key)])                        # the first of the least: the least node index
        ix, iy = node % nx, node // nx
        out["node"][e], out["ix"][e], out["iy"][e] = node, ix, iy
        out["count"][e], out["sw"][e], out["obj"][e], out["ref"][e] = n[iy, ix], sw[iy, ix], obj[iy, ix], ref
        out["t0"][e] = ref + tau[iy, ix]
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                if 0 <= iy + j < ny and 0 <= ix + i < nx:
                    out["win_obj"][e, j + 1, i + 1] = obj[iy + j, ix + i]
                    out["win_tau"][e, j + 1, i + 1] = tau[iy + j, ix + i]
        if grid is not None:
            r = refine(out["win_obj"][e], out["win_tau"][e], ref, sw[iy, ix], ix, iy, grid)
            for k, v in zip(("x", "y", "t0_refined", "dx", "dy", "cov", "refined"), r):
                out[k][e] = v
    return out
