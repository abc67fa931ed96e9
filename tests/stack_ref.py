"""Pick-free detection and location by stacking station traces, restated in numpy (include/rtmi.h, rtmi_locate_stack; DESIGN.md
section 30; raytracing_amd/csrc/rt_stack.h).  Every product, sum and quotient is one fp64 operation in the order of the header, so
the device's results are compared with these bit for bit: nodes and scan indices are vectorised, the stations are a loop, r
ascending.

    volume(T, c, ct0, cdt, o0, od, M, w=None, need=0) -> S [M, ny, nx], n [M, ny, nx] (contributing stations), cand
    project(S, cand) -> peak [M], peak_node [M], best [ny, nx], best_m [ny, nx]
    select(peak, peak_node, threshold, min_sep, max_events) -> (the scan indices taken, in order; whether eligible ones remained)
    refine_time(sm, s0, sp, o, od) -> (t0, dm, accepted)
    stack(T, c, ..., grid=None) -> dict with all of the above, the events, their windows and refinements
"""
import numpy as np

import locate_ref


def volume(T, c, ct0, cdt, o0, od, M, w=None, need=0):
    T = np.asarray(T, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    P, nt = c.shape
    ct0, o0, od = np.float64(ct0), np.float64(o0), np.float64(od)
    inv = np.float64(1.0) / np.float64(cdt)
    valid = np.ones(P, dtype=bool) if w is None else np.isfinite(w) & (np.asarray(w) > 0)
    o = o0 + np.arange(M, dtype=np.float64) * od
    shape = (M,) + T.shape[1:]
    n = np.zeros(shape, dtype=np.int32)
    s, sw = np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        for r in range(P):
            if not valid[r]:
                continue
            f = ((o[:, None, None] + T[r][None]) - ct0) * inv
            inside = (f >= 0.0) & (f < nt - 1)                     # no NaN and no infinite T passes
            jf = np.floor(f)
            j = np.where(inside, jf, 0.0).astype(np.int64)
            c0, c1 = c[r][j], c[r][j + 1]
            ok = inside & np.isfinite(c0) & np.isfinite(c1)
            a = f - jf
            v = (1.0 - a) * c0 + a * c1
            n += ok
            if w is None:
                s = np.where(ok, s + v, s)
            else:
                sw = np.where(ok, sw + w[r], sw)
                s = np.where(ok, s + w[r] * v, s)
        needv = max(int(need) if need else int(valid.sum()), 1)
        cand = n >= needv
        S = np.where(cand, s / (n.astype(np.float64) if w is None else sw), -np.inf)
    return S, n, cand


def project(S, cand):
    M, ny, nx = S.shape
    key = np.where(cand & ~np.isnan(S), S, -np.inf).reshape(M, ny * nx)     # a NaN counts as -inf; so does a node that is none
    C = cand.reshape(M, ny * nx)
    peak = key.max(axis=1)
    hit = C & (key == peak[:, None])
    peak_node = np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int32)   # argmax of booleans: the first True
    best = key.max(axis=0)
    hit = C & (key == best[None, :])
    best_m = np.where(hit.any(axis=0), hit.argmax(axis=0), -1).astype(np.int32)
    return peak, peak_node, best.reshape(ny, nx), best_m.reshape(ny, nx)


def select(peak, peak_node, threshold, min_sep, max_events):
    """the rule as the header states it, one event per turn of the loop"""
    M = len(peak)
    free = (peak >= threshold) & (np.asarray(peak_node) >= 0)
    taken = []
    while free.any():
        if len(taken) >= max_events:
            return taken, True
        idx = np.flatnonzero(free)
        m = int(idx[np.argmax(peak[idx])])                          # the first of the greatest: the least m
        taken.append(m)
        free[max(m - min_sep, 0):min(m + min_sep, M - 1) + 1] = False
    return taken, False


def refine_time(sm, s0, sp, o, od):
    sm, s0, sp, o, od = (np.float64(v) for v in (sm, s0, sp, o, od))
    if not (np.isfinite(sm) and np.isfinite(s0) and np.isfinite(sp)):
        return o, np.float64(0.0), 0
    with np.errstate(all="ignore"):
        den = (sm - 2.0 * s0) + sp
        if not den < 0.0:
            return o, np.float64(0.0), 0
        dm = ((sm - sp) / 2.0) / den
    if not abs(dm) <= 1.0:
        return o, np.float64(0.0), 0
    return o + dm * od, dm, 1


def refine(win, o, od, ix, iy, grid):
    """rt::stack_refine: win [3, 3, 3] -> (x, y, t0, dx, dy, dm, refined)"""
    win = np.asarray(win, dtype=np.float64).reshape(3, 3, 3)
    x, y, _, dx, dy, _, space = locate_ref.refine(-win[1], np.zeros((3, 3)), 0.0, 1.0, ix, iy, grid)
    t0, dm, time = refine_time(win[0, 1, 1], win[1, 1, 1], win[2, 1, 1], o, od)
    return x, y, t0, dx, dy, dm, int(space) | (int(time) << 1)


def window(S, m, ix, iy):
    M, ny, nx = S.shape
    win = np.full((3, 3, 3), np.nan)
    for d in (-1, 0, 1):
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                if 0 <= m + d < M and 0 <= iy + j < ny and 0 <= ix + i < nx:
                    win[d + 1, j + 1, i + 1] = S[m + d, iy + j, ix + i]
    return win


def stack(T, c, ct0, cdt, o0, od, M, w=None, need=0, threshold=np.inf, min_sep=0, max_events=0, grid=None):
    T = np.asarray(T, dtype=np.float64)
    _, ny, nx = T.shape
    S, n, cand = volume(T, c, ct0, cdt, o0, od, M, w, need)
    peak, peak_node, best, best_m = project(S, cand)
    taken, remained = select(peak, peak_node, threshold, min_sep, max_events)
    K = len(taken)
    out = {"volume": S, "n": n, "peak": peak, "peak_node": peak_node, "best": best, "best_m": best_m, "contributing": int(n.sum()),
           "truncated": bool(remained), "m": np.array(taken, dtype=np.int32), "node": peak_node[taken].astype(np.int32)}
    out["ix"], out["iy"] = (out["node"] % nx).astype(np.int32), (out["node"] // nx).astype(np.int32)
    out["count"] = np.array([n[m, iy, ix] for m, ix, iy in zip(taken, out["ix"], out["iy"])], dtype=np.int32)
    out["value"] = np.array([S[m, iy, ix] for m, ix, iy in zip(taken, out["ix"], out["iy"])], dtype=np.float64)
    out["t0_node"] = np.float64(o0) + out["m"].astype(np.float64) * np.float64(od)
    out["win"] = np.full((K, 3, 3, 3), np.nan)
    for k in range(K):
        out["win"][k] = window(S, taken[k], out["ix"][k], out["iy"][k])
    if grid is not None:
        cols = [refine(out["win"][k], out["t0_node"][k], od, out["ix"][k], out["iy"][k], grid) for k in range(K)]
        for q, name in enumerate(("x", "y", "t0", "dx", "dy", "dm")):
            out[name] = np.array([col[q] for col in cols], dtype=np.float64)
        out["refined"] = np.array([col[6] for col in cols], dtype=np.int32)
    return out
