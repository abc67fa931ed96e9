"""The location pdf of a search's map, restated (include/rtmi.h, rtmi_locate_pdf and rtmi_locate_edt_pdf; DESIGN.md section 33;
raytracing_amd/csrc/rt_pdf.h).  The density is numpy on the whole map, one fp64 operation per step in the header's order (exp is
the library's own host entry, as in tests/edt_ref.py); the masses are integers and every sum over them is a sum of Python ints;
the per-event results are Python floats, one rounded operation per step, with math.sqrt and math.atan2 (libm's, as the
library's host code calls them).  int -> float is the nearest double, ties to even: the header's D().

    pdf(maps, best, params, grid) -> dict of arrays over the E events
        maps    [E, ny, nx] as locate_ref.locate / edt_ref.locate return them
        best    that same dict: node, and obj and sw (least squares) or value and count (EDT)
        params  dict(kind="l2" | "edt", sigma=, power=0, levels=(), u=None or [E, S], marginals=False)
        grid    (gx0, gdx, nx, gy0, gdy, ny)
"""
import math

import numpy as np

from raytracing_amd import rt_bench

CUT = -700.0
ONE = 1 << 30
BINS = 992


def density_l2(obj, obj0, sw0, sigma):
    s2 = np.float64(sigma) * np.float64(sigma)
    c = np.float64(0.5) / s2
    b = np.float64(sw0) * c
    with np.errstate(all="ignore"):
        a = obj - np.float64(obj0)
        z = -(a * b)
        ok = z >= CUT                                              # a NaN is not
        return np.where(ok, rt_bench.edt_exp(np.where(ok, z, 0.0)), 0.0)


def density_edt(value, value0, p):
    with np.errstate(all="ignore"):
        ok = (value >= 0.0) & (np.float64(value0) > 0.0)
        r = np.where(ok, value, 0.0) / (np.float64(value0) if value0 > 0.0 else np.float64(1.0))
        acc = r.copy()
        for bit in range(int(p).bit_length() - 2, -1, -1):
            acc = acc * acc
            if p >> bit & 1:
                acc = acc * r
    return np.where(ok, acc, 0.0)


def masses(rho):
    """m = trunc(rho 2^30) as int64 (rho is in [0, 1])"""
    return np.floor(rho * float(ONE)).astype(np.int64)


def bin_of(m):
    b = m.bit_length() - 1
    sub = (m >> (b - 5) if b >= 5 else m << (5 - b)) & 31
    return 32 * b + sub


def bin_edge(k):
    b, top = k // 32, 32 + k % 32
    return top << (b - 5) if b >= 5 else top >> (5 - b)


def sums(m, ix0, iy0):
    """the integer sums of one event's masses m [ny, nx] about node (ix0, iy0), and the histogram"""
    ny, nx = m.shape
    mo = m.astype(object)
    di = (np.arange(nx) - ix0).astype(object)[None, :]
    dj = (np.arange(ny) - iy0).astype(object)[:, None]
    rim = np.zeros((ny, nx), dtype=bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    s = {"Z": int(mo.sum()), "Sx": int((mo * di).sum()), "Sy": int((mo * dj).sum()), "Sxx": int((mo * di * di).sum()),
         "Sxy": int((mo * di * dj).sum()), "Syy": int((mo * dj * dj).sum()), "rim": int(mo[rim].sum()), "nz": int((m > 0).sum())}
    count, mass = [0] * BINS, [0] * BINS
    for v in m[m > 0].tolist():
        k = bin_of(v)
        count[k] += 1
        mass[k] += v
    return s, count, mass


def level_target(c, Z):
    Zd = float(Z)
    want = math.ceil(float(c) * Zd)
    return Z if want >= Zd else int(want)


def finalize(s, count, mass, ix0, iy0, grid, levels):
    """rt::pdf_finalize: a dict of floats and ints; an event without a pdf has counts 0 and NaN"""
    nan = float("nan")
    L = len(levels)
    o = {"mean_x": nan, "mean_y": nan, "cov": [nan] * 3, "ellipse": [nan] * 3, "area": nan, "rim_fraction": nan, "nz": 0, "mass": 0,
         "level_count": [0] * L, "level_area": [nan] * L, "level_fraction": [nan] * L, "level_rho": [nan] * L}
    Z = s["Z"]
    if Z == 0:
        return o
    gx0, gdx, _, gy0, gdy, _ = (float(v) for v in grid)
    Zd = float(Z)
    ax, ay = float(s["Sx"]) / Zd, float(s["Sy"]) / Zd
    o["mean_x"] = (gx0 + float(ix0) * gdx) + ax * gdx
    o["mean_y"] = (gy0 + float(iy0) * gdy) + ay * gdy
    cxx = (float(s["Sxx"]) / Zd - ax * ax) * (gdx * gdx)
    cxy = (float(s["Sxy"]) / Zd - ax * ay) * (gdx * gdy)
    cyy = (float(s["Syy"]) / Zd - ay * ay) * (gdy * gdy)
    o["cov"] = [cxx, cxy, cyy]
    h, d = (cxx + cyy) * 0.5, (cxx - cyy) * 0.5
    r = math.sqrt(d * d + cxy * cxy)
    l1, l2 = h + r, h - r
    o["ellipse"] = [math.sqrt(l1) if l1 >= 0.0 else nan, math.sqrt(l2 if l2 > 0.0 else 0.0), 0.5 * math.atan2(cxy, d)]
    cell = gdx * gdy
    o["area"] = (Zd / float(ONE)) * cell
    o["rim_fraction"] = float(s["rim"]) / Zd
    o["nz"], o["mass"] = s["nz"], Z
    for k, c in enumerate(levels):
        tq = level_target(c, Z)
        C = M = 0
        B = BINS - 1
        while True:
            C += count[B]
            M += mass[B]
            if M >= tq or B == 0:
                break
            B -= 1
        o["level_count"][k] = C
        o["level_area"][k] = float(C) * cell
        o["level_fraction"][k] = float(M) / Zd
        o["level_rho"][k] = float(bin_edge(B)) / float(ONE)
    return o


def sample_quantum(u, Z):
    v = (float(u) if u > 0.0 else 0.0) * float(Z)
    if v >= float(Z):
        return Z - 1
    return min(int(v), Z - 1)


def sample_nodes(m, u):
    """the least node, in node order, whose inclusive cumulative mass exceeds q(u), for every u; -1 without mass"""
    flat = [int(v) for v in m.ravel().tolist()]
    Z = sum(flat)
    if Z == 0:
        return np.full(len(u), -1, dtype=np.int32)
    cum, c = [], 0
    for v in flat:
        c += v
        cum.append(c)
    out = np.empty(len(u), dtype=np.int32)
    for k, uk in enumerate(u):
        q = sample_quantum(uk, Z)
        lo, hi = 0, len(cum) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if cum[mid] > q:
                hi = mid
            else:
                lo = mid + 1
        out[k] = lo
    return out


def event_masses(maps_e, best, e, params):
    """m [ny, nx] of event e; all zero where the event has no best node"""
    if best["node"][e] < 0:
        return np.zeros(maps_e.shape, dtype=np.int64)
    if params["kind"] == "l2":
        rho = density_l2(maps_e, best["obj"][e], best["sw"][e], params["sigma"])
    else:
        p = int(params.get("power", 0)) or max(int(best["count"][e]), 1)
        rho = density_edt(maps_e, best["value"][e], p)
    return masses(rho)


def pdf(maps, best, params, grid):
    maps = np.asarray(maps, dtype=np.float64)
    E, ny, nx = maps.shape
    levels = tuple(params.get("levels", ()))
    L = len(levels)
    u = params.get("u")
    out = {k: np.full(E, np.nan) for k in ("mean_x", "mean_y", "area", "rim_fraction")}
    out.update(pdf_cov=np.full((E, 2, 2), np.nan), ellipse=np.full((E, 3), np.nan), nz=np.zeros(E, dtype=np.int64),
               mass=np.zeros(E, dtype=np.int64), level_count=np.zeros((E, L), dtype=np.int64), level_area=np.full((E, L), np.nan),
               level_fraction=np.full((E, L), np.nan), level_rho=np.full((E, L), np.nan), m=np.zeros((E, ny, nx), dtype=np.int64),
               sums=[], hist=[])
    if params.get("marginals"):
        out.update(mx=np.full((E, nx), np.nan), my=np.full((E, ny), np.nan))
    if u is not None:
        out["sample_node"] = np.full(np.shape(u), -1, dtype=np.int32)
    for e in range(E):
        m = event_masses(maps[e], best, e, params)
        out["m"][e] = m
        node = int(best["node"][e])
        ix0, iy0 = (node % nx, node // nx) if node >= 0 else (0, 0)
        s, count, mass = sums(m, ix0, iy0)
        out["sums"].append(s)
        out["hist"].append((count, mass))
        o = finalize(s, count, mass, ix0, iy0, grid, levels)
        for k in ("mean_x", "mean_y", "area", "rim_fraction", "nz", "mass", "ellipse", "level_count", "level_area", "level_fraction",
                  "level_rho"):
            out[k][e] = o[k]
        c = o["cov"]
        out["pdf_cov"][e] = [[c[0], c[1]], [c[1], c[2]]]
        Z = s["Z"]
        if params.get("marginals") and Z:
            mo = m.astype(object)
            out["mx"][e] = [float(int(v)) / float(Z) for v in mo.sum(axis=0)]
            out["my"][e] = [float(int(v)) / float(Z) for v in mo.sum(axis=1)]
        if u is not None:
            out["sample_node"][e] = sample_nodes(m, np.asarray(u)[e])
    return out
