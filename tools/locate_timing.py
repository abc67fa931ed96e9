#!/usr/bin/env python3
"""Event location by grid search against the same objective in plain torch, in one process: the search
kernel k_locate on the stock 737 x 539 grid (the vert_heterogeneous field's samples) with P = 32 tables, for E in {64, 1024,
4096} events, warmed, alternating, medians of --reps device times with min and max.

The yardstick exists without the library: broadcast tensor ops on the device, d = (t - ref)[:, :, None] - T[None], tau the mean
over the stations, obj the mean of (d - tau)^2, argmin over the nodes, chunked over the events to fit memory (--torch-chunk
events at a time, three [chunk, P, nodes] fp64 temporaries); timed with torch events around the whole loop.  Its node choices
are compared with the kernel's.  The rule is DESIGN.md section 24's: the kernel is accepted where its series lies below torch's
by more than the spread of the two.

Also printed: triples per second, and the two floors of the kernel -- the table bytes one pass over every (tile, chunk) block
must bring in over 6 TB/s, and the vector instructions per triple (counted in the ISA) at the chip's
issue rate.

    python tools/locate_timing.py [--events 64 1024 4096] [--tables 32] [--reps 5] [--weights] [--missing SHARE] [--out FILE.json]

--stack M [M ...] times the pick-free search instead: k_stack on the same grid and tables with traces of
8192 samples, a tenth of them NaN, for the scan lengths given, without and with weights, against the same S, peak and best in
plain torch (broadcast, gather, chunked over the scan), with the kernel's two floors: fp64 issue and gathered bytes.

    python tools/locate_timing.py --stack 256 4096 [--tables 32] [--reps 5] [--torch-chunk 8] [--out FILE.json]

--edt times the search by equal differential time instead: k_edt on the same grid and tables for the event
counts given (default 64 and 1024), without and with weights, and once more without weights with a tenth of the picks missing,
against the same objective in plain torch: per event the differences of all station pairs broadcast over the nodes, exp, the sum
over the pairs and argmax, one event at a time (five [pairs, nodes] fp64 temporaries of 1.6 GB at P = 32).  Pairs per second and the
kernel's fp64 issue floor are printed with it.

    python tools/locate_timing.py --edt [--events 64 1024] [--tables 32] [--reps 5] [--sigma 0.01] [--out FILE.json]

--pdf [--edt] times the location pdf of either search instead: Locator.pdf_device with two levels, both
marginals and --samples samples per event, for the event counts given (default 64 and 1024), against the same statistics in plain
torch on the device from the maps that locate_device(maps=True) / locate_edt_device(maps=True) return, which exists without the
pdf entries: exp (or the power), sums for the moments and the marginals, a sort and a cumulative sum for the regions,
searchsorted on a cumulative sum for the samples, --torch-chunk times 8 events at a time.  Both are timed as wall time between
two idle devices, since both do host work.  Also printed: the bare search without maps, what the pdf kernels add to it (their
own device time and the difference of the calls' device times), and their floor, one read of the maps at 6 TB/s.

    python tools/locate_timing.py --pdf [--edt] [--events 64 1024] [--tables 32] [--reps 5] [--pdf-sigma 0.05] [--samples 256]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.0e12                        # bytes per second
SIMDS, CLOCK = 1024, 2.4e9          # 256 CUs of 4 SIMDs; the clock the floor assumes (the chip holds less under load)
F64_OPS = {False: 6, True: 9}       # fp64 vector instructions per triple in k_locate's two loops where a chunk has all its picks,
                                    # without and with weights, read off the ISA (make asm UNIT=locate.hip); nothing else per triple
F64_CYCLES = 4                      # cycles a wave's fp64 add or multiply holds its SIMD: 16 lanes per cycle
CHUNK, TILE = 16, 256               # locate.hip's kChunk and kTile


def series(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def problem(P, E, seed=0):
    """a constant medium on the stock grid: the times do not depend on the values, the node choices do"""
    nx, ny = 737, 539
    grid = (-5.0, 13.0 / (nx - 1), nx, -5.5, 9.5 / (ny - 1), ny)
    rng = np.random.default_rng(seed)
    X, Y = grid[0] + grid[1] * np.arange(nx), grid[3] + grid[4] * np.arange(ny)
    sx, sy = rng.uniform(-6.0, 9.0, P), rng.uniform(-6.5, 5.0, P)
    T = (1.0 / 14.0) * np.hypot(X[None, None, :] - sx[:, None, None], Y[None, :, None] - sy[:, None, None])
    ex, ey = rng.uniform(X[0], X[-1], E), rng.uniform(Y[0], Y[-1], E)
    t = rng.uniform(0.0, 60.0, E)[:, None] + (1.0 / 14.0) * np.hypot(ex[:, None] - sx[None, :], ey[:, None] - sy[None, :])
    t += 1e-3 * rng.standard_normal(t.shape)
    return grid, T, t


def torch_locate(torch, Td, td, wd, chunk):
    """the yardstick: (nodes [E], device ms)"""
    P = Td.shape[0]
    Tf = Td.reshape(1, P, -1)
    nodes = torch.empty(td.shape[0], dtype=torch.int64, device=td.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for e0 in range(0, td.shape[0], chunk):
        tr = td[e0:e0 + chunk] - td[e0:e0 + chunk, :1]
        d = tr[:, :, None] - Tf
        if wd is None and torch.isnan(tr).any():                  # missing picks: weights of 0 and 1
            wd_ = torch.isfinite(td).to(torch.float64)
            d = torch.nan_to_num(d)
            w = wd_[e0:e0 + chunk, :, None]
            sw = w.sum(dim=1, keepdim=True)
            tau = (w * d).sum(dim=1, keepdim=True) / sw
            obj = (w * (d - tau) ** 2).sum(dim=1) / sw[:, 0]
        elif wd is None:
            tau = d.mean(dim=1, keepdim=True)
            obj = ((d - tau) ** 2).mean(dim=1)
        else:
            w = wd[e0:e0 + chunk, :, None]
            sw = w.sum(dim=1, keepdim=True)
            tau = (w * d).sum(dim=1, keepdim=True) / sw
            obj = (w * (d - tau) ** 2).sum(dim=1) / sw[:, 0]
        nodes[e0:e0 + chunk] = obj.argmin(dim=1)
    b.record()
    torch.cuda.synchronize()
    return nodes.cpu().numpy(), a.elapsed_time(b)


STACK_F64 = {False: 15, True: 17}   # fp64-rate vector instructions per triple in k_stack's station loop, without and with weights,
                                    # read off the ISA (make asm UNIT=stack.hip)
STACK_GATHER = 16                   # bytes a triple gathers from the traces: samples j and j + 1
L2_BYTES_PER_S = 256 * 64 * 2.4e9   # 64 bytes per CU and cycle from the vector L1s, the most the gathers can be served at


def torch_stack(torch, Td, cd, wd, o, ct0, inv, need, chunk):
    """the yardstick of --stack: S by broadcast ops and gather, chunked over m -> (peak [M], best [nodes], device ms)"""
    P, nt = cd.shape
    Tf = Td.reshape(1, P, -1)
    M = o.shape[0]
    peak = torch.empty(M, dtype=torch.float64, device=Td.device)
    best = torch.full((Tf.shape[2],), -np.inf, dtype=torch.float64, device=Td.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for m0 in range(0, M, chunk):
        f = ((o[m0:m0 + chunk, None, None] + Tf) - ct0) * inv
        inside = (f >= 0.0) & (f < nt - 1)
        jf = torch.floor(f)
        j = torch.where(inside, jf, torch.zeros_like(jf)).long()
        src = cd[None].expand(j.shape[0], -1, -1)
        c0, c1 = torch.gather(src, 2, j), torch.gather(src, 2, j + 1)
        ok = inside & torch.isfinite(c0) & torch.isfinite(c1)
        fr = f - jf
        v = torch.where(ok, (1.0 - fr) * c0 + fr * c1, torch.zeros_like(f))
        n = ok.sum(dim=1)
        if wd is None:
            s, sw = v.sum(dim=1), n.to(torch.float64)
        else:
            s, sw = (wd[None, :, None] * v).sum(dim=1), (wd[None, :, None] * ok).sum(dim=1)
        S = torch.where(n >= need, s / sw, torch.full_like(s, -np.inf))
        peak[m0:m0 + chunk] = S.max(dim=1).values
        best = torch.maximum(best, S.max(dim=0).values)
    b.record()
    torch.cuda.synchronize()
    return peak.cpu().numpy(), best.cpu().numpy(), a.elapsed_time(b)


def stack_main(a):
    """--stack M ...: the search kernel k_stack on the section-29 case with nt = 8192 samples per trace, a tenth of them NaN,
    without and with weights, against the same S, peak and best in plain torch"""
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_timing: no GPU; nothing is measured without one")
    P, nt = a.tables, 8192
    grid, T, _ = problem(P, 1)
    nn = T.shape[1] * T.shape[2]
    rng = np.random.default_rng(7)
    c = rng.uniform(0.0, 1.0, (P, nt))
    c[rng.random(c.shape) < 0.1] = np.nan
    ct0, cdt, o0, od = 0.0, 1e-3, 0.5, 1e-3                    # T < 1.5 s: every read falls inside the traces
    need = P // 2
    L = rb.Locator(T, grid)
    Td, cd = torch.from_numpy(T).cuda(), torch.from_numpy(c).cuda()
    out = {"grid": [grid[2], grid[5]], "tables": P, "nt": nt, "reps": a.reps, "cases": []}
    for M in a.stack:
        for weights in (False, True):
            wd = torch.from_numpy(rng.uniform(0.5, 2.0, P)).cuda() if weights else None
            o = o0 + od * torch.arange(M, dtype=torch.float64, device="cuda")
            kernel = lambda: L.stack_device(cd, cdt, t0=ct0, scan=(o0, od, M), weights=wd, min_stations=need, maps=True, stats=True)  # noqa: E731
            yard = lambda: torch_stack(torch, Td, cd, wd, o, ct0, 1.0 / cdt, need, a.torch_chunk)                                      # noqa: E731
            kernel(); yard()                                                        # warm both
            tk, tc, tt = [], [], []
            for _ in range(a.reps):                                                 # alternating
                r, st = kernel()
                tk.append(st["search_ms"])
                tc.append(st["kernel_ms"])
                peak, best, ms = yard()
                tt.append(ms)
            sk, st_, sc = series(tk), series(tt), series(tc)
            spread = max(sk["max_ms"] - sk["min_ms"], st_["max_ms"] - st_["min_ms"])
            triples = M * nn * P
            kp, kb = r["peak"].cpu().numpy(), r["best"].cpu().numpy().reshape(-1)
            floors = {"fp64_issue": triples / 64 * STACK_F64[weights] * F64_CYCLES / (SIMDS * CLOCK) * 1e3,
                      "gather_bytes": triples * STACK_GATHER / L2_BYTES_PER_S * 1e3}
            case = {"M": M, "weights": weights, "triples": triples, "contributing": st["contributing"], "parts": st["parts"],
                    "k_stack": sk, "all_kernels": sc, "torch": st_, "spread_ms": spread,
                    "ratio_of_medians": st_["median_ms"] / sk["median_ms"],
                    "kernel_is_faster_beyond_the_spread": bool(st_["median_ms"] - sk["median_ms"] > spread),
                    "triples_per_second": triples / (sk["median_ms"] * 1e-3),
                    "peak_max_abs_diff_to_torch": float(np.abs(kp - peak).max()), "best_max_abs_diff_to_torch": float(np.abs(kb - best).max()),
                    "floor_ms": floors, "binding_floor": max(floors, key=floors.get)}
            print(json.dumps(case), file=sys.stderr, flush=True)
            out["cases"].append(case)
    L.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


EDT_F64 = {False: 32, True: 34}     # fp64-rate vector instructions per (node, pair, event) in k_edt's inner loop where a chunk has
                                    # all its picks, without and with weights, read off the ISA (make asm UNIT=edt.hip; DESIGN.md
                                    # section 31): 513 and 545 in the loop body of 16 events


def torch_edt(torch, Td, td, wd, sigma):
    """the yardstick of --edt: (nodes [E], device ms); station 0 has a pick in every event"""
    P = Td.shape[0]
    Tf = Td.reshape(P, -1)
    ij = torch.triu_indices(P, P, 1, device=Td.device)
    ia, ib = ij[0], ij[1]
    s2 = sigma * sigma
    nodes = torch.empty(td.shape[0], dtype=torch.int64, device=td.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for e in range(td.shape[0]):
        d = (td[e] - td[e, 0])[:, None] - Tf
        u = d[ia] - d[ib]
        if wd is None:
            k = torch.exp(-(u * u) * (1.0 / (s2 + s2)))
            ok = torch.isfinite(td[e])
            if bool(ok.all()):
                value = k.sum(dim=0) / ia.shape[0]
            else:
                value = torch.nan_to_num(k).sum(dim=0) / (ok[ia] & ok[ib]).sum()
        else:
            v = 1.0 / wd[e] + s2
            g = 1.0 / (v[ia] + v[ib])
            h = torch.sqrt(g)
            value = (h[:, None] * torch.exp(-(u * u) * g[:, None])).sum(dim=0) / h.sum()
        nodes[e] = value.argmax()
    b.record()
    torch.cuda.synchronize()
    return nodes.cpu().numpy(), a.elapsed_time(b)


def edt_main(a):
    """--edt: the search kernel k_edt on the section-29 case against the same objective in plain torch"""
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_timing: no GPU; nothing is measured without one")
    P = a.tables
    grid, T, _ = problem(P, 1)
    nn = T.shape[1] * T.shape[2]
    npairs = P * (P - 1) // 2
    L = rb.Locator(T, grid)
    Td = torch.from_numpy(T).cuda()
    events = a.events if a.events != [64, 1024, 4096] else [64, 1024]
    rows = [(E, weights, 0.0) for E in events for weights in (False, True)] + [(events[-1], False, 0.1)]
    out = {"grid": [grid[2], grid[5]], "tables": P, "sigma": a.sigma, "reps": a.reps, "cases": []}
    for E, weights, missing in rows:
        _, _, t = problem(P, E, seed=E)
        rng = np.random.default_rng(E + 1)
        w = 1.0 / rng.uniform(0.005, 0.02, t.shape) ** 2 if weights else None
        if missing:
            t[:, 1:][rng.random((E, P - 1)) < missing] = np.nan           # station 0 keeps its pick: ref as the yardstick takes it
        td = torch.from_numpy(t).cuda()
        wd = None if w is None else torch.from_numpy(w).cuda()
        kernel = lambda: L.locate_edt_device(td, a.sigma, wd, stats=True)                # noqa: E731
        kernel(); torch_edt(torch, Td, td[:2], None if wd is None else wd[:2], a.sigma)     # warm both
        tk, tc, tt = [], [], []
        for _ in range(a.reps):                                                  # alternating
            r, st = kernel()
            tk.append(st["search_ms"])
            tc.append(st["kernel_ms"])
            nodes, ms = torch_edt(torch, Td, td, wd, a.sigma)
            tt.append(ms)
        sk, st_, sc = series(tk), series(tt), series(tc)
        spread = max(sk["max_ms"] - sk["min_ms"], st_["max_ms"] - st_["min_ms"])
        pairs = E * nn * npairs
        case = {"events": E, "weights": weights, "missing": missing, "pairs": pairs, "contributing": st["contributing"], "groups": st["groups"],
                "k_edt": sk, "all_kernels": sc, "torch": st_, "spread_ms": spread,
                "ratio_of_medians": st_["median_ms"] / sk["median_ms"],
                "kernel_is_faster_beyond_the_spread": bool(st_["median_ms"] - sk["median_ms"] > spread),
                "pairs_per_second": st["contributing"] / (sk["median_ms"] * 1e-3),
                "nodes_equal_to_torchs": int((nodes == r["node"]).sum()),
                "floor_ms": {"fp64_issue": st["contributing"] / 64 * EDT_F64[weights] * F64_CYCLES / (SIMDS * CLOCK) * 1e3}}
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
    L.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def torch_pdf(torch, maps, best, scale, power, levels, ud, nx, chunk):
    """the yardstick of --pdf from maps [E, ny, nx] on the device: mean, covariance, region counts, marginals, samples; best [E]
    (int64 nodes), scale [E] (least squares: sw* / (2 sigma^2)) or power [E] (EDT)"""
    E = maps.shape[0]
    flat = maps.reshape(E, -1)
    out = {k: [] for k in ("mean", "cov", "count", "mx", "my", "sample")}
    ix = (torch.arange(flat.shape[1], device=maps.device) % nx).to(torch.float64)
    iy = (torch.arange(flat.shape[1], device=maps.device) // nx).to(torch.float64)
    for e0 in range(0, E, chunk):
        m = flat[e0:e0 + chunk]
        ref = m.gather(1, best[e0:e0 + chunk, None])
        if scale is not None:
            rho = torch.exp(-(m - ref) * scale[e0:e0 + chunk, None])
        else:
            rho = torch.where(m >= 0, m / ref, torch.zeros_like(m)) ** power[e0:e0 + chunk, None]
        rho = torch.nan_to_num(rho, nan=0.0, posinf=0.0)
        Z = rho.sum(dim=1)
        ax, ay = (rho * ix).sum(dim=1) / Z, (rho * iy).sum(dim=1) / Z
        out["mean"].append(torch.stack([ax, ay], dim=1))
        out["cov"].append(torch.stack([(rho * ix * ix).sum(dim=1) / Z - ax * ax, (rho * ix * iy).sum(dim=1) / Z - ax * ay,
                                       (rho * iy * iy).sum(dim=1) / Z - ay * ay], dim=1))
        grid2 = rho.reshape(rho.shape[0], -1, nx)
        out["mx"].append(grid2.sum(dim=1) / Z[:, None])
        out["my"].append(grid2.sum(dim=2) / Z[:, None])
        top = torch.cumsum(torch.sort(rho, dim=1, descending=True).values, dim=1)
        want = torch.tensor(levels, dtype=torch.float64, device=maps.device)[None, :] * Z[:, None]
        out["count"].append(torch.searchsorted(top, want.contiguous()) + 1)
        if ud is not None:
            cum = torch.cumsum(rho, dim=1)
            out["sample"].append(torch.searchsorted(cum, (ud[e0:e0 + chunk] * Z[:, None]).contiguous(), right=True))
    return {k: torch.cat(v) for k, v in out.items() if v}


def pdf_main(a):
    """--pdf [--edt]: Locator.pdf_device against the same statistics in plain torch from the maps of the plain search"""
    import time
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_timing: no GPU; nothing is measured without one")
    P = a.tables
    grid, T, _ = problem(P, 1)
    nx, ny = grid[2], grid[5]
    nn = nx * ny
    L = rb.Locator(T, grid)
    kind = "edt" if a.edt else "l2"
    sigma = a.sigma if a.edt else a.pdf_sigma
    levels = (0.68, 0.95)
    events = a.events if a.events != [64, 1024, 4096] else [64, 1024]
    out = {"grid": [nx, ny], "tables": P, "kind": kind, "sigma": sigma, "samples": a.samples, "reps": a.reps, "cases": []}

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    for E in events:
        _, _, t = problem(P, E, seed=E)
        td = torch.from_numpy(t).cuda()
        ud = torch.from_numpy(np.random.default_rng(E).random((E, a.samples))).cuda() if a.samples else None
        search = (lambda **kw: L.locate_edt_device(td, sigma, stats=True, **kw)) if a.edt else (lambda **kw: L.locate_device(td, stats=True, **kw))
        ours = lambda: L.pdf_device(td, sigma, method=kind, levels=levels, marginals=True, samples=a.samples, u=ud, stats=True)  # noqa: E731

        def yard():
            r, _ = search(maps=True)
            best = torch.from_numpy(r["node"].astype(np.int64)).cuda()
            if a.edt:
                return torch_pdf(torch, r["maps"], best, None, torch.from_numpy(r["count"].astype(np.float64)).cuda(), levels, ud, nx,
                                 8 * a.torch_chunk)
            scale = torch.from_numpy(r["sw"] * (0.5 / (sigma * sigma))).cuda()
            return torch_pdf(torch, r["maps"], best, scale, None, levels, ud, nx, 8 * a.torch_chunk)

        ours(); yard(); search()                                                   # warm all three
        tw, tk, tp, ty, tb = [], [], [], [], []
        for _ in range(a.reps):                                                    # alternating
            (r, st), ms = wall(ours)
            tw.append(ms)
            tk.append(st["kernel_ms"])
            tp.append(st["pdf_ms"])
            y, ms = wall(yard)
            ty.append(ms)
            tb.append(search()[1]["kernel_ms"])
        sw_, sy, sk, sp, sb = series(tw), series(ty), series(tk), series(tp), series(tb)
        spread = max(sw_["max_ms"] - sw_["min_ms"], sy["max_ms"] - sy["min_ms"])
        has = r["mass"] > 0
        gx0, gdx, _, gy0, gdy, _ = grid
        mean = y["mean"].cpu().numpy()
        off = np.maximum(np.abs((r["mean_x"] - gx0) / gdx - mean[:, 0]), np.abs((r["mean_y"] - gy0) / gdy - mean[:, 1]))[has]
        count = y["count"].cpu().numpy()[has]
        case = {"events": E, "groups": st["groups"], "pdf_call_wall": sw_, "torch_wall": sy, "spread_ms": spread,
                "ratio_of_medians": sy["median_ms"] / sw_["median_ms"],
                "pdf_call_is_faster_beyond_the_spread": bool(sy["median_ms"] - sw_["median_ms"] > spread),
                "pdf_call_kernels": sk, "pdf_kernels": sp, "bare_search_kernels": sb,
                "added_to_the_bare_search_ms": sk["median_ms"] - sb["median_ms"],
                "floor_ms": {"one_read_of_the_maps": E * nn * 8 / HBM * 1e3},
                "events_with_a_pdf": int(has.sum()), "mean_max_abs_diff_to_torch_cells": float(off.max()) if has.any() else None,
                "median_nodes_in_the_95_region": float(np.median(r["level_count"][has, 1])) if has.any() else None,
                "events_with_region_counts_at_or_above_torchs": int((r["level_count"][has] >= count).all(axis=1).sum()),
                "region_count_least_difference_to_torchs": int((r["level_count"][has] - count).min()) if has.any() else None}
        if a.samples and has.any():
            case["samples_equal_to_torchs_share"] = float((r["sample_node"].cpu().numpy()[has] == y["sample"].cpu().numpy()[has]).mean())
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
    L.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stack", type=int, nargs="+", default=None, metavar="M",
                    help="time the stacking search k_stack (DESIGN.md section 30) for these scan lengths instead, e.g. --stack 256 4096")
    ap.add_argument("--edt", action="store_true", help="time the equal-differential-time search k_edt (DESIGN.md section 31) instead")
    ap.add_argument("--sigma", type=float, default=0.01, help="--edt: the pick error in seconds")
    ap.add_argument("--pdf", action="store_true", help="time the location pdf (DESIGN.md section 33) of the least-squares search, or with --edt of that one")
    ap.add_argument("--pdf-sigma", type=float, default=0.05, help="--pdf without --edt: the picks' standard deviation in seconds")
    ap.add_argument("--samples", type=int, default=256, help="--pdf: samples per event")
    ap.add_argument("--events", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=8)
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--missing", type=float, default=0.0, help="share of the picks that are missing (NaN): the masked variant of the kernel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stack:
        return stack_main(a)
    if a.pdf:
        return pdf_main(a)
    if a.edt:
        return edt_main(a)
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_timing: no GPU; nothing is measured without one")
    P = a.tables
    grid, T, _ = problem(P, 1)
    nn = T.shape[1] * T.shape[2]
    L = rb.Locator(T, grid)
    Td = torch.from_numpy(T).cuda()
    out = {"grid": [grid[2], grid[5]], "tables": P, "weights": bool(a.weights), "missing": a.missing, "reps": a.reps, "cases": []}
    for E in a.events:
        _, _, t = problem(P, E, seed=E)
        rng = np.random.default_rng(E + 1)
        w = rng.uniform(0.5, 2.0, t.shape) if a.weights else None
        if a.missing:
            t[:, 1:][rng.random((E, P - 1)) < a.missing] = np.nan         # station 0 keeps its pick: ref as the yardstick takes it
        td = torch.from_numpy(t).cuda()
        wd = None if w is None else torch.from_numpy(w).cuda()
        kernel = lambda: L.locate_device(td, wd, stats=True)                     # noqa: E731
        kernel(); torch_locate(torch, Td, td, wd, a.torch_chunk)                 # warm both
        tk, tc, tt = [], [], []
        for _ in range(a.reps):                                                  # alternating
            r, st = kernel()
            tk.append(st["search_ms"])
            tc.append(st["kernel_ms"])
            nodes, ms = torch_locate(torch, Td, td, wd, a.torch_chunk)
            tt.append(ms)
        sk, st_, sc = series(tk), series(tt), series(tc)
        spread = max(sk["max_ms"] - sk["min_ms"], st_["max_ms"] - st_["min_ms"])
        triples = E * nn * P
        blocks = -(-E // CHUNK) * -(-nn // TILE)
        case = {"events": E, "triples": triples, "k_locate": sk, "all_kernels": sc, "torch": st_, "spread_ms": spread,
                "ratio_of_medians": st_["median_ms"] / sk["median_ms"],
                "kernel_is_faster_beyond_the_spread": bool(st_["median_ms"] - sk["median_ms"] > spread),
                "triples_per_second": triples / (sk["median_ms"] * 1e-3),
                "nodes_equal_to_torchs": int((nodes == r["node"]).sum()),
                "floor_ms": {"table_bytes": 2 * blocks * P * TILE * 8 / HBM * 1e3,
                             "valu_issue": triples / 64 * F64_OPS[bool(a.weights)] * F64_CYCLES / (SIMDS * CLOCK) * 1e3}}
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
    L.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
