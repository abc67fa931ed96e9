#!/usr/bin/env python3
"""Several right-hand sides through the eikonal operator in one call against K calls of the single entries,
in one process: the case of tools/eikonal_lin_timing.py and tools/eikonal_tomo_timing.py (737 x 539, vert_heterogeneous sampled at
the nodes, 32 sources, tables from the source ball alone, 64 receivers off the nodes), with K = --cols columns.

Measured, each as wall time round calls on device tensors (the sweeps) or host vectors (the handle), warmed and alternating,
medians of --reps with min and max:
    tangent   rtmi_eikonal_tangent_multi_dev against K calls of rtmi_eikonal_tangent_dev
    adjoint   rtmi_eikonal_adjoint_multi_dev against K calls of rtmi_eikonal_adjoint_dev
    pair      EikonalTomography.matmat and rmatmat against K calls of apply and transpose
    solve     EikonalTomography.lsqr_multi of --iters iterations against K calls of lsqr
--rows picks among them; --width forces the sweeps' chunk width in place of the call's own choice, to compare the widths.  The
yardstick is the single entries' code, which the batched path does not touch.  The rule is section 24's: the batched series lies
below the K single calls by more than the larger of the two ranges, or it is not faster.  Every row also checks that column c of
the batched result has the bytes of single call c (NaN by place), in the same run.  For the sweeps
the kernels' own time is printed as ns per diagonal and column, beside section 35's 3 078 (tangent) and 3 855 (adjoint).

    python tools/eikonal_multi_timing.py [--cols 8] [--tables 32] [--receivers 64] [--iters 10] [--reps 5] [--rows tangent,adjoint,pair,solve]
                                         [--width 0] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.eikonal_timing import NX, NY, series      # noqa: E402

DAMP = 1e-3


def wall(torch, f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def verdict(multi, singles):
    """section 24's rule on two series of milliseconds"""
    spread = max(multi["max_ms"] - multi["min_ms"], singles["max_ms"] - singles["min_ms"])
    return {"ratio_of_medians": singles["median_ms"] / multi["median_ms"], "spread_ms": spread,
            "batched_is_faster_beyond_the_spread": bool(singles["median_ms"] - multi["median_ms"] > spread)}


def same(torch, a, b):
    """the same bytes, NaN by place"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    na = torch.isnan(a)
    return bool(torch.equal(na, torch.isnan(b)) and
                torch.equal(torch.where(na, 0.0, a).view(torch.int64), torch.where(na, 0.0, b).view(torch.int64)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--receivers", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="tangent,adjoint,pair,solve")
    ap.add_argument("--width", type=int, default=0, help="force the sweeps' chunk width (1, 4 or 8); 0: the call's own choice")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = a.rows.split(",")
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eikonal_multi_timing: no GPU; nothing is measured without one")
    P, Rn, K = a.tables, a.receivers, a.cols
    box = (-2.0, 5.0, -2.5, 1.0)
    grid = (-1.9, 6.8 / (NX - 1), NX, -2.4, 3.3 / (NY - 1), NY)
    gx0, gdx, _, gy0, gdy, _ = grid
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ys = np.linspace(-2.3, 0.8, P // 2)
    src = np.concatenate([np.stack([np.full(len(ys), 4.85), ys], axis=1), np.stack([np.full(P - len(ys), -1.85), ys[:P - len(ys)]], axis=1)])
    X, Y = np.meshgrid(gx0 + np.arange(NX) * gdx, gy0 + np.arange(NY) * gdy)
    n = F.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(NY, NX)
    ns = F.n_gradient(src[:, 0], src[:, 1])[0]
    F.close()
    half = Rn // 2
    cols = np.linspace(20, NX - 21, half).astype(np.int64)
    rec = np.array([[gx0 + (i + 0.5) * gdx, gy0 + (NY - 1) * gdy] for i in cols] + [[gx0 + (i + 0.5) * gdx, gy0] for i in cols[:Rn - half]])
    dev = torch.device("cuda:0")
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)        # noqa: E731
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    out = {"grid": [NX, NY], "tables": P, "receivers": Rn, "cols": K, "iters": a.iters, "reps": a.reps, "width": a.width}
    ndiag = NX + NY - 1

    if "tangent" in rows or "adjoint" in rows:
        d_n, d_src, d_ns = up(n), up(src), up(ns)
        fill = rb.eikonal_fill_device(d_n, d_src, grid, n_src=d_ns)
        assert fill["converged"].all()
        kw = dict(n_src=d_ns, stats=True)
        for name in ("tangent", "adjoint"):
            if name not in rows:
                continue
            if name == "tangent":
                v = 0.02 * torch.randn((K, NY, NX), dtype=torch.float64, device=dev, generator=gen)
                multi = lambda: rb.eikonal_tangent_multi_device(d_n, d_src, grid, fill, v, _width=a.width, **kw)  # noqa: E731
                single = lambda c: rb.eikonal_tangent_device(d_n, d_src, grid, fill, v[c], **kw)                 # noqa: E731
                keys = ("dT",)
            else:
                v = torch.randn((K, P, NY, NX), dtype=torch.float64, device=dev, generator=gen)
                multi = lambda: rb.eikonal_adjoint_multi_device(d_n, d_src, grid, fill, v, _width=a.width, **kw)  # noqa: E731
                single = lambda c: rb.eikonal_adjoint_device(d_n, d_src, grid, fill, v[c], **kw)                 # noqa: E731
                keys = ("lam", "g", "g_src")
            m, ones = multi(), [single(c) for c in range(min(K, 2))]                                            # warm
            tm, ts, km, ks = [], [], [], []
            equal = True
            for rep in range(a.reps):                                                                          # alternating
                m, ms = wall(torch, multi)
                tm.append(ms)
                km.append(m["stats"]["kernel_ms"])
                t0, kk = 0.0, 0.0
                for c in range(K):
                    one, ms = wall(torch, lambda: single(c))
                    t0 += ms
                    kk += one["stats"]["kernel_ms"]
                    if rep == 0:
                        equal = equal and all(same(torch, m[k][c], one[k]) for k in keys) and \
                            np.array_equal(m["rounds"][c], one["rounds"]) and np.array_equal(m["converged"][c], one["converged"])
                ts.append(t0)
                ks.append(kk)
                del one
            sm, ss = series(tm), series(ts)
            rounds = int(m["stats"]["rounds_max"])
            row = {"row": name, "path": m["stats"]["path"], "rounds_max": rounds, "batched": sm, "k_single_calls": ss, **verdict(sm, ss),
                   "batched_kernels": series(km), "single_kernels": series(ks), "bit_equal_to_the_single_calls": bool(equal),
                   "ns_per_diagonal_and_column": {"batched": float(np.median(km)) * 1e6 / (ndiag * 4 * rounds * K),
                                                  "single": float(np.median(ks)) * 1e6 / (ndiag * 4 * rounds * K)}}
            print(json.dumps(row), file=sys.stderr, flush=True)
            out[name] = row
            del v, m
        del fill
        torch.cuda.empty_cache()

    if "pair" in rows or "solve" in rows:
        T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, _width=a.width)
        rng = np.random.default_rng(1)
        bump = np.exp(-((X - 1.5) ** 2 + (Y + 0.8) ** 2) / 0.6 ** 2)
        Xc = 0.02 * n[None] * bump[None] * rng.uniform(0.5, 1.5, (K, 1, 1)) + 1e-4 * rng.standard_normal((K, NY, NX))
        Yc = rng.standard_normal((K, P * Rn))
        if "pair" in rows:
            T.matmat(Xc[:1]), T.rmatmat(Yc[:1]), T.apply(Xc[0]), T.transpose(Yc[0])                            # warm
            tm, ts = [], []
            equal = True
            for rep in range(a.reps):
                (ym, Gm), ms = wall(torch, lambda: (T.matmat(Xc), T.rmatmat(Yc)))
                tm.append(ms)
                ones, ms = wall(torch, lambda: [(T.apply(Xc[c]), T.transpose(Yc[c])) for c in range(K)])
                ts.append(ms)
                if rep == 0:
                    equal = all(same(torch, ym[c], ones[c][0]) and same(torch, Gm[c], ones[c][1]) for c in range(K))
            sm, ss = series(tm), series(ts)
            out["pair"] = {"row": "pair", "batched": sm, "k_single_calls": ss, **verdict(sm, ss), "bit_equal_to_the_single_calls": bool(equal),
                           "bytes_device": T.info()["bytes_device"]}
            print(json.dumps(out["pair"]), file=sys.stderr, flush=True)
        if "solve" in rows:
            rhs = T.matmat(Xc)
            T.lsqr(rhs[0], 1, damp=DAMP)                                                                        # warm
            tm, ts = [], []
            equal = True
            for rep in range(a.reps):
                om, ms = wall(torch, lambda: T.lsqr_multi(rhs, a.iters, damp=DAMP, stats=True))
                tm.append(ms)
                ones, ms = wall(torch, lambda: [T.lsqr(rhs[c], a.iters, damp=DAMP) for c in range(K)])
                ts.append(ms)
                if rep == 0:
                    equal = all(same(torch, om[c]["x"], ones[c]["x"]) and (om[c]["itn"], om[c]["istop"]) == (ones[c]["itn"], ones[c]["istop"])
                                for c in range(K))
            sm, ss = series(tm), series(ts)
            out["solve"] = {"row": "solve", "batched": sm, "k_single_calls": ss, **verdict(sm, ss), "bit_equal_to_the_single_calls": bool(equal),
                            "itn": [int(o["itn"]) for o in om], "operator_ms": om[0]["stats"]["operator_ms"],
                            "vector_ms": om[0]["stats"]["vector_ms"]}
            print(json.dumps(out["solve"]), file=sys.stderr, flush=True)
        T.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
