#!/usr/bin/env python3
"""First-arrival eikonal tomography on the device against what existed before it, in one process: the
737 x 539 grid of tools/eikonal_lin_timing.py (vert_heterogeneous sampled at the nodes, 32 sources on the lines x = 4.85 and
x = -1.85, tables from the source ball alone) with 64 receivers off the nodes on the far edges, the top and the bottom row of the
grid, half a cell between two nodes.

Measured: one product pair (A dn and A^T y) and a solve of --iters LSQR iterations with damp, each as host wall time from host
vectors in to host vectors out, and the handle's own device times beside them.  The yardstick is rt_bench.eikonal_operator on
the same receivers snapped to their nearest nodes (it takes nodes only), driven by scipy.sparse.linalg.lsqr with the same
iter_lim and damp: the same sweeps, with torch gathers, a torch sum over the sources and two PCIe crossings per product round
them.  Both sides run warmed and alternating; medians of --reps with min and max.  The rule is section 24's: one side is faster
only if the medians differ by more than the larger of the two ranges.

Also printed: k_etomo_reduce's own time beside its floor, (S + 1) 8 bytes per node (and 4 for its offsets) at 6 TB/s.

    python tools/eikonal_tomo_timing.py [--tables 32] [--receivers 64] [--iters 10] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.eikonal_timing import HBM, NX, NY, series      # noqa: E402

DAMP = 1e-3


def wall(torch, f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def verdict(new, old):
    """section 24's rule on two series of milliseconds"""
    spread = max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"])
    return {"ratio_of_medians": old["median_ms"] / new["median_ms"], "spread_ms": spread,
            "device_is_faster_beyond_the_spread": bool(old["median_ms"] - new["median_ms"] > spread),
            "yardstick_is_faster_beyond_the_spread": bool(new["median_ms"] - old["median_ms"] > spread)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--receivers", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from raytracing_amd import rt_bench as rb
    import torch
    from scipy.sparse.linalg import lsqr
    if not torch.cuda.is_available():
        raise SystemExit("eikonal_tomo_timing: no GPU; nothing is measured without one")
    P, Rn = a.tables, a.receivers
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
    # receivers: half of them on the top row, half on the bottom row, each half a cell between two nodes
    half = Rn // 2
    cols = np.linspace(20, NX - 21, half).astype(np.int64)
    rec = np.array([[gx0 + (i + 0.5) * gdx, gy0 + (NY - 1) * gdy] for i in cols] +
                   [[gx0 + (i + 0.5) * gdx, gy0] for i in cols[:Rn - half]])
    snapped = np.array([(NY - 1) * NX + i for i in cols] + [int(i) for i in cols[:Rn - half]])
    rng = np.random.default_rng(1)
    dn = 0.02 * n * np.exp(-((X - 1.5) ** 2 + (Y + 0.8) ** 2) / 0.6 ** 2)
    y = rng.standard_normal(P * Rn)

    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    info = T.info()
    fill = rb.eikonal_fill(n, src, grid, n_src=ns)
    assert fill["converged"].all()
    op = rb.eikonal_operator(n, src, grid, fill, snapped, n_src=ns)
    rhs_new, rhs_old = T.apply(dn), op.matvec(dn.reshape(-1))                              # warm, and each side's own right-hand side
    T.transpose(y), op.rmatvec(y)
    solve_new = lambda: T.lsqr(rhs_new, a.iters, damp=DAMP, stats=True)                      # noqa: E731
    solve_old = lambda: lsqr(op, rhs_old, damp=DAMP, atol=0.0, btol=0.0, conlim=0.0, iter_lim=a.iters)      # noqa: E731
    t = {k: [] for k in ("pair_new", "pair_old", "solve_new", "solve_old", "apply_kernels", "transpose_kernels", "reduce", "tangent_sweep",
                         "adjoint_sweep", "operator", "vector")}
    for _ in range(a.reps):                                                                # alternating
        (sa, st), ms = wall(torch, lambda: (T.apply(dn, stats=True)[1], T.transpose(y, stats=True)[1]))
        t["pair_new"].append(ms)
        t["apply_kernels"].append(sa["kernel_ms"]); t["tangent_sweep"].append(sa["sweep_ms"])
        t["transpose_kernels"].append(st["kernel_ms"]); t["reduce"].append(st["reduce_ms"]); t["adjoint_sweep"].append(st["sweep_ms"])
        _, ms = wall(torch, lambda: (op.matvec(dn.reshape(-1)), op.rmatvec(y)))
        t["pair_old"].append(ms)
        out, ms = wall(torch, solve_new)
        t["solve_new"].append(ms)
        t["operator"].append(out["stats"]["operator_ms"]); t["vector"].append(out["stats"]["vector_ms"])
        sc, ms = wall(torch, solve_old)
        t["solve_old"].append(ms)
    s = {k: series(v) for k, v in t.items()}
    nn = NX * NY
    fit_new = float(np.linalg.norm(T.apply(out["x"]) - rhs_new) / np.linalg.norm(rhs_new))
    fit_old = float(np.linalg.norm(op.matvec(sc[0]) - rhs_old) / np.linalg.norm(rhs_old))
    res = {"grid": [NX, NY], "tables": P, "receivers": Rn, "iters": a.iters, "damp": DAMP, "reps": a.reps,
           "handle": {k: info[k] for k in ("rows", "live_rows", "touched", "bytes_device", "path")},
           "product_pair": {"device_handle": s["pair_new"], "eikonal_operator": s["pair_old"], **verdict(s["pair_new"], s["pair_old"]),
                            "tangent_sweep": s["tangent_sweep"], "adjoint_sweep": s["adjoint_sweep"],
                            "apply_kernels_of_this_unit": s["apply_kernels"], "transpose_kernels_of_this_unit": s["transpose_kernels"]},
           "k_etomo_reduce": {**s["reduce"], "bytes": nn * ((P + 1) * 8 + 4), "floor_ms": nn * ((P + 1) * 8 + 4) / HBM * 1e3},
           "solve": {"device_handle": s["solve_new"], "scipy_on_eikonal_operator": s["solve_old"], **verdict(s["solve_new"], s["solve_old"]),
                     "operator_ms": s["operator"], "vector_ms": s["vector"], "itn": [int(out["itn"]), int(sc[2])],
                     "relative_misfit": [fit_new, fit_old]}}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    T.close()


if __name__ == "__main__":
    main()
