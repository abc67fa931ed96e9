"""Times rtmi_arrival_grid against rtmi_first_arrival_grid on the full record of the 1 M-ray vert_heterogeneous op6 fan onto a
1024 x 1024 grid (tools/ttgrid_timing.py's case): the calls interleaved in one process, device times from each call's own HIP
events, medians over --reps rounds.  Prints one JSON line per variant.
Usage: python tools/arrival_timing.py [--rays N] [--reps K]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)
GRID = (-2.0, 7.0 / 1023, 1024, -2.5, 3.5 / 1023, 1024)
# name -> (arrivals or None for rtmi_first_arrival_grid, order, amplitude columns)
VARIANTS = {"first": (None, None, False), "first+amp": (None, None, True), "k1 time": (1, "time", False), "k4 time": (4, "time", False),
            "k1 amplitude": (1, "amplitude", False), "k1 amplitude+amp": (1, "amplitude", True)}


def call(b, arrivals, order, amp):
    if arrivals is None:
        return b.first_arrival_grid(GRID, amplitude=amp, stats=True)
    return b.arrival_grid(GRID, arrivals=arrivals, order=order, amplitude=amp, stats=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, 1.5, a.rays)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    d = c.d_ray()[2]
    rows, mean_rows = int(d.max()) + 1, float(d.mean()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    for v in VARIANTS.values():
        call(b, *v)                                     # warm-up: code objects, allocations
    seen = {k: [] for k in VARIANTS}
    for _ in range(a.reps):                             # interleaved: every variant once per round
        for k, v in VARIANTS.items():
            b.sync()
            seen[k].append(call(b, *v)["stats"])
    for k, sts in seen.items():
        p = np.array([s["pass_ms"] for s in sts])
        scan = np.array([s.get("scan_ms", 0.0) for s in sts])
        tot = p.sum(axis=1) + scan
        print(json.dumps({"what": k, "rays": a.rays, "rec_rows": rows, "mean_rows": mean_rows, "reps": a.reps,
                          "device_ms_median": float(np.median(tot)), "device_ms_min": float(tot.min()), "device_ms_max": float(tot.max()),
                          "pass_ms_median": np.median(p, axis=0).tolist(), "scan_ms_median": float(np.median(scan)),
                          "candidates": sts[-1].get("candidates"), "list_bytes": 16 * sts[-1].get("candidates", 0),
                          "row_bytes_per_walk": int(32 * mean_rows * a.rays), "atomics": sts[-1]["atomics"],
                          "cells": sts[-1]["cells"], "triangles": sts[-1]["triangles"]}), flush=True)
    b.close()
    F.close()
