"""Times rtmi_first_arrival_grid on the full record of the 1 M-ray vert_heterogeneous op6 fan onto a 1024 x 1024 grid, and the
table case (64 sources x 4 096 rays onto 512 x 512 per source, traveltime_table end to end): prints one JSON line per
measurement.  The kernels' own times: run this under rocprofv3 --kernel-trace --stats.
Usage: python tools/ttgrid_timing.py [--rays N] [--reps K] [--sources S]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)


def fan_time(F, R, reps):
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, 1.5, R)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    d = c.d_ray()[2]
    rows, mean_rows = int(d.max()) + 1, float(d.mean()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    grid = (-2.0, 7.0 / 1023, 1024, -2.5, 3.5 / 1023, 1024)
    for amp in (False, True):
        b.first_arrival_grid(grid, amplitude=amp)            # warm-up: code objects, allocations
        ts, st = [], None
        for _ in range(reps):
            b.sync()
            t0 = time.perf_counter()
            r = b.first_arrival_grid(grid, amplitude=amp, stats=True)
            ts.append((time.perf_counter() - t0) * 1e3)
            st = r["stats"]
        print(json.dumps({"what": "rtmi_first_arrival_grid", "amplitude": amp, "rays": R, "rec_rows": rows, "mean_rows": mean_rows,
                          "xyT_bytes_per_pass": int(24 * mean_rows * R), "ms_median": float(np.median(ts)), "ms_all": ts,
                          "covered": int((r["count"] > 0).sum()), "stats": st,
                          "note": "host clock incl. allocation and the copy of the table to the host; pass_ms from HIP events"}),
              flush=True)
    b.close()


def table_time(F, S, M, reps):
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    rng = np.random.default_rng(3)
    src = np.c_[rng.uniform(-1.9, 4.9, S), rng.uniform(-2.4, -1.0, S)]
    th = np.linspace(0.02, np.pi - 0.02, M)
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 511, 512)
    for _ in range(reps):
        t0 = time.perf_counter()
        r = rb.traveltime_table(rb.op6, F, src, grid, thetas=th, step=rb.DELTA_S, max_size=ms, box=BOX, stats=True)
        tot = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"what": "traveltime_table", "sources": S, "fan": M, "grid": [512, 512], "ms_total": tot,
                          "covered_fraction": float((r["count"] > 0).mean()), "stats": r["stats"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--fan", type=int, default=4096)
    a = ap.parse_args()
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    fan_time(F, a.rays, a.reps)
    table_time(F, a.sources, a.fan, a.reps)
    F.close()
