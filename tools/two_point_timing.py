"""Times rtmi_crossings on a full record of the vert_heterogeneous fan and rtmi_two_point for 64 sources x 256 receivers (op6):
prints one JSON line per measurement.  Usage: python tools/two_point_timing.py [--rays N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)


def crossings_time(F, R):
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0, np.pi / 2, R)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    rows = int(c.d_ray()[2].max()) + 1
    mean_rows = float(c.d_ray()[2].mean()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    b.crossings((1.0, 0.0, 4.0))                      # warm-up: code object, allocations
    ts = []
    for _ in range(5):
        b.sync()
        t0 = time.perf_counter()
        b.crossings((1.0, 0.0, 4.0))                  # ends in a device-to-host copy (synchronous)
        ts.append((time.perf_counter() - t0) * 1e3)
    b.close()
    print(json.dumps({"what": "rtmi_crossings", "rays": R, "rec_rows": rows, "xy_bytes_read": int(16 * mean_rows * R),
                      "ms_median": float(np.median(ts)), "ms_all": ts, "note": "host clock incl. the copy of count/out to the host"}),
          flush=True)


def two_point_time(F):
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    src = [(-2.0, y) for y in np.linspace(-2.4, 0.8, 64)]
    ru = np.linspace(-2.4, 0.9, 256)
    kw = dict(thetas=np.linspace(-0.3, 1.5, 1024), step=rb.DELTA_S, max_size=ms, box=BOX, stats=True)
    rb.two_point(rb.op6, F, src[:2], (1.0, 0.0, 4.0), ru, **kw)          # warm-up
    t0 = time.perf_counter()
    r = rb.two_point(rb.op6, F, src, (1.0, 0.0, 4.0), ru, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    st = r["stats"]
    print(json.dumps({"what": "rtmi_two_point", "sources": 64, "receivers": 256, "fan": 1024, "wall_ms": wall, **st,
                      "per_iteration_ms": st["refine_ms"] / max(1, st["iterations"]),
                      "converged": int(r["count"].sum()), "not_converged": int(r["nbad"].sum())}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    a = ap.parse_args()
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    two_point_time(F)
    crossings_time(F, a.rays)
    F.close()
