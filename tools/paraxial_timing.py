"""Times rtmi_paraxial on a full record of the vert_heterogeneous op6 fan (the end of each ray, and with the receiver line
x = 4): prints one JSON line per measurement.  The kernel's own time: run this under rocprofv3 --kernel-trace --stats.
Usage: python tools/paraxial_timing.py [--rays N] [--reps K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)


def paraxial_time(F, R, reps):
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0, np.pi / 2, R)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    d = c.d_ray()[2]
    rows, mean_rows = int(d.max()) + 1, float(d.mean()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    for line in (None, (1.0, 0.0, 4.0)):
        b.paraxial(line)                              # warm-up: code object, allocations
        ts = []
        for _ in range(reps):
            b.sync()
            t0 = time.perf_counter()
            r = b.paraxial(line)                      # ends in a device-to-host copy (synchronous)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"what": "rtmi_paraxial", "line": line, "rays": R, "rec_rows": rows, "mean_rows": mean_rows,
                          "xytheta_bytes_read": int(24 * mean_rows * R), "ms_median": float(np.median(ts)), "ms_all": ts,
                          "finite_J": int(np.isfinite(r["J"]).sum()),
                          "note": "host clock incl. allocation and the copy of the results to the host"}), flush=True)
    b.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    paraxial_time(F, a.rays, a.reps)
    F.close()
