"""Times rtmi_traveltime_perturb (A) and rtmi_traveltime_backproject (A^T) on the full record of the 1 M-ray vert_heterogeneous
op6 fan: the kernels' HIP-event times (rtmi_sensitivity_stats.kernel_ms), at the ray ends and with the receiver line x = 4
(kmax 1), and the x, y bytes each walk reads (the floor at 6 TB/s).  Prints one JSON line per measurement.
Usage: python tools/sensitivity_timing.py [--rays N] [--reps K]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)
LINE = (1.0, 0.0, 4.0)


def main(R, reps):
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.0, np.pi / 2, R)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    walked = float(np.sum(b.d_ray()[2]) + R)
    xy_bytes = 16 * walked
    Z = F.arrays()[2]
    w = np.ones(R)
    calls = {
        "A end": lambda: b.traveltime_perturb(Z, stats=True)["stats"],
        "A line": lambda: b.traveltime_perturb(Z, line=LINE, kmax=1, stats=True)["stats"],
        "AT end": lambda: b.traveltime_backproject(w_end=w, stats=True)[1],
        "AT line": lambda: b.traveltime_backproject(w_end=w, w_line=w[None, :], line=LINE, kmax=1, stats=True)[1],
    }
    for what, call in calls.items():
        call()                                               # warm-up: code objects, allocations
        st = [call() for _ in range(reps)]
        ms_ = [s["kernel_ms"] for s in st]
        print(json.dumps({"what": what, "rays": R, "rec_rows": rows, "rows_walked": walked, "xy_bytes": xy_bytes,
                          "floor_ms_at_6TBps": xy_bytes / 6e12 * 1e3, "kernel_ms_median": float(np.median(ms_)), "kernel_ms": ms_,
                          "atomics": st[-1]["atomics"], "scale_exp": st[-1]["scale_exp"]}), flush=True)
    b.close()
    F.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    main(a.rays, a.reps)
