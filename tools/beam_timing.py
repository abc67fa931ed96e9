"""Times rtmi_gaussian_beams on the timing case of DESIGN.md section 13: vert_heterogeneous, op6 at DELTA_S, source (-2, -2), a
512-ray fan over [0.05, pi/2 - 0.05], 512 x 256 nodes over the box, 8 frequencies with source wavelengths from 0.2 to 0.05 and
eps = 4 / n0.  Prints one JSON line: each pass's device time (HIP events, medians of --reps calls), the counters, pairs and
pair-frequencies per second, and -- with --asm FILE, the device assembly of beams.hip (hipcc --cuda-device-only -S) -- the
gather's instruction counts.  Its inner loops, per basic block: tools/asm_stats.py on the same listing; DESIGN.md 13 derives
the VALU-issue floor from them at 4 cycles per fp64 and 2 per other VALU instruction per wave.
Usage: python tools/beam_timing.py [--reps K] [--asm beams_gfx950.s]"""
import argparse
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracing_amd import rt_bench as rb  # noqa: E402

BOX = (-2, 5, -2.5, 1)


def loop_counts(asm):
    """the gather kernel's VALU / fp64 instruction counts in the ISA listing (per basic block: tools/asm_stats.py NAME, which
    reads /tmp/rtmi_gfx950.s)"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import asm_stats
    name = next(l.split(":")[0] for l in open(asm) if re.match(r"_Z\w*k_gather\w*:", l))
    lines = asm_stats.kernel_lines(name, asm)
    valu = sum(1 for l in lines if re.match(r"\s+v_", l))
    f64 = sum(1 for l in lines if re.match(r"\s+v_\w*f64", l))
    return name, valu, f64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--asm", default=None)
    a = ap.parse_args()
    F = rb.Field.build("vert_heterogeneous", BOX, rb.DELTA)
    n0 = float(F.n_gradient(-2.0, -2.0)[0][0])
    lam = np.linspace(0.2, 0.05, 8)
    omegas = 2 * np.pi / (lam * n0)
    eps = 4.0 / n0
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, np.pi / 2 - 0.05, 512)
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, BOX, 1, th, -2.0, -2.0, keep_n_ray=False)
    b.run()
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    runs = [b.gaussian_beams(grid, omegas, eps, stats=True)[1] for _ in range(a.reps + 1)][1:]
    b.close(); F.close()
    med = {k: float(np.median([r[k] for r in runs])) for k in ("prep_ms", "bin_ms", "gather_ms")}
    st = runs[0]
    res = {"case": "vert_heterogeneous op6, 512 rays, 512x256 nodes, 8 omegas", "n0": n0, "eps": eps,
           "omegas": [float(w) for w in omegas], **{k: st[k] for k in ("segments", "tile_entries", "pairs_tested", "pairs_inside",
                                                                          "capped")},
           **med, "pairs_per_s": st["pairs_tested"] / (med["gather_ms"] * 1e-3),
           "pair_freqs_per_s": st["pairs_inside"] * len(omegas) / (med["gather_ms"] * 1e-3),
           "prep_bin_over_gather": (med["prep_ms"] + med["bin_ms"]) / med["gather_ms"]}
    if a.asm:
        name, valu, f64 = loop_counts(a.asm)
        res["gather_kernel"] = name
        res["gather_valu_static"] = valu
        res["gather_f64_static"] = f64
    print(json.dumps(res))


if __name__ == "__main__":
    main()
