#!/usr/bin/env python3
"""np.exp (float64 arrays) vs its restatement in oracle/rt_oracle.c (np_exp) and raytracing_amd/csrc/field.hip.

The reference samples the interface field with np.exp on the meshgrid (RT_bench.py:107).  On AVX512_SKX machines numpy's
wheels route float64 exp to Intel SVML's `__svml_exp8_ha` (numpy/_core/src/umath/svml/linux/avx512/svml_z0_exp_d_ha.s,
BSD-3, compiled into _multiarray_umath) -- not libm: the two differ in the last bit for 4.5 % of arguments.  The routine's
main path is 20 instructions; its constants (log2(e), the 1.5*2^48+1023 shifter, ln2 hi/lo, six polynomial coefficients, the
16-entry 2^(j/16) table and its correction table) were read from the `__svml_dexp_ha_data_internal_avx512` object of the numpy
2.2.6 binary of the build container (`--dump` below does it again) and the restatement is compared here bit for bit.

  python3 tools/check_np_exp.py            # 2.6e7 arguments: expects 0 mismatches for |x| < 707.7
  python3 tools/check_np_exp.py --dump     # print the data block of the installed numpy (needs readelf)
"""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump():
    import numpy._core._multiarray_umath as m
    so = m.__file__
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    if "__svml_exp8_ha" not in syms:
        sys.exit("this numpy carries no SVML")
    out = subprocess.check_output(["objdump", "-d", "--no-show-raw-insn", so]).decode()
    i = out.index("<__svml_exp8_ha>:")
    line = next(l for l in out[i:].splitlines() if "__svml_dexp_ha_data_internal_avx512+0x100" in l)
    base = int(line.split("#")[1].split()[0], 16) - 0x100
    segs = []
    for l in subprocess.check_output(["readelf", "-lW", so]).decode().splitlines():
        p = l.split()
        if p and p[0] == "LOAD":
            segs.append(tuple(int(v, 16) for v in (p[1], p[2], p[4])))
    off = next(o + base - va for o, va, fs in segs if va <= base < va + fs)
    data = open(so, "rb").read()[off:off + 0x480]
    tab = struct.unpack("<32d", data[:256])
    print("T16 ", [float.hex(v) for v in tab[:16]])
    print("TL16", [float.hex(v) for v in tab[16:]])
    for o in range(0x100, 0x480, 0x40):
        print(hex(o), float.hex(struct.unpack("<d", data[o:o + 8])[0]))


def main():
    if "--dump" in sys.argv:
        return dump()
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    if not feat.get("AVX512_SKX"):
        print("numpy does not dispatch float64 exp to SVML on this CPU: nothing to compare")
        return
    from oracle import rt_oracle as O
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-707, 707, 20_000_000), rng.uniform(-2, 2, 5_000_000), rng.normal(0, 1e-3, 1_000_000),
                        np.arange(-700, 700, 1 / 16.0), np.arange(-100, 100, 1 / 16.0) / 1.4426950408889634])
    bad = O.np_exp(x) != np.exp(x)
    print(f"{x.size} arguments, {int(bad.sum())} mismatches")
    sys.exit(1 if bad.any() else 0)


if __name__ == "__main__":
    main()
