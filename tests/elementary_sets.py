"""The argument sets on which the restated elementary functions -- numpy's float64 arctan2 (SVML __svml_atan28_ha) and array exp
(SVML __svml_exp8_ha) -- are compared bit for bit: the oracle against numpy on the CPU (tests/test_elementary_sets.py), the device
against the oracle on the GPU (tests/test_gpu_elementary.py).  Seeded: the same arguments in both.  Test infrastructure."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ATAN2_LO, ATAN2_HI = 2.0 ** -1020, 2.0 ** 993       # the main path: both |operands| in [LO, HI)
OCTANT_SWITCHES = (0.4375, 0.6875, 1.1875, 2.4375)
EXP_MAIN = float.fromhex("0x1.61da04cbafe44p+9")    # the main path: |x| < 707.7...
SPECIALS = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 5e-324, 1e-310, 1e300, np.nan)


def rcp14_table():
    """rt_rcp14_table.h decoded as k_rcp14_init decodes it: T[0] = RT_RCP14_T0 minus entry 0's delta, T[k] = T[k-1] - delta_k, the
    deltas two bits each, 32 per word, entry k in bits 2 * (k % 32) of word k / 32 -> uint16 [65536]."""
    src = open(os.path.join(ROOT, "raytracing_amd", "csrc", "rt_rcp14_table.h")).read()
    t0 = int(re.search(r"#define\s+RT_RCP14_T0\s+(0x[0-9a-fA-F]+)", src).group(1), 16)
    nwords = int(re.search(r"#define\s+RT_RCP14_WORDS\s+(\d+)", src).group(1))
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{1,16})ull", src.split("RT_RCP14_DELTAS", 1)[1])]
    assert nwords == 2048 and len(words) == nwords
    v, out = t0, np.empty(65536, dtype=np.uint16)
    for k in range(65536):
        v = (v - ((words[k >> 5] >> (2 * (k & 31))) & 3)) & 0xffff
        out[k] = v
    return out


def _signs(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)


def arctan2_pairs():
    """-> (y, x): every table entry under both signs of x, all five base points in all four quadrants, the four octant switches at
    equality and one ulp to either side, 600 decades of magnitudes, and the hand-over to the scalar fall-back at 2^-1020 and 2^993."""
    rng = np.random.default_rng(2024)
    ys, xs = [], []
    k = np.arange(65536)
    for e in (-3, 0, 7):                       # entry k is read: |y| < 0.4375 |x|, so the denominator is |x| itself
        for f in (0.2, 0.43):
            x = np.ldexp(1.0 + k / 65536.0, e)
            y = x * f * rng.uniform(0.5, 1.0, k.size)
            ys += [y, y]; xs += [x, -x]
    n = 400_000                                 # all five base points, all four quadrants
    x = rng.normal(0, 1, n)
    ys.append(np.abs(x) * rng.uniform(0, 4, n) * _signs(rng, n)); xs.append(x)
    for c in OCTANT_SWITCHES:                   # y = RN(c |x|) is the very product the routine compares |y| with: equality, +-1 ulp
        x = rng.uniform(0.5, 2.0, 20_000) * _signs(rng, 20_000)
        y = c * np.abs(x)
        for v in (y, np.nextafter(y, 0.0), np.nextafter(y, np.inf)):
            ys += [v, -v]; xs += [x, x]
    ys.append(rng.normal(0, 1, n) * 10.0 ** rng.uniform(-300, 290, n))
    xs.append(rng.normal(0, 1, n) * 10.0 ** rng.uniform(-300, 290, n))
    m = 2_000                                   # the hand-over, in both argument positions and both signs
    for h in (ATAN2_LO, ATAN2_HI):
        for v in (h, np.nextafter(h, 0.0), np.nextafter(h, np.inf)):
            for s in (1.0, -1.0):
                p = rng.normal(0, 1, m)
                ys += [np.full(m, s * v), p]; xs += [p, np.full(m, s * v)]
    return np.concatenate(ys), np.concatenate(xs)


def arctan2_special_grid():
    """The 10 x 10 grid of SPECIALS -> (y, x)"""
    s = np.array(SPECIALS)
    y, x = np.meshgrid(s, s, indexing="ij")
    return y.ravel().copy(), x.ravel().copy()


def arctan2_main(y, x):
    """True where the pair takes SVML's main path (the bit contract): both operands in [2^-1020, 2^993) in magnitude."""
    ay, ax = np.abs(y), np.abs(x)
    return (ay >= ATAN2_LO) & (ay < ATAN2_HI) & (ax >= ATAN2_LO) & (ax < ATAN2_HI)


def rcp14_indices_read(y, x):
    """The table indices VRCP14PD is asked for on main-path pairs, as vrcp14pd forms them: the top 16 mantissa bits of the
    denominator.  Counted only where the denominator is known without an fma here: |x| below the first switch, |y| above the last,
    and |x| + c |y| with c = 0.5 or 1 (c |y| exact: one rounding, the fma's); base point 1.5 is left out, which can only undercount."""
    ok = arctan2_main(y, x)
    ay, ax = np.abs(y[ok]), np.abs(x[ok])
    k5, k1, k2, k3 = (c * ax < ay for c in OCTANT_SWITCHES)
    den = [ax[~k5], ay[k3], ax[k5 & ~k1] + 0.5 * ay[k5 & ~k1], ax[k1 & ~k2] + ay[k1 & ~k2]]
    bits = np.concatenate(den).view(np.uint64)
    return np.unique((bits >> np.uint64(36)) & np.uint64(0xffff))


def exp_main_args():
    """Arguments of the main path, |x| < EXP_MAIN: dense, the 1/16 grid, and the multiples of ln2 / 16 with their neighbours, where
    x * log2(e) * 16 sits on or one ulp beside an integer (what np_exp's floor correction exists for)."""
    rng = np.random.default_rng(2025)
    k = np.arange(-16 * 1020, 16 * 1020)
    g = k / 16.0 * np.log(2.0)
    x = np.concatenate([rng.uniform(-707.7, 707.7, 2_000_000), rng.uniform(-2, 2, 500_000), np.arange(-707, 707, 1 / 16.0),
                        g, np.nextafter(g, -np.inf), np.nextafter(g, np.inf), -np.linspace(-5, 7, 681) / 0.005,
                        [0.0, -0.0, 707.6, -707.6, 1e-300, -1e-300, 5e-324]])
    return x[np.abs(x) < EXP_MAIN]


def exp_outside_args():
    """|x| >= 707.7 up to 800 (finite results, overflow, subnormal results, underflow), the infinities and NaN."""
    rng = np.random.default_rng(2026)
    a = np.concatenate([rng.uniform(707.7, 800.0, 20_000), np.linspace(707.7, 800.0, 1847), [EXP_MAIN, 709.0, 710.0, 745.0, 746.0, 800.0]])
    return np.concatenate([a, -a, [np.inf, -np.inf, np.nan]])


def interface_n(e):
    """The interface scenario's n from e = exp(-y / 0.005), as the reference's numpy evaluates it"""
    with np.errstate(over="ignore"):
        return np.sqrt(2.0) - (np.sqrt(2.0) - 1.0) / (1.0 + e)


def ulp_distance(a, b):
    """|a - b| in units of the spacing at the larger magnitude (finite a, b)"""
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def avx512_skx():
    """True where this host's numpy dispatches float64 exp and arctan2 to SVML"""
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    return bool(feat.get("AVX512_SKX"))
