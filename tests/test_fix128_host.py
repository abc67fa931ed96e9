"""The 128-bit fixed-point accumulator of the order-independent sums (raytracing_amd/csrc/rt_fix128.h) checked on the CPU: the
header compiled for the host with g++ (tests/native/fix128_check.cpp).  The one conversion back to double that
rtmi_traveltime_backproject (on the host) and rtmi_kirchhoff_model (on the device) share, against (double) of the value as an
__int128 and against Python's correctly rounded float(int); add128's carry and borrow into the high word.  No GPU involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_up = C.POINTER(C.c_ulonglong)
_dp = C.POINTER(C.c_double)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def fixlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fix128") / "libfix128_check.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "native", "fix128_check.cpp")])
    L = C.CDLL(so)
    L.fix_bias.restype = C.c_ulonglong
    L.fix_exponent.argtypes = [C.c_double]
    L.fix_convert.argtypes = [C.c_long, _up, _up, _dp, _dp]
    L.fix_add.argtypes = [_up, C.c_long, C.POINTER(C.c_longlong), C.POINTER(C.c_int), _up]
    return L


def _words(q):
    """(lo, hi) of the accumulator that holds q quanta: hi 2^64 + lo - 2^63 = q (mod 2^128)"""
    w = (q + (1 << 63)) % (1 << 128)
    return w & M64, w >> 64


def _value(lo, hi):
    w = ((int(hi) << 64) | int(lo)) - (1 << 63)
    return w - (1 << 128) if w >= (1 << 127) else w


def _convert(L, lo, hi):
    lo = np.ascontiguousarray(lo, dtype=np.uint64); hi = np.ascontiguousarray(hi, dtype=np.uint64)
    got = np.empty(len(lo)); want = np.empty(len(lo))
    L.fix_convert(len(lo), lo.ctypes.data_as(_up), hi.ctypes.data_as(_up), got.ctypes.data_as(_dp), want.ctypes.data_as(_dp))
    return got, want


def test_constants_and_exponent(fixlib):
    assert fixlib.fix_bits() == 57 and fixlib.fix_bias() == 1 << 63
    # bound = f 2^ex, f in [0.5, 1): the quantum is 2^(ex - 57), so that bound is at most 2^57 quanta
    for bound, ex in ((1.0, 1), (0.75, 0), (3.0, 2), (2.0 ** -40, -39), (1e300, 997), (0.0, 0)):
        assert fixlib.fix_exponent(bound) == ex - 57
        assert bound <= 2.0 ** 57 * 2.0 ** (ex - 57)


def test_conversion_edge_cases(fixlib):
    """hi = 0 and hi = all-ones, single carries, ties at the rounding position, small values of either sign, the ends of the
    range: the nearest double, ties to even."""
    q = [0, 1, -1, 2, -2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, -(1 << 63), -(1 << 63) - 1, -(1 << 63) + 1,
         (1 << 64) - 1, 1 << 64, (1 << 64) + 1, -(1 << 64), (1 << 127) - 1 - (1 << 63), -(1 << 127) + (1 << 63),
         (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3, -(1 << 53) - 1, -(1 << 53) - 3]
    for top in (54, 63, 64, 65, 70, 100, 120):             # a 53-bit mantissa below bit `top`: half-way cases and their neighbours
        ulp = 1 << (top - 53)
        for m in ((1 << 52) | 1, (1 << 52) | 2, (1 << 53) - 1):      # odd, even, all ones (rounds up into the next binade)
            for d in (-1, 0, 1):
                q += [m * ulp + ulp // 2 + d, -(m * ulp + ulp // 2 + d)]
    pairs = [_words(v) for v in q]
    pairs += [(lo, hi) for hi in (0, M64) for lo in (0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64)]
    lo, hi = zip(*pairs)
    got, want = _convert(fixlib, lo, hi)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    exact = np.array([float(_value(a, b)) for a, b in pairs])        # int -> float in Python rounds correctly
    assert np.array_equal(got, exact)


def test_conversion_random_pairs(fixlib):
    """10^5 accumulators of every magnitude and either sign: a random high word shifted down by a random count (complemented
    for a negative value), and under an empty high word a low word a random distance from the bias."""
    rng = np.random.default_rng(7)
    n = 100_000
    hi = rng.integers(0, 1 << 62, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)
    lo = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    small = (lo >> np.uint64(1)) >> rng.integers(0, 63, n).astype(np.uint64)          # |value| = small: lo = 2^63 +- small
    lo = np.where(hi == 0, np.where(rng.integers(0, 2, n) == 1, np.uint64(1 << 63) + small, np.uint64(1 << 63) - small), lo)
    hi = np.where(rng.integers(0, 2, n) == 1, ~hi, hi)
    got, want = _convert(fixlib, lo, hi)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    k = rng.integers(0, n, 2000)
    assert np.array_equal(got[k], np.array([float(_value(lo[i], hi[i])) for i in k]))
    assert (hi == 0).sum() > 1000 and (hi == np.uint64(M64)).sum() > 1000 and (np.abs(got) < 2.0 ** 53).sum() > 100


def _add(L, s):
    acc = (C.c_ulonglong * 2)(1 << 63, 0)
    s = np.ascontiguousarray(s, dtype=np.int64)
    issued = np.empty(len(s), dtype=np.int32); hi = np.empty(len(s), dtype=np.uint64)
    L.fix_add(acc, len(s), s.ctypes.data_as(C.POINTER(C.c_longlong)), issued.ctypes.data_as(C.POINTER(C.c_int)), hi.ctypes.data_as(_up))
    return _value(acc[0], acc[1]), issued, hi


def test_add128_carry_and_borrow(fixlib):
    """The low word starts at the bias 2^63.  Sums that stay within it issue one add and leave the high word alone; the third
    2^62 carries into it, the third -2^62 borrows from it (all-ones), and coming back undoes either; a zero issues nothing."""
    big = 1 << 62
    total, issued, hi = _add(fixlib, [big, big - 1, 0, 1, big])
    assert total == 3 * big and list(issued) == [1, 1, 0, 2, 1] and list(hi) == [0, 0, 0, 1, 1]
    total, issued, hi = _add(fixlib, [-big, -big, -1, 0, 1, -big])
    assert total == -3 * big and list(issued) == [1, 1, 2, 0, 2, 2] and list(hi) == [0, 0, M64, M64, 0, M64]
    total, issued, hi = _add(fixlib, [-(1 << 63), -(1 << 63), (1 << 63) - 1, (1 << 63) - 1, 2])
    assert total == 0 and list(hi) == [0, M64, M64, 0, 0] and list(issued) == [1, 2, 1, 2, 1]
    rng = np.random.default_rng(3)
    s = rng.integers(-(1 << 62), 1 << 62, 5000)
    s[::17] = 0
    total, issued, hi = _add(fixlib, s)
    assert total == sum(int(v) for v in s)
    before = np.concatenate([np.zeros(1, dtype=np.uint64), hi[:-1]])
    assert np.array_equal(issued == 0, s == 0)
    assert np.array_equal(issued == 2, hi != before)          # the high word is written exactly when it changes
    assert (hi != before).sum() > 500
