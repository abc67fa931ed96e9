"""CPU: rtmi_debug_arctan2, rtmi_debug_rcp14_table and rtmi_debug_exp are declared, exported and bound with the header's
signatures and report argument errors before any device work; and on the argument sets of tests/elementary_sets.py -- the ones
tests/test_gpu_elementary.py holds the device to -- the oracle's restatements give numpy's bits, so that a mismatch on the device
is the device's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import elementary_sets as E
from oracle import rt_oracle as O
from raytracing_amd import _lib

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_debug_arctan2", "rtmi_debug_rcp14_table", "rtmi_debug_exp")

svml = pytest.mark.skipif(not E.avx512_skx(), reason="numpy does not use SVML's exp and arctan2 on this CPU")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(E.ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_header_declares_the_entries():
    assert _prototype("rtmi_debug_arctan2") == ["int64_t n", "const double *y", "const double *x", "double *out"]
    assert _prototype("rtmi_debug_rcp14_table") == ["uint16_t *out65536"]
    assert _prototype("rtmi_debug_exp") == ["int64_t n", "const double *x", "double *out"]


def test_ctypes_signatures_and_exports():
    assert _lib.SYMBOLS["rtmi_debug_arctan2"] == (C.c_int, [C.c_int64, _dp, _dp, _dp])
    assert _lib.SYMBOLS["rtmi_debug_rcp14_table"] == (C.c_int, [C.POINTER(C.c_uint16)])
    assert _lib.SYMBOLS["rtmi_debug_exp"] == (C.c_int, [C.c_int64, _dp, _dp])
    _lib.lib()                                  # maps the HIP runtime first (raytracing_amd._lib)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7   # the entries are additive


def test_argument_errors_come_before_device_work():
    """-1 (argument), not the 'no device' error the first device call gives on a machine without a GPU; n == 0 is nothing to do."""
    L = _lib.lib()
    a = np.zeros(4)
    p = _lib.dptr(a)
    calls = [("rtmi_debug_arctan2", (4, None, p, p)), ("rtmi_debug_arctan2", (4, p, None, p)), ("rtmi_debug_arctan2", (4, p, p, None)),
             ("rtmi_debug_arctan2", (-1, p, p, p)), ("rtmi_debug_exp", (4, None, p)), ("rtmi_debug_exp", (4, p, None)),
             ("rtmi_debug_exp", (-1, p, p)), ("rtmi_debug_rcp14_table", (None,))]
    for name, args in calls:
        assert getattr(L, name)(*args) == -1 and name.encode() in L.rtmi_last_error()
    assert L.rtmi_debug_arctan2(0, p, p, p) == 0 and L.rtmi_debug_exp(0, p, p) == 0


def test_table_decoder_of_the_tests():
    """The decoder the GPU test compares the device's table with: 14-bit mantissas of 1/(1 + k/65536) on a 2^-16 grid, within the
    instruction's 2^-14 relative error, never increasing."""
    T = E.rcp14_table().astype(np.int64)
    assert T[0] == 0xfffc and np.all((np.diff(T) <= 0) & (np.diff(T) >= -2))
    k = np.arange(1, 65536)
    r = (1.0 + T[1:] / 65536.0) / 2.0            # vrcp14pd: exponent field 0x3fd - 0x3ff + bias, mantissa T
    assert np.abs(r * (1.0 + k / 65536.0) - 1.0).max() < 2.0 ** -14


def test_arctan2_sets_cover_every_table_entry_and_both_paths():
    y, x = E.arctan2_pairs()
    main = E.arctan2_main(y, x)
    assert E.rcp14_indices_read(y, x).size == 65536
    assert 1_800_000 < main.sum() < y.size and (~main).sum() > 8_000
    ay, ax = np.abs(y[main]), np.abs(x[main])
    for q in (((x > 0) & (y > 0)), ((x < 0) & (y > 0)), ((x < 0) & (y < 0)), ((x > 0) & (y < 0))):
        with np.errstate(over="ignore"):
            r = (np.abs(y) / np.abs(x))[main & q]
        edges = (0,) + E.OCTANT_SWITCHES + (np.inf,)
        assert all(np.any((r > lo) & (r < hi)) for lo, hi in zip(edges[:-1], edges[1:]))     # five base points per quadrant
    for c in E.OCTANT_SWITCHES:                  # equality itself, and both neighbours
        assert np.sum(c * ax == ay) >= 40_000 and np.sum(np.nextafter(c * ax, 0) == ay) >= 40_000 and np.sum(np.nextafter(c * ax, np.inf) == ay) >= 40_000


@svml
def test_oracle_arctan2_is_numpys_on_the_sets():
    y, x = E.arctan2_pairs()
    o, ref = O.np_arctan2(y, x), np.arctan2(y, x)
    main = E.arctan2_main(y, x)
    bad = _bits(o[main]) != _bits(ref[main])
    assert not bad.any(), f"{bad.sum()} of {main.sum()} main-path pairs differ"
    # outside the main path: SVML's scalar fall-back, libm's atan2 on both sides
    assert np.all(E.ulp_distance(o[~main], ref[~main]) <= 2)
    y, x = E.arctan2_special_grid()
    with np.errstate(invalid="ignore"):
        o, ref = O.np_arctan2(y, x), np.arctan2(y, x)
    nan = np.isnan(y) | np.isnan(x)
    assert np.all(np.isnan(o[nan])) and np.all(np.isnan(ref[nan]))
    exact = ~nan & ((y == 0) | (x == 0) | np.isinf(y) | np.isinf(x))
    assert np.array_equal(_bits(o[exact]), _bits(ref[exact]))
    rest = ~nan & ~exact
    assert np.all(E.ulp_distance(o[rest], ref[rest]) <= 2)


@svml
def test_oracle_exp_is_numpys_on_the_sets():
    x = E.exp_main_args()
    assert x.size > 2_600_000 and np.abs(x).max() < E.EXP_MAIN
    bad = _bits(O.np_exp(x)) != _bits(np.exp(x))
    assert not bad.any(), f"{bad.sum()} of {x.size} arguments differ"
    x = E.exp_outside_args()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e, ref = O.np_exp(x), np.exp(x)
    assert np.array_equal(_bits(E.interface_n(e)), _bits(E.interface_n(ref)))
    for f in (np.isinf, np.isnan, lambda v: v == 0):
        assert np.array_equal(f(e), f(ref))
