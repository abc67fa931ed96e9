"""CPU: rtmi_first_arrival_grid, rtmi_debug_grid_rows and rtmi_debug_paraxial_rows are declared, exported and bound with the
header's signatures; the parameter and statistics structs have gcc's layout; argument errors are reported before any device
work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_first_arrival_grid") == ["rtmi_batch *b", "int32_t fan_size", "const rtmi_grid_params *gp",
                                                     "int32_t *count", "double *out", "rtmi_grid_stats *st"]
    assert _prototype("rtmi_debug_grid_rows") == ["int32_t rows", "int32_t R", "int32_t fan_size", "const double *x",
                                                  "const double *y", "const double *T", "const double *theta",
                                                  "const int32_t *last", "const double *theta0", "const rtmi_grid_params *gp",
                                                  "int32_t *count", "double *out", "rtmi_grid_stats *st"]
    assert _prototype("rtmi_debug_paraxial_rows") == ["rtmi_batch *b", "double *J", "int32_t *kmah"]


def test_ctypes_signatures_and_exports():
    GP, GS = C.POINTER(_lib.GridParams), C.POINTER(_lib.GridStats)
    assert _lib.SYMBOLS["rtmi_first_arrival_grid"] == (C.c_int, [C.c_void_p, C.c_int32, GP, _ip, _dp, GS])
    assert _lib.SYMBOLS["rtmi_debug_grid_rows"] == (C.c_int, [C.c_int32] * 3 + [_dp] * 4 + [_ip, _dp, GP, _ip, _dp, GS])
    assert _lib.SYMBOLS["rtmi_debug_paraxial_rows"] == (C.c_int, [C.c_void_p, _dp, _ip])
    _lib.lib()                                  # maps the HIP runtime first (raytracing_amd._lib)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("rtmi_first_arrival_grid", "rtmi_debug_grid_rows", "rtmi_debug_paraxial_rows"):
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert rt_bench.GRID_FIELDS == ("T", "theta0", "theta", "ray", "step")
    assert rt_bench.GRID_AMPLITUDE_FIELDS == ("J", "G", "kmah")


def test_struct_layouts_match_gcc(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(rtmi_grid_params), sizeof(rtmi_grid_stats), offsetof(rtmi_grid_params, amplitude), '
                   'offsetof(rtmi_grid_params, ny), offsetof(rtmi_grid_stats, pass_ms), offsetof(rtmi_grid_stats, max_dtheta)); '
                   'return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    GP, GS = _lib.GridParams, _lib.GridStats
    assert got == [C.sizeof(GP), C.sizeof(GS), GP.amplitude.offset, GP.ny.offset, GS.pass_ms.offset, GS.max_dtheta.offset]


def _rows(R=8, rows=4):
    z = np.zeros((rows, R))
    return z, z, z, z, np.full(R, rows - 1, dtype=np.int32), np.zeros(R)


@pytest.mark.parametrize("grid,fan,msg", [
    ((0.0, 0.1, 0, 0.0, 0.1, 4), None, "nx and ny"),
    ((0.0, 0.1, 4, 0.0, 0.1, 0), None, "nx and ny"),
    ((0.0, 0.0, 4, 0.0, 0.1, 4), None, "gdx and gdy"),
    ((0.0, 0.1, 4, 0.0, -0.1, 4), None, "gdx and gdy"),
    ((0.0, np.inf, 4, 0.0, 0.1, 4), None, "gdx and gdy"),
    ((np.nan, 0.1, 4, 0.0, 0.1, 4), None, "gx0 and gy0"),
    ((0.0, 0.1, 4, 0.0, 0.1, 4), 3, "multiple of fan_size"),
])
def test_argument_errors_come_before_device_work(grid, fan, msg):
    """On a machine without a GPU these are argument errors (-1), not the 'no device' error (-2) the first device call gives."""
    with pytest.raises(_lib.RtmiError, match=msg) as e:
        rt_bench.debug_grid_rows(*_rows(), grid, fan_size=fan)
    assert e.value.code == -1


def test_null_and_amplitude_errors():
    L = _lib.lib()
    gp = rt_bench.grid_params((0.0, 0.1, 4, 0.0, 0.1, 4))
    cnt = (C.c_int32 * 16)()
    out = (C.c_double * 128)()
    assert L.rtmi_first_arrival_grid(None, 8, C.byref(gp), cnt, out, None) == -1
    assert b"rtmi_first_arrival_grid" in L.rtmi_last_error()
    assert L.rtmi_debug_paraxial_rows(None, out, cnt) == -1
    gp.amplitude = 1
    x = np.zeros((4, 8)); last = np.full(8, 3, dtype=np.int32); t0 = np.zeros(8)
    rc = L.rtmi_debug_grid_rows(4, 8, 8, *[_lib.dptr(x)] * 4, last.ctypes.data_as(_ip), _lib.dptr(t0), C.byref(gp), cnt, out, None)
    assert rc == -1 and b"amplitude" in L.rtmi_last_error()
