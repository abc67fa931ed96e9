"""CPU: rtmi_paraxial and rtmi_field_eval_dgrad are declared, exported and bound with the header's signatures; their argument
errors are reported before any device work."""
import ctypes as C
import os
import re

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_entries():
    assert _prototype("rtmi_paraxial") == ["rtmi_batch *b", "const double line[3]", "int32_t kmax", "int32_t *count",
                                           "double *at_line", "double *at_end"]
    assert _prototype("rtmi_field_eval_dgrad") == ["const rtmi_field *f", "int64_t npts", "const double *x", "const double *y",
                                                   "double *gx_x", "double *gx_y", "double *gy_x", "double *gy_y"]


def test_ctypes_signatures():
    assert _lib.SYMBOLS["rtmi_paraxial"] == (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip, _dp, _dp])
    assert _lib.SYMBOLS["rtmi_field_eval_dgrad"] == (C.c_int, [C.c_void_p, C.c_int64] + [_dp] * 6)
    L = _lib.lib()
    assert L.rtmi_paraxial.argtypes == _lib.SYMBOLS["rtmi_paraxial"][1]
    assert L.rtmi_field_eval_dgrad.argtypes == _lib.SYMBOLS["rtmi_field_eval_dgrad"][1]
    assert rt_bench.PARAXIAL_FIELDS == ("Q1", "P1", "Q2", "P2", "J", "G", "kmah")


def test_library_exports_both():
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "rtmi_paraxial") and hasattr(L, "rtmi_field_eval_dgrad")


def test_null_arguments_are_argument_errors():
    L = _lib.lib()
    out = (C.c_double * 7)()
    assert L.rtmi_paraxial(None, None, 0, None, None, out) == -1
    assert b"rtmi_paraxial" in L.rtmi_last_error()
    x = (C.c_double * 1)(0.0)
    assert L.rtmi_field_eval_dgrad(None, 1, x, x, x, x, x, x) == -1
    assert b"rtmi_field_eval_dgrad" in L.rtmi_last_error()
