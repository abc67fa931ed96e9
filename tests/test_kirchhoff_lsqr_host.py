"""CPU: the entries of the device-resident Kirchhoff pair and its least-squares solver (rtmi_kirchhoff_migrate_dev / _model_dev,
rtmi_kirchhoff_lsqr, rtmi_debug_fix_norm) are declared, exported and bound with the header's signatures; rtmi_lsqr_params and
rtmi_lsqr_stats have gcc's layout; the ABI version is still 7; every refusal that needs no handle is reported before any device
work (RTMI_ERR_ARG naming the argument, not the 'no device' error a device call gives on a machine without a GPU); the Python
methods check shapes and dtypes before the library is called.  The refusals that need a handle are in
tests/test_gpu_kirchhoff_lsqr.py."""
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
NAMES = ("rtmi_kirchhoff_migrate_dev", "rtmi_kirchhoff_model_dev", "rtmi_kirchhoff_lsqr", "rtmi_debug_fix_norm")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_kirchhoff_migrate_dev") == ["rtmi_kirchhoff *k", "const double *d_data0", "const double *d_data1",
                                                        "double *d_image", "rtmi_kirchhoff_stats *st"]
    assert _prototype("rtmi_kirchhoff_model_dev") == ["rtmi_kirchhoff *k", "const double *d_model", "double *d_data0", "double *d_data1",
                                                      "rtmi_kirchhoff_stats *st"]
    assert _prototype("rtmi_kirchhoff_lsqr") == ["rtmi_kirchhoff *k", "const rtmi_lsqr_params *lp", "const double *data", "double *x",
                                                 "double *history", "rtmi_lsqr_stats *st"]
    assert _prototype("rtmi_debug_fix_norm") == ["const double *x", "int64_t n", "double *norm", "int32_t *e"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_LSQR_RANGE\s+8\b", src) and _lib.LSQR_RANGE == 8
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)
    # no "Not covered" list names device-resident buffers as missing any more
    for m in re.finditer(r"Not covered:(.*?)\*/", src, flags=re.S):
        assert not re.search(r"device-resident\s+data", m.group(1))


def test_ctypes_signatures_and_exports():
    st = C.POINTER(_lib.KirchhoffStats)
    assert _lib.SYMBOLS["rtmi_kirchhoff_migrate_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, st])
    assert _lib.SYMBOLS["rtmi_kirchhoff_model_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, st])
    assert _lib.SYMBOLS["rtmi_kirchhoff_lsqr"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.LsqrParams), _dp, _dp, _dp,
                                                             C.POINTER(_lib.LsqrStats)])
    assert _lib.SYMBOLS["rtmi_debug_fix_norm"] == (C.c_int, [_dp, C.c_int64, _dp, _ip])
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("lsqr", "migrate_device", "model_device", "migrate", "model", "as_linear_operator"):
        assert callable(getattr(rt_bench.Kirchhoff, name))
    assert callable(rt_bench.debug_fix_norm)


def test_struct_layouts_match_gcc(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\n#define P rtmi_lsqr_params\n#define S rtmi_lsqr_stats\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(P), '
                   'offsetof(P, iter_lim), offsetof(P, damp), offsetof(P, atol), offsetof(P, btol), offsetof(P, reserved), sizeof(S), '
                   'offsetof(S, istop), offsetof(S, itn), offsetof(S, r1norm), offsetof(S, r2norm), offsetof(S, anorm), offsetof(S, arnorm), '
                   'offsetof(S, total_ms), offsetof(S, operator_ms), offsetof(S, vector_ms), offsetof(S, bytes_device), '
                   'offsetof(S, reserved)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P, S = _lib.LsqrParams, _lib.LsqrStats
    assert got == [C.sizeof(P), P.iter_lim.offset, P.damp.offset, P.atol.offset, P.btol.offset, P.reserved.offset, C.sizeof(S),
                   S.istop.offset, S.itn.offset, S.r1norm.offset, S.r2norm.offset, S.anorm.offset, S.arnorm.offset, S.total_ms.offset,
                   S.operator_ms.offset, S.vector_ms.offset, S.bytes_device.offset, S.reserved.offset]


def _params(**kw):
    d = dict(iter_lim=5, damp=0.0, atol=0.0, btol=0.0)
    d.update(kw)
    lp = _lib.LsqrParams()
    for k, v in d.items():
        setattr(lp, k, v)
    return lp


FAKE = C.c_void_p(8)              # never dereferenced: every check below comes before the handle is read
BUF = (C.c_double * 8)()
BAD = [
    (dict(k=None), b"handle"), (dict(lp=None), b"params"), (dict(data=None), b"data"), (dict(x=None), b"x"),
    (dict(lp=_params(iter_lim=0)), b"iter_lim"), (dict(lp=_params(iter_lim=-3)), b"iter_lim"),
    (dict(lp=_params(damp=-0.1)), b"damp"), (dict(lp=_params(damp=float("nan"))), b"damp"), (dict(lp=_params(damp=float("inf"))), b"damp"),
    (dict(lp=_params(atol=-1e-9)), b"atol"), (dict(lp=_params(atol=float("nan"))), b"atol"),
    (dict(lp=_params(btol=-1.0)), b"btol"), (dict(lp=_params(btol=float("inf"))), b"btol"),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_lsqr_refusals_come_before_device_work(case):
    kw, name = BAD[case]
    a = dict(k=FAKE, lp=_params(), data=BUF, x=BUF)
    a.update(kw)
    L = _lib.lib()
    st = _lib.LsqrStats()
    rc = L.rtmi_kirchhoff_lsqr(a["k"], None if a["lp"] is None else C.byref(a["lp"]), a["data"], a["x"], None, C.byref(st))
    msg = L.rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(b"rtmi_kirchhoff_lsqr: ")
    assert re.search(rb"\b" + re.escape(name) + rb"\b", msg[len(b"rtmi_kirchhoff_lsqr: "):]), msg


def test_null_handle_and_buffers_of_the_device_pair_and_the_norm():
    L = _lib.lib()
    p = C.c_void_p(64)
    assert L.rtmi_kirchhoff_migrate_dev(None, p, p, p, None) == -1 and b"handle" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_migrate_dev(FAKE, None, p, p, None) == -1 and b"d_data0" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_migrate_dev(FAKE, p, p, None, None) == -1 and b"d_image" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model_dev(None, p, p, p, None) == -1 and b"handle" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model_dev(FAKE, None, p, p, None) == -1 and b"d_model" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model_dev(FAKE, p, None, p, None) == -1 and b"d_data0" in L.rtmi_last_error()
    nrm, e = C.c_double(), C.c_int32()
    assert L.rtmi_debug_fix_norm(None, 8, C.byref(nrm), C.byref(e)) == -1 and b"x" in L.rtmi_last_error()
    assert L.rtmi_debug_fix_norm(BUF, 0, C.byref(nrm), C.byref(e)) == -1 and b"n must" in L.rtmi_last_error()
    bad = (C.c_double * 2)(1.0, float("nan"))
    assert L.rtmi_debug_fix_norm(bad, 2, C.byref(nrm), C.byref(e)) == -1 and b"not finite" in L.rtmi_last_error()


class _Shape(rt_bench.Kirchhoff):
    """the shape checks of a Kirchhoff without a handle: the library is never reached"""

    def __init__(self, N=3, nt=8, nb=1, ny=2, nx=5, kmah=False):
        self.N, self.nt, self.nb, self.nbin, self.ny, self.nx = N, nt, nb, 0 if nb == 1 else nb, ny, nx
        self.karr, self.has_kmah, self._h = 1, kmah, None


def test_python_methods_check_shapes_and_dtypes_first():
    import torch
    op = _Shape()
    with pytest.raises(ValueError, match=r"lsqr: d must be \[N, nt\]"):
        op.lsqr(np.zeros((3, 7)), 4)
    with pytest.raises(ValueError, match="iter_lim"):
        op.lsqr(np.zeros((3, 8)), 0)
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(np.zeros((3, 8)), 4)
    with pytest.raises(TypeError, match="torch tensor"):
        op.migrate_device(np.zeros((3, 8)))
    with pytest.raises(TypeError, match="float64"):
        op.migrate_device(torch.zeros((3, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="on a GPU, not on the host"):
        op.migrate_device(torch.zeros((3, 8), dtype=torch.float64))
    with pytest.raises(TypeError, match="float64"):
        op.model_device(torch.zeros((2, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="on a GPU, not on the host"):
        op.model_device(torch.zeros((2, 5), dtype=torch.float64))
    with pytest.raises(TypeError, match="torch tensor"):
        op.model_device([0.0] * 10)
    with pytest.raises(ValueError, match="d0 must have 24 values"):
        op.migrate_device(torch.zeros((3, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="d1 must have 24 values"):
        op.migrate_device(torch.zeros((3, 8), dtype=torch.float64), torch.zeros((2, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="m must have 10 values"):
        op.model_device(torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        op.model_device(torch.zeros((5, 2), dtype=torch.float64).T)
    with pytest.raises(ValueError, match="needs d1"):
        _Shape(kmah=True).migrate_device(torch.zeros((3, 8), dtype=torch.float64))
