"""CPU: the entry points of the Kirchhoff pair over several arrivals (rtmi_kirchhoff_create_multi / _migrate2 / _model2) are
declared, exported and bound with the header's signatures; rtmi_kirchhoff_multi_params has gcc's layout; the ABI version is
still 7; every argument error of create_multi is reported before any device work (RTMI_ERR_ARG naming the argument, not the
'no device' error a device call gives on a machine without a GPU) and creates nothing; a 3-D T still takes
rtmi_kirchhoff_create.  The refusals that need a handle (a null second channel with kmah, the one-arrival calls on a multi
handle) are in tests/test_gpu_kirchhoff_multi.py."""
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
NAMES = ("rtmi_kirchhoff_create_multi", "rtmi_kirchhoff_migrate2", "rtmi_kirchhoff_model2")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_kirchhoff_create_multi") == [
        "const rtmi_kirchhoff_multi_params *kp", "const double *T", "const double *amp", "const double *theta", "const double *kmah",
        "const int32_t *isrc", "const int32_t *irec", "const double *w", "rtmi_kirchhoff **out"]
    assert _prototype("rtmi_kirchhoff_migrate2") == ["rtmi_kirchhoff *k", "const double *data0", "const double *data1", "double *image",
                                                     "rtmi_kirchhoff_stats *st"]
    assert _prototype("rtmi_kirchhoff_model2") == ["rtmi_kirchhoff *k", "const double *model", "double *data0", "double *data1",
                                                   "rtmi_kirchhoff_stats *st"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_KIRCHHOFF_MAX_ARRIVALS\s+4\b", src) and _lib.KIRCHHOFF_MAX_ARRIVALS == 4


def test_ctypes_signatures_and_exports():
    KS = C.POINTER(_lib.KirchhoffStats)
    assert _lib.SYMBOLS["rtmi_kirchhoff_create_multi"] == (C.c_int, [C.POINTER(_lib.KirchhoffMultiParams), _dp, _dp, _dp, _dp, _ip, _ip,
                                                                     _dp, C.POINTER(C.c_void_p)])
    assert _lib.SYMBOLS["rtmi_kirchhoff_migrate2"] == (C.c_int, [C.c_void_p, _dp, _dp, _dp, KS])
    assert _lib.SYMBOLS["rtmi_kirchhoff_model2"] == (C.c_int, [C.c_void_p, _dp, _dp, _dp, KS])
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7
    for name in ("migrate_channels", "model_channels", "migrate", "model", "as_linear_operator", "from_table"):
        assert callable(getattr(rt_bench.Kirchhoff, name))
    assert callable(rt_bench.hilbert)


def test_params_layout_matches_gcc(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\n#define P rtmi_kirchhoff_multi_params\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(P), offsetof(P, nt), offsetof(P, t0), '
                   'offsetof(P, nbin), offsetof(P, karr), offsetof(P, dopen), offsetof(P, reserved), '
                   'sizeof(rtmi_kirchhoff_params)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = _lib.KirchhoffMultiParams
    assert got == [C.sizeof(P), P.nt.offset, P.t0.offset, P.nbin.offset, P.karr.offset, P.dopen.offset, P.reserved.offset,
                   C.sizeof(_lib.KirchhoffParams)]


def _params(**kw):
    d = dict(nx=5, ny=4, P=3, N=6, nt=16, t0=0.0, dt=0.001, nbin=0, karr=2, dopen=0.0)
    d.update(kw)
    kp = _lib.KirchhoffMultiParams()
    for k, v in d.items():
        setattr(kp, k, v)
    return kp


TAB = np.zeros(3 * 2 * 4 * 5)
SRC = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
REC = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)


def _create(kp=None, T=TAB, amp=None, theta=None, kmah=None, isrc=SRC, irec=REC, w=None, out=True, null_kp=False):
    L = _lib.lib()
    h = C.c_void_p(0xdead)
    ip = lambda a: None if a is None else a.ctypes.data_as(_ip)   # noqa: E731
    rc = L.rtmi_kirchhoff_create_multi(None if null_kp else C.byref(kp or _params()), _lib.dptr(T), _lib.dptr(amp), _lib.dptr(theta),
                                       _lib.dptr(kmah), ip(isrc), ip(irec), _lib.dptr(w), C.byref(h) if out else None)
    return rc, L.rtmi_last_error(), h


BAD = [
    (dict(kp=_params(karr=0)), b"karr"), (dict(kp=_params(karr=5)), b"karr"), (dict(kp=_params(karr=-1)), b"karr"),
    (dict(kp=_params(karr=16), kmah=TAB), b"karr"),
    # section 14's refusals carry over
    (dict(null_kp=True), b"kp"), (dict(T=None), b"T"), (dict(isrc=None), b"isrc"), (dict(irec=None), b"irec"),
    (dict(out=False), b"out"),
    (dict(kp=_params(nx=0)), b"nx"), (dict(kp=_params(ny=0)), b"ny"), (dict(kp=_params(P=0)), b"P"), (dict(kp=_params(N=0)), b"N"),
    (dict(kp=_params(nx=-3)), b"nx"), (dict(kp=_params(nt=1)), b"nt"),
    (dict(kp=_params(nx=1 << 16, ny=(1 << 15) + 1)), b"nx ny"), (dict(kp=_params(nx=1 << 40, ny=1 << 40)), b"nx ny"),
    (dict(kp=_params(dt=0.0)), b"dt"), (dict(kp=_params(dt=float("nan"))), b"dt"), (dict(kp=_params(t0=float("inf"))), b"t0"),
    (dict(kp=_params(nbin=-1)), b"nbin"), (dict(kp=_params(nbin=33, dopen=0.1), theta=TAB), b"nbin"),
    (dict(kp=_params(nbin=4, dopen=0.1)), b"theta"), (dict(kp=_params(nbin=4, dopen=0.0), theta=TAB), b"dopen"),
    (dict(kp=_params(nbin=4, dopen=float("nan")), theta=TAB), b"dopen"),
    (dict(isrc=np.array([0, 0, 1, 3, 2, 2], dtype=np.int32)), b"isrc"), (dict(irec=np.array([-1, 1, 2, 0, 1, 2], dtype=np.int32)), b"irec"),
    (dict(w=np.array([1, 1, float("nan"), 1, 1, 1.0])), b"w"),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_create_multi_argument_errors_come_before_device_work(case):
    kw, name = BAD[case]
    rc, msg, h = _create(**kw)
    assert rc == -1, msg
    assert msg.startswith(b"rtmi_kirchhoff_create_multi: ")
    assert re.search(rb"\b" + re.escape(name) + rb"\b", msg[len(b"rtmi_kirchhoff_create_multi: "):]), msg
    if kw.get("out", True):
        assert h.value is None                    # nothing was created


def test_null_handle_and_buffers():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    fake = C.c_void_p(8)                          # never dereferenced: the buffers are checked with the handle
    assert L.rtmi_kirchhoff_migrate2(None, buf, buf, buf, None) == -1 and b"handle" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_migrate2(fake, None, buf, buf, None) == -1 and b"data0" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_migrate2(fake, buf, buf, None, None) == -1 and b"image" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model2(None, buf, buf, buf, None) == -1 and b"handle" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model2(fake, None, buf, buf, None) == -1 and b"model" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model2(fake, buf, None, buf, None) == -1 and b"data0" in L.rtmi_last_error()


def test_python_class_picks_the_entry_by_the_rank_of_T():
    """an argument error names the create it came from: a 3-D T still takes rtmi_kirchhoff_create"""
    with pytest.raises(_lib.RtmiError, match=": rtmi_kirchhoff_create: .*dopen"):
        rt_bench.Kirchhoff(np.zeros((3, 4, 5)), SRC, REC, 16, 0.001, theta=np.zeros((3, 4, 5)), nbin=4)
    with pytest.raises(_lib.RtmiError, match=": rtmi_kirchhoff_create_multi: .*dopen"):
        rt_bench.Kirchhoff(np.zeros((3, 2, 4, 5)), SRC, REC, 16, 0.001, theta=np.zeros((3, 2, 4, 5)), nbin=4)
    with pytest.raises(_lib.RtmiError, match=": rtmi_kirchhoff_create_multi: .*karr"):
        rt_bench.Kirchhoff(np.zeros((3, 5, 4, 5)), SRC, REC, 16, 0.001)
    with pytest.raises(ValueError, match="kmah must have"):
        rt_bench.Kirchhoff(np.zeros((3, 2, 4, 5)), SRC, REC, 16, 0.001, kmah=np.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="kmah needs"):
        rt_bench.Kirchhoff(np.zeros((3, 4, 5)), SRC, REC, 16, 0.001, kmah=np.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="T must be"):
        rt_bench.Kirchhoff(np.zeros((4, 5)), SRC, REC, 16, 0.001)
