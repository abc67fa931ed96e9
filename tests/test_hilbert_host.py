"""CPU: the entries of the device's Hilbert transform and of least-squares migration of the full trace (rtmi_hilbert_taps,
rtmi_kirchhoff_hilbert, rtmi_kirchhoff_hilbert_dev, rtmi_kirchhoff_lsqr_full, rtmi_debug_hilbert) are declared, exported and bound
with the header's signatures; the ABI version is still 7; every refusal that needs no handle is reported before any device work
(RTMI_ERR_ARG naming the argument); the Python methods check shapes, dtypes and devices before the library is called.  The
refusals that need a handle are in tests/test_gpu_hilbert.py and tests/test_gpu_kirchhoff_lsqr_full.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_hilbert_taps", "rtmi_kirchhoff_hilbert", "rtmi_kirchhoff_hilbert_dev", "rtmi_kirchhoff_lsqr_full", "rtmi_debug_hilbert")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_hilbert_taps") == ["int64_t n", "double *taps"]
    assert _prototype("rtmi_kirchhoff_hilbert") == ["rtmi_kirchhoff *k", "const double *x", "double *y"]
    assert _prototype("rtmi_kirchhoff_hilbert_dev") == ["rtmi_kirchhoff *k", "const double *d_x", "const double *d_add", "int32_t negate",
                                                        "double *d_y"]
    assert _prototype("rtmi_kirchhoff_lsqr_full") == _prototype("rtmi_kirchhoff_lsqr")
    assert _prototype("rtmi_debug_hilbert") == ["const double *x", "int64_t N", "int64_t nt", "const double *add", "int32_t negate",
                                                "double *y"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)
    # no "Not covered" list names the Hilbert transform or handles with kmah as missing any more
    for m in re.finditer(r"Not covered:(.*?)\*/", src, flags=re.S):
        assert not re.search(r"\bH\b|kmah|Hilbert", m.group(1)), m.group(1)


def test_ctypes_signatures_and_exports():
    assert _lib.SYMBOLS["rtmi_hilbert_taps"] == (C.c_int, [C.c_int64, _dp])
    assert _lib.SYMBOLS["rtmi_kirchhoff_hilbert"] == (C.c_int, [C.c_void_p, _dp, _dp])
    assert _lib.SYMBOLS["rtmi_kirchhoff_hilbert_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
    assert _lib.SYMBOLS["rtmi_kirchhoff_lsqr_full"] == _lib.SYMBOLS["rtmi_kirchhoff_lsqr"]
    assert _lib.SYMBOLS["rtmi_debug_hilbert"] == (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, _dp])
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("hilbert", "hilbert_device", "lsqr"):
        assert callable(getattr(rt_bench.Kirchhoff, name))
    assert callable(rt_bench.hilbert_taps) and callable(rt_bench.debug_hilbert) and callable(rt_bench.hilbert)
    assert _lib.HILBERT_MAX_NT == 16384


FAKE = C.c_void_p(8)              # never dereferenced: every check below comes before the handle is read
BUF = (C.c_double * 8)()


def _refused(rc, who, name):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who + b": "), msg
    assert re.search(rb"\b" + re.escape(name) + rb"\b", msg[len(who) + 2:]), msg


def test_refusals_that_need_no_handle():
    L = _lib.lib()
    p = C.c_void_p(64)
    _refused(L.rtmi_hilbert_taps(8, None), b"rtmi_hilbert_taps", b"taps")
    for n in (0, -1, -(1 << 40)):
        _refused(L.rtmi_hilbert_taps(n, BUF), b"rtmi_hilbert_taps", b"n")
    _refused(L.rtmi_kirchhoff_hilbert(None, BUF, BUF), b"rtmi_kirchhoff_hilbert", b"handle")
    _refused(L.rtmi_kirchhoff_hilbert(FAKE, None, BUF), b"rtmi_kirchhoff_hilbert", b"x")
    _refused(L.rtmi_kirchhoff_hilbert(FAKE, BUF, None), b"rtmi_kirchhoff_hilbert", b"y")
    _refused(L.rtmi_kirchhoff_hilbert_dev(None, p, None, 0, p), b"rtmi_kirchhoff_hilbert_dev", b"handle")
    _refused(L.rtmi_kirchhoff_hilbert_dev(FAKE, None, None, 0, p), b"rtmi_kirchhoff_hilbert_dev", b"d_x")
    _refused(L.rtmi_kirchhoff_hilbert_dev(FAKE, p, None, 0, None), b"rtmi_kirchhoff_hilbert_dev", b"d_y")
    _refused(L.rtmi_debug_hilbert(None, 1, 8, None, 0, BUF), b"rtmi_debug_hilbert", b"x")
    _refused(L.rtmi_debug_hilbert(BUF, 1, 8, None, 0, None), b"rtmi_debug_hilbert", b"y")
    _refused(L.rtmi_debug_hilbert(BUF, 0, 8, None, 0, BUF), b"rtmi_debug_hilbert", b"N")
    _refused(L.rtmi_debug_hilbert(BUF, 1, 0, None, 0, BUF), b"rtmi_debug_hilbert", b"nt")
    _refused(L.rtmi_debug_hilbert(BUF, 1, 16385, None, 0, BUF), b"rtmi_debug_hilbert", b"nt")


def _params(**kw):
    d = dict(iter_lim=5, damp=0.0, atol=0.0, btol=0.0)
    d.update(kw)
    lp = _lib.LsqrParams()
    for k, v in d.items():
        setattr(lp, k, v)
    return lp


BAD = [
    (dict(k=None), b"handle"), (dict(lp=None), b"params"), (dict(data=None), b"data"), (dict(x=None), b"x"),
    (dict(lp=_params(iter_lim=0)), b"iter_lim"), (dict(lp=_params(damp=-0.1)), b"damp"), (dict(lp=_params(damp=float("nan"))), b"damp"),
    (dict(lp=_params(atol=-1e-9)), b"atol"), (dict(lp=_params(btol=float("inf"))), b"btol"),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_lsqr_full_refusals_come_before_device_work(case):
    kw, name = BAD[case]
    a = dict(k=FAKE, lp=_params(), data=BUF, x=BUF)
    a.update(kw)
    st = _lib.LsqrStats()
    rc = _lib.lib().rtmi_kirchhoff_lsqr_full(a["k"], None if a["lp"] is None else C.byref(a["lp"]), a["data"], a["x"], None, C.byref(st))
    _refused(rc, b"rtmi_kirchhoff_lsqr_full", name)


def test_taps_of_the_lengths_that_have_none():
    for n in (1, 2):
        assert rt_bench.hilbert_taps(n).shape == (0,)
    assert rt_bench.hilbert_taps(3).shape == (1,) and rt_bench.hilbert_taps(4).shape == (1,)
    with pytest.raises(_lib.RtmiError, match="rtmi_hilbert_taps: n must be >= 1"):
        rt_bench.hilbert_taps(0)


class _Shape(rt_bench.Kirchhoff):
    """the shape checks of a Kirchhoff without a handle: the library is never reached"""

    def __init__(self, N=3, nt=8, nb=1, ny=2, nx=5, kmah=False):
        self.N, self.nt, self.nb, self.nbin, self.ny, self.nx = N, nt, nb, 0 if nb == 1 else nb, ny, nx
        self.karr, self.has_kmah, self._h = 1, kmah, None


def test_python_methods_check_shapes_dtypes_and_devices_first():
    import torch
    op = _Shape(kmah=True)
    for bad in ("fft", "host", "", True, 1):
        with pytest.raises(ValueError, match="hilbert must be None or"):
            op.lsqr(np.zeros((3, 8)), 4, hilbert=bad)
    with pytest.raises(ValueError, match=r"lsqr: d must be \[N, nt\]"):
        op.lsqr(np.zeros((3, 7)), 4, hilbert="device")
    with pytest.raises(ValueError, match="iter_lim"):
        op.lsqr(np.zeros((3, 8)), 0, hilbert="device")
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(np.zeros((3, 8)), 4, hilbert="device")
    with pytest.raises(ValueError, match=r"hilbert: d must be \[N, nt\]"):
        op.hilbert(np.zeros((3, 9)))
    with pytest.raises(RuntimeError, match="closed"):
        op.hilbert(np.zeros((3, 8)))
    good = torch.zeros((3, 8), dtype=torch.float64)
    with pytest.raises(TypeError, match="x must be a torch tensor"):
        op.hilbert_device(np.zeros((3, 8)))
    with pytest.raises(TypeError, match="x must be float64"):
        op.hilbert_device(torch.zeros((3, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="x must have 24 values"):
        op.hilbert_device(torch.zeros((3, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="x must be contiguous"):
        op.hilbert_device(torch.zeros((8, 3), dtype=torch.float64).T)
    with pytest.raises(ValueError, match="x must be a tensor on a GPU, not on the host"):
        op.hilbert_device(good)
    with pytest.raises(TypeError, match="add must be a torch tensor"):
        op.hilbert_device(good, add=np.zeros((3, 8)))
    with pytest.raises(TypeError, match="add must be float64"):
        op.hilbert_device(good, add=torch.zeros((3, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="add must have 24 values"):
        op.hilbert_device(good, add=torch.zeros((2, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="add must be contiguous"):
        op.hilbert_device(good, add=torch.zeros((8, 3), dtype=torch.float64).T)
    with pytest.raises(ValueError, match="debug_hilbert: x must be"):
        rt_bench.debug_hilbert(np.zeros(8))
    with pytest.raises(ValueError, match="debug_hilbert: add must have"):
        rt_bench.debug_hilbert(np.zeros((2, 8)), add=np.zeros((2, 7)))
