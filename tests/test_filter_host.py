"""CPU: the entries of the device's trace filter and of least-squares migration with the filter inside the operator
(rtmi_half_derivative_taps, rtmi_kirchhoff_set_filter, rtmi_kirchhoff_filter, rtmi_kirchhoff_filter_dev,
rtmi_kirchhoff_lsqr_filtered) are declared, exported and bound with the header's signatures; the ABI version is still 7; the
library's half-derivative taps are the recurrence in np.longdouble rounded once; every refusal that needs no handle is reported
before any device work (RTMI_ERR_ARG naming the argument); the Python methods check shapes, dtypes and devices before the library
is called.  The refusals that need a handle are in tests/test_gpu_filter.py and tests/test_gpu_kirchhoff_lsqr_filtered.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

import filter_ref as FR

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_half_derivative_taps", "rtmi_kirchhoff_set_filter", "rtmi_kirchhoff_filter", "rtmi_kirchhoff_filter_dev",
         "rtmi_kirchhoff_lsqr_filtered")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_half_derivative_taps") == ["int64_t L", "double dt", "double *taps"]
    assert _prototype("rtmi_kirchhoff_set_filter") == ["rtmi_kirchhoff *k", "const double *taps", "int64_t L", "int64_t origin"]
    assert _prototype("rtmi_kirchhoff_filter") == ["rtmi_kirchhoff *k", "const double *x", "int32_t transpose", "double *y"]
    assert _prototype("rtmi_kirchhoff_filter_dev") == ["rtmi_kirchhoff *k", "const double *d_x", "int32_t transpose", "double *d_y"]
    assert _prototype("rtmi_kirchhoff_lsqr_filtered") == _prototype("rtmi_kirchhoff_lsqr")
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)
    # no "Not covered" list calls the half-derivative or the wavelet the caller's any more
    for m in re.finditer(r"Not covered:(.*?)\*/", src, flags=re.S):
        assert not re.search(r"half-derivative|pi/4|wavelet shaping|the caller filters", m.group(1)), m.group(1)


def test_ctypes_signatures_and_exports():
    assert _lib.SYMBOLS["rtmi_half_derivative_taps"] == (C.c_int, [C.c_int64, C.c_double, _dp])
    assert _lib.SYMBOLS["rtmi_kirchhoff_set_filter"] == (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int64])
    assert _lib.SYMBOLS["rtmi_kirchhoff_filter"] == (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp])
    assert _lib.SYMBOLS["rtmi_kirchhoff_filter_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
    assert _lib.SYMBOLS["rtmi_kirchhoff_lsqr_filtered"] == _lib.SYMBOLS["rtmi_kirchhoff_lsqr"]
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("set_filter", "filter", "filter_device", "lsqr"):
        assert callable(getattr(rt_bench.Kirchhoff, name))
    assert callable(rt_bench.half_derivative_taps)
    assert _lib.FILTER_MAX_NT == 16384 and _lib.FILTER_MAX_TAPS == 2048


@pytest.mark.parametrize("dt", (1.0, 0.004, 0.001))
@pytest.mark.parametrize("L", (1, 2, 3, 64, 2048))
def test_taps_are_the_recurrence_rounded_once(L, dt):
    taps = rt_bench.half_derivative_taps(L, dt)
    want = FR.half_derivative_formula(L, dt)
    assert taps.dtype == np.float64 and taps.shape == (L,) == want.shape
    assert np.all(np.isfinite(taps)) and taps[0] > 0 and np.all(taps[1:] < 0)
    ulp = np.spacing(np.abs(taps))
    err = float(np.max(np.abs(taps.astype(FR.LD) - want) / ulp.astype(FR.LD)))
    print(f"L {L} dt {dt}: largest distance from the recurrence in long double {err:.3f} ulp")
    assert err <= 1.0
    if dt == 1.0 and L >= 3:
        assert taps[0] == 1.0 and taps[1] == -0.5 and taps[2] == -0.125


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
    _refused(L.rtmi_half_derivative_taps(8, 1.0, None), b"rtmi_half_derivative_taps", b"taps")
    for n in (0, -1, -(1 << 40)):
        _refused(L.rtmi_half_derivative_taps(n, 1.0, BUF), b"rtmi_half_derivative_taps", b"L")
    for dt in (0.0, -0.004, float("inf"), float("nan")):
        _refused(L.rtmi_half_derivative_taps(8, dt, BUF), b"rtmi_half_derivative_taps", b"dt")
    _refused(L.rtmi_kirchhoff_set_filter(None, BUF, 8, 0), b"rtmi_kirchhoff_set_filter", b"handle")
    for n in (-1, 2049, 1 << 40):
        _refused(L.rtmi_kirchhoff_set_filter(FAKE, BUF, n, 0), b"rtmi_kirchhoff_set_filter", b"L")
    _refused(L.rtmi_kirchhoff_set_filter(FAKE, None, 8, 0), b"rtmi_kirchhoff_set_filter", b"taps")
    for o in (-1, 8, 1 << 40):
        _refused(L.rtmi_kirchhoff_set_filter(FAKE, BUF, 8, o), b"rtmi_kirchhoff_set_filter", b"origin")
    for bad in (float("nan"), float("inf"), -float("inf")):
        taps = (C.c_double * 8)(*([1.0] * 8))
        taps[5] = bad
        _refused(L.rtmi_kirchhoff_set_filter(FAKE, taps, 8, 0), b"rtmi_kirchhoff_set_filter", b"taps")
    _refused(L.rtmi_kirchhoff_filter(None, BUF, 0, BUF), b"rtmi_kirchhoff_filter", b"handle")
    _refused(L.rtmi_kirchhoff_filter(FAKE, None, 0, BUF), b"rtmi_kirchhoff_filter", b"x")
    _refused(L.rtmi_kirchhoff_filter(FAKE, BUF, 0, None), b"rtmi_kirchhoff_filter", b"y")
    _refused(L.rtmi_kirchhoff_filter_dev(None, p, 0, p), b"rtmi_kirchhoff_filter_dev", b"handle")
    _refused(L.rtmi_kirchhoff_filter_dev(FAKE, None, 0, p), b"rtmi_kirchhoff_filter_dev", b"d_x")
    _refused(L.rtmi_kirchhoff_filter_dev(FAKE, p, 0, None), b"rtmi_kirchhoff_filter_dev", b"d_y")


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
def test_lsqr_filtered_refusals_come_before_device_work(case):
    kw, name = BAD[case]
    a = dict(k=FAKE, lp=_params(), data=BUF, x=BUF)
    a.update(kw)
    st = _lib.LsqrStats()
    rc = _lib.lib().rtmi_kirchhoff_lsqr_filtered(a["k"], None if a["lp"] is None else C.byref(a["lp"]), a["data"], a["x"], None,
                                                 C.byref(st))
    _refused(rc, b"rtmi_kirchhoff_lsqr_filtered", name)


def test_half_derivative_taps_refuses_by_name():
    with pytest.raises(_lib.RtmiError, match="rtmi_half_derivative_taps: L must be >= 1"):
        rt_bench.half_derivative_taps(0, 0.004)
    with pytest.raises(_lib.RtmiError, match="rtmi_half_derivative_taps: dt must be"):
        rt_bench.half_derivative_taps(4, 0.0)


class _Shape(rt_bench.Kirchhoff):
    """the shape checks of a Kirchhoff without a handle: the library is never reached"""

    def __init__(self, N=3, nt=8, nb=1, ny=2, nx=5, kmah=False, filt=None):
        self.N, self.nt, self.nb, self.nbin, self.ny, self.nx = N, nt, nb, 0 if nb == 1 else nb, ny, nx
        self.karr, self.has_kmah, self._h, self._filter = 1, kmah, None, filt


def test_python_methods_check_shapes_dtypes_and_devices_first():
    import torch
    d = np.zeros((3, 8))
    op = _Shape(kmah=True)
    with pytest.raises(ValueError, match="filtered=True needs a filter"):
        op.lsqr(d, 4, hilbert="device", filtered=True)
    with pytest.raises(ValueError, match="filtered=True needs a filter"):
        _Shape().lsqr(d, 4, filtered=True)
    op = _Shape(kmah=True, filt=(3, 1))
    with pytest.raises(ValueError, match='filtered=True on a handle with kmah needs hilbert="device"'):
        op.lsqr(d, 4, filtered=True)
    with pytest.raises(ValueError, match=r"lsqr: d must be \[N, nt\]"):
        op.lsqr(np.zeros((3, 7)), 4, hilbert="device", filtered=True)
    with pytest.raises(ValueError, match="iter_lim"):
        op.lsqr(d, 0, hilbert="device", filtered=True)
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 4, hilbert="device", filtered=True)
    with pytest.raises(RuntimeError, match="closed"):
        _Shape(filt=(3, 1)).lsqr(d, 4, filtered=True)          # without kmah hilbert=None is allowed
    with pytest.raises(ValueError, match="taps must be a vector"):
        op.set_filter(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="taps must be a vector"):
        op.set_filter([])
    for taps in ([1.0, 2.0], None):
        with pytest.raises(RuntimeError, match="closed"):
            op.set_filter(taps)
    with pytest.raises(ValueError, match=r"filter: d must be \[N, nt\]"):
        op.filter(np.zeros((3, 9)))
    with pytest.raises(RuntimeError, match="closed"):
        op.filter(d, transpose=True)
    good = torch.zeros((3, 8), dtype=torch.float64)
    with pytest.raises(TypeError, match="x must be a torch tensor"):
        op.filter_device(d)
    with pytest.raises(TypeError, match="x must be float64"):
        op.filter_device(torch.zeros((3, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="x must have 24 values"):
        op.filter_device(torch.zeros((3, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="x must be contiguous"):
        op.filter_device(torch.zeros((8, 3), dtype=torch.float64).T)
    with pytest.raises(ValueError, match="x must be a tensor on a GPU, not on the host"):
        op.filter_device(good, transpose=True)
