"""CPU: the multi-vector tomography entries (rtmi_tomo_apply_multi, _transpose_multi, their _dev forms, rtmi_tomo_lsqr_multi;
DESIGN.md section 28) are declared, exported and bound with the header's signatures, and the ABI version stays 7; the refusals
that need no device -- a null handle, nrhs outside 1 .. 64, unknown flag bits, a regulariser weight that is negative or not
finite -- come before the handle is read; the pure-numpy helpers of the resolution and bootstrap tests (checkerboard, spikes,
bootstrap_weights) give the stated shapes and values.  What needs a handle is in tests/test_gpu_tomo_multi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_tomo_apply_multi", "rtmi_tomo_apply_multi_dev", "rtmi_tomo_transpose_multi", "rtmi_tomo_transpose_multi_dev",
         "rtmi_tomo_lsqr_multi")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    st = "rtmi_tomo_stats *st"
    assert _prototype("rtmi_tomo_apply_multi") == ["rtmi_tomo *t", "int32_t nrhs", "const double *x", "double *y", st]
    assert _prototype("rtmi_tomo_apply_multi_dev") == ["rtmi_tomo *t", "int32_t nrhs", "const double *d_x", "double *d_y", st]
    assert _prototype("rtmi_tomo_transpose_multi") == ["rtmi_tomo *t", "int32_t nrhs", "const double *w", "double *g", st]
    assert _prototype("rtmi_tomo_transpose_multi_dev") == ["rtmi_tomo *t", "int32_t nrhs", "const double *d_w", "double *d_g", st]
    assert _prototype("rtmi_tomo_lsqr_multi") == ["rtmi_tomo *t", "rtmi_tomo_basis *p", "const rtmi_lsqr_params *lp",
                                                  "const rtmi_lsqr_options *lo", "const rtmi_tomo_reg *reg", "int32_t nrhs",
                                                  "int32_t flags", "const double *rhs", "double *c", "double *x", "double *history",
                                                  "rtmi_lsqr_stats *st"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_LSQR_MULTI_MAX\s+64\b", src) and _lib.LSQR_MULTI_MAX == 64
    assert re.search(r"#define\s+RTMI_LSQR_MULTI_ROW_WEIGHT\s+1\b", src) and _lib.LSQR_MULTI_ROW_WEIGHT == 1
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)


def test_ctypes_signatures_and_exports():
    st = C.POINTER(_lib.TomoStats)
    assert _lib.SYMBOLS["rtmi_tomo_apply_multi"] == (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, st])
    assert _lib.SYMBOLS["rtmi_tomo_transpose_multi"] == (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, st])
    assert _lib.SYMBOLS["rtmi_tomo_apply_multi_dev"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, st])
    assert _lib.SYMBOLS["rtmi_tomo_transpose_multi_dev"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, st])
    assert _lib.SYMBOLS["rtmi_tomo_lsqr_multi"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.LsqrParams), C.POINTER(_lib.LsqrOptions),
                                                             C.POINTER(_lib.TomoReg), C.c_int32, C.c_int32, _dp, _dp, _dp, _dp,
                                                             C.POINTER(_lib.LsqrStats)])
    _lib.lib()                                                                # first: it maps the HIP runtime the library shares with torch
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("matmat", "rmatmat", "matmat_device", "rmatmat_device", "lsqr_multi", "recover", "bootstrap"):
        assert callable(getattr(rt_bench.Tomography, name))


FAKE = C.c_void_p(8)              # never dereferenced: every check below comes before the handle is read
BUF = (C.c_double * 8)()


def _refused(rc, who, *words):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who.encode() + b": "), msg
    for w in words:
        assert w.encode() in msg, msg


@pytest.mark.parametrize("name", NAMES[:4])
def test_products_refuse_a_null_handle_and_a_bad_nrhs_before_the_handle_is_read(name):
    fn = getattr(_lib.lib(), name)
    p = C.c_void_p(64) if name.endswith("_dev") else BUF
    _refused(fn(None, 1, p, p, None), name, "null handle")
    for nrhs in (0, -1, 65, 1 << 20):
        _refused(fn(FAKE, nrhs, p, p, None), name, "nrhs must be in 1 .. 64")


def test_solver_refusals_that_need_no_device():
    L = _lib.lib()
    who = "rtmi_tomo_lsqr_multi"
    lp = _lib.LsqrParams()
    lp.iter_lim = 3

    def call(t=FAKE, nrhs=2, flags=0, reg=None):
        return L.rtmi_tomo_lsqr_multi(t, None, C.byref(lp), None, None if reg is None else C.byref(reg), nrhs, flags, BUF, None, BUF, None, None)

    _refused(call(t=None), who, "null handle")
    for nrhs in (0, 65):
        _refused(call(nrhs=nrhs), who, "nrhs must be in 1 .. 64")
    for flags in (2, 3, -1, 1 << 16):
        _refused(call(flags=flags), who, "flags", "RTMI_LSQR_MULTI_ROW_WEIGHT")
    for field, pair in (("d1", (-1.0, 0.0)), ("d1", (0.0, float("nan"))), ("d2", (float("inf"), 0.0)), ("d2", (0.0, -2.0))):
        reg = _lib.TomoReg()
        getattr(reg, field)[0], getattr(reg, field)[1] = pair
        _refused(call(reg=reg), who, f"reg.{field} must be finite and >= 0")


def test_bootstrap_weights():
    rows, n = 253, 7
    w = rt_bench.bootstrap_weights(rows, n, 42)
    assert w.shape == (n, rows) and w.dtype == np.float64
    # a weight is the square root of a multiplicity: its square is that integer (the square root of a small integer, squared,
    # rounds back to it), the squares of a replicate sum to `rows` exactly, and a row not drawn is exactly 0.0
    mult = np.rint(w * w)
    assert np.array_equal(w, np.sqrt(mult))
    assert np.array_equal(mult.sum(axis=1), np.full(n, float(rows)))
    rng = np.random.Generator(np.random.PCG64(42))
    for k in range(n):
        drawn = np.bincount(rng.integers(0, rows, size=rows), minlength=rows)
        assert np.array_equal(mult[k], drawn)
        assert (drawn == 0).any() and not w[k][drawn == 0].any() and not np.signbit(w[k][drawn == 0]).any()
    assert rt_bench.bootstrap_weights(rows, n, 42).tobytes() == w.tobytes()
    assert rt_bench.bootstrap_weights(rows, n, 43).tobytes() != w.tobytes()
    assert rt_bench.bootstrap_weights(rows, 3, 42).tobytes() == w[:3].tobytes()          # the replicates come one after the other
    with pytest.raises(ValueError):
        rt_bench.bootstrap_weights(0, 3, 1)


def test_checkerboard_and_spikes():
    cb = rt_bench.checkerboard(7, 10, 3, 0.25)
    assert cb.shape == (7, 10) and cb.dtype == np.float64
    for i in range(7):
        for j in range(10):
            assert cb[i, j] == (0.25 if (i // 3 + j // 3) % 2 == 0 else -0.25)
    cb = rt_bench.checkerboard(5, 6, (2, 3))
    assert cb[0, 0] == 1.0 and cb[0, 2] == 1.0 and cb[0, 3] == -1.0 and cb[2, 0] == -1.0 and cb[2, 3] == 1.0
    assert set(np.unique(cb)) == {-1.0, 1.0}
    with pytest.raises(ValueError):
        rt_bench.checkerboard(5, 6, 0)
    sp = rt_bench.spikes(4, 5, [(0, 0), (3, 4), (1, 2)], 2.0)
    assert sp.shape == (3, 4, 5)
    for s, (i, j) in enumerate([(0, 0), (3, 4), (1, 2)]):
        assert sp[s, i, j] == 2.0 and np.count_nonzero(sp[s]) == 1
    assert rt_bench.spikes(4, 5, []).shape == (0, 4, 5)
    with pytest.raises(ValueError):
        rt_bench.spikes(4, 5, [(4, 0)])


class _Shape(rt_bench.Tomography):
    """the shape checks of a Tomography without a handle: the library is never reached"""

    def __init__(self, qy=4, qx=5, rows=6):
        self.qy, self.qx, self._rows, self._h = qy, qx, rows, None

    def info(self):
        return {"rows": self._rows}


def test_python_methods_check_shapes_first():
    T = _Shape()
    with pytest.raises(ValueError, match=r"matmat: X must be \[S, 4, 5\]"):
        T.matmat(np.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match=r"rmatmat: W must be \[S, 6\]"):
        T.rmatmat(np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"lsqr_multi: rhs must be \[S, 6\]"):
        T.lsqr_multi(np.zeros(6))
    with pytest.raises(ValueError, match="group must be in 1 .. 64"):
        T.lsqr_multi(np.zeros((2, 6)), group=65)
    with pytest.raises(ValueError, match=r"row_weight must be \[6\] or \[S, 6\]"):
        T.lsqr_multi(np.zeros((2, 6)), row_weight=np.ones((3, 6)))
    with pytest.raises(ValueError, match="col_scale must have 20 values"):
        T.lsqr_multi(np.zeros((2, 6)), col_scale=np.ones(19))
    with pytest.raises(ValueError, match="smooth2 must be a pair"):
        T.lsqr_multi(np.zeros((2, 6)), smooth2=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match=r"recover: models must be \[S, 4, 5\]"):
        T.recover(np.zeros((4, 5)))
    with pytest.raises(ValueError, match="bootstrap: rhs must have 6 values"):
        T.bootstrap(np.zeros(5), 3, 1)
    with pytest.raises(ValueError, match="closed"):
        T.matmat(np.zeros((2, 4, 5)))
