"""CPU: the restatement of the weighted, masked and warm-started solver (tests/lsqr_weighted_ref.py) against scipy's lsqr on the
explicitly weighted and scaled dense problem; the restated illumination against the squared column norms of L; the new entries
(rtmi_kirchhoff_lsqr_weighted, rtmi_tomo_lsqr_weighted, rtmi_kirchhoff_illumination, _dev) declared, exported and bound with the
header's signatures, rtmi_lsqr_options 64 bytes, the ABI version still 7, and the refusals that need no handle.  The device
against the restatement: tests/test_gpu_lsqr_weighted.py and tests/test_gpu_illumination.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import _lib, rt_bench

import kirchhoff_lsqr_ref as R
import kirchhoff_ref as K1
import lsqr_weighted_ref as WR

_dp = C.POINTER(C.c_double)
ROWS, COLS, ITERS = 23, 17, 12
MASKED = (2, 9, 16)


def dense_case():
    rng = np.random.default_rng(41)
    A = rng.standard_normal((ROWS, COLS))
    b = rng.standard_normal(ROWS)
    wr = 0.25 + 1.5 * rng.random(ROWS)
    dc = 0.5 + rng.random(COLS)
    dc[list(MASKED)] = 0.0
    x0 = rng.standard_normal(COLS)
    return A, b, wr, dc, x0


OPTIONS = {"wr": ("wr",), "dc": ("dc",), "x0": ("x0",), "all": ("wr", "dc", "x0")}


@pytest.mark.parametrize("damp", [0.0, 1e-3])
@pytest.mark.parametrize("which", list(OPTIONS))
def test_restatement_against_scipy_on_the_weighted_problem(which, damp):
    from scipy.sparse.linalg import lsqr
    A, b, wr, dc, x0 = dense_case()
    opt = {k: v for k, v in (("wr", wr), ("dc", dc), ("x0", x0)) if k in OPTIONS[which]}
    got = WR.lsqr_weighted(lambda v: A @ v, lambda u: A.T @ u, b, ITERS, damp=damp, **opt)
    W = np.diag(opt.get("wr", np.ones(ROWS)))
    D = np.diag(opt.get("dc", np.ones(COLS)))
    start = opt.get("x0", np.zeros(COLS))
    M, rhs = W @ A @ D, W @ (b - A @ start)
    ys = lsqr(M, rhs, damp=damp, atol=0, btol=0, iter_lim=ITERS)[0]
    xs = start + D @ ys
    # the bound of test_standard_case_against_scipy: the residual ratios agree to 1e-6 relative
    rd = float(np.linalg.norm(W @ (b - A @ got["x"])) / np.linalg.norm(rhs))
    rs = float(np.linalg.norm(W @ (b - A @ xs)) / np.linalg.norm(rhs))
    print(f"{which} damp {damp}: residual ratio restated {rd:.10f}, scipy {rs:.10f}; max |x - x_scipy| {np.max(np.abs(got['x'] - xs)):.3e}")
    assert got["itn"] == ITERS and got["istop"] == 7
    assert abs(rd - rs) <= 1e-6 * rs
    if damp == 0.0:
        assert abs(got["r1norm"] / float(np.linalg.norm(rhs)) - rd) <= 1e-6 * rd         # r1norm is |W (b - A x)|
    if "dc" in opt:                                   # a masked value is x0's exactly, or zero
        for i in MASKED:
            assert got["x"][i] == start[i]


def test_no_option_is_lsqr_loop_bit_for_bit():
    A, b, *_ = dense_case()
    mv, rmv = (lambda v: A @ v), (lambda u: A.T @ u)
    for damp in (0.0, 1e-3):
        got, want = WR.lsqr_weighted(mv, rmv, b, ITERS, damp=damp), R.lsqr_loop(mv, rmv, b, ITERS, damp=damp)
        assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["history"], want["history"])
        assert (got["itn"], got["istop"], got["r1norm"], got["anorm"]) == (want["itn"], want["istop"], want["r1norm"], want["anorm"])
        ones = WR.lsqr_weighted(mv, rmv, b, ITERS, damp=damp, wr=np.ones(ROWS), dc=np.ones(COLS))
        assert np.array_equal(ones["x"], want["x"]) and np.array_equal(ones["history"], want["history"])     # a factor 1.0 is exact


def test_rows_after_the_weights_carry_none():
    """A stacked operator [A | E]: the rows of E are not weighted and A x0 is not subtracted from their right-hand side"""
    A, b, wr, dc, x0 = dense_case()
    E = np.random.default_rng(5).standard_normal((6, COLS))
    S = np.vstack([A, E])
    rhs = np.concatenate([b, np.zeros(6)])
    got = WR.lsqr_weighted(lambda v: S @ v, lambda u: S.T @ u, rhs, ITERS, wr=wr, dc=dc, x0=x0)
    full = np.concatenate([wr, np.ones(6)])
    r = rhs.copy()
    r[:ROWS] = r[:ROWS] - (S @ x0)[:ROWS]
    want = R.lsqr_loop(lambda v: full * (S @ (dc * v)), lambda u: dc * (S.T @ (full * u)), full * r, ITERS)
    assert np.array_equal(got["y"], want["x"]) and np.array_equal(got["x"], x0 + dc * want["x"])


# ---------------------------------------------------------------- the illumination
P, NY, NX, N, NT, DT, tiny_case = WR.P, WR.NY, WR.NX, WR.N, WR.NT, WR.DT, WR.tiny_case


@pytest.mark.parametrize("kind", ["plain", "amp", "bins"])
def test_illumination_restated_is_the_squared_column_norm(kind):
    T, isrc, irec, kw = tiny_case(amp=kind == "amp", nbin=3 if kind == "bins" else 0)
    four = {k: (v[:, None] if k in ("amp", "theta") and v is not None else v) for k, v in kw.items()}
    ill, count = WR.illumination(T[:, None], isrc, irec, NT, DT, **four)
    L = K1.matrix(T, isrc, irec, NT, DT, **kw)
    want = np.array([float(np.sum(L[:, j].toarray() ** 2)) for j in range(L.shape[1])]).reshape(ill.shape)    # sum_k (L e_j)_k^2
    lit = want > 0
    err = float(np.max(np.abs(ill[lit] - want[lit]) / want[lit]))
    print(f"{kind}: {count} contributing pairs, {int(lit.sum())} of {want.size} values lit, largest relative distance {err:.3e}")
    assert 0 < count < N * NY * NX * max(kw["nbin"], 1) and lit.any()              # the NaN patch and the trace's ends leave pairs out
    assert np.array_equal(ill == 0.0, ~lit)
    assert err <= 1e-13


# ---------------------------------------------------------------- the entries on the host
NAMES = ("rtmi_kirchhoff_lsqr_weighted", "rtmi_tomo_lsqr_weighted", "rtmi_kirchhoff_illumination", "rtmi_kirchhoff_illumination_dev")


def _header():
    return open(os.path.join(ROOT, "include", "rtmi.h")).read()


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_and_documents_the_entries():
    assert _prototype("rtmi_kirchhoff_lsqr_weighted") == [
        "rtmi_kirchhoff *k", "const rtmi_lsqr_params *lp", "const rtmi_lsqr_options *lo", "int32_t op", "const double *data", "double *x",
        "double *history", "rtmi_lsqr_stats *st"]
    assert _prototype("rtmi_tomo_lsqr_weighted") == [
        "rtmi_tomo *t", "const rtmi_lsqr_params *lp", "const rtmi_lsqr_options *lo", "const double smooth[2]", "const double *rhs",
        "double *x", "double *history", "rtmi_lsqr_stats *st"]
    assert _prototype("rtmi_kirchhoff_illumination") == ["rtmi_kirchhoff *k", "double *illum", "rtmi_kirchhoff_stats *st"]
    assert _prototype("rtmi_kirchhoff_illumination_dev") == ["rtmi_kirchhoff *k", "double *d_illum", "rtmi_kirchhoff_stats *st"]
    src = _header()
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)
    for k, v in (("PLAIN", 0), ("FULL", 1), ("FILTERED", 2)):
        assert re.search(rf"#define\s+RTMI_LSQR_OP_{k}\s+{v}\b", src)
    comments = " ".join(re.findall(r"/\*.*?\*/", src, flags=re.S))
    for name in NAMES[:3] + ("row_weight", "col_scale", "x0", "damp acts on y", "diag(L^T L)", "r1norm is |W (b - A x)|"):
        assert name in comments, name
    # no "Not covered" list names row weights, masks, x0 or a diagonal preconditioner any more
    for m in re.finditer(r"Not covered:(.*?)\*/", src, flags=re.S):
        assert not re.search(r"row weights|model masks|\bx0\b|preconditioners", m.group(1)), m.group(1)


def test_ctypes_signatures_exports_and_sizes():
    assert C.sizeof(_lib.LsqrOptions) == 64
    assert [f[0] for f in _lib.LsqrOptions._fields_] == ["row_weight", "col_scale", "x0", "reserved"]
    lp, lo, ls, ks = C.POINTER(_lib.LsqrParams), C.POINTER(_lib.LsqrOptions), C.POINTER(_lib.LsqrStats), C.POINTER(_lib.KirchhoffStats)
    assert _lib.SYMBOLS["rtmi_kirchhoff_lsqr_weighted"] == (C.c_int, [C.c_void_p, lp, lo, C.c_int32, _dp, _dp, _dp, ls])
    assert _lib.SYMBOLS["rtmi_tomo_lsqr_weighted"] == (C.c_int, [C.c_void_p, lp, lo, _dp, _dp, _dp, _dp, ls])
    assert _lib.SYMBOLS["rtmi_kirchhoff_illumination"] == (C.c_int, [C.c_void_p, _dp, ks])
    assert _lib.SYMBOLS["rtmi_kirchhoff_illumination_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, ks])
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert (_lib.LSQR_OP_PLAIN, _lib.LSQR_OP_FULL, _lib.LSQR_OP_FILTERED) == (0, 1, 2)
    for name in ("illumination", "illumination_device", "lsqr"):
        assert callable(getattr(rt_bench.Kirchhoff, name))
    for name in ("coverage", "lsqr"):
        assert callable(getattr(rt_bench.Tomography, name))


FAKE = C.c_void_p(8)              # never dereferenced: every check below comes before the handle is read
BUF = (C.c_double * 8)()


def _refused(rc, who, name):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who + b": "), msg
    assert re.search(rb"\b" + re.escape(name) + rb"\b", msg[len(who) + 2:]), msg


def test_refusals_that_need_no_handle():
    L = _lib.lib()
    lp = _lib.LsqrParams()
    lp.iter_lim = 4
    lo = _lib.LsqrOptions()
    st = _lib.LsqrStats()
    who = b"rtmi_kirchhoff_lsqr_weighted"
    for op in (-1, 3, 99):
        _refused(L.rtmi_kirchhoff_lsqr_weighted(FAKE, C.byref(lp), C.byref(lo), op, BUF, BUF, None, C.byref(st)), who, b"op")
    _refused(L.rtmi_kirchhoff_lsqr_weighted(None, C.byref(lp), C.byref(lo), 0, BUF, BUF, None, C.byref(st)), who, b"handle")
    _refused(L.rtmi_kirchhoff_lsqr_weighted(FAKE, None, C.byref(lo), 0, BUF, BUF, None, C.byref(st)), who, b"params")
    _refused(L.rtmi_kirchhoff_lsqr_weighted(FAKE, C.byref(lp), None, 1, None, BUF, None, C.byref(st)), who, b"data")
    _refused(L.rtmi_kirchhoff_lsqr_weighted(FAKE, C.byref(lp), C.byref(lo), 2, BUF, None, None, C.byref(st)), who, b"x")
    bad = _lib.LsqrParams()
    bad.iter_lim, bad.damp = 4, -1.0
    _refused(L.rtmi_kirchhoff_lsqr_weighted(FAKE, C.byref(bad), C.byref(lo), 0, BUF, BUF, None, C.byref(st)), who, b"damp")
    who = b"rtmi_tomo_lsqr_weighted"
    _refused(L.rtmi_tomo_lsqr_weighted(None, C.byref(lp), C.byref(lo), None, BUF, BUF, None, C.byref(st)), who, b"handle")
    _refused(L.rtmi_tomo_lsqr_weighted(FAKE, C.byref(lp), C.byref(lo), None, None, BUF, None, C.byref(st)), who, b"rhs")
    _refused(L.rtmi_kirchhoff_illumination(None, BUF, None), b"rtmi_kirchhoff_illumination", b"handle")
    _refused(L.rtmi_kirchhoff_illumination(FAKE, None, None), b"rtmi_kirchhoff_illumination", b"illum")
    _refused(L.rtmi_kirchhoff_illumination_dev(None, C.c_void_p(64), None), b"rtmi_kirchhoff_illumination_dev", b"handle")
    _refused(L.rtmi_kirchhoff_illumination_dev(FAKE, None, None), b"rtmi_kirchhoff_illumination_dev", b"d_illum")


def test_python_methods_check_the_options_first():
    class Shape(rt_bench.Kirchhoff):
        def __init__(self):
            self.N, self.nt, self.nb, self.nbin, self.ny, self.nx = 3, 8, 1, 0, 2, 5
            self.karr, self.has_kmah, self._h, self._filter = 1, False, None, None

    op, d = Shape(), np.zeros((3, 8))
    with pytest.raises(ValueError, match="row_weight must have 24 values"):
        op.lsqr(d, 4, row_weight=np.ones(23))
    with pytest.raises(ValueError, match="col_scale must have 10 values"):
        op.lsqr(d, 4, col_scale=np.ones(11))
    with pytest.raises(ValueError, match="x0 must have 10 values"):
        op.lsqr(d, 4, x0=np.ones((5, 5)))
    with pytest.raises(ValueError, match='col_scale must be an array or "illumination"'):
        op.lsqr(d, 4, col_scale="coverage")
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 4, col_scale="illumination")
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 4, x0=np.ones((2, 5)))
    with pytest.raises(RuntimeError, match="closed"):
        op.illumination()
    s = rt_bench.illumination_scale(np.array([[0.0, 1.0], [3.0, 0.0]]), eps=1e-3)
    assert s[0, 0] == 0.0 and s[1, 1] == 0.0 and s[0, 1] == 1.0 / np.sqrt(1.0 + 1e-3 * 3.0) and s[1, 0] == 1.0 / np.sqrt(3.0 + 1e-3 * 3.0)
