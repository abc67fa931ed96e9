"""CPU: several right-hand sides through the linearised eikonal fill (rtmi_eikonal_tangent_multi, rtmi_eikonal_adjoint_multi and
their _dev forms).  The entries are declared, exported and bound with their argument counts and the ABI
version stays 7; every refusal comes before any device work and names the argument, nrhs of 0 and of 65 among them; and on the
restatement the corridor gives its zero column and its random column different numbers of rounds, which keeps the GPU test on
them (tests/test_gpu_eikonal_multi.py) from degenerating."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eikonal_lin_ref as L
from conftest import ROOT
from raytracing_amd import _lib, rt_bench
from test_eikonal_host import REFUSALS, params

SWEEPS = ["rtmi_eikonal_tangent_multi", "rtmi_eikonal_tangent_multi_dev", "rtmi_eikonal_adjoint_multi", "rtmi_eikonal_adjoint_multi_dev"]


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", header)
    _lib.lib()                                                                # first: it maps the HIP runtime the library shares with torch
    raw = C.CDLL(_lib.LIB_PATH)
    for e in SWEEPS:
        proto = _prototype(e)
        assert len(proto) == 14 and proto[7] == "int32_t nrhs", (e, proto)
        assert len(_lib.SYMBOLS[e][1]) == 14 and _lib.SYMBOLS[e][1][7] is C.c_int32
        assert hasattr(raw, e) and getattr(_lib.lib(), e).argtypes == _lib.SYMBOLS[e][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("eikonal_tangent_multi", "eikonal_adjoint_multi", "eikonal_tangent_multi_device", "eikonal_adjoint_multi_device"):
        assert callable(getattr(rt_bench, name))
    # the contract is stated above the entries
    k = header.index("int rtmi_eikonal_tangent_multi(")
    above = header[header.rindex("/*", 0, k):k]
    assert "CONTRACT" in above and "bits that the single entry gives on column c alone" in above


@pytest.mark.parametrize("entry", SWEEPS)
def test_sweep_refusals_come_before_any_device_work(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    K = 2
    n = np.ones((3, 4)); src = np.zeros((1, 2)); ns = np.ones(1); tab = np.ones((1, 3, 4)); filled = np.ones((1, 3, 4), dtype=np.uint8)
    cols = np.ones((K, 1, 3, 4)); out = np.zeros((K, 1, 3, 4))
    host = not entry.endswith("_dev")
    ptr = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.dtype == np.uint8 else _lib.dptr(a)) if host else (lambda a: a.ctypes.data)
    head = [ptr(src), ptr(ns), ptr(tab), ptr(filled)]
    # after nrhs: dn, dn_src, dT_seed, dT (tangent); r, lam, g, g_src (adjoint)
    tail = [ptr(cols), None, None, ptr(out)] if "tangent" in entry else [ptr(cols), ptr(out), None, None]

    def call(ep=None, n_=ptr(n), S=1, head_=head, nrhs=K, tail_=tail):
        return fn(C.byref(params()) if ep is None else ep, n_, S, *head_, nrhs, *tail_, None, None)

    for word, kw in REFUSALS:
        assert call(ep=C.byref(params(**kw))) == -1, kw
        msg = lib.rtmi_last_error().decode()
        assert entry + ":" in msg and word in msg, (kw, msg)
    for nrhs in (0, -1, 65, 1 << 20):
        assert call(nrhs=nrhs) == -1
        msg = lib.rtmi_last_error().decode()
        assert msg.startswith(entry + ": ") and "nrhs must be in [1, 64]" in msg and str(nrhs) in msg, msg
        assert call(S=0, n_=None, head_=[None] * 4, tail_=[None] * 4, nrhs=nrhs) == -1 and "nrhs" in lib.rtmi_last_error().decode()
    assert call(S=-1) == -1 and "S must be >= 0" in lib.rtmi_last_error().decode()
    for w in (2, 3, 16, -1):                                                  # the tests' chunk width is a compiled one, or 0
        ep = params()
        ep.reserved[1] = w
        assert call(ep=C.byref(ep)) == -1 and "reserved[1] must be 0 or a compiled chunk width" in lib.rtmi_last_error().decode()
    for k, name in enumerate(("null src", "null n_src", "null T", "null filled")):
        args = list(head)
        args[k] = None
        assert call(head_=args) == -1 and name in lib.rtmi_last_error().decode(), name
    names = ("null dn", None, None, "null dT") if "tangent" in entry else ("null r", "null lam", None, None)
    for k, name in enumerate(names):
        if name is None:
            continue
        args = list(tail)
        args[k] = None
        assert call(tail_=args) == -1 and name in lib.rtmi_last_error().decode(), name
    assert call(n_=None) == -1 and "null n" in lib.rtmi_last_error().decode()
    assert fn(None, ptr(n), 1, *head, K, *tail, None, None) == -1 and "null ep" in lib.rtmi_last_error().decode()


def test_no_sources_is_no_work():
    st = _lib.EikonalStats()
    for entry in ("rtmi_eikonal_tangent_multi", "rtmi_eikonal_adjoint_multi"):
        assert getattr(_lib.lib(), entry)(C.byref(params()), None, 0, *[None] * 4, 3, *[None] * 4, None, C.byref(st)) == 0
        assert (st.free_nodes, st.filled, st.changes, st.rounds_max) == (0, 0, 0, 0)


def test_python_layer_refuses_bad_shapes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    fill = {"T": np.ones((1, 3, 4)), "filled": np.ones((1, 3, 4), dtype=np.uint8)}
    with pytest.raises(ValueError, match=r"dn must be \[K, ny, nx\]"):
        rt_bench.eikonal_tangent_multi(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((3, 4)), n_src=[1.0])
    with pytest.raises(ValueError, match="dn_src must be"):
        rt_bench.eikonal_tangent_multi(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((2, 3, 4)), n_src=[1.0], dn_src=np.ones(2))
    with pytest.raises(ValueError, match="dT_seed must be"):
        rt_bench.eikonal_tangent_multi(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((2, 3, 4)), n_src=[1.0], dT_seed=np.ones((1, 3, 4)))
    with pytest.raises(ValueError, match=r"r must be \[K, S, ny, nx\]"):
        rt_bench.eikonal_adjoint_multi(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((1, 3, 4)), n_src=[1.0])


def test_corridor_gives_its_zero_column_and_its_random_column_different_rounds():
    """From the code a zero column is clean in its first round; the restatement agrees, and a random column needs more than three"""
    grid, n, src, ns, fill, nets = L.filled(L.corridor_case())
    rng = np.random.default_rng(3)
    zero_t, rand_t = L.tangent(nets, np.zeros(n.shape)), L.tangent(nets, rng.standard_normal(n.shape))
    zero_a, rand_a = L.adjoint(nets, np.zeros((len(src),) + n.shape)), L.adjoint(nets, rng.standard_normal((len(src),) + n.shape))
    for zero, rand in ((zero_t, rand_t), (zero_a, rand_a)):
        assert (zero["rounds"] == 1).all() and zero["converged"].all() and zero["changes"] == 0
        assert (rand["rounds"] > 3).all() and rand["converged"].all()
    assert not zero_t["dT"].any() and not zero_a["lam"].any()


# ------------------------------------------------------------------------------------------------ the handle's entries
_dp = C.POINTER(C.c_double)
PRODUCTS = ("rtmi_eikonal_tomo_apply_multi", "rtmi_eikonal_tomo_apply_multi_dev", "rtmi_eikonal_tomo_transpose_multi",
            "rtmi_eikonal_tomo_transpose_multi_dev")
FAKE = C.c_void_p(8)              # never dereferenced: every check below comes before the handle is read
BUF = (C.c_double * 8)()


def test_the_handles_entries_are_declared_exported_and_bound():
    st = "rtmi_eikonal_tomo_stats *st"
    assert _prototype("rtmi_eikonal_tomo_apply_multi") == ["rtmi_eikonal_tomo *h", "int32_t nrhs", "const double *dn", "double *y", st]
    assert _prototype("rtmi_eikonal_tomo_apply_multi_dev") == ["rtmi_eikonal_tomo *h", "int32_t nrhs", "const double *d_dn", "double *d_y", st]
    assert _prototype("rtmi_eikonal_tomo_transpose_multi") == ["rtmi_eikonal_tomo *h", "int32_t nrhs", "const double *y", "double *G", st]
    assert _prototype("rtmi_eikonal_tomo_transpose_multi_dev") == ["rtmi_eikonal_tomo *h", "int32_t nrhs", "const double *d_y", "double *d_G", st]
    assert _prototype("rtmi_eikonal_tomo_lsqr_multi") == ["rtmi_eikonal_tomo *h", "const rtmi_lsqr_params *lp", "const rtmi_lsqr_options *lo",
                                                          "const rtmi_tomo_reg *reg", "int32_t nrhs", "int32_t flags", "const double *rhs",
                                                          "double *x", "double *history", "rtmi_lsqr_stats *st"]
    assert _prototype("rtmi_eikonal_tomo_set_column_group") == ["rtmi_eikonal_tomo *h", "int32_t cg"]
    est = C.POINTER(_lib.EikonalTomoStats)
    for name in PRODUCTS:
        p = C.c_void_p if name.endswith("_dev") else _dp
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int32, p, p, est])
    assert _lib.SYMBOLS["rtmi_eikonal_tomo_lsqr_multi"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.LsqrParams), C.POINTER(_lib.LsqrOptions),
                                                                     C.POINTER(_lib.TomoReg), C.c_int32, C.c_int32, _dp, _dp, _dp,
                                                                     C.POINTER(_lib.LsqrStats)])
    assert _lib.SYMBOLS["rtmi_eikonal_tomo_set_column_group"] == (C.c_int, [C.c_void_p, C.c_int32])
    _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in PRODUCTS + ("rtmi_eikonal_tomo_lsqr_multi", "rtmi_eikonal_tomo_set_column_group"):
        assert hasattr(raw, name) and getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    for name in ("matmat", "rmatmat", "matmat_device", "rmatmat_device", "lsqr_multi", "recover", "bootstrap", "set_column_group"):
        assert callable(getattr(rt_bench.EikonalTomography, name))


def _refused(rc, who, *words):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who.encode() + b": "), msg
    for w in words:
        assert w.encode() in msg, msg


@pytest.mark.parametrize("name", PRODUCTS)
def test_products_refuse_a_null_handle_and_a_bad_nrhs_before_the_handle_is_read(name):
    fn = getattr(_lib.lib(), name)
    p = C.c_void_p(64) if name.endswith("_dev") else BUF
    _refused(fn(None, 1, p, p, None), name, "null handle")
    for nrhs in (0, -1, 65, 1 << 20):
        _refused(fn(FAKE, nrhs, p, p, None), name, "nrhs must be in [1, 64]", str(nrhs))


def test_solver_and_column_group_refusals_that_need_no_device():
    lib = _lib.lib()
    who = "rtmi_eikonal_tomo_lsqr_multi"
    lp = _lib.LsqrParams()
    lp.iter_lim = 3

    def call(h=FAKE, lp_=C.byref(lp), nrhs=2, flags=0, reg=None, rhs=BUF, x=BUF):
        return lib.rtmi_eikonal_tomo_lsqr_multi(h, lp_, None, None if reg is None else C.byref(reg), nrhs, flags, rhs, x, None, None)

    _refused(call(h=None), who, "null handle")
    for nrhs in (0, 65):
        _refused(call(nrhs=nrhs), who, "nrhs must be in [1, 64]", str(nrhs))
    for flags in (2, 3, -1, 1 << 16):
        _refused(call(flags=flags), who, "flags", "RTMI_LSQR_MULTI_ROW_WEIGHT")
    _refused(call(lp_=None), who, "null params")
    _refused(call(rhs=None), who, "null rhs")
    _refused(call(x=None), who, "null x")
    bad = _lib.LsqrParams()
    bad.iter_lim = 0
    _refused(call(lp_=C.byref(bad)), who, "iter_lim")
    for field, pair in (("d1", (-1.0, 0.0)), ("d2", (0.0, float("nan")))):
        reg = _lib.TomoReg()
        getattr(reg, field)[0], getattr(reg, field)[1] = pair
        _refused(call(reg=reg), who, f"reg.{field} must be finite and >= 0")
    who = "rtmi_eikonal_tomo_set_column_group"
    _refused(lib.rtmi_eikonal_tomo_set_column_group(None, 0), who, "null handle")
    for cg in (-1, 65):
        _refused(lib.rtmi_eikonal_tomo_set_column_group(FAKE, cg), who, "cg must be in [0, 64]", str(cg))


class _Shape(rt_bench.EikonalTomography):
    """the shape checks of an EikonalTomography without a handle: the library is never reached"""

    def __init__(self, S=2, R=3, ny=4, nx=5):
        self.S, self.R, self.ny, self.nx, self._h = S, R, ny, nx, None


def test_python_methods_check_shapes_first():
    T = _Shape()
    with pytest.raises(ValueError, match=r"matmat: X must be \[K, 4, 5\]"):
        T.matmat(np.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match=r"rmatmat: Y must be \[K, 6\]"):
        T.rmatmat(np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"lsqr_multi: rhs must be \[K, 6\]"):
        T.lsqr_multi(np.zeros(6), 3)
    with pytest.raises(ValueError, match="group must be in 1 .. 64"):
        T.lsqr_multi(np.zeros((2, 6)), 3, group=65)
    with pytest.raises(ValueError, match=r"row_weight must be \[6\] or \[K, 6\]"):
        T.lsqr_multi(np.zeros((2, 6)), 3, row_weight=np.ones((3, 6)))
    with pytest.raises(ValueError, match="col_scale must have 20 values"):
        T.lsqr_multi(np.zeros((2, 6)), 3, col_scale=np.ones(19))
    with pytest.raises(ValueError, match="smooth2 must be a pair"):
        T.lsqr_multi(np.zeros((2, 6)), 3, smooth2=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match=r"recover: models must be \[K, 4, 5\]"):
        T.recover(np.zeros((4, 5)))
    with pytest.raises(ValueError, match="bootstrap: rhs must have 6 values"):
        T.bootstrap(np.zeros(5), 3, 1)
    with pytest.raises(ValueError, match="closed"):
        T.matmat(np.zeros((2, 4, 5)))
