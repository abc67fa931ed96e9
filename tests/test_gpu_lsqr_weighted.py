"""GPU: weighted, masked and warm-started LSQR on the device (rtmi_kirchhoff_lsqr_weighted, rtmi_tomo_lsqr_weighted;
rt_bench.Kirchhoff.lsqr / Tomography.lsqr with row_weight, col_scale, x0; include/rtmi.h) against the
restatement (tests/lsqr_weighted_ref.py) driven with the device's own operator calls: every bit of x, of the history and of the
final scalars, for each option singly and all together, on the three Kirchhoff operators (plain with an odd data and model
length, which ends the 16-byte path in a single item; K = 2 with kmah: FULL; the same with a 5-tap filter: FILTERED) and on the
tomography matrix with and without smoothing rows.  Null options against the entries without options, masks, a range stop and
the refusals that need a handle."""
import ctypes as C
import struct

import numpy as np
import pytest

import filter_ref as FR
import hilbert_ref as HR
import kirchhoff_multi_ref as KM
import lsqr_weighted_ref as WR
import tomo_ref as TR
from conftest import LIMITS

pytestmark = pytest.mark.gpu

ITERS = 6
TAPS5, ORIGIN5 = np.array([0.25, -0.5, 1.0, 0.375, -0.125]), 2
ODD_GRID, ODD_N, ODD_NT = (21, 31), 23, 63            # 651 nodes: two full blocks and a partial one; 1449 samples


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


def make(rb, kind, weights=None):
    """-> (handle, kwargs of lsqr that choose its operator, op of the C entry)"""
    from raytracing_amd import _lib
    if kind == "plain":
        rng = np.random.default_rng(3)
        T = 0.002 + 0.55 * ODD_NT * KM.SM_DT * rng.random((KM.SM_P,) + ODD_GRID)
        T[rng.random(T.shape) < 0.05] = np.nan
        isrc = np.sort(rng.integers(0, KM.SM_P, ODD_N)).astype(np.int32)
        irec = rng.integers(0, KM.SM_P, ODD_N).astype(np.int32)
        op = rb.Kirchhoff(T, isrc, irec, ODD_NT, KM.SM_DT, weights=weights)
        assert (op.N * op.nt) % 2 == 1 and (op.ny * op.nx) % 2 == 1
        return op, dict(), _lib.LSQR_OP_PLAIN
    T, isrc, irec, kw = KM.small_case(2, seed=3, amp=True, kmah=True, holes=True)
    op = rb.Kirchhoff(T, isrc, irec, KM.SM_NT, KM.SM_DT, amp=kw["amp"], kmah=kw["kmah"], weights=weights)
    assert (op.N * op.nt) % 2 == 0 and (op.ny * op.nx) % 2 == 0
    if kind == "full":
        return op, dict(hilbert="device"), _lib.LSQR_OP_FULL
    op.set_filter(TAPS5, origin=ORIGIN5)
    return op, dict(hilbert="device", filtered=True), _lib.LSQR_OP_FILTERED


def operators(rb, op, kind):
    """the operator of the handle's solver from the device's pair, with H and F restated: (A, A^T) on flat arrays"""
    htaps = rb.hilbert_taps(op.nt)
    filt = kind == "filtered"

    def model(m):
        m = m.reshape(op.nb, op.ny, op.nx)
        if op.karr:
            c0, c1 = op.model_channels(m)
            b = c0 + HR.hilbert(c1, htaps)
        else:
            b = op.model(m)
        return (FR.apply(b, TAPS5, ORIGIN5) if filt else b).reshape(-1)

    def migrate(d):
        d = d.reshape(op.N, op.nt)
        if filt:
            d = FR.apply(d, TAPS5, ORIGIN5, transpose=True)
        if op.karr:
            return op.migrate_channels(d, -HR.hilbert(d, htaps)).reshape(-1)
        return op.migrate(d).reshape(-1)
    return model, migrate


def options(op, which, seed=7):
    rng = np.random.default_rng(seed)
    wr = 0.25 + 1.5 * rng.random((op.N, op.nt))
    dc = 0.5 + rng.random((op.ny, op.nx))
    dc.reshape(-1)[[0, 5, 300, op.ny * op.nx - 1]] = 0.0
    x0 = rng.standard_normal((op.ny, op.nx))
    full = dict(row_weight=wr, col_scale=dc, x0=x0)
    return {k: v for k, v in full.items() if which in ("all", k)}


def restated(mv, rmv, d, iter_lim, opt, **kw):
    return WR.lsqr_weighted(mv, rmv, d, iter_lim, wr=opt.get("row_weight"), dc=opt.get("col_scale"), x0=opt.get("x0"), **kw)


def bits(v):
    return struct.pack("<d", float(v))


def assert_same_run(got, want):
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert np.asarray(got["x"]).tobytes() == np.asarray(want["x"]).tobytes()
    assert got["history"].shape == want["history"].shape and np.array_equal(got["history"], want["history"])
    for key in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(got[key]) == bits(want[key]), key


def raw_weighted(op, opnum, d, iter_lim, lo, damp=0.0):
    """rtmi_kirchhoff_lsqr_weighted itself, lo a _lib.LsqrOptions or None -> the dict of Kirchhoff.lsqr with stats"""
    from raytracing_amd import _lib
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.damp = iter_lim, damp
    x = np.empty((op.nb, op.ny, op.nx))
    hist = np.zeros((iter_lim, 4))
    st = _lib.LsqrStats()
    dd = np.ascontiguousarray(d, dtype=np.float64)
    _lib.check(_lib.lib().rtmi_kirchhoff_lsqr_weighted(op._h, C.byref(lp), None if lo is None else C.byref(lo), opnum, _lib.dptr(dd),
                                                       _lib.dptr(x), _lib.dptr(hist), C.byref(st)))
    return {"x": x[0], "istop": int(st.istop), "itn": int(st.itn), "r1norm": st.r1norm, "r2norm": st.r2norm, "anorm": st.anorm,
            "arnorm": st.arnorm, "history": hist[:st.itn].copy(), "bytes_device": int(st.bytes_device)}


# ---------------------------------------------------------------- Kirchhoff: the solver against the restatement
@pytest.mark.parametrize("damp", [0.0, 1e-3])
@pytest.mark.parametrize("which", ["row_weight", "col_scale", "x0", "all"])
@pytest.mark.parametrize("kind", ["plain", "full", "filtered"])
def test_kirchhoff_solver_equals_the_restatement_bit_for_bit(rb, kind, which, damp):
    op, sel, _ = make(rb, kind)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    opt = options(op, which)
    got = op.lsqr(d, ITERS, damp=damp, history=True, stats=True, **sel, **opt)
    want = restated(*operators(rb, op, kind), d, ITERS, opt, damp=damp)
    none = op.lsqr(d, ITERS, damp=damp, stats=True, **sel)
    st = got["stats"]
    print(f"{kind} {which} damp {damp}: itn {got['itn']} istop {got['istop']} r1norm {got['r1norm']:.6e}; per iteration operators "
          f"{st['operator_ms'] / ITERS:.3f} ms, vector passes {st['vector_ms'] / ITERS:.3f} ms; {st['bytes_device']} bytes")
    assert got["itn"] == ITERS and got["istop"] == 7
    assert_same_run(got, want)
    assert not np.array_equal(got["x"], none["x"])
    per, nm = op.N * op.nt, op.ny * op.nx
    added = (2 * per if "row_weight" in opt else 0) + (2 * nm if "col_scale" in opt else 0) + (nm if "x0" in opt else 0)
    assert st["bytes_device"] == none["stats"]["bytes_device"] + 8 * added
    if "col_scale" in opt:                             # a masked value is x0's exactly, or zero
        start = opt.get("x0", np.zeros((op.ny, op.nx)))
        dark = opt["col_scale"] == 0.0
        assert dark.sum() == 4 and np.array_equal(got["x"][dark], start[dark])
    op.close()


@pytest.mark.parametrize("kind", ["plain", "full", "filtered"])
def test_null_options_are_the_entries_without_options(rb, kind):
    from raytracing_amd import _lib
    op, sel, opnum = make(rb, kind)
    d = np.random.default_rng(13).standard_normal((op.N, op.nt))
    old = op.lsqr(d, ITERS, damp=1e-3, history=True, stats=True, **sel)
    for lo in (None, _lib.LsqrOptions()):
        got = raw_weighted(op, opnum, d, ITERS, lo, damp=1e-3)
        assert_same_run(got, old)
        assert got["bytes_device"] == old["stats"]["bytes_device"]
    # a factor 1.0 is exact: weights and a scale of ones give the x of no option
    ones = op.lsqr(d, ITERS, damp=1e-3, history=True, row_weight=np.ones((op.N, op.nt)), col_scale=np.ones((op.ny, op.nx)), **sel)
    assert_same_run(ones, old)
    zero = op.lsqr(d, ITERS, damp=1e-3, history=True, x0=np.zeros((op.ny, op.nx)), **sel)
    assert np.array_equal(zero["x"], old["x"])         # b - A 0 = b, 0 + y = y
    op.close()


def test_muted_traces_against_a_handle_with_zero_weights(rb):
    """row_weight 0 on four traces against a handle with w[k] = 0 there and no option.  Each run is held to its own restatement;
    the two are asserted equal only where the two restatements are: the muted samples of the data still count in the unweighted
    run's first norm, so in general they differ."""
    mute = [2, 3, 11, 20]
    w = np.ones(ODD_N)
    w[mute] = 0.0
    a, _, _ = make(rb, "plain")
    b, _, _ = make(rb, "plain", weights=w)
    d = np.random.default_rng(14).standard_normal((a.N, a.nt))
    wr = np.repeat(w[:, None], a.nt, axis=1)
    got_a = a.lsqr(d, ITERS, history=True, row_weight=wr)
    got_b = b.lsqr(d, ITERS, history=True)
    want_a = restated(*operators(rb, a, "plain"), d, ITERS, dict(row_weight=wr))
    want_b = restated(*operators(rb, b, "plain"), d, ITERS, dict())
    assert_same_run(got_a, want_a)
    assert_same_run(got_b, want_b)
    same = np.array_equal(want_a["x"], want_b["x"]) and np.array_equal(want_a["history"], want_b["history"])
    print(f"muted by row_weight against muted by w: the restatements are {'equal' if same else 'different'}; "
          f"max |x_a - x_b| {np.max(np.abs(got_a['x'] - got_b['x'])):.3e}")
    if same:
        assert_same_run(got_a, got_b)
    # with the muted traces' data zero as well the two problems are one
    d0 = d.copy()
    d0[mute] = 0.0
    want_a0 = restated(*operators(rb, a, "plain"), d0, ITERS, dict(row_weight=wr))
    want_b0 = restated(*operators(rb, b, "plain"), d0, ITERS, dict())
    got_a0, got_b0 = a.lsqr(d0, ITERS, history=True, row_weight=wr), b.lsqr(d0, ITERS, history=True)
    assert_same_run(got_a0, want_a0)
    assert_same_run(got_b0, want_b0)
    if np.array_equal(want_a0["x"], want_b0["x"]) and np.array_equal(want_a0["history"], want_b0["history"]):
        assert_same_run(got_a0, got_b0)
    a.close(); b.close()


def test_range_stop_and_refusals(rb):
    from raytracing_amd import _lib
    op, _, _ = make(rb, "plain")
    d = np.random.default_rng(15).standard_normal((op.N, op.nt))
    x0 = np.random.default_rng(16).standard_normal((op.ny, op.nx))
    tiny = np.full((op.N, op.nt), 1e-170)              # max |wr d|^2 is below the normal range
    got = op.lsqr(d, 4, history=True, row_weight=tiny)
    assert (got["istop"], got["itn"]) == (_lib.LSQR_RANGE, 0) and not got["x"].any()
    want = restated(*operators(rb, op, "plain"), d, 4, dict(row_weight=tiny))
    assert_same_run(got, want)
    got = op.lsqr(d, 4, history=True, row_weight=tiny, x0=x0)
    assert (got["istop"], got["itn"]) == (_lib.LSQR_RANGE, 0) and np.array_equal(got["x"], x0)
    for name, shape in (("row_weight", (op.N, op.nt)), ("col_scale", (op.ny, op.nx)), ("x0", (op.ny, op.nx))):
        for bad in (np.nan, np.inf, -np.inf):
            a = np.ones(shape)
            a.reshape(-1)[-1] = bad
            with pytest.raises(_lib.RtmiError, match=f"rtmi_kirchhoff_lsqr_weighted: {name} has a value that is not finite") as ei:
                op.lsqr(d, 3, **{name: a})
            assert ei.value.code == -1
    lp = _lib.LsqrParams()
    lp.iter_lim = 3
    lo = _lib.LsqrOptions()
    x = np.empty((op.ny, op.nx))
    assert _lib.lib().rtmi_kirchhoff_lsqr_weighted(op._h, C.byref(lp), C.byref(lo), 0, None, _lib.dptr(x), None, None) == -1
    assert b"null data" in _lib.lib().rtmi_last_error()
    assert op.lsqr(d, 2, x0=x0)["itn"] == 2            # the handle still works
    op.close()
    km, _, _ = make(rb, "full")
    dk = np.ones((km.N, km.nt))
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr_weighted: .*kmah") as ei:
        km.lsqr(dk, 3, x0=np.zeros((km.ny, km.nx)))    # op PLAIN on a handle with kmah
    assert ei.value.code == -1
    km.close()


# ---------------------------------------------------------------- tomography
@pytest.fixture(scope="module")
def torch(rb):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def tomo(rb):
    """65 rays, one full slice of 64 rows and one row more, ends only, on the stock field coarsened to a few thousand samples"""
    scen = "vert_heterogeneous"
    F = rb.Field.build(scen, LIMITS[scen], 4 * rb.DELTA)
    th = np.linspace(0.05, np.pi / 2 - 0.05, 65)
    step, ms = rb.DELTA_S, int(np.ceil(80 / rb.DELTA_S) + 1)
    c = rb.Batch(F, rb.METHODS[6], step, ms, LIMITS[scen], 1.0, th, -2.0, -2.0, record_stride=0)
    c.run()
    rec_rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.METHODS[6], step, ms, LIMITS[scen], 1.0, th, -2.0, -2.0, rec_rows=rec_rows)
    b.run()
    T = rb.Tomography(F)
    T.append(b)
    b.close()
    yield T
    T.close()
    F.close()


def tomo_operators(T, torch, smooth):
    """the stacked operator [A | Dx | Dy] with A and A^T the device-pointer products"""
    rows = T.info()["rows"]

    def mv(x):
        y = T.matvec_device(torch.tensor(np.asarray(x, dtype=np.float64).reshape(T.qy, T.qx), device="cuda")).cpu().numpy()
        return y if smooth is None else np.r_[y, TR.diff_forward(x, T.qx, T.qy, *smooth)]

    def rmv(u):
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        g = T.rmatvec_device(torch.tensor(u[:rows].copy(), device="cuda")).cpu().numpy().reshape(-1)
        return g if smooth is None else g + TR.diff_transpose(u[rows:], T.qx, T.qy, *smooth)
    return mv, rmv


@pytest.mark.parametrize("damp", [0.0, 1e-3])
@pytest.mark.parametrize("smooth", [None, (0.5, 0.25)])
@pytest.mark.parametrize("which", ["row_weight", "col_scale", "x0", "all"])
def test_tomography_solver_equals_the_restatement_bit_for_bit(rb, tomo, torch, which, smooth, damp):
    T = tomo
    rows = T.info()["rows"]
    assert rows == 65
    rng = np.random.default_rng(31)
    rhs = rng.standard_normal(rows)
    cover = T.coverage()
    assert cover.shape == (T.qy, T.qx) and np.any(cover == 0) and np.any(cover != 0)
    dc = (0.5 + rng.random((T.qy, T.qx))) * (cover != 0)                   # samples no ray passes are frozen
    full = dict(row_weight=0.25 + 1.5 * rng.random(rows), col_scale=dc, x0=1e-2 * rng.standard_normal((T.qy, T.qx)))
    opt = {k: v for k, v in full.items() if which in ("all", k)}
    got = T.lsqr(rhs, damp=damp, smooth=smooth, iter_lim=ITERS, history=True, stats=True, **opt)
    nd = 0 if smooth is None else T.qy * (T.qx - 1) + (T.qy - 1) * T.qx
    want = restated(*tomo_operators(T, torch, smooth), np.r_[rhs, np.zeros(nd)], ITERS, opt, ndata=rows, damp=damp)
    none = T.lsqr(rhs, damp=damp, smooth=smooth, iter_lim=ITERS, stats=True)
    print(f"{which} smooth {smooth} damp {damp}: itn {got['itn']} istop {got['istop']} r1norm {got['r1norm']!r}; vectors "
          f"{got['stats']['vector_ms']:.3f} ms")
    assert got["itn"] == ITERS and got["istop"] == 7
    assert_same_run(got, want)
    per, nm = rows + nd, T.qy * T.qx
    added = (2 * per if "row_weight" in opt else 0) + (2 * nm if "col_scale" in opt else 0) + (nm if "x0" in opt else 0)
    assert got["stats"]["bytes_device"] == none["stats"]["bytes_device"] + 8 * added
    if "col_scale" in opt:                             # the samples outside the coverage stay at x0, or zero
        start = opt.get("x0", np.zeros((T.qy, T.qx)))
        assert np.array_equal(got["x"][cover == 0], start[cover == 0])
        assert not np.array_equal(got["x"][cover != 0], start[cover != 0])


def test_tomography_null_options_and_refusals(rb, tomo):
    from raytracing_amd import _lib
    T = tomo
    rows = T.info()["rows"]
    rhs = np.random.default_rng(32).standard_normal(rows)
    old = T.lsqr(rhs, damp=1e-3, smooth=(0.5, 0.25), iter_lim=ITERS, history=True, stats=True)
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.damp = ITERS, 1e-3
    sm = np.array([0.5, 0.25])
    for lo in (None, _lib.LsqrOptions()):
        x, hist, st = np.empty((T.qy, T.qx)), np.zeros((ITERS, 4)), _lib.LsqrStats()
        _lib.check(_lib.lib().rtmi_tomo_lsqr_weighted(T._h, C.byref(lp), None if lo is None else C.byref(lo), _lib.dptr(sm), _lib.dptr(rhs),
                                                      _lib.dptr(x), _lib.dptr(hist), C.byref(st)))
        assert x.tobytes() == old["x"].tobytes() and np.array_equal(hist, old["history"])
        assert (st.itn, st.istop, st.bytes_device) == (old["itn"], old["istop"], old["stats"]["bytes_device"])
        assert bits(st.r1norm) == bits(old["r1norm"]) and bits(st.anorm) == bits(old["anorm"])
    ones = T.lsqr(rhs, damp=1e-3, smooth=(0.5, 0.25), iter_lim=ITERS, history=True, row_weight=np.ones(rows), col_scale=np.ones((T.qy, T.qx)))
    assert_same_run(ones, old)
    for name, n in (("row_weight", rows), ("col_scale", T.qy * T.qx), ("x0", T.qy * T.qx)):
        a = np.ones(n)
        a[n // 2] = np.nan
        with pytest.raises(_lib.RtmiError, match=f"rtmi_tomo_lsqr_weighted: {name} has a value that is not finite"):
            T.lsqr(rhs, iter_lim=2, **{name: a})
    with pytest.raises(ValueError, match="row_weight must have 65 values"):
        T.lsqr(rhs, iter_lim=2, row_weight=np.ones(64))
    got = T.lsqr(rhs, iter_lim=3, row_weight=np.full(rows, 1e-170))
    assert (got["istop"], got["itn"]) == (_lib.LSQR_RANGE, 0) and not got["x"].any()
