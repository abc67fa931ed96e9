"""GPU: many vectors at once on the tomography matrix (rtmi_tomo_apply_multi, _transpose_multi, their _dev forms,
rtmi_tomo_lsqr_multi).  The yardstick of every check is the single-vector entry on the same column: the
bytes must be equal.  Products: every compiled chunk width (1, 2, 4, 8), a partial last chunk and 64 columns, at the slice edges
of the row storage, over three appends, with skipped rays, empty rows and permuted rays; columns whose exponents differ by
hundreds, a zero column, weights that are not finite; the refusal of a column out of range; repetition; the device-pointer
forms.  Solver: with and without a basis, every regulariser, shared and per-column options; columns that stop at different
iterations in one call; history past itn; a swap of two columns; recover, bootstrap and the grouping of lsqr_multi; refusals.
The single entries are the batched code with one column, so section 3 holds the columns of one call to
the host restatement directly, and checks planes of odd and even length and vectors 8 bytes off a 16-byte boundary."""
import ctypes as C

import numpy as np
import pytest

import tomo_basis_ref as BR
from conftest import LIMITS

pytestmark = pytest.mark.gpu

VERT_BOX = LIMITS["vert_heterogeneous"]
LINE = (1.0, 0.0, 2.0)                   # tests/test_gpu_tomo.py's line of the scenario: x = 2
NRHS = (1, 2, 3, 4, 5, 8, 9, 64)         # widths 1, 2, 4, 8 alone; 2 + 1 of 2, 4 + 1 of 4, 8 + 1 of 8 (partial chunks); 8 chunks of 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def fan(rb, F, R, thetas=None):
    """tests/test_gpu_tomo_basis.py's vert_heterogeneous op6 fan from (-2, -2) with its full record"""
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = thetas if thetas is not None else (np.linspace(0.05, np.pi / 2 - 0.05, R) if R > 1 else np.array([np.pi / 4]))
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1.0, th, -2.0, -2.0, record_stride=0)
    c.run()
    rec_rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1.0, th, -2.0, -2.0, rec_rows=rec_rows)
    b.run()
    return b


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def field(rb):
    """the field at 4 DELTA: a few thousand samples, so that 64 columns of accumulators stay small"""
    F = rb.Field.build("vert_heterogeneous", VERT_BOX, 4 * rb.DELTA)
    yield F
    F.close()


@pytest.fixture(scope="module")
def coarse(rb, field):
    """tests/test_gpu_tomo_basis.py's: 65 rays of op6 compiled on the field at 4 DELTA"""
    b = fan(rb, field, 65)
    T = rb.Tomography(field)
    T.append(b)
    b.close()
    yield T
    T.close()


def singles(T, X, W):
    """the yardstick, once per handle: matvec and rmatvec column by column"""
    return np.stack([T.matvec(x) for x in X]), np.stack([T.rmatvec(w) for w in W])


def check_columns(T, seed, widths=NRHS):
    rng = np.random.default_rng(seed)
    rows, top = T.info()["rows"], max(widths)
    X, W = rng.standard_normal((top, T.qy, T.qx)), rng.standard_normal((top, rows))
    Y1, G1 = singles(T, X, W)
    assert G1.any() and (rows == 0 or Y1.any())
    for n in widths:
        Y, G = T.matmat(X[:n]), T.rmatmat(W[:n])
        assert Y.shape == (n, rows) and G.shape == (n, T.qy, T.qx)
        assert bits(Y) == bits(Y1[:n]), n
        assert bits(G) == bits(G1[:n]), n
    return X, W, Y1, G1


# ---------------------------------------------------------------- 1. products
@pytest.mark.parametrize("R", [1, 63, 65, 130])
def test_every_column_has_the_single_products_bits(rb, field, R):
    """three appends -- ends, then crossings 0 and 1 of the line --, R at the edges of the 64-row slices"""
    b = fan(rb, field, R)
    T = rb.Tomography(field)
    T.append(b)
    for c in (0, 1):
        T.append(b, which=np.full(R, c, dtype=np.int32), line=LINE, kmax=4)
    b.close()
    assert T.info()["rows"] == 3 * R
    check_columns(T, R)
    T.close()


def test_skipped_rays_empty_rows_and_permuted_rays(rb, field):
    R = 130
    rng = np.random.default_rng(5)
    th = np.linspace(0.05, np.pi / 2 - 0.05, R)[rng.permutation(R)]
    which = np.tile(np.array([-1, 0, rb._lib.TOMO_SKIP, 1, 3], dtype=np.int32), R // 5)      # no ray crosses four times: empty rows
    b = fan(rb, field, R, thetas=th)
    T = rb.Tomography(field)
    _, nseg = T.append(b, which=which, line=LINE, kmax=4)
    T.append(b)
    b.close()
    assert (nseg[which == rb._lib.TOMO_SKIP] == -1).all() and (nseg[which == 3] == 0).all()
    assert T.info()["rows"] == R + int((which != rb._lib.TOMO_SKIP).sum())
    X, W, Y1, _ = check_columns(T, 6, widths=(3, 9))
    empty = np.nonzero(nseg[which != rb._lib.TOMO_SKIP] == 0)[0]
    assert len(empty) and not Y1[:, empty].any() and not np.signbit(T.matmat(X[:3])[:, empty]).any()
    T.close()


def test_columns_of_very_different_size_and_weights_that_are_not_finite(rb, coarse, torch):
    """One call, side by side: a zero column; magnitudes 1e-150 and 1e+150, whose exponents the single calls report hundreds
    apart; an infinite and a NaN weight among finite ones (they count as 0; the device-pointer form takes them); zero on every
    second row."""
    T = coarse
    rows = T.info()["rows"]
    rng = np.random.default_rng(7)
    W = rng.standard_normal((5, rows))
    W[0] = 0.0
    W[1] *= 1e-150
    W[2] *= 1e150
    W[3, 5], W[3, 17] = np.inf, np.nan
    W[4, ::2] = 0.0
    dW = torch.tensor(W, device="cuda")
    G, st = T.rmatmat_device(dW, stats=True)
    G = G.cpu().numpy()
    one = [T.rmatvec_device(dW[s].contiguous(), stats=True) for s in range(5)]
    for s in range(5):
        assert bits(G[s]) == bits(one[s][0].cpu().numpy()), s
    e = [o[1]["scale_exp"] for o in one]
    assert e[2] - e[1] > 900 and e[0] == 0                                  # per-column exponents, not one for the call
    assert st["scale_exp"] == max(e[1:]) and st["atomics"] > 0            # which lanes add together may differ: the count is not the singles' sum
    assert not G[0].any() and not np.signbit(G[0]).any()                     # W = 0: +0.0 everywhere
    clean = W[3].copy()
    clean[[5, 17]] = 0.0
    assert bits(G[3]) == bits(T.rmatvec(clean)) and G[3].any()
    # the host form takes the finite columns and gives the same bytes; it refuses the others as the single call does
    keep = [0, 1, 2, 4]
    assert bits(T.rmatmat(W[keep])) == bits(G[keep])
    with pytest.raises(rb._lib.RtmiError, match="w has a value that is not finite"):
        T.rmatmat(W)


def test_a_column_out_of_range_is_refused_as_the_single_call_refuses_it(rb, coarse):
    """The single call refuses a w whose fl(Vmax max|w|) is not a normal number.  Whether magnitude 1e+300 is such a w depends on
    Vmax; 1e-320 always is.  For both, the call with that column among ordinary ones must do what the single call does, and a
    refusal names the first such column."""
    T = coarse
    rows = T.info()["rows"]
    w = np.random.default_rng(8).standard_normal(rows)
    refusals = 0
    for mag in (1e300, 1e-320):
        W = np.stack([w, w * mag, w, w * mag])
        try:
            want = T.rmatvec(W[1])
        except rb._lib.RtmiError as err:
            assert "not a normal number" in str(err)
            refusals += 1
            with pytest.raises(rb._lib.RtmiError, match=r"column 1: Vmax max\|w\| is not a normal number"):
                T.rmatmat(W)
        else:
            G = T.rmatmat(W)
            assert bits(G[1]) == bits(want) == bits(G[3]) and bits(G[0]) == bits(T.rmatvec(w))
    assert refusals >= 1
    assert bits(T.rmatmat(W[[0, 2]])) == bits(np.stack([T.rmatvec(w)] * 2))  # the handle still works


def test_repeating_a_call_gives_the_same_bytes(rb, coarse):
    T = coarse
    rng = np.random.default_rng(9)
    X, W = rng.standard_normal((9, T.qy, T.qx)), rng.standard_normal((9, T.info()["rows"]))
    assert bits(T.matmat(X)) == bits(T.matmat(X))
    g1, s1 = T.rmatmat(W, stats=True)
    g64 = T.rmatmat(np.concatenate([W] * 7 + [W[:1]]))                        # 64 columns in between: the accumulators grow
    g2, s2 = T.rmatmat(W, stats=True)
    assert bits(g1) == bits(g2) == bits(g64[:9]) == bits(g64[9:18]) and s1["atomics"] == s2["atomics"] > 0
    assert s2["bytes_device"] >= s1["bytes_device"] >= 9 * 128 * T.qy * T.qx
    assert T.matmat(np.zeros((0, T.qy, T.qx))).shape == (0, T.info()["rows"])


def test_device_pointer_forms(rb, coarse, torch):
    from raytracing_amd import _lib
    T = coarse
    L = _lib.lib()
    nz, rows, S = T.qx * T.qy, T.info()["rows"], 5
    rng = np.random.default_rng(10)
    X, W = rng.standard_normal((S, T.qy, T.qx)), rng.standard_normal((S, rows))
    dX, dW = torch.tensor(X, device="cuda"), torch.tensor(W, device="cuda")
    assert bits(T.matmat_device(dX).cpu().numpy()) == bits(T.matmat(X))
    assert bits(T.rmatmat_device(dW).cpu().numpy()) == bits(T.rmatmat(W))
    out = torch.empty((S, rows), dtype=torch.float64, device="cuda")
    assert T.matmat_device(dX, out=out) is out and bits(out.cpu().numpy()) == bits(T.matmat(X))
    with pytest.raises(ValueError, match="on a GPU"):
        T.matmat_device(torch.tensor(X))
    with pytest.raises(ValueError, match="on a GPU"):
        T.rmatmat_device(torch.tensor(W))
    torch.cuda.synchronize()
    hx, hw = np.zeros((S, nz)), np.zeros((S, rows))
    dY, dG = torch.zeros((S, rows), dtype=torch.float64, device="cuda"), torch.zeros((S, nz), dtype=torch.float64, device="cuda")
    for fn, args, name in ((L.rtmi_tomo_apply_multi_dev, (hx.ctypes.data, dY.data_ptr()), b"d_x"),
                           (L.rtmi_tomo_apply_multi_dev, (dX.data_ptr(), hw.ctypes.data), b"d_y"),
                           (L.rtmi_tomo_transpose_multi_dev, (hw.ctypes.data, dG.data_ptr()), b"d_w"),
                           (L.rtmi_tomo_transpose_multi_dev, (dW.data_ptr(), hx.ctypes.data), b"d_g")):
        assert fn(T._h, S, *args, None) == -1
        assert name in L.rtmi_last_error() and b"handle's device" in L.rtmi_last_error()
    # short buffers: an allocation of the runtime's own, whose end the test knows
    hip = C.CDLL(_lib.mapped_hip_runtimes()[0])
    for f in (hip.hipMalloc, hip.hipFree, hip.hipMemGetAddressRange):
        f.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(p), 2 * S * nz * 8) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), p) == 0 and size.value >= 2 * S * nz * 8
        end = base.value + size.value
        # room for S - 1 planes and all but one value of the last: one column would fit, S do not
        assert L.rtmi_tomo_apply_multi_dev(T._h, S, end - 8 * S * nz + 8, dY.data_ptr(), None) == -1
        assert b"d_x is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_apply_multi_dev(T._h, S, dX.data_ptr(), end - 8 * S * rows + 8, None) == -1
        assert b"d_y is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_transpose_multi_dev(T._h, S, end - 8 * S * rows + 8, dG.data_ptr(), None) == -1
        assert b"d_w is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_transpose_multi_dev(T._h, S, dW.data_ptr(), end - 8 * S * nz + 8, None) == -1
        assert b"d_g is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_transpose_multi_dev(T._h, S, dW.data_ptr(), end - 8 * S * nz, None) == 0, L.rtmi_last_error()   # just fits
    finally:
        assert hip.hipFree(p) == 0


# ---------------------------------------------------------------- 2. the solver, column by column against Tomography.lsqr
D1, D2 = (0.5, 0.25), (0.3, 0.2)
REG = {"none": (None, None), "smooth": (D1, None), "smooth2": (None, D2)}


def same(out, ref, keys=("x", "c")):
    """tests/test_gpu_tomo_basis.py's comparison: x, c, the history, itn, istop and the four norms"""
    assert (out["itn"], out["istop"]) == (ref["itn"], ref["istop"])
    for k in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(out[k]) == bits(ref[k]), k
    assert bits(out["history"]) == bits(ref["history"])
    for k in keys:
        assert bits(out[k]) == bits(ref[k]), k


def options(T, gy, gx, S, kind, seed=51):
    """none; shared: one row_weight, a col_scale with a zero entry, an x0; percol: the same with one weighting per column, the
    second of them a jackknife that zeroes half the rows"""
    if kind == "none":
        return {}
    rng = np.random.default_rng(seed)
    rows = T.info()["rows"]
    dc = 0.5 + rng.random((gy, gx))
    dc[1, 2] = 0.0
    o = dict(row_weight=0.5 + rng.random(rows), col_scale=dc, x0=1e-2 * rng.standard_normal((T.qy, T.qx)))
    if kind == "percol":
        wr = 0.5 + rng.random((S, rows))
        wr[1, rng.permutation(rows)[:rows // 2]] = 0.0
        o["row_weight"] = wr
    return o


def column(o, s):
    """the options of column s alone"""
    c = dict(o)
    if "row_weight" in c and np.ndim(c["row_weight"]) == 2:
        c["row_weight"] = c["row_weight"][s]
    return c


@pytest.mark.parametrize("kind", ["none", "shared", "percol"])
@pytest.mark.parametrize("with_basis", [False, True], ids=["fine", "basis"])
def test_solver_columns_equal_the_single_solver_bit_for_bit(rb, coarse, with_basis, kind):
    T = coarse
    S = 3
    P = rb.TomoBasis.bspline(T, 9, 7) if with_basis else None
    gy, gx = (7, 9) if with_basis else (T.qy, T.qx)
    keys = ("x", "c") if with_basis else ("x",)
    rhs = np.random.default_rng(31).standard_normal((S, T.info()["rows"]))
    o = options(T, gy, gx, S, kind)
    for reg, (d1, d2) in REG.items():
        for damp in (0.0, 1e-3):
            kw = dict(damp=damp, smooth=d1, smooth2=d2, basis=P, iter_lim=6, history=True)
            outs = T.lsqr_multi(rhs, **kw, **o)
            assert len(outs) == S
            for s in range(S):
                ref = T.lsqr(rhs[s], **kw, **column(o, s))
                assert ref["itn"] == 6 and ref["x"].any()
                same(outs[s], ref, keys)
                assert ("c" in outs[s]) == with_basis
    if P is not None:
        P.close()


def test_columns_that_stop_at_different_points(rb, coarse):
    """One call holds: a zero right-hand side (itn 0, istop 0); rhs 1e-170 (RTMI_LSQR_RANGE at the start); a random right-hand
    side, which 63 coefficients cannot fit and which runs to iter_lim; consistent right-hand sides A P c, which stop on btol in
    between.  The single solver must give at least three distinct itn over the columns, one of them strictly inside; then every
    column of the one call must equal it, and the history past a column's itn must be zero."""
    from raytracing_amd import _lib
    T = coarse
    rows = T.info()["rows"]
    P = rb.TomoBasis.bspline(T, 9, 7)
    rng = np.random.default_rng(61)
    r = rng.standard_normal(rows)
    jj, ii = np.meshgrid(np.linspace(0, 1, 9), np.linspace(0, 1, 7))
    smooth_c = 1.0 + 0.3 * ii + 0.2 * jj
    rough_c = smooth_c + 0.2 * rng.standard_normal((7, 9))
    rhs = np.stack([np.zeros(rows), r * 1e-170, r, T.matvec(P.prolong(smooth_c)), T.matvec(P.prolong(rough_c))])
    kw = dict(basis=P, iter_lim=12, atol=0.0, btol=0.05, history=True)
    refs = [T.lsqr(b, **kw) for b in rhs]
    itn = [o["itn"] for o in refs]
    print("single solver: itn", itn, "istop", [o["istop"] for o in refs])
    assert (refs[0]["itn"], refs[0]["istop"]) == (0, 0)
    assert (refs[1]["itn"], refs[1]["istop"]) == (0, rb._lib.LSQR_RANGE)
    assert (refs[2]["itn"], refs[2]["istop"]) == (12, 7)
    assert len(set(itn)) >= 3 and any(0 < k < 12 and o["istop"] in (1, 2) for k, o in zip(itn, refs))
    outs = T.lsqr_multi(rhs, **kw)
    for s in range(len(rhs)):
        same(outs[s], refs[s])
    # through the C entry, with a history that starts from garbage: rows past itn come back zero
    S = len(rhs)
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.btol = 12, 0.05
    hist = np.full((S, 12, 4), np.nan)
    x, c = np.empty((S, T.qy, T.qx)), np.empty((S, 7, 9))
    st = (_lib.LsqrStats * S)()
    _lib.check(_lib.lib().rtmi_tomo_lsqr_multi(T._h, P._h, C.byref(lp), None, None, S, 0, _lib.dptr(rhs), _lib.dptr(c), _lib.dptr(x),
                                               _lib.dptr(hist), st))
    for s in range(S):
        assert st[s].itn == itn[s] and bits(hist[s, :itn[s]]) == bits(refs[s]["history"])
        assert not hist[s, itn[s]:].any() and not np.isnan(hist[s]).any()
        assert bits(x[s]) == bits(refs[s]["x"]) and bits(c[s]) == bits(refs[s]["c"])
        assert st[s].total_ms == st[0].total_ms and st[s].bytes_device == st[0].bytes_device
    P.close()


def test_swapping_two_columns_swaps_the_outputs(rb, coarse):
    T = coarse
    rhs = np.random.default_rng(62).standard_normal((4, T.info()["rows"]))
    rhs[2] *= 1e-3
    kw = dict(damp=1e-3, smooth2=D2, iter_lim=5, history=True)
    a = T.lsqr_multi(rhs, **kw)
    b = T.lsqr_multi(rhs[[0, 3, 2, 1]], **kw)
    for s, q in enumerate([0, 3, 2, 1]):
        same(b[s], a[q], keys=("x",))
    assert bits(a[1]["x"]) != bits(a[3]["x"])


def test_recover_is_lsqr_of_matvec_per_model(rb, coarse):
    T = coarse
    models = np.concatenate([rb.checkerboard(T.qy, T.qx, 8, 0.01)[None], rb.spikes(T.qy, T.qx, [(T.qy // 2, T.qx // 2), (3, 5)], 0.05)])
    kw = dict(damp=1e-3, iter_lim=5, history=True)
    rec, outs = T.recover(models, **kw)
    assert rec.shape == models.shape and len(outs) == 3
    for s in range(3):
        ref = T.lsqr(T.matvec(models[s]), **kw)
        same(outs[s], ref, keys=("x",))
        assert bits(rec[s]) == bits(ref["x"])


def test_bootstrap_is_numpys_mean_and_deviation_of_the_single_solves(rb, coarse):
    T = coarse
    rows = T.info()["rows"]
    rng = np.random.default_rng(63)
    rhs, base = rng.standard_normal(rows), 0.5 + rng.random(rows)
    kw = dict(damp=1e-3, iter_lim=4)
    for row_weight in (None, base):
        mean, std, outs = T.bootstrap(rhs, 6, 11, results=True, row_weight=row_weight, **kw)
        w = rb.bootstrap_weights(rows, 6, 11)
        if row_weight is not None:
            w = w * base[None, :]
        xs = np.stack([T.lsqr(rhs, row_weight=w[k], **kw)["x"] for k in range(6)])
        for k in range(6):
            assert bits(outs[k]["x"]) == bits(xs[k])
        assert bits(mean) == bits(xs.mean(axis=0)) and bits(std) == bits(xs.std(axis=0, ddof=1))
        assert std.any()
    assert len(T.bootstrap(rhs, 3, 11, **kw)) == 2


def test_grouping_changes_no_byte(rb, coarse):
    T = coarse
    S = 70
    rhs = np.random.default_rng(64).standard_normal((S, T.info()["rows"]))
    wr = 0.5 + np.random.default_rng(65).random((S, T.info()["rows"]))
    kw = dict(damp=1e-3, iter_lim=3, history=True, row_weight=wr)
    a = T.lsqr_multi(rhs, group=64, **kw)
    b = T.lsqr_multi(rhs, group=3, **kw)
    assert len(a) == len(b) == S
    for s in range(S):
        same(b[s], a[s], keys=("x",))
    for s in (0, 63, 64, 69):
        same(a[s], T.lsqr(rhs[s], damp=1e-3, iter_lim=3, history=True, row_weight=wr[s]), keys=("x",))


# ---------------------------------------------------------------- 3. one code for every width
# The single solver is the batched one with one column, so "every column equals the single solver" compares two widths of one
# code.  What holds a column to independent arithmetic is the host restatement, and what could differ between the widths is the
# 16-byte form of the vector passes, which a launch of S > 1 columns takes only when every plane stride is even.
def cubic(rb, T, mx, my):
    """the cubic B-spline basis on the device and its restatement"""
    (fx, wx), (fy, wy) = BR.bspline_axis(T.qx, mx, 3), BR.bspline_axis(T.qy, my, 3)
    return rb.TomoBasis(T, fx, wx, fy, wy, mx, my), BR.Basis(fx, wx, fy, wy, mx, my)


@pytest.fixture(scope="module")
def matrix(coarse):
    """what the restatement needs of `coarse`, read once"""
    return coarse.read() + (coarse.info()["vmax"],)


@pytest.mark.parametrize("kind", ["shared", "percol"])
@pytest.mark.parametrize("reg", ["smooth", "smooth2"])
@pytest.mark.parametrize("with_basis", [False, True], ids=["fine", "basis"])
def test_solver_columns_equal_the_host_restatement_bit_for_bit(rb, coarse, matrix, with_basis, reg, kind):
    T = coarse
    rp, base, val, vmax = matrix
    S = 3
    P, R = cubic(rb, T, 9, 7) if with_basis else (None, None)
    gy, gx = (7, 9) if with_basis else (T.qy, T.qx)
    d1, d2 = REG[reg]
    rhs = np.random.default_rng(71).standard_normal((S, T.info()["rows"]))
    o = options(T, gy, gx, S, kind, seed=72)
    outs = T.lsqr_multi(rhs, damp=1e-3, smooth=d1, smooth2=d2, basis=P, iter_lim=6, history=True, **o)
    if P is not None:
        P.close()
    for s in range(S):
        k = column(o, s)
        ref = BR.lsqr(rp, base, val, T.qx, T.qy, rhs[s], 6, basis=R, d1=d1, d2=d2, wr=k["row_weight"], dc=k["col_scale"], x0=k["x0"],
                      vmax=vmax, damp=1e-3)
        assert ref["itn"] == 6 and ref["x"].any()
        same(outs[s], ref, ("x", "c") if with_basis else ("x",))


@pytest.fixture(scope="module")
def skipped(rb, field):
    """`coarse` less one ray: 64 rows"""
    which = np.full(65, -1, dtype=np.int32)
    which[17] = rb._lib.TOMO_SKIP
    b = fan(rb, field, 65)
    T = rb.Tomography(field)
    T.append(b, which=which, line=LINE, kmax=4)
    b.close()
    yield T
    T.close()


def test_planes_of_odd_and_even_length(rb, coarse, skipped):
    """The planes of a call with S > 1 columns start `per` (data) and `ng` (model) values apart: an odd one puts every second
    plane 8 bytes off a 16-byte boundary.  65 or 64 rows with first differences on a 9 x 7 or an 8 x 7 coefficient grid give all
    four parities of (per, ng); every pass of the loop has a diagonal to read or a copy to write."""
    seen = set()
    for T in (coarse, skipped):
        rows = T.info()["rows"]
        for mx in (9, 8):
            P, _ = cubic(rb, T, mx, 7)
            ng, per = mx * 7, rows + 7 * (mx - 1) + 6 * mx
            seen.add((per % 2, ng % 2))
            for S in (2, 3):
                rhs = np.random.default_rng(81 + S).standard_normal((S, rows))
                o = options(T, 7, mx, S, "percol", seed=82)
                kw = dict(damp=1e-3, smooth=D1, basis=P, iter_lim=5, history=True)
                outs = T.lsqr_multi(rhs, **kw, **o)
                for s in range(S):
                    ref = T.lsqr(rhs[s], **kw, **column(o, s))
                    assert ref["itn"] == 5 and ref["x"].any()
                    same(outs[s], ref)
            P.close()
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_device_pointer_forms_take_a_view_that_is_8_bytes_off(rb, coarse, torch):
    """one vector that starts 8 bytes past a 16-byte boundary is neither refused nor read 16 bytes wide: the bytes are those of
    the host call, and the value before the view and the one after it are not touched"""
    T = coarse
    nz, rows = T.qy * T.qx, T.info()["rows"]
    rng = np.random.default_rng(91)
    x, w = rng.standard_normal(nz), rng.standard_normal(rows)

    def off8(n, fill=None):
        buf = torch.full((n + 3,), 7.0, dtype=torch.float64, device="cuda")
        v = buf[1:n + 1] if buf.data_ptr() % 16 == 0 else buf[2:n + 2]
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        if fill is not None:
            v.copy_(torch.tensor(fill, device="cuda"))
        return buf, v
    (_, dx), (_, dw) = off8(nz, x), off8(rows, w)
    (by, dy), (bg, dg) = off8(rows), off8(nz)
    assert bits(T.matvec_device(dx, out=dy).cpu().numpy()) == bits(T.matvec(x))
    assert bits(T.rmatvec_device(dw, out=dg).cpu().numpy()) == bits(T.rmatvec(w))
    for buf, n in ((by, rows), (bg, nz)):
        assert int((buf == 7.0).sum()) >= 3 and float(buf[0]) == 7.0 and float(buf[-1]) == 7.0
    # one column of the batched form goes the same way
    assert bits(T.matmat_device(dx.reshape(1, T.qy, T.qx)).cpu().numpy()) == bits(T.matvec(x))
    assert bits(T.rmatmat_device(dw.reshape(1, rows)).cpu().numpy()) == bits(T.rmatvec(w))


# ---------------------------------------------------------------- 4. refusals
def test_refusals(rb, coarse):
    from raytracing_amd import _lib
    T = coarse
    L = _lib.lib()
    rows, nz = T.info()["rows"], T.qy * T.qx
    lp = _lib.LsqrParams()
    lp.iter_lim = 2
    rhs, x = np.ones((65, rows)), np.empty((65, T.qy, T.qx))

    def call(nrhs=2, flags=0, lo=None, p=None, rhs=rhs, lp=lp, x=x):
        return L.rtmi_tomo_lsqr_multi(T._h, p, None if lp is None else C.byref(lp), None if lo is None else C.byref(lo), None, nrhs, flags,
                                      _lib.dptr(rhs), None, _lib.dptr(x), None, None)

    def refused(code, *texts):
        assert code == -1
        for t in texts:
            assert t.encode() in L.rtmi_last_error(), L.rtmi_last_error()
    for nrhs in (0, 65):
        refused(call(nrhs=nrhs), "nrhs must be in 1 .. 64")
        refused(L.rtmi_tomo_apply_multi(T._h, nrhs, _lib.dptr(x), _lib.dptr(rhs), None), "nrhs must be in 1 .. 64")
        refused(L.rtmi_tomo_transpose_multi(T._h, nrhs, _lib.dptr(rhs), _lib.dptr(x), None), "nrhs must be in 1 .. 64")
    refused(call(flags=2), "flags has bits other than RTMI_LSQR_MULTI_ROW_WEIGHT")
    refused(call(flags=5), "flags has bits other than RTMI_LSQR_MULTI_ROW_WEIGHT")
    refused(call(lp=None), "null params")
    refused(call(rhs=None), "null rhs")
    refused(call(x=None), "null x")
    bad = rhs.copy()
    bad[1, 3] = np.inf                                                       # in the second column
    refused(call(rhs=bad), "rhs has a value that is not finite")
    assert call(nrhs=1, rhs=bad) == 0, L.rtmi_last_error()                   # which a call of one column does not read
    # options: a value that is not finite, the per-column weights checked over all their columns
    wr = np.ones((2, rows))
    wr[1, 7] = np.nan
    lo = _lib.LsqrOptions()
    lo.row_weight = _lib.dptr(wr)
    refused(call(lo=lo, flags=_lib.LSQR_MULTI_ROW_WEIGHT), "row_weight has a value that is not finite")
    assert call(lo=lo) == 0, L.rtmi_last_error()                             # shared: only the first `rows` values are the call's
    with pytest.raises(_lib.RtmiError, match="col_scale has a value that is not finite"):
        T.lsqr_multi(rhs[:2], col_scale=np.full((T.qy, T.qx), np.inf), iter_lim=2)
    badx = np.zeros((T.qy, T.qx)); badx[-1, -1] = np.nan
    with pytest.raises(_lib.RtmiError, match="x0 has a value that is not finite"):
        T.lsqr_multi(rhs[:2], x0=badx, iter_lim=2)
    with pytest.raises(_lib.RtmiError, match="reg.d2 must be finite and >= 0"):
        T.lsqr_multi(rhs[:2], smooth2=(-1.0, 0.0), iter_lim=2)
    with pytest.raises(_lib.RtmiError, match="x has a value that is not finite"):
        T.matmat(np.full((2, T.qy, T.qx), np.nan))
    # a basis made on a handle of another shape
    xa, ya = np.linspace(-2.0, 5.0, T.qx + 1), np.linspace(-2.5, 1.0, T.qy)
    Fo = rb.Field.from_samples(xa, ya, np.ones((T.qy, T.qx + 1)), rb.DELTA)
    To = rb.Tomography(Fo)
    Fo.close()
    Po = rb.TomoBasis.bspline(To, 9, 7)
    To.close()
    with pytest.raises(_lib.RtmiError, match="another shape or device"):
        T.lsqr_multi(rhs[:2], basis=Po, iter_lim=2)
    Po.close()
    Fe = rb.Field.from_samples(xa[:-1], ya, np.ones((T.qy, T.qx)), rb.DELTA)
    E = rb.Tomography(Fe)
    Fe.close()
    refused(L.rtmi_tomo_lsqr_multi(E._h, None, C.byref(lp), None, None, 2, 0, _lib.dptr(rhs), None, _lib.dptr(x), None, None), "no rows")
    E.close()
    assert [o["itn"] for o in T.lsqr_multi(rhs[:2], iter_lim=2)] == [2, 2]  # the handle still works
