"""GPU: the tomography model basis, second-difference smoothing and the solver that takes both (rtmi_tomo_basis_*,
rtmi_tomo_lsqr_basis) against the restatement (tests/tomo_basis_ref.py): prolong and restrict bit for bit at
the shapes where the restrict kernel's tiles end; adjointness and P 1 = 1 on the device; restrict's bits under repetition and
through the device-pointer call; the solver bit for bit with every combination of regulariser and options; the entry without a
basis against the solvers it then equals; the identity basis; masked and unreached coefficients; a start model alone; early
returns; every refusal; crosswell tomography on a coarse cubic grid."""
import ctypes as C

import numpy as np
import pytest

import tomo_basis_ref as BR
from conftest import LIMITS

pytestmark = pytest.mark.gpu

VERT_BOX = LIMITS["vert_heterogeneous"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def fan(rb, F, R):
    """tests/test_gpu_tomo.py's vert_heterogeneous op6 fan from (-2, -2) with its full record"""
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, np.pi / 2 - 0.05, R)
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
def coarse(rb):
    """tests/test_gpu_tomo.py's: the field at 4 DELTA, 65 rays of op6 compiled on it, and what the restatement needs of them"""
    F = rb.Field.build("vert_heterogeneous", VERT_BOX, 4 * rb.DELTA)
    b = fan(rb, F, 65)
    T = rb.Tomography(F)
    T.append(b)
    b.close()
    yield F, T, T.read() + (T.info()["vmax"],)
    T.close()
    F.close()


def caller_axis(q):
    """B = 2 onto m = 9 for any q >= 8: repeated first, a jump of B (1 -> 3), a jump past B that leaves coefficient 5 unreached
    (3 -> 6), a sample with both weights zero and one with one"""
    first = np.zeros(q, dtype=np.int32)
    for lo, hi, v in zip([0, q // 4, q // 2, (5 * q) // 8, q - 2], [q // 4, q // 2, (5 * q) // 8, q - 2, q], [0, 1, 3, 6, 7]):
        first[lo:hi] = v
    wgt = np.random.default_rng(q).standard_normal((q, 2))
    wgt[1] = 0.0
    wgt[q // 2, 1] = 0.0
    return first, wgt, 9


def empty_handle(rb, qx, qy):
    x, y = np.linspace(-2.0, 5.0, qx), np.linspace(-2.5, 1.0, qy)
    F = rb.Field.from_samples(x, y, 1.0 + 0.1 * np.add.outer(np.linspace(0, 1, qy), np.linspace(0, 1, qx)), rb.DELTA)
    T = rb.Tomography(F)
    F.close()                                                                # the handle keeps no reference to the field
    return T


def pair(rb, T, axes_x, axes_y):
    """the device basis and its restatement from (first, wgt, m) per axis"""
    (fx, wx, mx), (fy, wy, my) = axes_x, axes_y
    return rb.TomoBasis(T, fx, wx, fy, wy, mx, my), BR.Basis(fx, wx, fy, wy, mx, my)


def bspl(q, m, d):
    return BR.bspline_axis(q, m, d) + (m,)


# ---------------------------------------------------------------- 1. the pair against the restatement
# k_basis_restrict_x gives a block 256 neighbouring coefficients of one fine row (one per lane) and moves the run of fine samples
# they reach through LDS in pieces of 1024.  What each width straddles:
#   qx 8      less than a wave of coefficients and of samples
#   qx 63, 64, 65   the identity basis has mx = qx: the edge of the first wave of a block, from below, exactly, and from above
#   qx 257    the identity basis has 257 coefficients: the second block of a row holds one lane; mx = 1 walks 257 samples in one lane
#   qx 1025   mx = 1: the one range of 1025 samples takes two pieces, the second of one sample; the identity has five blocks, the
#             last with one lane; the cubic basis's 9 ranges make one run of 1025 samples, and the last coefficient's range
#             crosses the piece's edge at sample 1024
# qy 8 and 65 do the same for k_basis_restrict_y's loop over fine rows (ranges of 1, of all 65, of about 16 for the linear axis).
@pytest.mark.parametrize("qy", [8, 65])
@pytest.mark.parametrize("qx", [8, 63, 64, 65, 257, 1025])
def test_prolong_and_restrict_bit_for_bit(rb, qx, qy):
    T = empty_handle(rb, qx, qy)
    rng = np.random.default_rng(qx + qy)
    x = rng.standard_normal((qy, qx))
    cases = {
        "cubic x linear 9 x 7": (bspl(qx, 9, 3), bspl(qy, 7, 1)),
        "degree 0, one coefficient": (bspl(qx, 1, 0), bspl(qy, 1, 0)),
        "identity": (bspl(qx, qx, 0), bspl(qy, qy, 0)),
        "caller-made x, linear y": (caller_axis(qx), bspl(qy, 7, 1)),
    }
    for name, (ax, ay) in cases.items():
        P, R = pair(rb, T, ax, ay)
        assert P.shape == (qy * qx, R.my * R.mx)
        c = rng.standard_normal((R.my, R.mx))
        px, g = P.prolong(c), P.restrict(x)
        assert bits(px) == bits(R.prolong(c)), name
        assert bits(g) == bits(R.restrict(x)), name
        if name == "identity":
            assert np.array_equal(px, c) and np.array_equal(g, x)
        if name.startswith("caller"):
            assert not g[:, 5].any() and not np.signbit(g[:, 5]).any()       # the unreached coefficient: +0.0, sign bit clear
        P.close()
    T.close()


def test_adjointness_and_constants_on_the_device(rb, coarse):
    F, T, _ = coarse
    rng = np.random.default_rng(11)
    P, R = pair(rb, T, bspl(T.qx, 9, 3), bspl(T.qy, 7, 1))
    c, x = rng.standard_normal((7, 9)), rng.standard_normal((T.qy, T.qx))
    Pc, Ptx = P.prolong(c), P.restrict(x)
    lhs, rhs = float(np.sum(Pc * x)), float(np.sum(c * Ptx))
    scale = float(np.sum(np.abs(R.axis_matrix("y")) @ np.abs(c) @ np.abs(R.axis_matrix("x")).T * np.abs(x)))
    print(f"<P c, x> - <c, P^T x> = {abs(lhs - rhs) / scale:.2e} of sum |terms|")
    assert abs(lhs - rhs) <= 1e-15 * scale
    P.close()
    for d in (0, 1, 3):
        P = rb.TomoBasis.bspline(T, 9, 7, degree=d)
        one = float(np.max(np.abs(P.prolong(np.ones((7, 9))) - 1.0)))
        print(f"degree {d}: |P 1 - 1| {one:.2e}")
        assert one <= 4.5e-16
        P.close()
    P = rb.TomoBasis.bspline(T, 9, 7, degree=(3, 1))
    assert P.shape == (T.qy * T.qx, 63)
    P.close()


def test_restrict_bits_repeat_and_through_the_device_call(rb, coarse, torch):
    F, T, _ = coarse
    rng = np.random.default_rng(12)
    P = rb.TomoBasis.bspline(T, 9, 7)
    x, c = rng.standard_normal((T.qy, T.qx)), rng.standard_normal((7, 9))
    g1, g2 = P.restrict(x), P.restrict(x)
    gd = P.restrict_device(torch.tensor(x, device="cuda"))
    out = torch.empty((7, 9), dtype=torch.float64, device="cuda")
    assert P.restrict_device(torch.tensor(x, device="cuda"), out=out) is out
    assert bits(g1) == bits(g2) == bits(gd.cpu().numpy()) == bits(out.cpu().numpy())
    assert bits(P.prolong_device(torch.tensor(c, device="cuda")).cpu().numpy()) == bits(P.prolong(c))
    with pytest.raises(ValueError, match="on a GPU"):
        P.restrict_device(torch.tensor(x))
    P.close()
    with pytest.raises(ValueError, match="closed"):
        P.restrict(x)


# ---------------------------------------------------------------- 2. the solver against the restatement
D1, D2 = (0.5, 0.25), (0.3, 0.2)
REG = {"none": (None, None), "d1": (D1, None), "d2": (None, D2), "both": (D1, D2)}


def options(T, gy, gx, seed=51):
    rng = np.random.default_rng(seed)
    dc = 0.5 + rng.random((gy, gx))
    dc[1, 2] = 0.0                                                           # a masked coefficient
    return dict(row_weight=0.5 + rng.random(T.info()["rows"]), col_scale=dc, x0=1e-2 * rng.standard_normal((T.qy, T.qx)))


def same(out, ref, keys=("x", "c")):
    assert (out["itn"], out["istop"]) == (ref["itn"], ref["istop"])
    for k in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(out[k]) == bits(ref[k]), k
    assert bits(out["history"]) == bits(ref["history"])
    for k in keys:
        assert bits(out[k]) == bits(ref[k]), k


@pytest.mark.parametrize("opts", [False, True], ids=["plain", "options"])
@pytest.mark.parametrize("reg", list(REG))
@pytest.mark.parametrize("damp", [0.0, 1e-3])
def test_solver_equals_the_restatement_bit_for_bit(rb, coarse, damp, reg, opts):
    F, T, (rp, base, val, vmax) = coarse
    d1, d2 = REG[reg]
    P, R = pair(rb, T, bspl(T.qx, 9, 3), bspl(T.qy, 7, 3))
    rhs = np.random.default_rng(31).standard_normal(T.info()["rows"])
    o = options(T, 7, 9) if opts else {}
    out = T.lsqr(rhs, damp=damp, smooth=d1, smooth2=d2, basis=P, iter_lim=6, history=True, **o)
    ref = BR.lsqr(rp, base, val, T.qx, T.qy, rhs, 6, basis=R, d1=d1, d2=d2, wr=o.get("row_weight"), dc=o.get("col_scale"),
                  x0=o.get("x0"), vmax=vmax, damp=damp)
    P.close()
    assert out["c"].shape == (7, 9) and out["itn"] == 6 and out["istop"] == 7
    same(out, ref)
    if opts:
        assert out["c"][1, 2] == 0.0                                         # a zero col_scale entry gives c = 0 there


@pytest.mark.parametrize("opts", [False, True], ids=["plain", "options"])
def test_without_a_basis_and_second_differences_it_is_the_weighted_solver(rb, coarse, opts):
    F, T, _ = coarse
    rhs = np.random.default_rng(32).standard_normal(T.info()["rows"])
    o = options(T, T.qy, T.qx) if opts else {}
    for smooth in (None, D1):
        old = T.lsqr(rhs, damp=1e-3, smooth=smooth, iter_lim=6, history=True, **o)
        new = T.lsqr(rhs, damp=1e-3, smooth=smooth, smooth2=(0.0, 0.0), iter_lim=6, history=True, **o)     # rtmi_tomo_lsqr_basis, p NULL, d2 absent
        assert "c" not in new
        same(new, old, keys=("x",))


@pytest.mark.parametrize("opts", [False, True], ids=["plain", "options"])
def test_second_differences_without_a_basis_equal_the_restatement(rb, coarse, opts):
    F, T, (rp, base, val, vmax) = coarse
    rhs = np.random.default_rng(33).standard_normal(T.info()["rows"])
    o = options(T, T.qy, T.qx) if opts else {}
    for d1 in (None, D1):
        out = T.lsqr(rhs, damp=1e-3, smooth=d1, smooth2=D2, iter_lim=6, history=True, **o)
        ref = BR.lsqr(rp, base, val, T.qx, T.qy, rhs, 6, d1=d1, d2=D2, wr=o.get("row_weight"), dc=o.get("col_scale"), x0=o.get("x0"),
                      vmax=vmax, damp=1e-3)
        same(out, ref, keys=("x",))


def test_c_without_a_basis_is_x_less_the_start_model(rb, coarse):
    """c through the C entry with p NULL: x is c plus x0, with and without the launches of the weighted solver"""
    from raytracing_amd import _lib
    F, T, _ = coarse
    L = _lib.lib()
    rhs = np.random.default_rng(34).standard_normal(T.info()["rows"])
    o = options(T, T.qy, T.qx)
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.damp = 4, 1e-3
    for x0 in (None, o["x0"]):
        lo = _lib.LsqrOptions()
        dc = np.ascontiguousarray(o["col_scale"])
        lo.col_scale = _lib.dptr(dc)
        if x0 is not None:
            lo.x0 = _lib.dptr(x0)
        c, x = np.empty((T.qy, T.qx)), np.empty((T.qy, T.qx))
        _lib.check(L.rtmi_tomo_lsqr_basis(T._h, None, C.byref(lp), C.byref(lo), None, _lib.dptr(rhs), _lib.dptr(c), _lib.dptr(x), None, None))
        want = T.lsqr(rhs, damp=1e-3, iter_lim=4, col_scale=dc, x0=x0)["x"]
        assert bits(x) == bits(want)
        assert bits(x) == bits(c if x0 is None else x0 + c)


def test_identity_basis_gives_the_solve_without_a_basis(rb, coarse):
    F, T, _ = coarse
    rhs = np.random.default_rng(35).standard_normal(T.info()["rows"])
    P = rb.TomoBasis.bspline(T, T.qx, T.qy, degree=0)
    for smooth in (None, D1):
        old = T.lsqr(rhs, damp=1e-3, smooth=smooth, iter_lim=6, history=True)
        new = T.lsqr(rhs, damp=1e-3, smooth=smooth, basis=P, iter_lim=6, history=True)
        assert (new["itn"], new["istop"]) == (old["itn"], old["istop"])
        for k in ("x", "history", "r1norm", "r2norm", "anorm", "arnorm"):    # as numbers: prolong's +0.0 + ... turns a -0.0
            assert np.array_equal(new[k], old[k]), k
        assert np.array_equal(new["c"], new["x"])
    P.close()


def test_unreached_coefficient_start_model_alone_and_early_returns(rb, coarse):
    F, T, _ = coarse
    n = T.info()["rows"]
    rhs = np.random.default_rng(36).standard_normal(n)
    P, _ = pair(rb, T, caller_axis(T.qx), bspl(T.qy, 7, 3))
    out = T.lsqr(rhs, basis=P, iter_lim=6)
    assert out["itn"] == 6 and out["c"].any()
    assert not out["c"][:, 5].any()                                          # a column of zeros: exactly 0
    P.close()
    P = rb.TomoBasis.bspline(T, 9, 7)
    x0 = 1e-2 * np.random.default_rng(37).standard_normal((T.qy, T.qx))
    out = T.lsqr(T.matvec(x0), basis=P, smooth2=D2, x0=x0, iter_lim=4)
    assert (out["istop"], out["itn"]) == (0, 0) and bits(out["x"]) == bits(x0) and not out["c"].any()
    out = T.lsqr(np.zeros(n), basis=P, smooth2=D2, iter_lim=4)
    assert (out["istop"], out["itn"]) == (0, 0) and not out["x"].any() and not out["c"].any()
    out = T.lsqr(rhs * 1e-170, basis=P, smooth2=D2, iter_lim=4)            # max|rhs|^2 is below the normal range
    assert (out["istop"], out["itn"]) == (rb._lib.LSQR_RANGE, 0) and not out["x"].any()
    P.close()


# ---------------------------------------------------------------- 3. refusals
def test_device_pointer_calls_refuse_host_memory_and_short_buffers(rb, coarse, torch):
    from raytracing_amd import _lib
    F, T, _ = coarse
    L = _lib.lib()
    P = rb.TomoBasis.bspline(T, 9, 7)
    nf, ng = T.qx * T.qy, 63
    dx = torch.zeros(nf, dtype=torch.float64, device="cuda")
    dc = torch.zeros(ng, dtype=torch.float64, device="cuda")
    hx, hc = np.zeros(nf), np.zeros(ng)
    torch.cuda.synchronize()
    for fn, args, name in ((L.rtmi_tomo_basis_prolong_dev, (hc.ctypes.data, dx.data_ptr()), b"d_c"),
                           (L.rtmi_tomo_basis_prolong_dev, (dc.data_ptr(), hx.ctypes.data), b"d_x"),
                           (L.rtmi_tomo_basis_restrict_dev, (hx.ctypes.data, dc.data_ptr()), b"d_x"),
                           (L.rtmi_tomo_basis_restrict_dev, (dx.data_ptr(), hc.ctypes.data), b"d_g")):
        assert fn(P._h, *args) == -1
        assert name in L.rtmi_last_error() and b"handle's device" in L.rtmi_last_error()
    # an allocation of the runtime's own, whose end the test knows
    hip = C.CDLL(_lib.mapped_hip_runtimes()[0])
    for f in (hip.hipMalloc, hip.hipFree, hip.hipMemGetAddressRange):
        f.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(p), 2 * nf * 8) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), p) == 0 and size.value >= 2 * nf * 8
        end = base.value + size.value
        assert L.rtmi_tomo_basis_prolong_dev(P._h, end - 8 * ng + 8, dx.data_ptr()) == -1
        assert b"d_c is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_basis_prolong_dev(P._h, dc.data_ptr(), end - 8 * nf + 8) == -1
        assert b"d_x is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_basis_restrict_dev(P._h, end - 8 * nf + 8, dc.data_ptr()) == -1
        assert b"d_x is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_basis_restrict_dev(P._h, dx.data_ptr(), end - 8 * ng + 8) == -1
        assert b"d_g is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_basis_restrict_dev(P._h, dx.data_ptr(), end - 8 * ng) == 0, L.rtmi_last_error()   # one that just fits
    finally:
        assert hip.hipFree(p) == 0
    P.close()


def test_refusals(rb, coarse):
    from raytracing_amd import _lib
    F, T, _ = coarse
    L = _lib.lib()
    ip = lambda a: a.ctypes.data_as(_lib._ip)                                # noqa: E731
    fx, wx = BR.bspline_axis(T.qx, 9, 1)
    fy, wy = BR.bspline_axis(T.qy, 7, 1)
    h = C.c_void_p()

    def create(fx=fx, wx=wx, mx=9, bx=2):
        return L.rtmi_tomo_basis_create(T._h, mx, bx, ip(np.ascontiguousarray(fx, dtype=np.int32)), _lib.dptr(np.ascontiguousarray(wx)), 7, 2,
                                        ip(fy), _lib.dptr(wy), C.byref(h))

    def refused(code, *texts):
        assert code == -1
        for t in texts:
            assert t.encode() in L.rtmi_last_error(), L.rtmi_last_error()
    refused(create(bx=5, wx=np.ones((T.qx, 5))), "axis x", "the bandwidth must be in 1 .. 4")
    k = T.qx // 2
    down = fx.copy(); down[k] = down[k - 1] - 1                             # first[k - 1] is 3 or 4 in the middle of the axis
    refused(create(fx=down), f"axis x, index {k}", "first decreases")
    refused(create(mx=8), "axis x", f"index {int(np.argmax(fx > 6))}", "first is outside 0 .. m - B")
    nanw = wx.copy(); nanw[3, 1] = np.nan
    refused(create(wx=nanw), "axis x, index 3", "a weight is not finite")
    rev = fy[::-1].copy()
    refused(L.rtmi_tomo_basis_create(T._h, 9, 2, ip(fx), _lib.dptr(wx), 7, 2, ip(rev), _lib.dptr(wy), C.byref(h)),
            f"axis y, index {int(np.argmax(np.diff(rev) < 0)) + 1}", "first decreases")
    refused(L.rtmi_tomo_basis_create(T._h, 0, 2, ip(fx), _lib.dptr(wx), 7, 2, ip(fy), _lib.dptr(wy), C.byref(h)), "mx and my must be >= 1")
    with pytest.raises(ValueError, match="qx and qy"):
        rb.TomoBasis(T, fx[:-1], wx[:-1], fy, wy, 9, 7)
    # a basis made on a handle of another shape
    x, y = np.linspace(-2.0, 5.0, T.qx + 1), np.linspace(-2.5, 1.0, T.qy)
    Fo = rb.Field.from_samples(x, y, np.ones((T.qy, T.qx + 1)), rb.DELTA)
    To = rb.Tomography(Fo)
    Fo.close()
    Po = rb.TomoBasis.bspline(To, 9, 7)
    To.close()                                                               # the basis keeps no reference to its handle
    rhs = np.ones(T.info()["rows"])
    with pytest.raises(_lib.RtmiError, match="another shape or device"):
        T.lsqr(rhs, basis=Po, iter_lim=2)
    Po.close()
    P = rb.TomoBasis.bspline(T, 9, 7)
    for s2 in ((-1.0, 0.0), (0.0, np.nan)):
        with pytest.raises(_lib.RtmiError, match="reg.d2 must be finite and >= 0"):
            T.lsqr(rhs, basis=P, smooth2=s2, iter_lim=2)
    with pytest.raises(_lib.RtmiError, match="reg.d1 must be finite and >= 0"):
        T.lsqr(rhs, basis=P, smooth=(-1.0, 0.0), iter_lim=2)
    with pytest.raises(ValueError, match="col_scale must have 63 values"):
        T.lsqr(rhs, basis=P, col_scale=np.ones((T.qy, T.qx)), iter_lim=2)
    bad = np.ones((7, 9)); bad[2, 2] = np.inf
    with pytest.raises(_lib.RtmiError, match="col_scale has a value that is not finite"):
        T.lsqr(rhs, basis=P, col_scale=bad, iter_lim=2)
    badx = np.zeros((T.qy, T.qx)); badx[-1, -1] = np.nan                     # x0 is a fine model: checked over all qy qx values
    with pytest.raises(_lib.RtmiError, match="x0 has a value that is not finite"):
        T.lsqr(rhs, basis=P, x0=badx, iter_lim=2)
    with pytest.raises(_lib.RtmiError, match="rhs has a value that is not finite"):
        T.lsqr(rhs * np.inf, basis=P, iter_lim=2)
    lp = _lib.LsqrParams()
    lp.iter_lim = 0
    g = np.zeros((T.qy, T.qx))
    refused(L.rtmi_tomo_lsqr_basis(T._h, P._h, C.byref(lp), None, None, _lib.dptr(rhs), None, _lib.dptr(g), None, None), "iter_lim")
    lp.iter_lim = 2
    refused(L.rtmi_tomo_lsqr_basis(T._h, P._h, None, None, None, _lib.dptr(rhs), None, _lib.dptr(g), None, None), "null params")
    refused(L.rtmi_tomo_lsqr_basis(T._h, P._h, C.byref(lp), None, None, None, None, _lib.dptr(g), None, None), "null rhs")
    refused(L.rtmi_tomo_lsqr_basis(T._h, P._h, C.byref(lp), None, None, _lib.dptr(rhs), None, None, None, None), "null x")
    E = rb.Tomography(F)
    Pe = rb.TomoBasis.bspline(E, 9, 7)
    refused(L.rtmi_tomo_lsqr_basis(E._h, Pe._h, C.byref(lp), None, None, _lib.dptr(rhs), None, _lib.dptr(g), None, None), "no rows")
    Pe.close(); E.close()
    bad = np.ones((7, 9)); bad[0, 0] = np.nan
    refused(L.rtmi_tomo_basis_prolong(P._h, _lib.dptr(bad), _lib.dptr(g)), "c has a value that is not finite")
    g[1, 1] = np.inf
    refused(L.rtmi_tomo_basis_restrict(P._h, _lib.dptr(g), _lib.dptr(bad)), "x has a value that is not finite")
    assert T.lsqr(rhs, basis=P, iter_lim=2)["itn"] == 2                      # the handles still work
    P.close()


# ---------------------------------------------------------------- 4. crosswell tomography on a coarse cubic grid
def bump(x, y, cx, cy, w):
    X_, Y_ = np.meshgrid(x, y)
    return np.exp(-((X_ - cx) ** 2 + (Y_ - cy) ** 2) / (2 * w * w))


SRC = np.stack([np.full(8, -1.5), np.linspace(-2.2, 0.6, 8)], axis=1)


def crosswell(rb, F, **kw):
    ru = np.linspace(-2.3, 0.8, 32)
    return rb.two_point(rb.op6, F, SRC, (1.0, 0.0, 4.0), ru, thetas=np.linspace(-1.5, 3.0, 512), step=rb.DELTA_S,
                        max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=VERT_BOX, **kw)


def test_crosswell_step_on_a_coarse_cubic_grid(rb):
    """tests/test_gpu_tomo.py's crosswell set-up.  A cubic basis of one coefficient per 8 samples per axis, second differences
    on, damp 0, 30 iterations: r1norm never rises, and the re-traced misfit is below the starting one -- an update that does not
    reduce it is wrong, whatever its size.  The ratio is printed beside that of the fine-grid solve of the existing test (damp
    1e-3, no smoothing); DESIGN.md section 27 has both."""
    F = rb.Field.build("vert_heterogeneous", VERT_BOX, rb.DELTA)
    x, y, Z0 = F.arrays()[:3]
    F.close()
    Ft = rb.Field.from_samples(x, y, Z0 * (1 + 0.01 * bump(x, y, 1.0, -1.0, 0.7)), rb.DELTA)
    obs = crosswell(rb, Ft)
    Ft.close()
    F0 = rb.Field.from_samples(x, y, Z0, rb.DELTA)
    r0 = crosswell(rb, F0, sensitivity=True)
    sens = r0["sensitivity"]
    s_, j, a = sens.index.T
    use = (r0["count"][s_, j] == 1) & (obs["count"][s_, j] == 1) & (a == 0)
    rows = np.nonzero(use)[0]
    assert len(rows) >= 128
    res0 = obs["T"][s_[rows], j[rows], 0] - r0["T"][s_[rows], j[rows], 0]
    T = rb.Tomography(F0)
    T.append_sensitivity(sens, rows=rows)
    sens.close()
    F0.close()
    mx, my = T.qx // 8, T.qy // 8
    P = rb.TomoBasis.bspline(T, mx, my)
    out = T.lsqr(res0, damp=0.0, smooth2=(1e-3, 1e-3), basis=P, iter_lim=30, history=True, stats=True)
    fine = T.lsqr(res0, damp=1e-3, iter_lim=30, stats=True)
    P.close()
    T.close()
    r1 = out["history"][:, 2]
    assert out["itn"] == 30 and (np.diff(r1) <= 0.0).all()
    m0 = np.sqrt(np.mean(res0 ** 2))
    ratio = {}
    for name, dz in (("basis", out["x"]), ("fine", fine["x"])):
        F1 = rb.Field.from_samples(x, y, Z0 + dz, rb.DELTA)
        r = crosswell(rb, F1)
        F1.close()
        ok = r["count"][s_[rows], j[rows]] >= 1
        res1 = obs["T"][s_[rows], j[rows], 0][ok] - r["T"][s_[rows], j[rows], 0][ok]
        ratio[name] = (float(np.sqrt(np.mean(res1 ** 2)) / m0), int(ok.sum()))
    print(f"crosswell on {my} x {mx} cubic coefficients for {T.qy} x {T.qx} samples, {len(rows)} arrivals: RMS misfit ratio "
          f"{ratio['basis'][0]:.3f} ({ratio['basis'][1]} re-traced; r1norm {r1[0]:.3e} -> {r1[-1]:.3e}; operator "
          f"{out['stats']['operator_ms'] / 30:.3f} ms, vectors {out['stats']['vector_ms'] / 30:.3f} ms per iteration), fine grid "
          f"{ratio['fine'][0]:.3f} ({ratio['fine'][1]} re-traced; operator {fine['stats']['operator_ms'] / 30:.3f} ms, vectors "
          f"{fine['stats']['vector_ms'] / 30:.3f} ms per iteration)")
    assert ratio["basis"][1] >= 0.9 * len(rows)
    assert ratio["basis"][0] < 1.0
