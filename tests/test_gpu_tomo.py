"""GPU: recorded rays compiled into a ray-tomography matrix on the device (rtmi_tomo_*).  The compiled
segments against the restatement (tests/tomo_ref.py) on the device's own rows; the products bit for bit on the read-back segments
at the shapes where the sliced layout can go wrong; the products against rtmi_traveltime_perturb / _backproject; the transposed
product's bits under every order; the solver against the restatement bit for bit; the device-pointer calls; crosswell tomography
through the handle, from one batch and from eight that are destroyed one by one; every refusal."""
import ctypes as C

import numpy as np
import pytest

import kirchhoff_lsqr_ref as K
import sensitivity_ref as S
import tomo_ref as TR
from conftest import LIMITS

pytestmark = pytest.mark.gpu

VERT_BOX = LIMITS["vert_heterogeneous"]


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    cache = {}

    def get(scen, dtype=None, delta=None):
        key = (scen, dtype, delta)
        if key not in cache:
            kw = {} if dtype is None else {"dtype": dtype}
            cache[key] = rb.Field.build(scen, LIMITS[scen], rb.DELTA if delta is None else delta, **kw)
        return cache[key]
    yield get
    for F in cache.values():
        F.close()


# scenario -> (step, launch point, fan, line): tests/test_gpu_sensitivity.py's
SCEN = {
    "interface": (None, (-2.0, -2.0), (2 * np.pi / 60, np.pi / 2), (0.0, 1.0, 1.0)),
    "fisheye": (2 * np.pi / 303, (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4), (0.0, 1.0, 0.3)),
    "vert_heterogeneous": (None, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
    "anisotropy": (None, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
}


def batch(rb, F, scen, m, R, rec_rows=None, per_ray=None, **kw):
    step, (x0, y0), fan, _ = SCEN[scen]
    step = rb.DELTA_S if step is None else step
    ms = rb.N * 304 if scen == "fisheye" else int(np.ceil(80 / step) + 1)
    th = kw.pop("thetas", np.linspace(*fan, R) if R > 1 else np.array([0.5 * (fan[0] + fan[1])]))
    gamma = 3.0 if scen == "anisotropy" else 1.0
    if rec_rows is None:
        c = rb.Batch(F, rb.METHODS[m], step, ms, LIMITS[scen], gamma, th, x0, y0, record_stride=0)
        if per_ray is not None:
            c.set_per_ray(step, per_ray)
        c.run()
        rec_rows = int(c.d_ray()[2].max()) + 1
        c.close()
    b = rb.Batch(F, rb.METHODS[m], step, ms, LIMITS[scen], gamma, th, x0, y0, rec_rows=rec_rows, **kw)
    if per_ray is not None:
        b.set_per_ray(step, per_ray)
    b.run()
    return b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def restated(rb, F, b, scen, m, which=None, line=None, kmax=4):
    x, y = F.arrays()[:2]
    ax, ay = S.axes(x, y)
    if F.dtype == rb.F32:                  # an fp32 field's axes are its own fp32 origin, end and 1 / h, widened
        ax, ay = (tuple(float(np.float32(v)) for v in a[:3]) + (a[3],) for a in (ax, ay))
    last = b.d_ray()[2].astype(np.int64)
    gamma = 3.0 if scen == "anisotropy" else 1.0
    return TR.segments(b.rows(), last, ax, ay, which=which, line=line, kmax=kmax, method=m, gamma=gamma, rec_rows=b.rec_rows)


def value_error(rp, val, val_ref):
    """the largest |difference| of a segment value over its row's largest value"""
    if len(val) == 0:
        return 0.0
    n = np.diff(rp)
    r = np.repeat(np.arange(len(n)), n)
    big = np.zeros(len(n))
    np.maximum.at(big, r, np.max(np.abs(val_ref), axis=1))
    return float(np.max(np.max(np.abs(val - val_ref), axis=1) / big[r]))


def check_products(T, seed):
    """matvec and rmatvec of the handle against the restatement on the segments read back, bit for bit"""
    rp, base, val = T.read()
    i = T.info()
    assert len(rp) == i["rows"] + 1 and rp[-1] == i["segments"] == len(base) and i["padded_segments"] >= i["segments"]
    assert i["vmax"] == (float(np.max(np.abs(val))) if len(val) else 0.0)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T.qy, T.qx))
    w = rng.standard_normal(i["rows"])
    y = T.matvec(x)
    g, st = T.rmatvec(w, stats=True)
    assert bits(y) == bits(TR.apply(rp, base, val, T.qx, x))
    assert bits(g) == bits(TR.transpose(rp, base, val, T.qx, T.qy, w, vmax=i["vmax"]))
    assert not np.signbit(y[np.diff(rp) == 0]).any()
    return rp, base, val, st


# ---------------------------------------------------------------- 1. compile against the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("scen,m", [("vert_heterogeneous", 6), ("interface", 2), ("fisheye", 9), ("anisotropy", 11)])
def test_compiled_segments_match_the_restatement(rb, fields, scen, m, dtype):
    """Values within 1e-12 of the row's largest, the bound of this summation order; counts and columns equal."""
    F = fields(scen, rb.F32 if dtype == "f32" else None)
    R = 300
    b = batch(rb, F, scen, m, R)
    line = SCEN[scen][3]
    cnt = b.crossings(line, kmax=4)["count"]
    worst = 0.0
    for wh in (None, 0, 1):
        which = None if wh is None else np.full(R, wh, dtype=np.int32)
        T = rb.Tomography(F)
        first, nseg = T.append(b, which=which, line=None if wh is None else line, kmax=4)
        rp, base, val = T.read()
        T.close()
        nseg_r, rp_r, base_r, val_r = restated(rb, F, b, scen, m, which=which, line=line, kmax=4)
        assert first == 0 and np.array_equal(nseg, nseg_r) and np.array_equal(rp, rp_r) and np.array_equal(base, base_r)
        if wh is not None:
            assert np.array_equal(nseg > 0, cnt > wh)
        e = value_error(rp, val, val_r)
        print(f"{scen} op{m} {dtype} which {wh}: {rp[-1]} segments in {len(rp) - 1} rows, values {e:.2e} of the row's largest"
              f"{', bit-equal' if bits(val) == bits(val_r) else ''}")
        worst = max(worst, e)
    b.close()
    if scen == "fisheye":
        assert (cnt >= 2).sum() >= R // 2                                   # fisheye rays cross their line twice
    assert worst <= 1e-12


# ---------------------------------------------------------------- 2. shapes where the layout can go wrong
@pytest.mark.parametrize("R", [1, 63, 65, 130])
def test_products_bit_for_bit_at_slice_edges(rb, fields, R):
    F = fields("vert_heterogeneous")
    b = batch(rb, F, "vert_heterogeneous", 6, R)
    T = rb.Tomography(F)
    T.append(b)
    b.close()
    check_products(T, R)
    assert T.info()["rows"] == R
    T.close()


def test_rows_of_one_segment_next_to_rows_of_hundreds(rb, fields):
    F = fields("vert_heterogeneous")
    R = 70
    ms = np.full(R, 1100, dtype=np.int32)                # every ray of this fan would take more than 1130 steps
    ms[0], ms[1], ms[2], ms[40] = 2, 3, 40, 2
    ms[10], ms[50] = 1200, 1200                          # past the 1150 rows of the record
    b = batch(rb, F, "vert_heterogeneous", 6, R, rec_rows=1150, per_ray=ms)
    last = b.d_ray()[2].astype(np.int64)
    assert last[0] == 1 and (last >= 1150).sum() == 2 and (last == 1099).sum() >= 60
    T = rb.Tomography(F)
    _, nseg = T.append(b)
    nseg_r = restated(rb, F, b, "vert_heterogeneous", 6)[0]
    b.close()
    assert np.array_equal(nseg, nseg_r)
    assert nseg[0] == 1 and nseg.max() >= 200 and np.array_equal(nseg == 0, last >= 1150)
    i = T.info()
    print(f"per-ray max_size: rows of {nseg.min()} .. {nseg.max()} segments, {i['segments']} segments in {i['padded_segments']} slots")
    check_products(T, 2)
    T.close()


def test_which_mixes_end_crossing_and_skip(rb, fields):
    F = fields("fisheye")
    R = 130
    b = batch(rb, F, "fisheye", 9, R)
    line = SCEN["fisheye"][3]
    which = np.tile(np.array([-1, 0, rb._lib.TOMO_SKIP, 1, 3], dtype=np.int32), R // 5)
    T = rb.Tomography(F)
    first, nseg = T.append(b, which=which, line=line, kmax=4)
    cnt = b.crossings(line, kmax=4)["count"]
    nseg_r, rp_r, base_r, _ = restated(rb, F, b, "fisheye", 9, which=which, line=line, kmax=4)
    b.close()
    assert first == 0 and np.array_equal(nseg, nseg_r)
    assert (nseg[which == rb._lib.TOMO_SKIP] == -1).all() and (nseg[(which == 3) & (cnt < 4)] == 0).all() and (which == 3).sum() > 0
    rp, base, _, _ = check_products(T, 3)
    assert np.array_equal(rp, rp_r) and np.array_equal(base, base_r)
    assert T.info()["rows"] == int((which != rb._lib.TOMO_SKIP).sum())
    T.close()


def test_rays_that_leave_the_sample_grid(rb):
    """The samples cover a part of the box: past them the cells are clamped to the rim."""
    lim = (-2.0, 1.0, -2.5, 0.0)
    F = rb.Field.build("vert_heterogeneous", lim, rb.DELTA)
    b = batch(rb, F, "vert_heterogeneous", 6, 65)
    s, last = b.rows(), b.d_ray()[2].astype(np.int64)
    xe = s[last, 0, np.arange(65)]
    assert (xe > lim[1]).sum() >= 8
    T = rb.Tomography(F)
    _, nseg = T.append(b)
    nseg_r, rp_r, base_r, val_r = restated(rb, F, b, "vert_heterogeneous", 6)
    b.close()
    rp, base, val, _ = check_products(T, 4)
    assert np.array_equal(nseg, nseg_r) and np.array_equal(base, base_r) and value_error(rp, val, val_r) <= 1e-12
    T.close()
    F.close()


def test_three_appends_of_different_sizes(rb, fields):
    F = fields("vert_heterogeneous")
    T = rb.Tomography(F)
    line = SCEN["vert_heterogeneous"][3]
    firsts, parts = [], []
    for R, wh in ((70, None), (1, None), (130, 0)):
        b = batch(rb, F, "vert_heterogeneous", 6, R)
        which = None if wh is None else np.full(R, wh, dtype=np.int32)
        firsts.append(T.append(b, which=which, line=None if wh is None else line)[0])
        One = rb.Tomography(F)
        One.append(b, which=which, line=None if wh is None else line)
        parts.append(One.read())
        One.close()
        b.close()
    assert firsts == [0, 70, 71] and T.info()["rows"] == 201
    rp, base, val, _ = check_products(T, 5)
    assert np.array_equal(np.diff(rp), np.concatenate([np.diff(p[0]) for p in parts]))
    assert np.array_equal(base, np.concatenate([p[1] for p in parts])) and bits(val) == bits(np.concatenate([p[2] for p in parts]))
    T.close()


# ---------------------------------------------------------------- 3. against the existing kernels
@pytest.mark.parametrize("scen,m", [("vert_heterogeneous", 6), ("fisheye", 9), ("anisotropy", 11)])
def test_products_against_perturb_and_backproject(rb, fields, scen, m):
    F = fields(scen)
    R, kmax = 256, 2
    b = batch(rb, F, scen, m, R)
    line = SCEN[scen][3]
    Z = F.arrays()[2]
    rng = np.random.default_rng(m)
    dz = rng.standard_normal(Z.shape)
    we, wl = rng.standard_normal(R), rng.standard_normal((kmax, R))
    d = b.traveltime_perturb(dz, line=line, kmax=kmax)
    g = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=kmax)
    T_end = b.final()[8]
    T_line = b.crossings(line, kmax=kmax)["T"]
    T = rb.Tomography(F)
    T.append(b)
    for c in range(kmax):
        T.append(b, which=np.full(R, c, dtype=np.int32), line=line, kmax=kmax)
    b.close()                                                               # the products run without the record
    want = np.r_[d["end"], d["line"].ravel()]
    have = np.isfinite(want)
    y = T.matvec(dz)
    assert not y[~have].any()                                               # no observation: an empty row
    e_y = float(np.max(np.abs(y[have] - want[have])) / np.max(np.abs(want[have])))
    w = np.r_[we, wl.ravel()]
    gt = T.rmatvec(w)
    e_g = float(np.max(np.abs(gt - g)) / np.max(np.abs(g)))
    lhs, rhs = float(np.dot(y, w)), float(np.dot(dz.ravel(), gt.ravel()))
    scale = float(np.sum(np.abs(y * w)))
    tz = T.matvec(Z)
    rec = np.r_[T_end, T_line.ravel()]
    e_T = float(np.max(np.abs(tz[have] - rec[have])) / np.max(np.abs(rec[have])))
    T.close()
    print(f"{scen} op{m}: matvec - perturb {e_y:.2e}, rmatvec - backproject {e_g:.2e}, adjointness {abs(lhs - rhs) / scale:.2e}, "
          f"A Z - T {e_T:.2e}")
    assert e_y <= 1e-12 and e_g <= 1e-12 and e_T <= 1e-12
    assert abs(lhs - rhs) <= 1e-12 * scale


# ---------------------------------------------------------------- 4. the transposed product's bits
def test_transposed_bits_do_not_depend_on_any_order(rb, fields):
    F = fields("vert_heterogeneous")
    R = 200
    line = SCEN["vert_heterogeneous"][3]
    th = np.linspace(*SCEN["vert_heterogeneous"][2], R)
    rng = np.random.default_rng(21)
    w_end, w_line = rng.standard_normal(R), rng.standard_normal(R)
    zero = np.zeros(R, dtype=np.int32)

    def run(order=("end", "line"), perm=None, **kw):
        p = np.arange(R) if perm is None else perm
        b = batch(rb, F, "vert_heterogeneous", 6, R, thetas=th[p], **kw)
        T = rb.Tomography(F)
        w = []
        for what in order:
            if what == "end":
                T.append(b)
                w.append(w_end[p])
            else:
                T.append(b, which=zero, line=line)
                w.append(w_line[p])
        b.close()
        g1 = T.rmatvec(np.concatenate(w))
        g2 = T.rmatvec(np.concatenate(w))
        T.close()
        assert bits(g1) == bits(g2)
        return g1
    ref = run()
    assert ref.any()
    assert bits(run(perm=rng.permutation(R))) == bits(ref)
    assert bits(run(order=("line", "end"))) == bits(ref)
    for mode, sort in (("plain", True), ("sliced", False), ("refill", True)):
        assert bits(run(launch_mode=mode, sort_rays=sort)) == bits(ref), (mode, sort)


# ---------------------------------------------------------------- 5. the solver against the restatement
@pytest.fixture(scope="module")
def coarse(rb):
    """a field of a few thousand samples, so that the restated norms (Python integers) take no time, and rays compiled on it"""
    F = rb.Field.build("vert_heterogeneous", VERT_BOX, 4 * rb.DELTA)
    b = batch(rb, F, "vert_heterogeneous", 6, 65)
    T = rb.Tomography(F)
    T.append(b)
    E = rb.Tomography(F)
    E.append(b, which=np.full(65, 3, dtype=np.int32), line=SCEN["vert_heterogeneous"][3], kmax=4)    # no ray crosses four times
    b.close()
    yield F, T, E
    T.close()
    E.close()
    F.close()


@pytest.mark.parametrize("damp", [0.0, 1e-3])
@pytest.mark.parametrize("smooth", [None, (0.5, 0.25)])
def test_solver_equals_the_restatement_bit_for_bit(rb, coarse, damp, smooth):
    F, T, _ = coarse
    rp, base, val = T.read()
    rhs = np.random.default_rng(31).standard_normal(T.info()["rows"])
    out = T.lsqr(rhs, damp=damp, smooth=smooth, iter_lim=6, history=True, stats=True)
    ref = TR.lsqr(rp, base, val, T.qx, T.qy, rhs, 6, damp=damp, smooth=smooth, vmax=T.info()["vmax"])
    print(f"damp {damp} smooth {smooth}: itn {out['itn']}, istop {out['istop']}, r1norm {out['r1norm']!r}; operator "
          f"{out['stats']['operator_ms']:.3f} ms, vectors {out['stats']['vector_ms']:.3f} ms")
    assert (out["itn"], out["istop"]) == (ref["itn"], ref["istop"]) == (6, 7)
    for k in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(out[k]) == bits(ref[k]), k
    assert bits(out["history"]) == bits(ref["history"])
    assert bits(out["x"]) == bits(ref["x"])


def test_solver_early_returns_and_range(rb, coarse):
    F, T, E = coarse
    n = T.info()["rows"]
    out = T.lsqr(np.zeros(n), iter_lim=4)
    assert (out["istop"], out["itn"]) == (0, 0) and not out["x"].any()
    assert E.info()["rows"] == n and E.info()["segments"] == 0
    out = E.lsqr(np.ones(n), iter_lim=4, smooth=None)
    assert (out["istop"], out["itn"]) == (0, 0) and not out["x"].any()
    rhs = np.random.default_rng(33).standard_normal(n)
    out = T.lsqr(rhs * 1e-170, iter_lim=4)                                   # max|rhs|^2 is below the normal range
    assert (out["istop"], out["itn"]) == (rb._lib.LSQR_RANGE, 0) and not out["x"].any()
    rp, base, val = T.read()
    ref = TR.lsqr(rp, base, val, T.qx, T.qy, rhs * 1e-170, 4, vmax=T.info()["vmax"])
    assert ref["istop"] == K.LSQR_RANGE and ref["itn"] == 0


# ---------------------------------------------------------------- 6. device-pointer calls
@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def test_device_pointer_calls_give_the_host_calls_bits(rb, coarse, torch):
    F, T, _ = coarse
    rng = np.random.default_rng(41)
    x, w = rng.standard_normal((T.qy, T.qx)), rng.standard_normal(T.info()["rows"])
    y = T.matvec_device(torch.tensor(x, device="cuda"))
    g, st = T.rmatvec_device(torch.tensor(w, device="cuda"), stats=True)
    gh, sth = T.rmatvec(w, stats=True)
    assert bits(y.cpu().numpy()) == bits(T.matvec(x)) and bits(g.cpu().numpy()) == bits(gh)
    assert (st["atomics"], st["scale_exp"]) == (sth["atomics"], sth["scale_exp"]) and st["atomics"] > 0
    with pytest.raises(ValueError, match="on a GPU"):
        T.matvec_device(torch.tensor(x))


def test_device_pointer_calls_refuse_host_memory_and_short_buffers(rb, coarse, torch):
    from raytracing_amd import _lib
    F, T, _ = coarse
    L = _lib.lib()
    nz, rows = T.qx * T.qy, T.info()["rows"]
    dx = torch.zeros(nz, dtype=torch.float64, device="cuda")
    dy = torch.zeros(rows, dtype=torch.float64, device="cuda")
    hx, hy = np.zeros(nz), np.zeros(rows)
    torch.cuda.synchronize()
    for fn, args, name in ((L.rtmi_tomo_apply_dev, (hx.ctypes.data, dy.data_ptr()), b"d_x"),
                           (L.rtmi_tomo_apply_dev, (dx.data_ptr(), hy.ctypes.data), b"d_y"),
                           (L.rtmi_tomo_transpose_dev, (hy.ctypes.data, dx.data_ptr()), b"d_w"),
                           (L.rtmi_tomo_transpose_dev, (dy.data_ptr(), hx.ctypes.data), b"d_g")):
        assert fn(T._h, *args, None) == -1
        assert name in L.rtmi_last_error() and b"handle's device" in L.rtmi_last_error()
    # an allocation of the runtime's own, whose end the test knows
    hip = C.CDLL(_lib.mapped_hip_runtimes()[0])
    for f in (hip.hipMalloc, hip.hipFree, hip.hipMemGetAddressRange):
        f.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    need = nz * 8
    p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(p), 2 * need) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), p) == 0 and size.value >= 2 * need
        end = base.value + size.value
        assert L.rtmi_tomo_transpose_dev(T._h, dy.data_ptr(), end - 64, None) == -1
        assert b"d_g is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_apply_dev(T._h, end - need + 8, dy.data_ptr(), None) == -1
        assert b"d_x is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_apply_dev(T._h, dx.data_ptr(), end - 8 * rows + 8, None) == -1
        assert b"d_y is shorter" in L.rtmi_last_error()
        assert L.rtmi_tomo_transpose_dev(T._h, dy.data_ptr(), end - need, None) == 0, L.rtmi_last_error()   # one that just fits
    finally:
        assert hip.hipFree(p) == 0


# ---------------------------------------------------------------- 7. and 8. crosswell tomography through the handle
def bump(x, y, cx, cy, w):
    X_, Y_ = np.meshgrid(x, y)
    return np.exp(-((X_ - cx) ** 2 + (Y_ - cy) ** 2) / (2 * w * w))


SRC = np.stack([np.full(8, -1.5), np.linspace(-2.2, 0.6, 8)], axis=1)


def crosswell(rb, F, src=SRC, **kw):
    ru = np.linspace(-2.3, 0.8, 32)
    return rb.two_point(rb.op6, F, src, (1.0, 0.0, 4.0), ru, thetas=np.linspace(-1.5, 3.0, 512), step=rb.DELTA_S,
                        max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=VERT_BOX, **kw)


def test_crosswell_step_with_the_record_gone_and_source_by_source(rb, fields):
    from scipy.sparse.linalg import LinearOperator, lsqr
    F = fields("vert_heterogeneous")
    x, y, Z0 = F.arrays()[:3]
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

    def rmv(r):
        w = np.zeros(sens.shape[0])
        w[rows] = r
        return sens.rmatvec(w)
    op = LinearOperator((len(rows), sens.shape[1]), matvec=lambda v: sens.matvec(v)[rows], rmatvec=rmv, dtype=np.float64)
    # scipy with the handle's stop rules (atol = btol = 0, no conlim): both solvers take all 30 iterations
    sc = lsqr(op, res0, damp=1e-3, atol=0.0, btol=0.0, conlim=0.0, iter_lim=30)
    dz_ref = sc[0].reshape(Z0.shape)
    fit_ref = float(np.linalg.norm(sens.matvec(dz_ref)[rows] - res0))
    T = rb.Tomography(F0)
    first, nseg = T.append_sensitivity(sens, rows=rows)
    sens.close()                                                            # the record is gone: the matrix stays
    assert first == 0 and T.info()["rows"] == len(rows) and (nseg[rows] > 0).all()
    out = T.lsqr(res0, damp=1e-3, iter_lim=30, stats=True)
    dz = out["x"]
    fit = float(np.linalg.norm(T.matvec(dz) - res0))
    i = T.info()
    print(f"crosswell: {len(rows)} arrivals, {i['segments']} segments ({i['padded_segments']} slots, {i['bytes_device']} B); "
          f"|A dz - res0| {fit:.6e} here (itn {out['itn']}, istop {out['istop']}), {fit_ref:.6e} scipy over the row-walking operator "
          f"(itn {sc[2]}, istop {sc[1]}); |res0| {np.linalg.norm(res0):.3e}; solver {out['stats']['total_ms']:.1f} ms")
    assert abs(fit - fit_ref) <= 1e-6 * fit_ref
    # 8. the same matrix from eight batches, one per source, each destroyed after its append
    one = T.read()
    J = rb.Tomography(F0)
    for s in range(len(SRC)):
        rs = crosswell(rb, F0, src=SRC[s:s + 1], sensitivity=True)
        ss = rs["sensitivity"]
        mine = rows[s_[rows] == s]
        # this source's arrivals in the one-batch order: (j, a) of sens.index restricted to s
        sj, sa = ss.index[:, 1], ss.index[:, 2]
        pick = [int(np.nonzero((sj == j[r]) & (sa == a[r]))[0][0]) for r in mine]
        assert pick == sorted(pick)
        J.append_sensitivity(ss, rows=np.array(pick, dtype=np.int64))
        ss.close()
    many = J.read()
    J.close()
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]) and bits(one[2]) == bits(many[2])
    T.close()
    F0.close()
    F1 = rb.Field.from_samples(x, y, Z0 + dz, rb.DELTA)
    r1 = crosswell(rb, F1)
    F1.close()
    ok = r1["count"][s_[rows], j[rows]] >= 1
    res1 = obs["T"][s_[rows], j[rows], 0][ok] - r1["T"][s_[rows], j[rows], 0][ok]
    m0, m1 = np.sqrt(np.mean(res0 ** 2)), np.sqrt(np.mean(res1 ** 2))
    print(f"crosswell: RMS misfit {m0:.3e} -> {m1:.3e} ({m1 / m0:.3f}), {ok.sum()} re-traced")
    assert ok.sum() >= 0.9 * len(rows)
    assert m1 <= 0.2 * m0


# ---------------------------------------------------------------- refusals
def test_refusals(rb, fields, coarse):
    from raytracing_amd import _lib
    L = _lib.lib()
    F = fields("vert_heterogeneous")
    Fc, T, _ = coarse
    R = 8
    b = batch(rb, F, "vert_heterogeneous", 6, R)
    H = rb.Tomography(F)
    line = np.array(SCEN["vert_heterogeneous"][3])
    ip = lambda a: a.ctypes.data_as(_lib._ip)                                # noqa: E731

    def refused(code, text, expect=-1):
        assert code == expect
        assert text.encode() in L.rtmi_last_error(), L.rtmi_last_error()
    wh = np.zeros(R, dtype=np.int32)
    refused(L.rtmi_tomo_append(H._h, None, None, 0, None, None, None), "null batch")
    refused(L.rtmi_tomo_append(T._h, b._h, None, 0, None, None, None), "other sample axes")
    refused(L.rtmi_tomo_append(H._h, b._h, None, 0, ip(wh), None, None), "needs a line")
    refused(L.rtmi_tomo_append(H._h, b._h, _lib.dptr(line), 2, ip(np.full(R, 2, dtype=np.int32)), None, None), "above kmax - 1")
    refused(L.rtmi_tomo_append(H._h, b._h, _lib.dptr(line), 2, ip(np.full(R, -3, dtype=np.int32)), None, None), "below RTMI_TOMO_SKIP")
    refused(L.rtmi_tomo_append(H._h, b._h, _lib.dptr(line), 65, ip(wh), None, None), "kmax must be in 1..64")
    refused(L.rtmi_tomo_append(H._h, b._h, _lib.dptr(np.zeros(3)), 2, ip(wh), None, None), "the line needs")
    c = rb.Batch(F, rb.op6, rb.DELTA_S, 100, VERT_BOX, 1, np.linspace(0.1, 1.0, R), -2.0, -2.0, record_stride=4)
    c.run()
    refused(L.rtmi_tomo_append(H._h, c._h, None, 0, None, None, None), "record_stride 1")
    b2 = batch(rb, F, "vert_heterogeneous", 6, R)
    b2.restore_state(*b2.get_state())                                       # a state at a row other than 0
    refused(L.rtmi_tomo_append(H._h, b2._h, None, 0, None, None, None), "rtmi_batch_set_state", expect=-4)
    b2.close()
    c.close()
    assert H.info()["rows"] == 0
    nz = H.qx * H.qy
    x, g = np.zeros(nz), np.zeros(nz)
    lp = _lib.LsqrParams()
    lp.iter_lim = 2
    ls = _lib.LsqrStats()
    refused(L.rtmi_tomo_lsqr(H._h, C.byref(lp), None, _lib.dptr(x), _lib.dptr(g), None, C.byref(ls)), "no rows")
    H.append(b)
    b.close()
    rhs = np.ones(R)
    bad = x.copy(); bad[3] = np.inf
    refused(L.rtmi_tomo_apply(H._h, _lib.dptr(bad), _lib.dptr(rhs), None), "x has a value that is not finite")
    badw = rhs.copy(); badw[2] = np.nan
    refused(L.rtmi_tomo_transpose(H._h, _lib.dptr(badw), _lib.dptr(g), None), "w has a value that is not finite")
    refused(L.rtmi_tomo_transpose(H._h, _lib.dptr(rhs * 1e-320), _lib.dptr(g), None), "not a normal number")
    refused(L.rtmi_tomo_apply(H._h, None, _lib.dptr(rhs), None), "null x")
    refused(L.rtmi_tomo_apply(H._h, _lib.dptr(x), None, None), "null y")
    refused(L.rtmi_tomo_transpose(H._h, None, _lib.dptr(g), None), "null w")
    refused(L.rtmi_tomo_transpose(H._h, _lib.dptr(rhs), None, None), "null g")
    refused(L.rtmi_tomo_info(H._h, None), "null stats")
    refused(L.rtmi_tomo_read(H._h, None, ip(np.zeros(4, dtype=np.int32)), None), "need row_ptr")
    refused(L.rtmi_tomo_lsqr(H._h, None, None, _lib.dptr(rhs), _lib.dptr(g), None, None), "null params")
    refused(L.rtmi_tomo_lsqr(H._h, C.byref(lp), None, None, _lib.dptr(g), None, None), "null rhs")
    refused(L.rtmi_tomo_lsqr(H._h, C.byref(lp), None, _lib.dptr(rhs), None, None, None), "null x")
    refused(L.rtmi_tomo_lsqr(H._h, C.byref(lp), None, _lib.dptr(badw), _lib.dptr(g), None, None), "rhs has a value that is not finite")
    for sm in ((-1.0, 0.0), (0.0, np.inf)):
        refused(L.rtmi_tomo_lsqr(H._h, C.byref(lp), _lib.dptr(np.array(sm)), _lib.dptr(rhs), _lib.dptr(g), None, None), "smooth must be")
    for field, value, text in (("iter_lim", 0, "iter_lim"), ("damp", -1.0, "damp"), ("atol", np.nan, "atol"), ("btol", -1.0, "btol")):
        q = _lib.LsqrParams()
        q.iter_lim = 2
        setattr(q, field, value)
        refused(L.rtmi_tomo_lsqr(H._h, C.byref(q), None, _lib.dptr(rhs), _lib.dptr(g), None, None), text)
    assert H.lsqr(rhs, iter_lim=2)["itn"] == 2                               # the handle still works
    H.close()
    with pytest.raises(ValueError, match="closed"):
        H.info()
