"""GPU: the Kirchhoff pair on device pointers and least-squares migration that stays on the device (rtmi_kirchhoff_migrate_dev /
_model_dev, rtmi_kirchhoff_lsqr, rtmi_debug_fix_norm; rt_bench.Kirchhoff.migrate_device / model_device / lsqr).  The device-pointer
calls against the host-pointer calls bit for bit on every kind of handle; the norm kernel against the restatement's integers
(tests/kirchhoff_lsqr_ref.py) bit for bit; the solver against the restatement driven with the host-pointer calls, every bit of x,
of the history and of the final scalars; stops and refusals; the standard case against scipy's lsqr over as_linear_operator().
Measured values: DESIGN.md 21."""
import ctypes as C
import math
import struct
import time

import numpy as np
import pytest

import kirchhoff_aa_ref as KA
import kirchhoff_lsqr_ref as R
import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def torch(rb):
    import torch
    assert torch.cuda.is_available()
    return torch


# kind -> (karr of the tables, kwargs of small_case, anti-aliased levels or None, the handle takes 3-D tables)
KINDS = {
    "plain": (1, dict(), None, True),
    "plain_amp_w": (1, dict(amp=True, w=True), None, True),
    "plain_bins": (1, dict(nbin=6), None, True),
    "plain_full": (1, dict(nbin=6, amp=True, w=True, holes=True), None, True),
    "multi2": (2, dict(amp=True, holes=True), None, False),
    "multi2_kmah": (2, dict(amp=True, kmah=True, holes=True), None, False),
    "aa1": (1, dict(amp=True, holes=True), KA.HW8[:3], False),
}


def make(rb, kind, seed=3):
    karr, skw, hw, flat = KINDS[kind]
    pt = aa = None
    if hw is None:
        T, isrc, irec, kw = KM.small_case(karr, seed=seed, **skw)
    else:
        T, pt, aa, isrc, irec, kw = KA.small_case(karr, hw=hw, seed=seed, **skw)
    cut = (lambda a: None if a is None else a[:, 0]) if flat else (lambda a: a)
    return rb.Kirchhoff(cut(T), isrc, irec, KM.SM_NT, KM.SM_DT, amp=cut(kw["amp"]), theta=cut(kw["theta"]), kmah=kw["kmah"],
                        weights=kw["w"], nbin=kw["nbin"], dopen=kw["dopen"], pt=pt, antialias=aa)


def bits(v):
    return struct.pack("<d", float(v))


def host_pair(op, d0, d1, m):
    """the host-pointer calls -> (image, stats), ((ch0, ch1), stats)"""
    if op.karr:
        return op.migrate_channels(d0, d1 if op.has_kmah else None, stats=True), op.model_channels(m, stats=True)
    img, si = op.migrate(d0, stats=True)
    dm, sm = op.model(m, stats=True)
    return (img, si), ((dm, None), sm)


# ---------------------------------------------------------------- the pair on device pointers
@pytest.mark.parametrize("kind", list(KINDS))
def test_device_pointer_calls_equal_the_host_pointer_calls(rb, torch, kind):
    op = make(rb, kind)
    rng = np.random.default_rng(8)
    d0, d1 = rng.standard_normal((op.N, op.nt)), rng.standard_normal((op.N, op.nt))
    m = rng.standard_normal((op.nb, op.ny, op.nx))
    m.reshape(-1)[5], m.reshape(-1)[77] = np.nan, np.inf              # the device's absmax ignores them as the host pass did
    m.reshape(-1)[200] = 37.5                                         # the largest finite value: it sets the quantum
    (img, si), ((c0, c1), sm) = host_pair(op, d0, d1, m)
    dev = torch.device("cuda")
    t0, t1 = torch.from_numpy(d0).to(dev), torch.from_numpy(d1).to(dev)
    buf = torch.empty(m.size + 1, dtype=torch.float64, device=dev)    # a model that is 8- but not 16-byte aligned
    tm = buf[1:]
    tm.copy_(torch.from_numpy(m.reshape(-1)))
    assert tm.data_ptr() % 16 == 8
    timg, sdi = op.migrate_device(t0, t1 if op.has_kmah else None, stats=True)
    out, sdm = op.model_device(tm, stats=True)
    assert timg.is_cuda and timg.dtype == torch.float64
    assert np.array_equal(timg.cpu().numpy().reshape(img.shape), img, equal_nan=True)
    if op.has_kmah:
        assert out[0].is_cuda and out[1].is_cuda
        assert np.array_equal(out[0].cpu().numpy(), c0) and np.array_equal(out[1].cpu().numpy(), c1)
        assert np.any(c1 != 0)
    else:
        assert out.is_cuda and np.array_equal(out.cpu().numpy(), c0)
    assert np.any(c0 != 0) and np.all(np.isfinite(c0))
    for a, b in ((sdi, si), (sdm, sm)):
        assert a["contributing"] == b["contributing"] > 0 and a["scale_exp"] == b["scale_exp"] and a["pairs"] == b["pairs"]
        assert a["upload_ms"] == 0.0
    if kind == "plain":                                               # no amp, no w: the bound is max|m| over the finite values
        assert sdm["scale_exp"] == math.frexp(37.5)[1] - 57
    # an aligned model gives the same bits as the misaligned one
    again = op.model_device(torch.from_numpy(m).to(dev))
    assert np.array_equal((again[0] if op.has_kmah else again).cpu().numpy(), c0)
    op.close()


def test_device_pointer_calls_on_a_trace_of_three_windows(rb, torch):
    rng = np.random.default_rng(3)
    T = 0.5 + 2.4 * rng.random((3, 6, 50))
    isrc = np.array([0, 0, 1, 2], dtype=np.int32); irec = np.array([1, 2, 2, 0], dtype=np.int32)
    nt = 9000
    op = rb.Kirchhoff(T, isrc, irec, nt, 0.001)
    m, d = rng.standard_normal(T.shape[1:]), rng.standard_normal((4, nt))
    dev = torch.device("cuda")
    (img, si), ((dm, _), sm) = host_pair(op, d, None, m)
    timg, sdi = op.migrate_device(torch.from_numpy(d).to(dev), stats=True)
    tdm, sdm = op.model_device(torch.from_numpy(m).to(dev), stats=True)
    assert np.array_equal(timg.cpu().numpy(), img) and np.array_equal(tdm.cpu().numpy(), dm)
    assert (sdi["contributing"], sdm["contributing"], sdm["scale_exp"]) == (si["contributing"], sm["contributing"], sm["scale_exp"])
    op.close()


def test_device_pointer_calls_refuse_host_memory(rb, torch):
    from raytracing_amd import _lib
    op = make(rb, "plain")
    L = _lib.lib()
    dev = torch.device("cuda")
    d = torch.zeros((op.N, op.nt), dtype=torch.float64, device=dev)
    img = torch.zeros((op.ny, op.nx), dtype=torch.float64, device=dev)
    hd, hi = np.zeros((op.N, op.nt)), np.zeros((op.ny, op.nx))
    torch.cuda.synchronize()
    for args, name in (((hd.ctypes.data, None, img.data_ptr()), b"d_data0"), ((d.data_ptr(), None, hi.ctypes.data), b"d_image")):
        assert L.rtmi_kirchhoff_migrate_dev(op._h, *args, None) == -1
        assert name in L.rtmi_last_error() and b"handle's device" in L.rtmi_last_error()
    for args, name in (((hi.ctypes.data, d.data_ptr(), None), b"d_model"), ((img.data_ptr(), hd.ctypes.data, None), b"d_data0")):
        assert L.rtmi_kirchhoff_model_dev(op._h, *args, None) == -1
        assert name in L.rtmi_last_error() and b"handle's device" in L.rtmi_last_error()
    # the handle still works
    assert op.migrate_device(d).shape == (op.ny, op.nx)
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.migrate_device(d)


# ---------------------------------------------------------------- the norm kernel alone
def norm_vectors():
    rng = np.random.default_rng(17)
    out = {f"n{n}": rng.standard_normal(n) for n in (1, 255, 256, 257, 65537)}
    out["span"] = rng.standard_normal(4099) * 2.0 ** rng.integers(-30, 1, 4099)
    out["span"][7] = 1.0
    out["carries"] = np.full(65537, 0.9999)       # every term is near 2^57 quanta: the high word takes carries
    out["zero"] = np.zeros(300)
    return out


@pytest.mark.parametrize("name", list(norm_vectors()))
def test_norm_kernel_equals_the_restatement(rb, name):
    x = norm_vectors()[name]
    want, e = R.fix_norm(x, with_exponent=True)
    got = rb.debug_fix_norm(x)
    perm = rb.debug_fix_norm(np.random.default_rng(1).permutation(x))
    print(f"{name}: norm {got[0]!r}, quantum 2^{got[1]}, numpy's {float(np.linalg.norm(x))!r}")
    assert got[1] == e and bits(got[0]) == bits(want)
    assert perm[1] == e and bits(perm[0]) == bits(want)
    if name == "carries":
        assert 65537 * round(math.ldexp(0.9999 * 0.9999, -e)) >= 1 << 72          # the sum needs the high word


def test_norm_range_is_refused_by_the_debug_entry(rb):
    from raytracing_amd import _lib
    for M in (1e200, 1e-200):
        with pytest.raises(_lib.RtmiError, match="RTMI_LSQR_RANGE"):
            rb.debug_fix_norm(np.array([M, 0.0, -0.5 * M]))


# ---------------------------------------------------------------- the solver against the restatement
def restated(op, d, iter_lim, **kw):
    return R.lsqr_loop(lambda v: op.model(v.reshape(op.nb, op.ny, op.nx)).reshape(-1), lambda u: op.migrate(u.reshape(op.N, op.nt)).reshape(-1),
                       d, iter_lim, **kw)


def assert_same_run(got, want):
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert np.array_equal(got["x"].reshape(-1), want["x"])
    assert got["history"].shape == want["history"].shape and np.array_equal(got["history"], want["history"])
    for key in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(got[key]) == bits(want[key]), key


@pytest.mark.parametrize("damp", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["plain", "plain_full", "multi2", "aa1"])
def test_solver_equals_the_restatement_bit_for_bit(rb, kind, damp):
    op = make(rb, kind)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    got = op.lsqr(d, 6, damp=damp, history=True, stats=True)
    want = restated(op, d, 6, damp=damp)
    again = op.lsqr(d, 6, damp=damp, history=True)
    st = got["stats"]
    print(f"{kind} damp {damp}: itn {got['itn']} istop {got['istop']} r1norm {got['r1norm']:.6e} arnorm {got['arnorm']:.6e}; per iteration "
          f"total {st['total_ms'] / 6:.3f} ms, operators {st['operator_ms'] / 6:.3f} ms, vector passes {st['vector_ms'] / 6:.3f} ms; "
          f"{st['bytes_device']} bytes on the device")
    assert got["itn"] == 6 and got["istop"] == 7
    assert got["x"].shape == ((op.nb, op.ny, op.nx) if op.nbin else (op.ny, op.nx))
    assert_same_run(got, want)
    assert np.array_equal(again["x"], got["x"]) and np.array_equal(again["history"], got["history"])
    nlev = len(KINDS[kind][2] or (0,))
    assert st["bytes_device"] >= 8 * ((2 + nlev) * op.N * op.nt + 5 * op.nb * op.ny * op.nx)
    op.close()


def test_stops_where_the_restatement_does(rb):
    op = make(rb, "plain_amp_w")
    d = op.model(np.random.default_rng(4).standard_normal((op.ny, op.nx)))
    got = op.lsqr(d, 300, atol=1e-3, btol=1e-3, history=True)
    want = restated(op, d, 300, atol=1e-3, btol=1e-3)
    print(f"atol = btol = 1e-3 on consistent data: itn {got['itn']} istop {got['istop']}")
    assert got["istop"] in (1, 2) and 0 < got["itn"] < 300
    assert_same_run(got, want)
    one = op.lsqr(d, 1, history=True)
    assert_same_run(one, restated(op, d, 1))
    assert one["itn"] == 1 and one["istop"] == 7 and one["history"].shape == (1, 4)
    zero = op.lsqr(np.zeros_like(d), 5, history=True)
    assert (zero["itn"], zero["istop"]) == (0, 0) and not zero["x"].any() and zero["history"].shape == (0, 4)
    assert bits(zero["r1norm"]) == bits(0.0)
    op.close()


def test_an_operator_that_is_zero_returns_early(rb):
    T, isrc, irec, kw = KM.small_case(1)
    op = rb.Kirchhoff(np.full_like(T[:, 0], np.nan), isrc, irec, KM.SM_NT, KM.SM_DT)
    d = np.random.default_rng(2).standard_normal((op.N, op.nt))
    got = op.lsqr(d, 5, history=True)
    assert (got["itn"], got["istop"]) == (0, 0) and not got["x"].any() and got["arnorm"] == 0.0
    assert bits(got["r1norm"]) == bits(R.fix_norm(d))
    assert_same_run(got, restated(op, d, 5))
    op.close()


def test_a_norm_out_of_range_stops_the_solver(rb):
    from raytracing_amd import _lib
    op = make(rb, "plain")
    d = np.random.default_rng(6).standard_normal((op.N, op.nt))
    for scale in (1e200, 1e-200):
        got = op.lsqr(d * scale, 4, history=True)
        assert got["istop"] == _lib.LSQR_RANGE == R.LSQR_RANGE and got["itn"] == 0 and not got["x"].any()
        assert_same_run(got, restated(op, d * scale, 4))
    # the data's norm is in range, the second one (of L^T u scaled by the weights) is not
    T, isrc, irec, kw = KM.small_case(1, seed=3)
    big = rb.Kirchhoff(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT, weights=np.full(len(isrc), 1e160))
    got = big.lsqr(d, 4, history=True)
    assert got["istop"] == _lib.LSQR_RANGE and got["itn"] == 0
    assert_same_run(got, restated(big, d, 4))
    op.close(); big.close()


@pytest.mark.parametrize("w, itn", [(1.95e-154, 2), (1.05e154, 0)])
def test_a_norm_out_of_range_inside_the_loop_abandons_its_iteration(rb, w, itn):
    """Data = one column of L, so that the first L^T u has a peak and the later vectors are flatter; uniform weights scale every
    norm but the data's.  1.95e-154: max|u| of the third iteration (0.71 w against 0.84 w in the first) is the first whose
    square is below 2^-1022: two iterations stand.  1.05e154: max|v| of the first iteration (4.4 w against 3.7 w at the start)
    is the first whose square overflows, after that iteration's beta step: none stands, itn is 0 and anorm 0."""
    from raytracing_amd import _lib
    unit = make(rb, "plain")
    m = np.zeros((unit.ny, unit.nx))
    m.reshape(-1)[100] = 1.0
    d = unit.model(m)
    unit.close()
    T, isrc, irec, kw = KM.small_case(1, seed=3)
    op = rb.Kirchhoff(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT, weights=np.full(len(isrc), w))
    got = op.lsqr(d, 6, history=True)
    want = restated(op, d, 6)
    print(f"w {w}: itn {got['itn']} istop {got['istop']} anorm {got['anorm']!r} r1norm {got['r1norm']!r}")
    assert got["istop"] == _lib.LSQR_RANGE and got["itn"] == itn and got["history"].shape == (itn, 4)
    assert math.isfinite(got["anorm"]) and math.isfinite(got["arnorm"]) and np.all(np.isfinite(got["x"]))
    assert_same_run(got, want)
    op.close()


def test_a_device_buffer_that_is_too_short_is_refused(rb, torch):
    """An allocation of the runtime's own, whose end the test knows: a pointer 64 bytes before it cannot hold an image."""
    from raytracing_amd import _lib
    op = make(rb, "plain")
    L = _lib.lib()
    hip = C.CDLL(_lib.mapped_hip_runtimes()[0])
    for f in (hip.hipMalloc, hip.hipFree, hip.hipMemGetAddressRange):
        f.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    need = op.ny * op.nx * 8
    p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(p), 2 * need) == 0
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), p) == 0 and base.value == p.value and size.value >= 2 * need
        d = torch.zeros((op.N, op.nt), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        end = base.value + size.value
        assert L.rtmi_kirchhoff_migrate_dev(op._h, d.data_ptr(), None, end - 64, None) == -1
        assert b"d_image is shorter" in L.rtmi_last_error()
        assert L.rtmi_kirchhoff_model_dev(op._h, end - need + 8, d.data_ptr(), None, None) == -1
        assert b"d_model is shorter" in L.rtmi_last_error()
        # the buffer that just fits is taken
        assert L.rtmi_kirchhoff_migrate_dev(op._h, d.data_ptr(), None, end - need, None) == 0, L.rtmi_last_error()
    finally:
        assert hip.hipFree(p) == 0
    op.close()


def test_refusals_that_need_a_handle(rb):
    from raytracing_amd import _lib
    op = make(rb, "multi2_kmah")
    d = np.ones((op.N, op.nt))
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr: .*kmah") as ei:
        op.lsqr(d, 3)
    assert ei.value.code == -1
    op.close()
    op = make(rb, "plain")
    bad = d.copy()
    bad[3, 9] = np.inf
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr: .*data.*not finite") as ei:
        op.lsqr(bad, 3)
    assert ei.value.code == -1
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 3)


# ---------------------------------------------------------------- the standard case against scipy
def test_standard_case_against_scipy(rb):
    from scipy.sparse.linalg import lsqr
    isrc, irec = K1.geometry()
    T = K1.closed_T()
    L = K1.matrix(T, isrc, irec, K1.NT, K1.DT)
    d = L @ K1.lsm_model().reshape(-1)
    op = rb.Kirchhoff(T, isrc, irec, K1.NT, K1.DT, t0=K1.T0)
    t0 = time.perf_counter()
    got = op.lsqr(d, 10, stats=True)
    t1 = time.perf_counter()
    xs = lsqr(op.as_linear_operator(), d, atol=0, btol=0, iter_lim=10)[0]
    t2 = time.perf_counter()
    op.close()
    rd = float(np.linalg.norm(L @ got["x"].reshape(-1) - d) / np.linalg.norm(d))
    rs = float(np.linalg.norm(L @ xs - d) / np.linalg.norm(d))
    st = got["stats"]
    print(f"LSQR, 10 iterations: residual ratio on the device {rd:.8f}, scipy over as_linear_operator() {rs:.8f}; wall per iteration "
          f"{(t1 - t0) * 100:.2f} ms on the device (operators {st['operator_ms'] / 10:.2f} ms, vector passes {st['vector_ms'] / 10:.2f} ms) "
          f"against {(t2 - t1) * 100:.2f} ms")
    assert got["itn"] == 10 and got["istop"] == 7
    assert abs(rd - rs) <= 1e-6 * rs
    assert rd < 0.3
    assert abs(got["r1norm"] / float(np.linalg.norm(d)) - rd) <= 1e-6 * rd
