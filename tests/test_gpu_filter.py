"""GPU: the trace filter of a Kirchhoff handle and its transpose (rtmi_kirchhoff_set_filter, rtmi_kirchhoff_filter / _filter_dev;
rt_bench.Kirchhoff.set_filter / filter / filter_device) against the restatement tests/filter_ref.py, every bit, on normal deviates
with random taps.  The kernel (kirchhoff_filter.hip) gives a lane 9 consecutive outputs, in blocks of 64 to 1024 lanes, one block
per trace, and unrolls its tap loop by 9; the lengths below stand on both sides of each of those boundaries:
  a full or partial last chunk of 9 outputs                              nt = 17, 18, 19
  a tap loop of whole groups of 9, with and without a tail               L = 8, 9, 10, 17, 18, 19
  64 lanes hold the trace, or 128 do                                     nt = 575, 576, 577
  1024 lanes hold the trace in one pass, or some lanes take a second     nt = 9215, 9216, 9217
and L > nt, where every output has terms outside the trace on both sides.  The trace and the filter's zeros are in LDS in one
piece: nt = 16384 with L = 2048 is the largest, nt = 16385 and L = 2049 are refused.  The kernel does not stride over traces and
has no wide-load path; an input at an address that is 8- but not 16-byte aligned is run all the same.  Measured values: DESIGN.md
25."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as FR

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 8, 9, 63, 64, 65, 255, 256, 257, 1000, 1001)
TAPS = (1, 2, 3, 9, 10, 64, 65, 257)


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


def handle(rb, N, nt):
    """any handle does: it supplies the device, N and nt"""
    T = 0.5 + np.arange(12.0).reshape(2, 2, 3) * 0.01
    return rb.Kirchhoff(T, np.arange(N, dtype=np.int32) % 2, (np.arange(N, dtype=np.int32) + 1) % 2, nt, 0.001)


def deviates(N, nt, seed=0):
    return np.random.default_rng(1000 * N + nt + seed).standard_normal((N, nt))


def origins(L):
    return sorted({0, L // 2, L - 1})


def both_directions_equal(op, x, f, o):
    op.set_filter(f, origin=o)
    for tr in (False, True):
        got = op.filter(x, transpose=tr)
        want = FR.apply(x, f, o, transpose=tr)
        assert got.shape == want.shape and np.array_equal(got, want), (x.shape, len(f), o, tr)
        assert np.any(got != 0)


@pytest.mark.parametrize("nt", LENGTHS)
def test_host_call_equals_the_restatement(rb, nt):
    op = handle(rb, 3, nt)
    x = deviates(3, nt)
    rng = np.random.default_rng(nt)
    for L in TAPS:                                     # L > nt at the short traces
        f = rng.standard_normal(L)
        for o in origins(L):
            both_directions_equal(op, x, f, o)
    op.close()


@pytest.mark.parametrize("nt", (17, 18, 19, 575, 576, 577, 9215, 9216, 9217))
def test_both_sides_of_the_kernels_boundaries(rb, nt):
    N = 2 if nt < 9000 else 1
    op = handle(rb, N, nt)
    x = deviates(N, nt)
    rng = np.random.default_rng(nt)
    for L in (8, 9, 10, 17, 18, 19):
        both_directions_equal(op, x, rng.standard_normal(L), origins(L)[L % 3])
    op.close()


def test_a_filter_longer_than_the_trace(rb):
    op = handle(rb, 3, 8)
    x = deviates(3, 8)
    f = np.random.default_rng(65).standard_normal(65)
    for o in (0, 3, 32, 57, 64):
        both_directions_equal(op, x, f, o)
    op.close()


@pytest.mark.parametrize("N, nt, L", [(1, 9000, 2048), (2, 16384, 2048)])
def test_the_longest_filter_and_the_longest_trace(rb, N, nt, L):
    op = handle(rb, N, nt)
    x = deviates(N, nt)
    f = np.random.default_rng(L).standard_normal(L)
    both_directions_equal(op, x, f, L // 3)
    op.close()


def test_one_beyond_the_longest_is_refused(rb):
    from raytracing_amd import _lib
    op = handle(rb, 2, _lib.FILTER_MAX_NT + 1)
    with pytest.raises(_lib.RtmiError, match=r"rtmi_kirchhoff_set_filter: .*\bnt\b") as ei:
        op.set_filter(np.ones(4))
    assert ei.value.code == -1
    with pytest.raises(_lib.RtmiError) as ei:                       # and so no filter is set
        op.filter(np.zeros((2, _lib.FILTER_MAX_NT + 1)))
    assert ei.value.code == -4 and "no filter is set" in str(ei.value)
    op.close()
    op = handle(rb, 2, 64)
    with pytest.raises(_lib.RtmiError, match=r"rtmi_kirchhoff_set_filter: .*\bL\b") as ei:
        op.set_filter(np.ones(_lib.FILTER_MAX_TAPS + 1))
    assert ei.value.code == -1
    op.set_filter(np.ones(_lib.FILTER_MAX_TAPS), origin=_lib.FILTER_MAX_TAPS - 1)
    x = deviates(2, 64)
    assert np.array_equal(op.filter(x), FR.apply(x, np.ones(_lib.FILTER_MAX_TAPS), _lib.FILTER_MAX_TAPS - 1))
    op.close()


@pytest.mark.parametrize("N, nt, L, o", [(1, 65, 9, 4), (3, 64, 10, 0), (700, 38, 10, 9), (5, 1001, 65, 32)])
def test_device_pointers(rb, torch, N, nt, L, o):
    op = handle(rb, N, nt)
    x = deviates(N, nt)
    f = np.random.default_rng(L).standard_normal(L)
    op.set_filter(f, origin=o)
    dev = torch.device("cuda")
    tx = torch.from_numpy(x).to(dev)
    for tr in (False, True):
        want = FR.apply(x, f, o, transpose=tr)
        got = op.filter_device(tx, transpose=tr)
        assert got.data_ptr() != tx.data_ptr() and got.shape == (N, nt)
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(op.filter(x, transpose=tr), want)      # the host-pointer call and the device-pointer call: equal bits
    assert np.array_equal(tx.cpu().numpy(), x)                       # x is never written
    # an input that is 8- but not 16-byte aligned
    buf = torch.empty(N * nt + 1, dtype=torch.float64, device=dev)
    odd = buf[1:].view(N, nt)
    odd.copy_(tx)
    assert odd.data_ptr() % 16 == 8
    for tr in (False, True):
        assert np.array_equal(op.filter_device(odd, transpose=tr).cpu().numpy(), FR.apply(x, f, o, transpose=tr))
    op.close()


@pytest.mark.parametrize("nt", (8, 9, 64, 65))
def test_the_devices_transpose_is_the_transpose_in_every_bit(rb, nt):
    op = handle(rb, nt, nt)
    rng = np.random.default_rng(nt)
    for L, o in ((5, 2), (nt + 3, 0), (nt + 3, (nt + 3) // 2), (nt + 3, nt + 2)):
        f = rng.standard_normal(L)
        op.set_filter(f, origin=o)
        F = op.filter(np.eye(nt)).T                    # column j = F e_j
        Ft = op.filter(np.eye(nt), transpose=True).T
        assert np.array_equal(Ft, F.T) and np.any(F != 0)
        assert np.array_equal(F, FR.matrix(nt, f, o)) and np.array_equal(Ft, FR.matrix(nt, f, o, transpose=True))
    op.close()


def test_set_filter_replaces_clears_and_refuses(rb):
    from raytracing_amd import _lib
    N, nt = 3, 64
    op = handle(rb, N, nt)
    x = deviates(N, nt)
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_filter: no filter is set") as ei:        # none yet
        op.filter(x)
    assert ei.value.code == -4
    f1, f2 = np.array([1.0, -2.0, 0.5]), np.random.default_rng(2).standard_normal(20)
    op.set_filter(f1, origin=1)
    assert np.array_equal(op.filter(x), FR.apply(x, f1, 1))
    op.set_filter(f2, origin=19)                                                                       # replace
    assert np.array_equal(op.filter(x), FR.apply(x, f2, 19))
    for bad in (np.nan, np.inf, -np.inf):                                                              # a refusal keeps the filter
        f = f1.copy()
        f[2] = bad
        with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_set_filter: taps has a value that is not finite") as ei:
            op.set_filter(f)
        assert ei.value.code == -1
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_set_filter: origin"):
        op.set_filter(f1, origin=3)
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_set_filter: origin"):
        op.set_filter(f1, origin=-1)
    assert np.array_equal(op.filter(x, transpose=True), FR.apply(x, f2, 19, transpose=True))
    op.set_filter(None)                                                                                # clear
    for call in (lambda: op.filter(x), lambda: op.filter(x, transpose=True)):
        with pytest.raises(_lib.RtmiError, match="no filter is set") as ei:
            call()
        assert ei.value.code == -4
    op.set_filter(None)                                                                                # clearing twice is fine
    op.set_filter(f1, origin=0)
    assert np.array_equal(op.filter(x), FR.apply(x, f1, 0))
    # the other calls ignore the filter
    before = op.hilbert(x)
    img = op.migrate(x)
    op.set_filter(None)
    assert np.array_equal(op.hilbert(x), before) and np.array_equal(op.migrate(x), img)
    op.close()


def test_refusals_that_need_a_handle(rb, torch):
    from raytracing_amd import _lib
    N, nt = 3, 64
    op = handle(rb, N, nt)
    L = _lib.lib()
    dev = torch.device("cuda")
    x = deviates(N, nt)
    f = np.array([0.25, 1.0, -0.5, 0.125])
    tx = torch.from_numpy(x).to(dev)
    ty = torch.zeros((N, nt), dtype=torch.float64, device=dev)
    hx = np.zeros((N, nt))
    torch.cuda.synchronize()
    assert L.rtmi_kirchhoff_filter_dev(op._h, tx.data_ptr(), 0, ty.data_ptr()) == -4                  # no filter set
    assert L.rtmi_last_error().startswith(b"rtmi_kirchhoff_filter_dev: no filter is set")
    op.set_filter(f, origin=1)
    for args, name in (((hx.ctypes.data, 0, ty.data_ptr()), b"d_x"), ((tx.data_ptr(), 0, hx.ctypes.data), b"d_y")):
        assert L.rtmi_kirchhoff_filter_dev(op._h, *args) == -1
        msg = L.rtmi_last_error()
        assert msg.startswith(b"rtmi_kirchhoff_filter_dev: ") and name in msg and b"handle's device" in msg, msg
    for tr in (0, 1):
        assert L.rtmi_kirchhoff_filter_dev(op._h, tx.data_ptr(), tr, tx.data_ptr()) == -1              # d_x == d_y
        assert b"d_y may not be d_x" in L.rtmi_last_error()
        assert L.rtmi_kirchhoff_filter_dev(op._h, tx.data_ptr(), tr, tx.data_ptr() + 8 * nt) == -1     # and overlapping it
        assert b"d_y may not be d_x" in L.rtmi_last_error()
    short = torch.zeros(N * nt - 1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rc = L.rtmi_kirchhoff_filter_dev(op._h, tx.data_ptr(), 0, short.data_ptr())
    if rc == -1:                                     # torch's allocator may have handed out a block that is long enough
        assert b"d_y is shorter" in L.rtmi_last_error()
    # the handle still works
    assert np.array_equal(op.filter_device(tx).cpu().numpy(), FR.apply(x, f, 1))
    assert np.array_equal(tx.cpu().numpy(), x)
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.filter_device(tx)
    with pytest.raises(RuntimeError, match="closed"):
        op.filter(x)
    with pytest.raises(RuntimeError, match="closed"):
        op.set_filter(f)
