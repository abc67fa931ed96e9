"""GPU: least-squares migration of the full trace of a handle with kmah, every vector on the device (rtmi_kirchhoff_lsqr_full;
rt_bench.Kirchhoff.lsqr(hilbert="device")), on tests/kirchhoff_multi_ref.py's small case.  The solver against the restatement
tests/kirchhoff_lsqr_ref.py driven with the host-pointer channel calls and the restated H (tests/hilbert_ref.py), every bit of x,
of the history and of the final scalars; adjointness of the operator the device entries make up; the solver against scipy's lsqr
over as_linear_operator(), whose H is the FFT form; a handle without kmah, where the call is rtmi_kirchhoff_lsqr; the stops and
refusals of DESIGN.md 21.  Measured values: DESIGN.md 23."""
import ctypes as C
import struct

import numpy as np
import pytest

import hilbert_ref as HR
import kirchhoff_aa_ref as KA
import kirchhoff_lsqr_ref as R
import kirchhoff_multi_ref as KM

pytestmark = pytest.mark.gpu

# kind -> (kwargs of small_case, anti-aliased levels or None)
KINDS = {
    "multi2_kmah": (dict(amp=True, kmah=True, holes=True), None),
    "multi2_kmah_bins": (dict(nbin=6, amp=True, kmah=True, holes=True), None),
    "aa2_kmah": (dict(amp=True, kmah=True, holes=True), KA.HW8[:3]),
}


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


@pytest.fixture(scope="module")
def taps(rb):
    return rb.hilbert_taps(KM.SM_NT)


def make(rb, kind, seed=3, **more):
    skw, hw = KINDS[kind]
    skw = dict(skw, **more)
    pt = aa = None
    if hw is None:
        T, isrc, irec, kw = KM.small_case(2, seed=seed, **skw)
    else:
        T, pt, aa, isrc, irec, kw = KA.small_case(2, hw=hw, seed=seed, **skw)
    op = rb.Kirchhoff(T, isrc, irec, KM.SM_NT, KM.SM_DT, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], weights=kw["w"],
                      nbin=kw["nbin"], dopen=kw["dopen"], pt=pt, antialias=aa)
    return op, (T, isrc, irec, kw)


def bits(v):
    return struct.pack("<d", float(v))


def restated(op, taps, d, iter_lim, **kw):
    """the restated loop over the full-trace operator: A m = ch0 + H ch1 and A^T d = migrate2(d, -H d), H restated"""
    def model(m):
        c0, c1 = op.model_channels(m.reshape(op.nb, op.ny, op.nx))
        return (c0 + HR.hilbert(c1, taps)).reshape(-1)

    def migrate(d):
        d = d.reshape(op.N, op.nt)
        return op.migrate_channels(d, -HR.hilbert(d, taps)).reshape(-1)
    return R.lsqr_loop(model, migrate, d, iter_lim, norm=R.fix_norm, **kw)


def assert_same_run(got, want):
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert np.array_equal(got["x"].reshape(-1), want["x"])
    assert got["history"].shape == want["history"].shape and np.array_equal(got["history"], want["history"])
    for key in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(got[key]) == bits(want[key]), key


@pytest.mark.parametrize("damp", [0.0, 0.1])
@pytest.mark.parametrize("kind", list(KINDS))
def test_solver_equals_the_restatement_bit_for_bit(rb, taps, kind, damp):
    op, _ = make(rb, kind)
    assert op.has_kmah
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    got = op.lsqr(d, 6, damp=damp, history=True, stats=True, hilbert="device")
    want = restated(op, taps, d, 6, damp=damp)
    again = op.lsqr(d, 6, damp=damp, history=True, hilbert="device")
    st = got["stats"]
    print(f"{kind} damp {damp}: itn {got['itn']} istop {got['istop']} r1norm {got['r1norm']:.6e} arnorm {got['arnorm']:.6e}; per iteration "
          f"total {st['total_ms'] / 6:.3f} ms, operators {st['operator_ms'] / 6:.3f} ms, vector passes {st['vector_ms'] / 6:.3f} ms; "
          f"{st['bytes_device']} bytes on the device")
    assert got["itn"] == 6 and got["istop"] == 7
    assert got["x"].shape == ((op.nb, op.ny, op.nx) if op.nbin else (op.ny, op.nx))
    assert_same_run(got, want)
    assert np.array_equal(again["x"], got["x"]) and np.array_equal(again["history"], got["history"])
    for key in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(again[key]) == bits(got[key])
    # the call's own vectors (4 N nt + 4 model-sized), the staging of two channels per level and the image, the taps
    nlev = len(KINDS[kind][1] or (0,))
    assert st["bytes_device"] >= 8 * ((4 + 2 * nlev) * op.N * op.nt + 5 * op.nb * op.ny * op.nx + taps.size)
    # the solver of one channel still refuses the handle, and says where to go
    from raytracing_amd import _lib
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr: .*kmah.*rtmi_kirchhoff_lsqr_full"):
        op.lsqr(d, 3)
    op.close()


@pytest.mark.parametrize("kind", ["multi2_kmah", "multi2_kmah_bins"])
def test_adjointness_of_the_device_entries(rb, torch, kind):
    op, (T, isrc, irec, kw) = make(rb, kind)
    rng = np.random.default_rng(9)
    d = rng.standard_normal((op.N, op.nt))
    m = rng.standard_normal((op.nb, op.ny, op.nx))
    L = abs(KM.matrix(T, isrc, irec, op.nt, KM.SM_DT, **kw))
    dev = torch.device("cuda")
    td, tm = torch.from_numpy(d).to(dev), torch.from_numpy(m).to(dev)
    c0, c1 = op.model_device(tm)
    Am = op.hilbert_device(c1, add=c0).cpu().numpy()                                        # A m = ch0 + H ch1
    Atd = op.migrate_device(td, op.hilbert_device(td, negate=True)).cpu().numpy()           # A^T d = migrate2(d, -H d)
    lhs, rhs = float(Am.reshape(-1) @ d.reshape(-1)), float(m.reshape(-1) @ Atd.reshape(-1))
    scale = float(np.abs(np.concatenate([d.reshape(-1), op.hilbert(d).reshape(-1)])) @ (L @ np.abs(m.reshape(-1))))
    op.close()
    print(f"{kind}: <A m, d> - <m, A^T d> = {abs(lhs - rhs) / scale:.2e} of sum|terms|")
    assert np.any(c1.cpu().numpy() != 0)
    assert abs(lhs - rhs) <= 1e-13 * scale


def test_against_scipy_over_the_fft_form(rb):
    from scipy.sparse.linalg import lsqr
    op, _ = make(rb, "multi2_kmah")
    d = op.model(np.random.default_rng(4).standard_normal((op.ny, op.nx)))
    got = op.lsqr(d, 10, stats=True, hilbert="device")
    xs = lsqr(op.as_linear_operator(), d.reshape(-1), atol=0, btol=0, iter_lim=10)[0]
    nd = float(np.linalg.norm(d))
    rd = float(np.linalg.norm(op.model(got["x"]) - d)) / nd
    rs = float(np.linalg.norm(op.model(xs.reshape(op.ny, op.nx)) - d)) / nd
    op.close()
    print(f"LSQR of the full trace, 10 iterations: residual ratio on the device {rd:.8f}, scipy over as_linear_operator() {rs:.8f}")
    assert got["itn"] == 10 and got["istop"] == 7
    assert abs(rd - rs) <= 1e-6 * rs
    assert rd < 1.0


@pytest.mark.parametrize("kind", ["multi2_kmah", "aa2_kmah"])
def test_a_handle_without_kmah_is_the_solver_of_one_channel(rb, kind):
    op, _ = make(rb, kind, kmah=False)
    assert not op.has_kmah
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    a = op.lsqr(d, 6, damp=0.1, history=True, stats=True)
    b = op.lsqr(d, 6, damp=0.1, history=True, stats=True, hilbert="device")
    op.close()
    assert_same_run(b, dict(a, x=a["x"].reshape(-1)))
    assert a["stats"]["bytes_device"] == b["stats"]["bytes_device"]


def test_stops_and_refusals_are_those_of_the_solver_of_one_channel(rb, taps):
    from raytracing_amd import _lib
    op, _ = make(rb, "multi2_kmah")
    d = np.random.default_rng(6).standard_normal((op.N, op.nt))
    one = op.lsqr(d, 1, history=True, hilbert="device")
    assert_same_run(one, restated(op, taps, d, 1))
    assert one["itn"] == 1 and one["istop"] == 7 and one["history"].shape == (1, 4)
    zero = op.lsqr(np.zeros_like(d), 5, history=True, hilbert="device")
    assert (zero["itn"], zero["istop"]) == (0, 0) and not zero["x"].any() and zero["history"].shape == (0, 4)
    assert bits(zero["r1norm"]) == bits(0.0)
    for value in (np.inf, np.nan):
        bad = d.copy()
        bad[3, 9] = value
        with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr_full: .*data.*not finite") as ei:
            op.lsqr(bad, 3, hilbert="device")
        assert ei.value.code == -1
    for scale in (1e200, 1e-200):                     # a norm out of range stops the solver before its first iteration
        got = op.lsqr(d * scale, 4, history=True, hilbert="device")
        assert got["istop"] == _lib.LSQR_RANGE and got["itn"] == 0 and not got["x"].any()
    # the handle still works
    assert_same_run(op.lsqr(d, 1, history=True, hilbert="device"), dict(one, x=one["x"].reshape(-1)))
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 3, hilbert="device")


def test_a_trace_too_long_for_the_kernel_is_refused_by_name(rb):
    from raytracing_amd import _lib
    nt = _lib.HILBERT_MAX_NT + 2
    T, isrc, irec, kw = KM.small_case(2, amp=True, kmah=True, N=2, nt=nt)
    op = rb.Kirchhoff(T, isrc, irec, nt, KM.SM_DT, amp=kw["amp"], kmah=kw["kmah"])
    with pytest.raises(_lib.RtmiError, match=r"rtmi_kirchhoff_lsqr_full: .*\bnt\b"):
        op.lsqr(np.ones((2, nt)), 2, hilbert="device")
    op.close()
