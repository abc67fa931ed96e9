"""GPU: least-squares migration with the trace filter inside the operator, every vector on the device
(rtmi_kirchhoff_lsqr_filtered; rt_bench.Kirchhoff.lsqr(filtered=True)): A x = F (ch0 + H ch1) and A^T u = migrate2(F^T u, -H F^T u).
The solver against the restatement tests/kirchhoff_lsqr_ref.py driven with the host-pointer channel calls, the restated H
(tests/hilbert_ref.py) and the restated F and F^T (tests/filter_ref.py), every bit of x, of the history and of the final scalars, on
tests/kirchhoff_multi_ref.py's small cases with kmah and on a handle without kmah from tests/kirchhoff_ref.py; with no filter set
the call is rtmi_kirchhoff_lsqr_full; an identity filter gives its x; adjointness of the operator the device entries make up; the
solver against scipy's lsqr over a host LinearOperator of the same operator (FFT H, numpy convolution); the stops and refusals
of DESIGN.md 21 with a filter set; the other solvers ignore a set filter.  The filter is a 9-tap wavelet convolved with 8
half-derivative taps: 16 taps, the origin at the wavelet's centre.  Measured values: DESIGN.md 25."""
import ctypes as C
import struct

import numpy as np
import pytest

import filter_ref as FR
import hilbert_ref as HR
import kirchhoff_aa_ref as KA
import kirchhoff_lsqr_ref as R
import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1

pytestmark = pytest.mark.gpu

# kind -> (kwargs of small_case, anti-aliased levels or None); "plain": a handle of rtmi_kirchhoff_create, no kmah
KINDS = {
    "multi2_kmah": (dict(amp=True, kmah=True, holes=True), None),
    "multi2_kmah_bins": (dict(nbin=6, amp=True, kmah=True, holes=True), None),
    "aa2_kmah": (dict(amp=True, kmah=True, holes=True), KA.HW8[:3]),
    "plain": None,
}
PLAIN_GRID = (-1.0, 0.1, 51, -2.0, 0.1, 26)
PLAIN_NT = 256
ORIGIN = 4


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


def wavelet_taps(rb, dt):
    """a 9-tap Ricker whose side lobes fit the 9 taps, convolved with 8 half-derivative taps; origin 4"""
    ricker = K1.ricker((np.arange(9) - ORIGIN) * dt, f=0.2 / dt)
    f = np.convolve(ricker, rb.half_derivative_taps(8, dt))
    assert f.shape == (16,) and np.all(np.isfinite(f))
    return f


def make(rb, kind, seed=3, filt=True, **more):
    """-> (handle, (T, isrc, irec, kwargs), taps of H, taps of F)"""
    if KINDS[kind] is None:
        pos_x = K1.POS_X[::8]
        isrc, irec = K1.geometry(pos=len(pos_x), every=2)
        T = K1.closed_T(pos_x=pos_x, grid=PLAIN_GRID)
        # the traveltimes in samples span the trace: the longest two-way time is the last sample
        dt = float(np.max(T[isrc] + T[irec])) / (PLAIN_NT - 2)
        op = rb.Kirchhoff(T, isrc, irec, PLAIN_NT, dt)
        case = (T, isrc, irec, None)
    else:
        skw, hw = KINDS[kind]
        skw = dict(skw, **more)
        pt = aa = None
        if hw is None:
            T, isrc, irec, kw = KM.small_case(2, seed=seed, **skw)
        else:
            T, pt, aa, isrc, irec, kw = KA.small_case(2, hw=hw, seed=seed, **skw)
        dt = KM.SM_DT
        op = rb.Kirchhoff(T, isrc, irec, KM.SM_NT, dt, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], weights=kw["w"],
                          nbin=kw["nbin"], dopen=kw["dopen"], pt=pt, antialias=aa)
        case = (T, isrc, irec, kw)
    f = wavelet_taps(rb, dt)
    if filt:
        op.set_filter(f, origin=ORIGIN)
    return op, case, rb.hilbert_taps(op.nt), f


def bits(v):
    return struct.pack("<d", float(v))


def restated(op, htaps, f, d, iter_lim, **kw):
    """the restated loop over A m = F (ch0 + H ch1) and A^T d = migrate2(F^T d, -H F^T d), with H, F and F^T restated"""
    def model(m):
        m = m.reshape(op.nb, op.ny, op.nx)
        if op.karr:
            c0, c1 = op.model_channels(m)
            b = c0 + HR.hilbert(c1, htaps) if op.has_kmah else c0
        else:
            b = op.model(m)
        return FR.apply(b, f, ORIGIN).reshape(-1)

    def migrate(d):
        ft = FR.apply(d.reshape(op.N, op.nt), f, ORIGIN, transpose=True)
        if op.karr:
            return op.migrate_channels(ft, -HR.hilbert(ft, htaps) if op.has_kmah else None).reshape(-1)
        return op.migrate(ft).reshape(-1)
    return R.lsqr_loop(model, migrate, d, iter_lim, norm=R.fix_norm, **kw)


def assert_same_run(got, want):
    assert (got["itn"], got["istop"]) == (want["itn"], want["istop"])
    assert np.array_equal(got["x"].reshape(-1), np.asarray(want["x"]).reshape(-1))
    assert got["history"].shape == want["history"].shape and np.array_equal(got["history"], want["history"])
    for key in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert bits(got[key]) == bits(want[key]), key


@pytest.mark.parametrize("damp", [0.0, 0.1])
@pytest.mark.parametrize("kind", list(KINDS))
def test_solver_equals_the_restatement_bit_for_bit(rb, kind, damp):
    op, _, htaps, f = make(rb, kind)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    got = op.lsqr(d, 6, damp=damp, history=True, stats=True, hilbert="device", filtered=True)
    want = restated(op, htaps, f, d, 6, damp=damp)
    again = op.lsqr(d, 6, damp=damp, history=True, hilbert="device", filtered=True)
    plain = op.lsqr(d, 6, damp=damp, history=True, stats=True, hilbert="device")
    st = got["stats"]
    print(f"{kind} damp {damp}: itn {got['itn']} istop {got['istop']} r1norm {got['r1norm']:.6e} arnorm {got['arnorm']:.6e}; per iteration "
          f"total {st['total_ms'] / 6:.3f} ms, operators {st['operator_ms'] / 6:.3f} ms, vector passes {st['vector_ms'] / 6:.3f} ms; "
          f"{st['bytes_device']} bytes on the device")
    assert got["itn"] == 6 and got["istop"] == 7
    assert got["x"].shape == ((op.nb, op.ny, op.nx) if op.nbin else (op.ny, op.nx))
    assert_same_run(got, want)
    assert_same_run(again, got)
    assert not np.array_equal(got["x"], plain["x"])                 # the filter is inside the operator
    # one more N nt vector and the 16 taps than the unfiltered call
    assert st["bytes_device"] == plain["stats"]["bytes_device"] + 8 * (op.N * op.nt + f.size)
    op.close()


@pytest.mark.parametrize("kind", ["multi2_kmah", "aa2_kmah", "plain"])
def test_no_filter_set_is_the_unfiltered_solver(rb, kind):
    from raytracing_amd import _lib
    op, _, _, f = make(rb, kind, filt=False)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    want = op.lsqr(d, 6, damp=0.1, history=True, stats=True, hilbert="device")
    with pytest.raises(ValueError, match="filtered=True needs a filter"):
        op.lsqr(d, 6, hilbert="device", filtered=True)
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.damp, lp.atol, lp.btol = 6, 0.1, 0.0, 0.0
    x, hist, st = np.empty((op.nb, op.ny, op.nx)), np.zeros((6, 4)), _lib.LsqrStats()
    _lib.check(_lib.lib().rtmi_kirchhoff_lsqr_filtered(op._h, C.byref(lp), _lib.dptr(d), _lib.dptr(x), _lib.dptr(hist), C.byref(st)))
    got = dict(x=x, itn=st.itn, istop=st.istop, history=hist[:st.itn], r1norm=st.r1norm, r2norm=st.r2norm, anorm=st.anorm,
               arnorm=st.arnorm)
    assert_same_run(got, want)
    assert x.tobytes() == want["x"].tobytes()
    assert st.bytes_device == want["stats"]["bytes_device"]
    # set and cleared again: the same
    op.set_filter(f, origin=ORIGIN)
    op.set_filter(None)
    st2 = _lib.LsqrStats()
    x2 = np.empty_like(x)
    _lib.check(_lib.lib().rtmi_kirchhoff_lsqr_filtered(op._h, C.byref(lp), _lib.dptr(d), _lib.dptr(x2), None, C.byref(st2)))
    assert x2.tobytes() == x.tobytes() and st2.bytes_device == st.bytes_device
    op.close()


@pytest.mark.parametrize("kind", ["multi2_kmah", "plain"])
def test_the_identity_filter_gives_the_unfiltered_x(rb, kind):
    op, _, _, _ = make(rb, kind, filt=False)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    want = op.lsqr(d, 6, damp=0.1, history=True, hilbert="device")
    op.set_filter([1.0])
    got = op.lsqr(d, 6, damp=0.1, history=True, hilbert="device", filtered=True)
    op.close()
    assert np.array_equal(got["x"], want["x"])         # as values: 1.0 * (-0.0) added to +0.0 is +0.0
    assert np.array_equal(got["history"], want["history"]) and got["itn"] == want["itn"]


@pytest.mark.parametrize("kind", ["multi2_kmah", "multi2_kmah_bins"])
def test_adjointness_of_the_device_entries(rb, torch, kind):
    op, (T, isrc, irec, kw), htaps, f = make(rb, kind)
    rng = np.random.default_rng(9)
    d = rng.standard_normal((op.N, op.nt))
    m = rng.standard_normal((op.nb, op.ny, op.nx))
    dev = torch.device("cuda")
    td, tm = torch.from_numpy(d).to(dev), torch.from_numpy(m).to(dev)
    c0, c1 = op.model_device(tm)
    Am = op.filter_device(op.hilbert_device(c1, add=c0)).cpu().numpy()                      # A m = F (ch0 + H ch1)
    ftd = op.filter_device(td, transpose=True)
    Atd = op.migrate_device(ftd, op.hilbert_device(ftd, negate=True)).cpu().numpy()         # A^T d = migrate2(F^T d, -H F^T d)
    lhs, rhs = float(Am.reshape(-1) @ d.reshape(-1)), float(m.reshape(-1) @ Atd.reshape(-1))
    # sum of |terms|: |d|^T |F| [I |H|] |L| |m|, every factor entry by entry
    g = FR.apply(np.abs(d), np.abs(f), ORIGIN, transpose=True)
    gh = g @ np.abs(HR.matrix(op.nt, htaps))                                                # row k: |H|^T g[k]
    L = abs(KM.matrix(T, isrc, irec, op.nt, KM.SM_DT, **kw))
    scale = float(np.concatenate([g.reshape(-1), gh.reshape(-1)]) @ (L @ np.abs(m.reshape(-1))))
    op.close()
    print(f"{kind}: <A m, d> - <m, A^T d> = {abs(lhs - rhs) / scale:.2e} of sum|terms|")
    assert np.any(c1.cpu().numpy() != 0) and lhs != 0.0
    assert abs(lhs - rhs) <= 1e-13 * scale


def test_against_scipy_over_a_host_operator(rb):
    from scipy.sparse.linalg import LinearOperator, lsqr
    op, _, _, f = make(rb, "multi2_kmah")

    def F(b, transpose=False):
        """numpy's convolution sliced at the origin (tests/test_filter_ref.py)"""
        L, nt = f.size, b.shape[-1]
        if transpose:
            return np.stack([np.convolve(row, f[::-1])[L - 1 - ORIGIN:L - 1 - ORIGIN + nt] for row in b])
        return np.stack([np.convolve(row, f)[ORIGIN:ORIGIN + nt] for row in b])

    def model(m):                                      # op.model and op.migrate: the FFT form of H on the host
        return F(op.model(m.reshape(op.ny, op.nx)))
    host = LinearOperator(op.shape, matvec=lambda m: model(m).reshape(-1),
                          rmatvec=lambda u: op.migrate(F(u.reshape(op.N, op.nt), transpose=True)).reshape(-1), dtype=np.float64)
    d = model(np.random.default_rng(4).standard_normal((op.ny, op.nx)))
    got = op.lsqr(d, 10, hilbert="device", filtered=True)
    xs = lsqr(host, d.reshape(-1), atol=0, btol=0, iter_lim=10)[0]
    nd = float(np.linalg.norm(d))
    rd = float(np.linalg.norm(model(got["x"]) - d)) / nd
    rs = float(np.linalg.norm(model(xs) - d)) / nd
    op.close()
    print(f"filtered LSQR, 10 iterations: residual ratio on the device {rd:.8f}, scipy over the host operator {rs:.8f}")
    assert got["itn"] == 10 and got["istop"] == 7
    assert abs(rd - rs) <= 1e-6 * rs
    assert rd < 1.0


def test_stops_and_refusals_are_those_of_the_unfiltered_solver(rb):
    from raytracing_amd import _lib
    op, _, htaps, f = make(rb, "multi2_kmah")
    kw = dict(history=True, hilbert="device", filtered=True)
    d = np.random.default_rng(6).standard_normal((op.N, op.nt))
    one = op.lsqr(d, 1, **kw)
    assert_same_run(one, restated(op, htaps, f, d, 1))
    assert one["itn"] == 1 and one["istop"] == 7 and one["history"].shape == (1, 4)
    zero = op.lsqr(np.zeros_like(d), 5, **kw)
    assert (zero["itn"], zero["istop"]) == (0, 0) and not zero["x"].any() and zero["history"].shape == (0, 4)
    assert bits(zero["r1norm"]) == bits(0.0)
    for value in (np.inf, np.nan):
        bad = d.copy()
        bad[3, 9] = value
        with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr_filtered: .*data.*not finite") as ei:
            op.lsqr(bad, 3, **kw)
        assert ei.value.code == -1
    for scale in (1e200, 1e-200):                     # a norm out of range stops the solver before its first iteration
        got = op.lsqr(d * scale, 4, **kw)
        assert got["istop"] == _lib.LSQR_RANGE and got["itn"] == 0 and not got["x"].any()
    with pytest.raises(ValueError, match='needs hilbert="device"'):
        op.lsqr(d, 3, filtered=True)
    # the handle still works
    assert_same_run(op.lsqr(d, 1, **kw), one)
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.lsqr(d, 3, **kw)


@pytest.mark.parametrize("kind", ["multi2_kmah", "plain"])
def test_the_other_solvers_ignore_a_set_filter(rb, kind):
    from raytracing_amd import _lib
    op, _, _, f = make(rb, kind, filt=False)
    d = np.random.default_rng(12).standard_normal((op.N, op.nt))
    calls = [dict(hilbert="device")] + ([] if op.has_kmah else [dict()])       # _lsqr_full, and _lsqr where it takes the handle
    before = [op.lsqr(d, 5, damp=0.1, history=True, stats=True, **kw) for kw in calls]
    op.set_filter(f, origin=ORIGIN)
    after = [op.lsqr(d, 5, damp=0.1, history=True, stats=True, **kw) for kw in calls]
    for a, b in zip(before, after):
        assert_same_run(b, a)
        assert a["x"].tobytes() == b["x"].tobytes() and a["stats"]["bytes_device"] == b["stats"]["bytes_device"]
    if op.has_kmah:
        with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_lsqr: .*kmah.*rtmi_kirchhoff_lsqr_full"):
            op.lsqr(d, 3)
    op.close()
