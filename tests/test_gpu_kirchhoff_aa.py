"""GPU: the Kirchhoff pair anti-aliased by operator slope (rtmi_kirchhoff_create_aa / rtmi_kirchhoff_aa_filter, rt_bench.Kirchhoff
with pt).  aa_filter against the restatement's triangle bit for bit; migrate_channels against the loop restatement
(tests/kirchhoff_aa_ref.py) bit for bit; model_channels against its CSR matrix, the same bits twice and in any trace order; traces
of two windows; the degenerate cases against today's create_multi handle bit for bit; adjointness; a pt that is not finite
silences exactly its slots; the refusals that need a handle; and end to end from traveltime_table: position_slope against the
central difference of the closed form, and the acceptance case of a flat reflector in a zero-offset section.
Shapes: kirchhoff_multi_ref's small case (960 nodes, 5 positions, 23 traces, 64 samples).  Bounds and measured values: DESIGN.md 20."""
import ctypes as C

import numpy as np
import pytest

import kirchhoff_aa_ref as KA
import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1
from conftest import LIMITS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


def operator(rb, T, pt, aa, isrc, irec, kw, nt=KM.SM_NT, order=None):
    w = kw["w"]
    if order is not None:
        isrc, irec, w = isrc[order], irec[order], None if w is None else w[order]
    return rb.Kirchhoff(T, isrc, irec, nt, KM.SM_DT, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], weights=w, nbin=kw["nbin"],
                        dopen=kw["dopen"], pt=pt, antialias=aa)


# ---------------------------------------------------------------- the bank
@pytest.mark.parametrize("nt", [64, 5])
def test_aa_filter_is_the_triangle_bit_for_bit(rb, nt):
    T, pt, aa, isrc, irec, kw = KA.small_case(1, seed=1, nt=nt)
    d = np.random.default_rng(nt).standard_normal((len(isrc), nt))
    for kmah in (None, np.zeros_like(T)):                       # one and two channels in the handle: the bank is of one channel
        op = operator(rb, T, pt, aa, isrc, irec, dict(kw, kmah=kmah), nt=nt)
        bank = op.aa_filter(d)
        op.close()
        assert bank.shape == (8, len(isrc), nt)
        for l, k in enumerate(KA.HW8):
            assert np.array_equal(bank[l], KA.tri(d, k)), (l, k)
        assert np.array_equal(bank[0], d)


# ---------------------------------------------------------------- the pair against the restatement
# (K, nbin, amp, w, kmah, holes in T, holes in pt, shot-ordered, nlev): every K with each of the bin layouts (none, 256 lanes, 128
# lanes), each option on and off, both trace orders, 2, 4 and 8 levels
CASES = [(1, 0, False, False, False, False, False, True, 8), (1, 5, True, True, True, True, False, False, 4),
         (1, 17, False, True, True, False, True, True, 2), (2, 0, True, False, True, True, False, True, 4),
         (2, 5, False, False, False, False, True, False, 8), (2, 17, True, True, True, True, False, True, 2),
         (3, 0, False, True, True, True, False, False, 8), (3, 5, True, True, True, False, True, True, 2),
         (3, 17, False, False, False, True, False, True, 4), (4, 0, True, True, True, True, False, True, 8),
         (4, 0, False, False, False, False, True, False, 2), (4, 5, False, True, True, True, False, True, 4),
         (4, 17, True, False, True, False, True, False, 8), (4, 17, True, True, False, True, False, True, 4)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_channels_against_the_restatement(rb, case):
    karr, nbin, amp, w, kmah, holes, pt_holes, ordered, nlev = CASES[case]
    T, pt, aa, isrc, irec, kw = KA.small_case(karr, hw=KA.HW8[:nlev], pt_holes=pt_holes, nbin=nbin, amp=amp, w=w, kmah=kmah, holes=holes,
                                              seed=300 + case, shot_ordered=ordered)
    seen, beyond = KA.levels_hit(T, pt, aa, isrc, irec, KM.SM_NT, kw)
    assert seen == set(range(nlev)) and beyond                 # every level is selected, and some pairs are steeper than the last
    rng = np.random.default_rng(case)
    N, nt = len(isrc), KM.SM_NT
    d0, d1 = rng.standard_normal((2, N, nt))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    ref, cnt = KA.migrate(T, pt, aa, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    L = KA.matrix(T, pt, aa, isrc, irec, nt, KM.SM_DT, **kw)
    op = operator(rb, T, pt, aa, isrc, irec, kw)
    img, st = op.migrate_channels(d0, d1 if kmah else None, stats=True)
    assert img.shape == ((nbin,) + T.shape[2:] if nbin else T.shape[2:])
    assert np.array_equal(img.reshape(ref.shape), ref), f"{np.max(np.abs(img.reshape(ref.shape) - ref)):.3e}"
    assert st["contributing"] == cnt and st["pairs"] == N * T[0, 0].size * karr * karr
    assert 0 < cnt < st["pairs"]
    # model
    (c0, c1), sm = op.model_channels(m, stats=True)
    dref = (L @ m.reshape(-1)).reshape(2, N, nt)
    e = max(np.max(np.abs(c0 - dref[0])), np.max(np.abs(c1 - dref[1]))) / np.max(np.abs(dref))
    assert sm["contributing"] == cnt and sm["pairs"] == st["pairs"]
    assert kmah or not np.any(c1)
    a0, a1 = op.model_channels(m)
    assert np.array_equal(a0, c0) and np.array_equal(a1, c1)
    # the traces in a random order: the model's rows keep their bits, the image moves by rounding only
    order = np.random.default_rng(5).permutation(N)
    opp = operator(rb, T, pt, aa, isrc, irec, kw, order=order)
    p0, p1 = opp.model_channels(m)
    ip = opp.migrate_channels(d0[order], d1[order] if kmah else None)
    ei = np.max(np.abs(ip - img)) / np.max(np.abs(img))
    op.close(); opp.close()
    print(f"{CASES[case]}: contributing {cnt} of {st['pairs']}, model against the matrix {e:.2e}, scale_exp {sm['scale_exp']}, "
          f"migrate under a permutation {ei:.2e}, kernel ms migrate {st['kernel_ms']:.3f} (filter {st['aux_ms']:.3f}) "
          f"model {sm['kernel_ms']:.3f} (sum over levels {sm['aux_ms']:.3f})")
    assert e <= 1e-12
    assert np.array_equal(p0, c0[order]) and np.array_equal(p1, c1[order])
    assert ei <= 1e-12


@pytest.mark.parametrize("kmah", [True, False])
def test_a_trace_of_two_windows(rb, kmah):
    """W = 4096 / (levels x channels) = 512 with 4 levels and kmah, and with 8 levels without: 515 samples are two windows"""
    nt, nlev = 515, 4 if kmah else 8
    T, pt, aa, isrc, irec, kw = KA.small_case(2, hw=KA.HW8[:nlev], amp=True, kmah=kmah, holes=True, seed=5, N=3, nt=nt)
    rng = np.random.default_rng(6)
    m = rng.standard_normal(T.shape[2:])
    d0, d1 = rng.standard_normal((2, 3, nt))
    L = KA.matrix(T, pt, aa, isrc, irec, nt, KM.SM_DT, **kw)
    ref, cnt = KA.migrate(T, pt, aa, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    op = operator(rb, T, pt, aa, isrc, irec, kw, nt=nt)
    (c0, c1), st = op.model_channels(m, stats=True)
    dref = (L @ m.reshape(-1)).reshape(2, 3, nt)
    e = max(np.max(np.abs(c0 - dref[0])), np.max(np.abs(c1 - dref[1]))) / np.max(np.abs(dref))
    S = KM.matrix(T, isrc, irec, nt, KM.SM_DT, **kw) @ m.reshape(-1)            # the unfiltered spreads: where pairs land
    j = np.nonzero(np.any(S.reshape(2, 3, nt) != 0, axis=(0, 1)))[0]
    print(f"kmah {kmah}: nt {nt}, {nlev} levels, samples hit {j.min()} .. {j.max()}, model against the matrix {e:.2e}, contributing {cnt}")
    assert j.min() < 512 <= j.max()                             # both windows receive pairs
    assert st["contributing"] == cnt and e <= 1e-12
    assert np.array_equal(op.migrate_channels(d0, d1 if kmah else None), ref[0])
    op.close()


@pytest.mark.parametrize("degenerate", ["nlev 1", "lengths 0"])
@pytest.mark.parametrize("case", [(1, 0, False, False, False), (2, 5, True, True, True), (4, 17, True, False, True), (3, 0, False, True, True)])
def test_degenerate_cases_are_todays_multi_handle_bit_for_bit(rb, degenerate, case):
    karr, nbin, amp, w, kmah = case
    T, pt, aa, isrc, irec, kw = KA.small_case(karr, nbin=nbin, amp=amp, w=w, kmah=kmah, holes=True, seed=40 + karr)
    aa = dict(aa, hw=(0,)) if degenerate == "nlev 1" else dict(hw=KA.HW8, asrc=0.0, arec=0.0, amid=0.0)
    rng = np.random.default_rng(2)
    d0, d1 = rng.standard_normal((2, len(isrc), KM.SM_NT))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    old = rb.Kirchhoff(T, isrc, irec, KM.SM_NT, KM.SM_DT, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], weights=kw["w"], nbin=nbin,
                       dopen=kw["dopen"])
    new = operator(rb, T, pt, aa, isrc, irec, kw)
    io, so = old.migrate_channels(d0, d1 if kmah else None, stats=True)
    i2, s2 = new.migrate_channels(d0, d1 if kmah else None, stats=True)
    assert np.array_equal(io, i2) and so["contributing"] == s2["contributing"] and so["pairs"] == s2["pairs"]
    (o0, o1), mo = old.model_channels(m, stats=True)
    (c0, c1), m2 = new.model_channels(m, stats=True)
    assert np.array_equal(o0, c0) and np.array_equal(o1, c1)
    assert mo["scale_exp"] == m2["scale_exp"] and mo["contributing"] == m2["contributing"]
    assert np.array_equal(new.migrate(d0), old.migrate(d0)) and np.array_equal(new.model(m), old.model(m))
    old.close(); new.close()


@pytest.mark.parametrize("case", [(2, 0), (2, 5), (4, 0), (4, 5)])
def test_adjointness_on_the_device(rb, case):
    karr, nbin = case
    T, pt, aa, isrc, irec, kw = KA.small_case(karr, pt_holes=True, nbin=nbin, amp=True, w=True, kmah=True, holes=True, seed=50 + karr)
    N, nt = len(isrc), KM.SM_NT
    rng = np.random.default_rng(9)
    d0, d1, d = rng.standard_normal((3, N, nt))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    L = abs(KA.matrix(T, pt, aa, isrc, irec, nt, KM.SM_DT, **kw))
    op = operator(rb, T, pt, aa, isrc, irec, kw)
    c0, c1 = op.model_channels(m)
    lhs = float(c0.reshape(-1) @ d0.reshape(-1) + c1.reshape(-1) @ d1.reshape(-1))
    rhs = float(m.reshape(-1) @ op.migrate_channels(d0, d1).reshape(-1))
    scale = float(np.abs(np.concatenate([d0.reshape(-1), d1.reshape(-1)])) @ (L @ np.abs(m.reshape(-1))))
    # and the full traces: model = ch0 + H ch1, migrate = L^T (d, -H d)
    lhs2 = float(op.model(m).reshape(-1) @ d.reshape(-1))
    rhs2 = float(m.reshape(-1) @ op.migrate(d).reshape(-1))
    scale2 = float(np.abs(np.concatenate([d.reshape(-1), rb.hilbert(d).reshape(-1)])) @ (L @ np.abs(m.reshape(-1))))
    A = op.as_linear_operator()
    assert A.shape == (N * nt, max(nbin, 1) * T[0, 0].size) and np.array_equal(A.matvec(m.reshape(-1)), op.model(m).reshape(-1))
    op.close()
    print(f"K {karr} nbin {nbin}: channels |diff| / sum|terms| {abs(lhs - rhs) / scale:.2e}, full traces {abs(lhs2 - rhs2) / scale2:.2e}")
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert abs(lhs2 - rhs2) <= 1e-12 * scale2


def test_a_pt_that_is_not_finite_silences_exactly_its_slots(rb):
    """NaN and +-inf in pt: the image and the traces are those of tables with T = NaN in these slots"""
    T, pt, aa, isrc, irec, kw = KA.small_case(3, nbin=5, amp=True, w=True, kmah=True, seed=77)
    rng = np.random.default_rng(8)
    bad = rng.random(T.shape) < 0.08
    pb = pt.copy()
    pb[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    N, nt = len(isrc), KM.SM_NT
    d0, d1 = rng.standard_normal((2, N, nt))
    m = rng.standard_normal((5,) + T.shape[2:])
    clean = operator(rb, T, pt, aa, isrc, irec, kw)
    dirty = operator(rb, T, pb, aa, isrc, irec, kw)
    gone = operator(rb, np.where(bad, np.nan, T), pt, aa, isrc, irec, kw)
    ic, sc = clean.migrate_channels(d0, d1, stats=True)
    idy, sd = dirty.migrate_channels(d0, d1, stats=True)
    ig, sg = gone.migrate_channels(d0, d1, stats=True)
    ref, cnt = KA.migrate(T, pb, aa, isrc, irec, d0, d1, KM.SM_DT, **kw)
    assert np.array_equal(idy, ig) and np.array_equal(idy, ref) and sd["contributing"] == sg["contributing"] == cnt
    assert sd["contributing"] < sc["contributing"] and not np.array_equal(idy, ic)
    (y0, y1), md = dirty.model_channels(m, stats=True)
    (g0, g1), mg = gone.model_channels(m, stats=True)
    assert np.array_equal(y0, g0) and np.array_equal(y1, g1) and md["contributing"] == mg["contributing"] == cnt
    clean.close(); dirty.close(); gone.close()


def test_refusals_that_need_a_handle(rb):
    from raytracing_amd import _lib
    T, pt, aa, isrc, irec, kw = KA.small_case(2, kmah=True, seed=1)
    d = np.zeros((len(isrc), KM.SM_NT))
    m = np.zeros(T.shape[2:])
    img = np.zeros(T.shape[2:])
    bank = np.zeros((8,) + d.shape)
    L = _lib.lib()
    op = operator(rb, T, pt, aa, isrc, irec, kw)
    assert L.rtmi_kirchhoff_migrate(op._h, _lib.dptr(d), _lib.dptr(img), None) == -1 and b"migrate2" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model(op._h, _lib.dptr(m), _lib.dptr(d), None) == -1 and b"model2" in L.rtmi_last_error()
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_migrate2: .*data1") as e:
        op.migrate_channels(d, None)
    assert e.value.code == -1
    assert L.rtmi_kirchhoff_model2(op._h, _lib.dptr(m), _lib.dptr(d), None, None) == -1 and b"data1" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_aa_filter(op._h, None, _lib.dptr(bank)) == -1 and b"data" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_aa_filter(op._h, _lib.dptr(d), _lib.dptr(bank)) == 0
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.aa_filter(d)
    for old in (rb.Kirchhoff(T, isrc, irec, KM.SM_NT, KM.SM_DT), rb.Kirchhoff(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT)):
        assert L.rtmi_kirchhoff_aa_filter(old._h, _lib.dptr(d), _lib.dptr(bank)) == -1
        assert b"rtmi_kirchhoff_aa_filter: " in L.rtmi_last_error() and b"create_aa" in L.rtmi_last_error()
        with pytest.raises(ValueError, match="no pt"):
            old.aa_filter(d)
        old.close()


# ---------------------------------------------------------------- end to end on the device's own tables
SCEN = "vert_heterogeneous"


@pytest.fixture(scope="module")
def survey(rb):
    """the standard positions and grid from traveltime_table: op6 at DELTA_S, a 1 024-ray fan; n at the positions from the field"""
    F = rb.Field.build(SCEN, LIMITS[SCEN], rb.DELTA)
    src = np.stack([K1.POS_X, np.full(len(K1.POS_X), K1.POS_Y)], axis=1)
    tab = rb.traveltime_table(rb.op6, F, src, K1.GRID, thetas=np.linspace(0.05, np.pi - 0.05, 1024), step=rb.DELTA_S,
                              max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=LIMITS[SCEN])
    n = F.n_gradient(K1.POS_X, np.full(len(K1.POS_X), K1.POS_Y))[0]
    F.close()
    return tab, n


def test_position_slope_of_the_devices_tables(rb, survey):
    tab, n = survey
    pt = rb.position_slope(tab, n)
    ref = KA.closed_pt_central()
    ok = np.isfinite(pt)
    e = np.max(np.abs(pt - ref)[ok]) / np.max(np.abs(ref))
    print(f"position_slope of traveltime_table's theta0 against the central difference of vert_T: {e:.2e} of max|pt| "
          f"= {np.max(np.abs(ref)):.4f}; {ok.mean():.4f} of the nodes covered; n at the positions {n.min():.6f} .. {n.max():.6f}")
    assert pt.shape == tab["T"].shape and np.array_equal(ok, np.isfinite(tab["T"])) and ok.mean() > 0.9
    assert e <= 1e-3


def test_acceptance_flat_reflector_zero_offset_on_the_device(rb, survey):
    """Artefact / reflector anti-aliased over plain <= 0.1 and the reflector kept >= 0.9 (kirchhoff_aa_ref.acceptance_*)."""
    tab, n = survey
    isrc, irec, d, amid = KA.acceptance_data()
    plain_op = rb.Kirchhoff(tab["T"], isrc, irec, K1.NT, K1.DT, t0=K1.T0)
    plain = plain_op.migrate(d)
    plain_op.close()
    op = rb.Kirchhoff.from_table(tab, isrc, irec, K1.NT, K1.DT, t0=K1.T0,
                                 antialias=dict(hw=KA.ACC_HW, amid=amid, n_at_positions=n, direction=(1.0, 0.0)))
    assert op.karr == 1 and op.nlev == 6 and op.antialias == dict(hw=KA.ACC_HW, asrc=0.0, arec=0.0, amid=amid)
    img, st = op.migrate(d, stats=True)
    op.close()
    rp, ap = KA.acceptance_figures(plain)
    ra, aa = KA.acceptance_figures(img)
    print(f"plain: artefact / reflector {ap / rp:.4f}; anti-aliased: {aa / ra:.4f}; ratio {(aa / ra) / (ap / rp):.4f}; "
          f"reflector kept {ra / rp:.4f}; kernel ms {st['kernel_ms']:.3f} (filter {st['aux_ms']:.3f})")
    assert img.shape == plain.shape
    assert (aa / ra) / (ap / rp) <= 0.1
    assert ra / rp >= 0.9
