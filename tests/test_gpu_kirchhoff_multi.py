"""GPU: Kirchhoff migration and modelling over several arrivals per node with caustic phase (rtmi_kirchhoff_create_multi /
_migrate2 / _model2, rt_bench.Kirchhoff with T [P, K, ny, nx]).  migrate_channels against the loop restatement
(tests/kirchhoff_multi_ref.py) bit for bit; model_channels against its CSR matrix, the same bits twice and in any trace order;
one arrival without kmah against today's one-arrival handle, bit for bit; adjointness; kmah values that silence their pairs;
a trace of two windows; the refusals that need a handle; the lens bed end to end from traveltime_table(arrivals=3).
Shapes: 40 x 24 = 960 nodes (a partial last block), 5 positions, 23 traces (a tail of every unroll), 64 samples.
Bounds and their measured values: DESIGN.md 19."""
import ctypes as C

import numpy as np
import pytest

import arrival_ref as A
import kirchhoff_multi_ref as KM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


def operator(rb, T, isrc, irec, kw, nt=KM.SM_NT, order=None):
    w = kw["w"]
    if order is not None:
        isrc, irec, w = isrc[order], irec[order], None if w is None else w[order]
    return rb.Kirchhoff(T, isrc, irec, nt, KM.SM_DT, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], weights=w, nbin=kw["nbin"],
                        dopen=kw["dopen"])


# (K, nbin, amp, w, kmah, holes, shot-ordered): every K with each of the bin layouts (none, 256 lanes, 128 lanes), each option on
# and off, both trace orders
CASES = [(1, 0, False, False, False, False, True), (1, 5, True, True, True, True, False), (1, 17, False, True, True, False, True),
         (2, 0, True, False, True, True, True), (2, 5, False, False, False, True, False), (2, 17, True, True, True, True, True),
         (3, 0, False, True, True, True, False), (3, 5, True, True, True, False, True), (3, 17, False, False, False, True, True),
         (4, 0, True, True, True, True, True), (4, 0, False, False, False, False, False), (4, 5, False, True, True, True, True),
         (4, 17, True, False, True, True, False), (4, 17, True, True, False, True, True)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_channels_against_the_restatement(rb, case):
    karr, nbin, amp, w, kmah, holes, ordered = CASES[case]
    T, isrc, irec, kw = KM.small_case(karr, nbin, amp, w, kmah, holes, seed=200 + case, shot_ordered=ordered)
    if kmah:
        assert set(np.unique(kw["kmah"][np.isfinite(kw["kmah"])] % 4)) == {0.0, 1.0, 2.0, 3.0}
    rng = np.random.default_rng(case)
    N, nt = len(isrc), KM.SM_NT
    d0, d1 = rng.standard_normal((2, N, nt))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    ref, cnt = KM.migrate(T, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    L = KM.matrix(T, isrc, irec, nt, KM.SM_DT, **kw)
    op = operator(rb, T, isrc, irec, kw)
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
    opp = operator(rb, T, isrc, irec, kw, order=order)
    p0, p1 = opp.model_channels(m)
    ip = opp.migrate_channels(d0[order], d1[order] if kmah else None)
    ei = np.max(np.abs(ip - img)) / np.max(np.abs(img))
    op.close(); opp.close()
    print(f"{CASES[case]}: contributing {cnt} of {st['pairs']}, model against the matrix {e:.2e}, scale_exp {sm['scale_exp']}, "
          f"migrate under a permutation {ei:.2e}, kernel ms migrate {st['kernel_ms']:.3f} model {sm['kernel_ms']:.3f}")
    assert e <= 1e-12
    assert np.array_equal(p0, c0[order]) and np.array_equal(p1, c1[order])
    assert ei <= 1e-12


@pytest.mark.parametrize("case", [(0, False, False, False), (0, True, True, True), (5, True, False, True), (17, False, True, True)])
def test_one_arrival_without_kmah_is_todays_operator_bit_for_bit(rb, case):
    nbin, amp, w, holes = case
    T, isrc, irec, kw = KM.small_case(1, nbin, amp, w, False, holes, seed=31 + nbin)
    rng = np.random.default_rng(2)
    d = rng.standard_normal((len(isrc), KM.SM_NT))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    first = lambda a: None if a is None else a[:, 0]             # noqa: E731
    old = rb.Kirchhoff(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT, amp=first(kw["amp"]), theta=first(kw["theta"]), weights=kw["w"],
                       nbin=nbin, dopen=kw["dopen"])
    new = operator(rb, T, isrc, irec, kw)
    io, so = old.migrate(d, stats=True)
    i2, s2 = new.migrate_channels(d, None, stats=True)
    assert np.array_equal(io, i2) and so["contributing"] == s2["contributing"] and so["pairs"] == s2["pairs"]
    assert np.array_equal(new.migrate(d), io)                    # without kmah there is no second channel to transform
    do, mo = old.model(m, stats=True)
    (c0, c1), m2 = new.model_channels(m, stats=True)
    assert np.array_equal(do, c0) and not np.any(c1) and mo["scale_exp"] == m2["scale_exp"] and mo["contributing"] == m2["contributing"]
    assert np.array_equal(new.model(m), do)
    old.close(); new.close()


@pytest.mark.parametrize("case", [(2, 0), (3, 5), (4, 17)])
def test_adjointness_on_the_device(rb, case):
    karr, nbin = case
    T, isrc, irec, kw = KM.small_case(karr, nbin, True, True, True, True, seed=50 + karr)
    N, nt = len(isrc), KM.SM_NT
    rng = np.random.default_rng(9)
    d0, d1, d = rng.standard_normal((3, N, nt))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    L = abs(KM.matrix(T, isrc, irec, nt, KM.SM_DT, **kw))
    op = operator(rb, T, isrc, irec, kw)
    c0, c1 = op.model_channels(m)
    lhs = float(c0.reshape(-1) @ d0.reshape(-1) + c1.reshape(-1) @ d1.reshape(-1))
    rhs = float(m.reshape(-1) @ op.migrate_channels(d0, d1).reshape(-1))
    scale = float(np.abs(np.concatenate([d0.reshape(-1), d1.reshape(-1)])) @ (L @ np.abs(m.reshape(-1))))
    # and the full traces: model = ch0 + H ch1, migrate = L^T (d, -H d)
    lhs2 = float(op.model(m).reshape(-1) @ d.reshape(-1))
    rhs2 = float(m.reshape(-1) @ op.migrate(d).reshape(-1))
    scale2 = float(np.abs(np.concatenate([d.reshape(-1), rb.hilbert(d).reshape(-1)])) @ (L @ np.abs(m.reshape(-1))))
    op.close()
    print(f"K {karr} nbin {nbin}: channels |diff| / sum|terms| {abs(lhs - rhs) / scale:.2e}, full traces {abs(lhs2 - rhs2) / scale2:.2e}")
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert abs(lhs2 - rhs2) <= 1e-12 * scale2


def test_a_kmah_that_is_no_count_silences_exactly_its_pairs(rb):
    """non-integer, negative, NaN and infinite kmah: the image and the traces are those of tables without these slots"""
    T, isrc, irec, kw = KM.small_case(3, 5, True, True, True, False, seed=77)
    rng = np.random.default_rng(8)
    bad = rng.random(T.shape) < 0.08
    km = kw["kmah"].copy()
    km[bad] = rng.choice([0.5, -1.0, np.nan, np.inf, -3.0, 2.25], size=int(bad.sum()))
    N, nt = len(isrc), KM.SM_NT
    d0, d1 = rng.standard_normal((2, N, nt))
    m = rng.standard_normal((5,) + T.shape[2:])
    clean = operator(rb, T, isrc, irec, kw)
    dirty = operator(rb, T, isrc, irec, dict(kw, kmah=km))
    gone = operator(rb, np.where(bad, np.nan, T), isrc, irec, kw)
    ic, sc = clean.migrate_channels(d0, d1, stats=True)
    idy, sd = dirty.migrate_channels(d0, d1, stats=True)
    ig, sg = gone.migrate_channels(d0, d1, stats=True)
    ref, cnt = KM.migrate(T, isrc, irec, d0, d1, KM.SM_DT, **dict(kw, kmah=km))
    assert np.array_equal(idy, ig) and np.array_equal(idy, ref) and sd["contributing"] == sg["contributing"] == cnt
    assert sd["contributing"] < sc["contributing"] and not np.array_equal(idy, ic)
    (y0, y1), md = dirty.model_channels(m, stats=True)
    (g0, g1), mg = gone.model_channels(m, stats=True)
    assert np.array_equal(y0, g0) and np.array_equal(y1, g1) and md["contributing"] == mg["contributing"] == cnt
    clean.close(); dirty.close(); gone.close()


@pytest.mark.parametrize("kmah", [True, False])
def test_a_trace_of_two_windows(rb, kmah):
    """nt just above the window (2 048 samples with kmah, 4 096 without): the model runs two windows"""
    nt = 2 * 1024 + 3 if kmah else 4 * 1024 + 3
    T, isrc, irec, kw = KM.small_case(2, 0, True, False, kmah, True, seed=5, N=3, nt=nt)
    rng = np.random.default_rng(6)
    m = rng.standard_normal(T.shape[2:])
    d0, d1 = rng.standard_normal((2, 3, nt))
    L = KM.matrix(T, isrc, irec, nt, KM.SM_DT, **kw)
    ref, cnt = KM.migrate(T, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    op = operator(rb, T, isrc, irec, kw, nt=nt)
    (c0, c1), st = op.model_channels(m, stats=True)
    dref = (L @ m.reshape(-1)).reshape(2, 3, nt)
    e = max(np.max(np.abs(c0 - dref[0])), np.max(np.abs(c1 - dref[1]))) / np.max(np.abs(dref))
    j = np.nonzero(np.any(dref != 0, axis=(0, 1)))[0]
    print(f"kmah {kmah}: nt {nt}, samples hit {j.min()} .. {j.max()}, model against the matrix {e:.2e}, contributing {cnt}")
    assert j.min() < nt - 3 <= j.max()                          # both windows: the second holds the last three samples
    assert st["contributing"] == cnt and e <= 1e-12
    assert np.array_equal(op.migrate_channels(d0, d1 if kmah else None), ref[0])
    op.close()


def test_refusals_that_need_a_handle(rb):
    from raytracing_amd import _lib
    T, isrc, irec, kw = KM.small_case(2, 0, False, False, True, False, seed=1)
    d = np.zeros((len(isrc), KM.SM_NT))
    m = np.zeros(T.shape[2:])
    img = np.zeros(T.shape[2:])
    L = _lib.lib()
    op = operator(rb, T, isrc, irec, kw)
    with pytest.raises(_lib.RtmiError, match="rtmi_kirchhoff_migrate2: .*data1") as e:
        op.migrate_channels(d, None)
    assert e.value.code == -1
    assert L.rtmi_kirchhoff_model2(op._h, _lib.dptr(m), _lib.dptr(d), None, None) == -1 and b"data1" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_migrate(op._h, _lib.dptr(d), _lib.dptr(img), None) == -1 and b"migrate2" in L.rtmi_last_error()
    assert L.rtmi_kirchhoff_model(op._h, _lib.dptr(m), _lib.dptr(d), None) == -1 and b"model2" in L.rtmi_last_error()
    op.close()
    nokmah = operator(rb, T, isrc, irec, dict(kw, kmah=None))
    assert L.rtmi_kirchhoff_model2(nokmah._h, _lib.dptr(m), _lib.dptr(d), None, None) == 0      # no kmah: data1 may be NULL
    nokmah.close()
    old = rb.Kirchhoff(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT)
    assert L.rtmi_kirchhoff_migrate2(old._h, _lib.dptr(d), _lib.dptr(d), _lib.dptr(img), None) == -1
    assert b"rtmi_kirchhoff_migrate" in L.rtmi_last_error()
    with pytest.raises(ValueError, match="one arrival"):
        old.migrate_channels(d, d)
    old.close()


# ---------------------------------------------------------------- the lens bed end to end
LENS_Y = np.linspace(-0.3, 0.3, 6)
LENS_NT, LENS_DT = 1024, 0.01


@pytest.fixture(scope="module")
def lens(rb):
    x, y, Z, h = A.lens_samples()
    F = rb.Field.from_samples(x, y, Z, h)
    src = np.stack([np.full(6, A.LENS_SOURCE[0]), LENS_Y], axis=1)
    tab = rb.traveltime_table(rb.op6, F, src, A.LENS_GRID, thetas=A.LENS_THETA, step=A.LENS_STEP, max_size=A.LENS_MAX_SIZE,
                              box=A.LENS_BOX, arrivals=3, order="time", amplitude=True)
    F.close()
    s, r = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    return tab, s.reshape(-1).astype(np.int32), r.reshape(-1).astype(np.int32)


def test_lens_bed_from_tables_to_image(rb, lens):
    tab, isrc, irec = lens
    T, G, km = tab["T"], tab["G"], tab["kmah"]
    triple = (tab["count"] == 3).reshape(6, -1).sum(axis=1)
    print(f"lens bed: nodes of count 3 per position {triple.tolist()}, kmah values {np.unique(km[np.isfinite(km)]).tolist()}")
    assert T.shape == (6, 3) + (A.LENS_GRID[5], A.LENS_GRID[2]) and triple.max() >= 400
    N = len(isrc)
    rng = np.random.default_rng(12)
    d0, d1 = rng.standard_normal((2, N, LENS_NT))
    op = rb.Kirchhoff.from_table(tab, isrc, irec, LENS_NT, LENS_DT, amplitude=True)
    assert op.karr == 3 and op.has_kmah
    img, st = op.migrate_channels(d0, d1, stats=True)
    ref, cnt = KM.migrate(T, isrc, irec, d0, d1, LENS_DT, amp=G, kmah=km)
    assert np.array_equal(img, ref[0]) and st["contributing"] == cnt
    # a scatterer on a node of count 3: of every position's table if there is one, else of the best-covered position's
    every = (tab["count"] == 3).all(axis=0)
    iy, ix = np.argwhere(every if every.any() else tab["count"][int(np.argmax(triple))] == 3)[0]
    assert (tab["count"][:, iy, ix] == 3).any()
    m = np.zeros(T.shape[2:])
    m[iy, ix] = 1.0
    c0, c1 = op.model_channels(m)
    I = op.migrate_channels(c0, c1)[iy, ix]
    op.close()
    # the sum of c^2 over the contributing pairs: with the interpolation weights, and with pairs of one trace that share a sample
    # in one channel added before squaring, it is the squared norm of the matrix's column
    L = KM.matrix(T, isrc, irec, LENS_NT, LENS_DT, amp=G, kmah=km)
    col = L[:, iy * T.shape[3] + ix].toarray().reshape(-1)
    want = float(col @ col)
    pairs = sum(int((KM.pair_terms(T, isrc[k], ks, irec[k], kr, None, LENS_NT, LENS_DT, amp=G, kmah=km)[0] == iy * T.shape[3] + ix).sum())
                for k in range(N) for ks in range(3) for kr in range(3))
    print(f"scatterer at {(int(ix), int(iy))}: {pairs} contributing pairs, channel 1 share of the energy "
          f"{float(np.sum(c1 ** 2) / np.sum(c0 ** 2 + c1 ** 2)):.3f}, I(x0) {I:.12e}, sum c^2 {want:.12e}, "
          f"relative difference {abs(I - want) / want:.2e}")
    assert pairs > N and np.any(c1)
    assert abs(I - want) <= 1e-12 * want
