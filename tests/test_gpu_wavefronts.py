"""GPU: rtmi_isochrones (k_isochrone<double>, <float>) and rtmi_wavefronts (both wavefront.hip) against tests/pchip_ref.py -- scipy's
PCHIP restated in longdouble -- applied to the DEVICE's OWN rows (b.rows(), b.d_ray()): the trajectory is not in question here,
the interpolation is.  tests/test_pchip_ref.py holds the restatement to scipy and shows, on the oracle's rows of the same fans,
that they visit every derivative rule; the census is asserted again here from the rows read back.

Bound: the device within 8 x the ceiling that test_pchip_ref.py asserts for scipy against the restatement (4 eps x scale), i.e.
32 eps x scale; scale = the largest magnitude of the interpolated column over the data set, for dx/dy the largest |dx/dy| of
the wavefront.  For the angles: normal = (pi/2 - arctan(dx/dy)) - pi/2 moves by at most
the error of dx/dy (arctan's slope is <= 1) and rounds twice at the size of pi, and angle_diff subtracts the ray angle, so their
scale is max |dx/dy| + pi + max |ray angle|.  Where an evaluation lands on a recorded point, s = 0 in the interval that starts
there, and both the power sum (k_isochrone, scipy) and Horner's form (k_fine) are that point's value plus exact zeros, so
there the test asks for the SAME BITS.  A column that is finite in the restatement must be finite on the device, entry by entry.

Measured on an MI355X, largest device - restatement in eps x scale (the build does not contract to FMA):
  per-ray values 1.71     dx/dy 2.00     normal, angle_diff 0.37     x_fine 1.24     y_fine 0 (numpy.linspace's bits)
Before rtmi_wavefronts flagged ties (k_ties) the tie tests failed with a finite dx/dy = 0 at the tied points."""
import numpy as np
import pytest

import pchip_ref as P
from conftest import LIMITS, golden

pytestmark = pytest.mark.gpu
BOUND = P.DEVICE_BOUND          # eps x scale
NEAR_SHARE = 1e-3               # entries that pchip_ref.near_guard marks may be left out, up to this share
COLS = (0, 1, 5)                # x, y, theta of a row


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    cache = {}

    def get(scen, width="f64"):
        if (scen, width) not in cache:
            cache[scen, width] = rb.Field.build(scen, LIMITS[scen], rb.DELTA, rb.F64 if width == "f64" else rb.F32)
        return cache[scen, width]
    yield get
    for F in cache.values():
        F.close()


def _launch(fan):
    """-> scenario, step, max_size, box, x0, y0, theta of a fan of pchip_ref"""
    if fan == "F":
        F = P.F_FAN
        return F["scen"], F["step"], F["max_size"], LIMITS["fisheye"], F["x0"], F["y0"], F["theta"]
    g = golden(P.I_FAN["fixture"])
    return P.I_FAN["scen"], float(g["step"]), int(g["max_size"]), g["box"], g["pos_x"], P.I_FAN["y0"], g["theta"]


def _batch(rb, fields, fan, width="f64", cut=0, theta=None, **kw):
    scen, step, max_size, box, x0, y0, th = _launch(fan)
    th = th if theta is None else theta
    x0 = x0 if np.ndim(x0) == 0 else np.resize(x0, len(th))
    b = rb.Batch(fields(scen, width), 6, step, max_size, box, 1, th, x0, y0, record_stride=1, rec_rows=cut, **kw)
    b.run()
    return b


def _err(dev, ref, scale):
    """|dev - ref| in eps x scale, elementwise; 0 where both are NaN"""
    d = np.abs(np.asarray(dev, dtype=P.LD) - ref) / (P.EPS * scale)
    return np.where(np.isnan(np.asarray(ref, dtype=np.float64)) & np.isnan(dev), 0.0, d.astype(np.float64))


def _compare_per_ray(pts, rows, nrow, times):
    """the device's isochrone points against the restatement on the same rows -> (worst eps x scale, labels)"""
    val, lab, near = P.fan_isochrones(rows, nrow, times)
    assert pts.shape == val.shape
    assert np.array_equal(np.isnan(pts), np.isnan(val.astype(np.float64)))          # the same rays reach the same times
    scale = np.array([[np.abs(rows[:nrow[k], q, k]).max() for k in range(rows.shape[2])] for q in COLS])
    err = _err(pts, val, scale[None])
    assert near.sum() <= NEAR_SHARE * near.size
    worst = float(err[~near].max())
    assert worst <= BOUND, np.argwhere(~(err <= BOUND))[:5]          # ~(<=): a NaN fails too
    return worst, lab


PER_RAY = [(f, c, w, False) for f, cuts in (("F", P.F_FAN["cuts"]), ("I", P.I_FAN["cuts"])) for c in (0,) + cuts for w in ("f64", "f32")]
PER_RAY.append(("F", 0, "f64", True))


@pytest.mark.parametrize("fan,cut,width,shuffled", PER_RAY, ids=[f"{f}-{c or 'full'}-{w}{'-sorted' if s else ''}" for f, c, w, s in PER_RAY])
def test_isochrones_equal_the_restatement_on_the_device_rows(fan, cut, width, shuffled, rb, fields):
    """Every entry of [ntimes, 3, R] at pchip_ref.time_list's times -- each ray's first, last and one middle recorded T exactly,
    the midpoints of its end intervals and of the intervals either side of its slope flips and flat stretches -- for the full
    record and for records cut to 2 (the straight line), 3 (both end rules in every interval), 60, 79 and 150 rows, fp64 and
    fp32, and once on shuffled rays that the batch sorts."""
    theta = np.random.default_rng(5).permutation(_launch(fan)[6]) if shuffled else None
    b = _batch(rb, fields, fan, width, cut, theta, sort_rays=shuffled)
    rows, last = b.rows(), b.d_ray()[2]
    R = rows.shape[2]
    nrow = P.ray_lengths(last, rows.shape[0])
    assert nrow.min() >= 2 and (cut == 0 or nrow.max() == cut)
    times = P.time_list(rows, nrow)
    assert 0 < len(times) <= 4096
    k = np.arange(R)
    T0, Tmid, Tend = rows[0, 4], rows[nrow // 2, 4, k], rows[nrow - 1, 4, k]
    pts = b.isochrones(times)
    above = b.isochrones(np.nextafter(Tend, np.inf))
    below = b.isochrones(np.nextafter(T0, -np.inf))
    b.close()
    worst, lab = _compare_per_ray(pts, rows, nrow, times)
    worst = max(worst, _compare_per_ray(above, rows, nrow, np.nextafter(Tend, np.inf))[0])
    print(f"isochrones {fan} cut {cut} {width}: device - restatement {worst:.2f} eps*scale, census {P.census(lab)}")
    # one ulp beyond either end of a ray's record is outside it; the ends themselves are inside
    assert np.isnan(above[k, :, k]).all() and np.isnan(below[k, :, k]).all()
    for q, c in zip(COLS, range(3)):
        at0, atm, ate = (pts[np.searchsorted(times, T), c, k] for T in (T0, Tmid, Tend))
        assert np.array_equal(at0, rows[0, q]), "t == T[0] is the first row"
        inner = nrow // 2 < nrow - 1
        assert np.array_equal(atm[inner], rows[nrow // 2, q, k][inner]), "t == T[j] is row j"
        scale = np.array([np.abs(rows[:nrow[r], q, r]).max() for r in k])
        assert np.isfinite(ate).all() and _err(ate, rows[nrow - 1, q, k].astype(P.LD), scale).max() <= BOUND
    cen = P.census(lab)
    if cut == 2:            # two rows: the straight line between them
        assert set(cen) == {"two"}
        r0, r1 = rows[0].astype(P.LD), rows[1].astype(P.LD)
        for c, q in enumerate(COLS):
            line = r0[q] + (r1[q] - r0[q]) / (r1[4] - r0[4]) * (times.astype(P.LD)[:, None] - r0[4])
            ok = ~np.isnan(pts[:, c])
            assert _err(pts[:, c], line, np.maximum(np.abs(rows[0, q]), np.abs(rows[1, q])))[ok].max() <= BOUND
    if width == "f64":      # the rules this case is here for were visited (floors: half of what the oracle's rows give)
        P.assert_census_floors(cen, fan, cut)


# ------------------------------------------------------------------ across rays
@pytest.fixture(scope="module")
def full(rb, fields):
    """fan -> (the traced fp64 batch, its isochrone points at the fan's times), kept for the tests below"""
    cache = {}

    def get(fan):
        if fan not in cache:
            b = _batch(rb, fields, fan)
            cache[fan] = (b, b.isochrones((P.F_FAN if fan == "F" else P.I_FAN)["times"]))
        return cache[fan]
    yield get
    for b, _ in cache.values():
        b.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _take(worst, key, dev, ref, scale):
    """worst[key] <- the largest |dev - ref| in eps x scale of a column that is finite in the restatement: the device's must be
    finite too, entry by entry (a NaN would otherwise drop out of every max), and of the same length"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape and np.isfinite(ref.astype(np.float64)).all(), key
    assert np.isfinite(dev).all(), (key, "not finite on the device, finite in the restatement", np.nonzero(~np.isfinite(dev))[0][:5])
    if not scale:                   # every entry of the restatement is 0 (a flat wavefront's dx/dy): 0 under any rounding
        assert not np.any(dev), key
        return
    e = float(np.abs(dev.astype(P.LD) - ref).max() / (P.EPS * scale))
    assert e == e, key
    worst[key] = max(worst[key], e)


def _compare_wavefront(w, iso_t, nfine, worst):
    """one wavefront of the device against the restatement on the isochrone points iso_t [3, R] it was made from; -> the
    restatement, or None where near_guard lets the derived columns be left out"""
    have = nfine and w["count"] >= 2
    ref = P.wavefront(iso_t[0], iso_t[1], iso_t[2], nfine, y_fine=w["y_fine"] if have else None)
    assert w["count"] == ref["count"]
    assert np.array_equal(w["ray"], ref["ray"])                                   # the stable argsort, keys of either sign
    for key, col in (("x", 0), ("y", 1), ("angle", 2)):
        assert _bits(w[key], iso_t[col, ref["ray"]]), key
    if ref["count"] < 2:
        assert all(len(w[key]) == 0 for key in ("dxdy", "normal", "angle_diff", "x_fine", "y_fine"))
        return ref
    if ref["tie"]:
        for key in ("dxdy", "normal", "angle_diff"):
            assert len(w[key]) == ref["count"] and np.isnan(w[key]).all(), key
        assert nfine == 0 or (len(w["x_fine"]) == nfine and np.isnan(w["x_fine"]).all() and np.isnan(w["y_fine"]).all())
        return ref
    if nfine:
        lin = np.linspace(w["y"][0], w["y"][-1], nfine)
        _take(worst, "y_fine", w["y_fine"], lin.astype(P.LD), np.abs(w["y"]).max())
        assert w["y_fine"][0] == w["y"][0] and w["y_fine"][-1] == w["y"][-1]
    if ref["near"]:                 # an end-rule decision on its threshold: the values may differ, NaN they may not be
        assert all(np.isfinite(w[key]).all() and len(w[key]) == ref["count"] for key in ("dxdy", "normal", "angle_diff"))
        assert not nfine or np.isfinite(w["x_fine"]).all()
        return None
    sd = float(np.abs(ref["dxdy"]).max())
    sa = sd + np.pi + np.abs(w["angle"]).max()
    _take(worst, "dxdy", w["dxdy"], ref["dxdy"], sd)                             # sd == 0: a flat wavefront, dx/dy is 0 exactly
    _take(worst, "angles", w["normal"], ref["normal"], sa)
    _take(worst, "angles", w["angle_diff"], ref["angle_diff"], sa)
    if nfine:
        _take(worst, "x_fine", w["x_fine"], ref["x_fine"], np.abs(w["x"]).max())
        hit = np.nonzero(np.isin(w["y_fine"][:-1], w["y"][:-1]))[0]             # on a point (not the last): that point's x, exactly
        assert np.array_equal(w["x_fine"][hit], w["x"][np.searchsorted(w["y"], w["y_fine"][hit])])
    return ref


def _new_worst():
    return dict(dxdy=0.0, angles=0.0, x_fine=0.0, y_fine=0.0)


def _assert_worst(worst, what):
    print(f"wavefronts {what}: device - restatement, eps*scale: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= BOUND for v in worst.values()), worst                       # a NaN fails


@pytest.mark.parametrize("nfine", [2, 100, 257])
@pytest.mark.parametrize("fan", ["F", "I"])
def test_wavefronts_equal_the_restatement_on_the_device_points(fan, nfine, full):
    """count, the stable order by y (keys of both signs on I), y, x, angle bit for bit the isochrone stage's, and dx/dy -- the
    last point's from PPoly.derivative() on the last interval --, normal, angle_diff and the fine curve within the bound: F at 36
    times (179 sign flips between neighbouring rays, points 1.4e-6 apart in y), I at 40 (the 0 and the 3 m0 guard at wavefront
    ends, twelve two-point wavefronts)."""
    b, iso = full(fan)
    times = (P.F_FAN if fan == "F" else P.I_FAN)["times"]
    wf = b.wavefronts(times, nfine=nfine)
    assert len(wf) == len(times)
    worst, cen, two, both, skipped, drawn = _new_worst(), {}, 0, 0, 0, 0
    for it, w in enumerate(wf):
        ref = _compare_wavefront(w, iso[it], nfine, worst)
        if ref is None:
            skipped += 1
            continue
        assert not ref["tie"]
        if ref["count"] < 2:
            continue
        drawn += 1
        for lab, c in P.census(ref["label"]).items():
            cen[lab] = cen.get(lab, 0) + c
        two += ref["count"] == 2
        both += bool(w["y"][0] < 0 < w["y"][-1])
    _assert_worst(worst, f"{fan} nfine {nfine} (census {cen}, two-point {two}, y of both signs {both})")
    assert drawn >= 30 and skipped <= NEAR_SHARE * len(wf)
    P.assert_census_floors(cen, fan, "across")
    if fan == "I":
        assert 2 * two >= P.I_ACROSS_TWO_POINT and 2 * both >= P.I_ACROSS_BOTH_SIGNS


def test_wavefronts_chunked_and_without_a_fine_curve(full, monkeypatch):
    b, _ = full("I")
    times = P.I_FAN["times"]
    wf = b.wavefronts(times, nfine=100)
    none = b.wavefronts(times, nfine=0)
    monkeypatch.setenv("RTMI_WF_CHUNK", "7")                                      # 40 times: five chunks of 7 and one of 5
    chunked = b.wavefronts(times, nfine=100)
    monkeypatch.delenv("RTMI_WF_CHUNK")
    for w, c, z in zip(wf, chunked, none):
        assert w["count"] == c["count"] == z["count"]
        for key in ("ray", "y", "x", "angle", "dxdy", "normal", "angle_diff", "x_fine", "y_fine"):
            assert _bits(w[key], c[key]), key
            if "fine" in key:
                assert len(z[key]) == 0
            else:
                assert _bits(w[key], z[key]), key


def _launch_point_wavefront(rb, fields, y0, x0, nfine, later=False):
    """A wavefront whose points the caller sets: with two rows kept the isochrone stage returns row 0 at t = T[0] = 0, and row 0
    is the launch point.  -> the device's wavefronts at t = 0 (and, if asked, halfway to the nearest second row), their
    isochrone points"""
    y0, x0 = np.asarray(y0, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    scen = "vert_heterogeneous"
    b = rb.Batch(fields(scen), 6, rb.DELTA_S, 4, LIMITS[scen], 1, np.linspace(0.3, 1.2, len(y0)), x0, y0, record_stride=1, rec_rows=2)
    b.run()
    rows = b.rows()
    assert np.all(b.d_ray()[2] >= 1) and np.all(rows[0, 4] == 0) and np.all(rows[1, 4] > 0)
    times = [0.0, 0.5 * rows[1, 4].min()] if later else [0.0]
    wf, iso = b.wavefronts(times, nfine=nfine), b.isochrones(times)
    b.close()
    assert np.array_equal(iso[0, 0], x0) and np.array_equal(iso[0, 1], y0)        # == : the sign of a zero is not asked for
    return wf, iso


def test_wavefronts_through_caller_set_points_take_every_rule(rb, fields):
    """pchip_ref.RULE_SETS -- every derivative rule at n = 2, 3, 4, unequal spacings -- scaled into the medium and launched as
    rays in shuffled order, and one 40-point set whose every point the 129-point fine curve lands on."""
    worst, seen = _new_worst(), set()
    for i, (t, v, _) in enumerate(P.RULE_SETS):
        perm = np.random.default_rng(i).permutation(len(t))
        y0, x0 = (0.125 * np.array(t) - 0.5)[perm], (0.0625 * np.array(v) + 1.0)[perm]
        for nfine in (2, 33):
            wf, iso = _launch_point_wavefront(rb, fields, y0, x0, nfine)
            ref = _compare_wavefront(wf[0], iso[0], nfine, worst)
            assert ref is not None and not ref["tie"] and np.array_equal(ref["ray"], np.argsort(perm))
            seen |= set(ref["label"])
    assert seen == set(P.LABELS)
    # every point on the device's own 129-point abscissae (numpy.linspace's bits), unequally spaced, x rough: a fine abscissa that
    # lands on a point belongs to the interval that STARTS there, whose polynomial is that point's x plus exact zeros; the
    # interval before would give it back only to a rounding
    rng = np.random.default_rng(11)
    idx = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 128), 38, replace=False)), [128]])
    y0, x0 = np.linspace(-1.3, 0.41, 129)[idx], rng.uniform(-1.5, 4.5, 40)
    perm = rng.permutation(40)
    wf, iso = _launch_point_wavefront(rb, fields, y0[perm], x0[perm], 129)
    ref = _compare_wavefront(wf[0], iso[0], 129, worst)
    assert ref is not None and P.census(ref["label"]).get("flip", 0) >= 10
    on = np.isin(wf[0]["y_fine"], y0[:-1])
    assert on.sum() == 39 and _bits(wf[0]["x_fine"][on], x0[:-1])
    _assert_worst(worst, "caller-set points")


TIES = [([-0.5, -0.0, 0.0, 0.3], [0, 1, 2, 3]),             # -0.0 and +0.0 are one y
        ([0.2, -0.4, 0.2], [1, 0, 2]),
        ([-1.0, -1.0], [0, 1]),
        ([0.1, 0.1, 0.1, -0.3, 0.4], [3, 0, 1, 2, 4])]


@pytest.mark.parametrize("y0,order", TIES, ids=[f"n{len(t[0])}" for t in TIES])
def test_wavefront_with_equal_y_has_no_interpolant(y0, order, rb, fields):
    """Two points of one y make scipy raise for the whole data set: count, y, x, angle and ray as ever (equal keys in the
    callers' order), dx/dy, normal, angle_diff and the fine curve NaN at EVERY point -- and the wavefront of the same call a
    little later, on which the rays have moved apart, is whole."""
    x0 = 1.0 + 0.37 * np.arange(len(y0))
    wf, iso = _launch_point_wavefront(rb, fields, y0, x0, 17, later=True)
    worst = _new_worst()
    ref = _compare_wavefront(wf[0], iso[0], 17, worst)
    assert ref["tie"] and list(wf[0]["ray"]) == order and len(wf[0]["dxdy"]) == len(y0)
    ref = _compare_wavefront(wf[1], iso[1], 17, worst)
    assert ref is not None and not ref["tie"] and np.isfinite(wf[1]["dxdy"]).all() and np.isfinite(wf[1]["x_fine"]).all()
    _assert_worst(worst, "after a tie")


def test_ray_launched_twice_ties_the_wavefronts_it_reaches_and_no_other(rb, fields, full):
    """F with theta[10] once more as ray 64: two bit-identical points on every wavefront that the pair reaches, which then has
    no interpolant; the wavefronts it does not reach are those of the fan without it, bit for bit."""
    b1, _ = full("F")
    times = P.F_FAN["times"]
    plain = b1.wavefronts(times, nfine=100)
    b = _batch(rb, fields, "F", theta=np.append(P.F_FAN["theta"], P.F_FAN["theta"][10]))
    wf, iso = b.wavefronts(times, nfine=100), b.isochrones(times)
    b.close()
    tied = whole = 0
    worst = _new_worst()
    for it, (w, p) in enumerate(zip(wf, plain)):
        assert _bits(iso[it, :, 10], iso[it, :, 64])
        ref = _compare_wavefront(w, iso[it], 100, worst)
        assert ref is not None, "no end-rule decision of this fan lies near its threshold (test_pchip_ref.py)"
        if np.isnan(iso[it, 1, 10]):
            whole += 1
            assert w["count"] == p["count"] and not ref["tie"]
            for key in ("ray", "y", "x", "angle", "dxdy", "normal", "angle_diff", "x_fine", "y_fine"):
                assert _bits(w[key], p[key]), (it, key)
        else:
            tied += 1
            j = list(w["ray"]).index(10)
            assert ref["tie"] and w["count"] == p["count"] + 1 and w["ray"][j + 1] == 64
            assert np.isnan(w["dxdy"]).all() and np.isnan(w["angle_diff"]).all() and np.isnan(w["x_fine"]).all()
    assert tied >= 1 and whole >= 1
    _assert_worst(worst, "F with a ray launched twice")
