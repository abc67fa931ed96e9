"""CPU: tests/pchip_ref.py (the longdouble restatement of scipy's PCHIP that tests/test_gpu_wavefronts.py holds the device
to) against scipy itself, and the proof that the fans of that GPU test visit every derivative rule: the census of the rules
on the oracle's rows of the same fans, none of the end-rule decisions within 2^-40 of its threshold.

scipy against the restatement, in eps x scale, over everything below (asserted <= pchip_ref.SCIPY_CEILING = 4): per-ray
values 1.47, dx/dy 2.00, x_fine 1.20 on the fans."""
import numpy as np
import pytest
from scipy.interpolate import PchipInterpolator

import pchip_ref as P
from conftest import LIMITS, golden

EPS = P.EPS


def _eps_scale(a, b, scale):
    """largest |a - b| in units of eps x scale"""
    worst = float(np.max(np.abs(np.asarray(a, dtype=P.LD) - np.asarray(b, dtype=P.LD)))) if len(a) else 0.0
    return worst / (EPS * scale) if worst else 0.0


SETS = P.RULE_SETS


@pytest.mark.parametrize("t,v,rules", SETS, ids=[f"n{len(s[0])}-{'-'.join(s[2])}" for s in SETS])
def test_restatement_on_sets_that_take_every_rule(t, v, rules):
    t, v = np.array(t), np.array(v)
    d, lab, near = P.derivatives(t, v)
    assert list(lab) == rules and not near.any()
    sp = PchipInterpolator(t, v)
    scale = np.abs(v).max()
    q = np.unique(np.concatenate([t, np.linspace(t[0], t[-1], 257), 0.5 * (t[1:] + t[:-1]), np.nextafter(t[1:], -np.inf)]))
    assert _eps_scale(sp(q), P.evaluate(t, v, d, q), scale) <= P.SCIPY_CEILING
    # the derivative between the points is a sum of three terms that cancel: each rounds at its own size, so that is the scale
    c0, c1, c2, _ = P.coefficients(t.astype(P.LD), v.astype(P.LD), d, np.arange(len(t) - 1))
    dx = np.diff(t)
    terms = float(np.max(np.abs(c2) + 2 * np.abs(c1) * dx + 3 * np.abs(c0) * dx * dx))
    assert _eps_scale(sp.derivative()(q), P.evaluate(t, v, d, q, nu=1), terms) <= P.SCIPY_CEILING
    dscale = float(np.abs(P.evaluate(t, v, d, t, nu=1)).max())                       # at the points: the largest |dx/dy| there
    # the reach rule of the isochrone stage; labels of the interval each time falls in
    val, il, _ = P.isochrone(t, v, np.array([np.nextafter(t[0], -np.inf), t[0], t[-1], np.nextafter(t[-1], np.inf)]))
    assert np.isnan(val[0]) and np.isnan(val[3]) and val[1] == v[0] and abs(float(val[2]) - v[-1]) <= 4 * EPS * scale
    assert list(il[1]) == rules[:2] and list(il[2]) == rules[-2:] and not il[0].any() and not il[3].any()
    # ... and the across-ray stage on the same numbers, handed over in shuffled order with a ray that does not arrive
    perm = np.random.default_rng(len(t)).permutation(len(t) + 1)
    yy, xx = np.append(t, np.nan)[perm], np.append(v, np.nan)[perm]
    w = P.wavefront(xx, yy, 0.1 * xx, 33)
    assert w["count"] == len(t) and np.array_equal(perm[w["ray"]], np.arange(len(t))) and not w["tie"]
    assert list(w["label"]) == rules
    assert _eps_scale(sp.derivative()(t), w["dxdy"], dscale) <= P.SCIPY_CEILING
    assert np.array_equal(w["y_fine"], np.linspace(t[0], t[-1], 33))
    assert _eps_scale(sp(w["y_fine"]), w["x_fine"], scale) <= P.SCIPY_CEILING
    assert np.array_equal(w["normal"], (P.LD(np.pi) / 2 - np.arctan(w["dxdy"])) - P.LD(np.pi) / 2)


def test_near_guard_marks_a_decision_on_its_threshold_and_no_other():
    t = np.array([0.0, 1.0, 2.0])
    assert P.near_guard(t, np.array([0.0, 1.0, 4.0])) == (True, False)            # d = (3 - 3) / 2: exactly on 0
    assert P.near_guard(t, np.array([0.0, 1.0, 4.0 + 1e-9])) == (False, False)    # 5e-10 of 3 away: far, in these terms
    assert P.near_guard(t, np.array([0.0, 1.0, 4.0 + 1e-13]))[0]                  # 2^-44 of it: near
    assert P.near_guard(t, np.array([0.0, 1.0, -2.0])) == (True, False)           # d = (3 + 3) / 2 = 3 m0 exactly
    assert P.near_guard(t, np.array([0.0, 1.0, -2.0 - 1e-9])) == (False, False)
    assert P.near_guard(t, np.array([1.0, 1.0, 1.0])) == (False, False)           # m0 = m1 = 0: every rounding gives 0
    assert P.near_guard(t, np.array([1.0, 1.0, 7.0])) == (False, False)           # m0 = 0: the guard gives 0 whatever d's bits
    assert P.near_guard(t[:2], np.array([1.0, 2.0])) == (False, False)


def test_ties_are_flagged_and_give_nan_throughout():
    y = np.array([0.3, -0.0, 0.0, np.nan, -1.0])
    w = P.wavefront(np.arange(5.0), y, np.zeros(5), 7)
    assert w["tie"] and w["count"] == 4 and list(w["ray"]) == [4, 1, 2, 0]        # stable: -0.0 before +0.0 as handed over
    for key in ("dxdy", "normal", "angle_diff", "x_fine", "y_fine"):
        assert np.isnan(w[key]).all() and len(w[key]) == (7 if "fine" in key else 4)
    one = P.wavefront(np.arange(5.0), np.where(np.arange(5) == 2, 1.0, np.nan), np.zeros(5), 7)
    assert one["count"] == 1 and len(one["dxdy"]) == 0 and len(one["x_fine"]) == 0 and not one["tie"]


def test_restatement_on_the_committed_isochrone_and_wavefront_fixtures():
    """The reference's own scipy results: the per-ray stage is in isochrones_vert_op6 only as results (the rows are not), so it
    is the across-ray stage that is restated from fixture data here -- x(y) of wavefronts_* from their sorted points."""
    seen = 0
    for name in ("wavefronts_vert_op6", "wavefronts_aniso_op11"):
        g = golden(name)
        for it in range(len(g["times"])):
            n = int(g[f"count{it}"])
            if n < 2:
                continue
            y, x = g[f"y{it}"], g[f"x{it}"]
            w = P.wavefront(x, y, g[f"angle_rayorder{it}"], 100)
            assert w["count"] == n and np.array_equal(w["ray"], np.arange(n)) and not w["tie"] and not w["near"]
            assert _eps_scale(g[f"dxdy{it}"], w["dxdy"], np.abs(g[f"dxdy{it}"]).max()) <= P.SCIPY_CEILING
            assert _eps_scale(g[f"x_fine{it}"], w["x_fine"], np.abs(x).max()) <= P.SCIPY_CEILING
            assert np.array_equal(g[f"y_fine{it}"], w["y_fine"])
            assert _eps_scale(g[f"normal{it}"], w["normal"], np.abs(g[f"dxdy{it}"]).max() + np.pi) <= P.SCIPY_CEILING
            seen += 1
    assert seen >= 16
    g = golden("isochrones_vert_op6")
    pts = g["points"]
    for it in range(len(g["times"])):                     # ... and its points, as one more set of across-ray data
        w = P.wavefront(pts[it, 0], pts[it, 1], pts[it, 2], 100)
        if w["count"] >= 2:
            sp = PchipInterpolator(w["y"], w["x"])
            assert _eps_scale(sp(w["y_fine"]), w["x_fine"], np.abs(w["x"]).max()) <= P.SCIPY_CEILING


# ------------------------------------------------------------------ the fans of tests/test_gpu_wavefronts.py, on the oracle's rows
@pytest.fixture(scope="module")
def fans(oracle_fields):
    """name -> (rows [rec_rows, 6, R], last row of each ray), traced by the oracle once"""
    from oracle import rt_oracle as O
    F, g = P.F_FAN, golden(P.I_FAN["fixture"])
    f = O.trazar(oracle_fields("fisheye"), F["method"], 1, F["step"], F["max_size"], LIMITS["fisheye"], F["x0"], F["y0"], F["theta"])
    i = O.trazar(oracle_fields("interface"), P.I_FAN["method"], 1, float(g["step"]), int(g["max_size"]), g["box"], g["pos_x"],
                 P.I_FAN["y0"], g["theta"])
    return {"F": (f["s_ray"], f["d_ray"][2]), "I": (i["s_ray"], i["d_ray"][2])}


def _through_float32(rows):
    return rows.astype(np.float32).astype(np.float64)


def _per_ray(rows, last, cut):
    rec = cut or rows.shape[0]
    nrow = P.ray_lengths(last, rec)
    times = P.time_list(rows[:rec], nrow)
    assert 0 < len(times) <= 4096
    return nrow, times, P.fan_isochrones(rows[:rec], nrow, times)


CASES = [(f, c, w) for f, cuts in (("F", P.F_FAN["cuts"]), ("I", P.I_FAN["cuts"])) for c in (0,) + cuts for w in ("f64", "f32")]


@pytest.mark.parametrize("fan,cut,width", CASES, ids=[f"{f}-{c or 'full'}-{w}" for f, c, w in CASES])
def test_per_ray_stage_on_the_fans(fan, cut, width, fans):
    """Every entry of the isochrone stage at the time list of the GPU test: scipy (RT_bench.py:993-1001) against the restatement,
    the census of the derivative rules behind the entries, and no end-rule decision near its threshold."""
    rows, last = fans[fan]
    if width == "f32":
        rows = _through_float32(rows)
    nrow, times, (val, lab, near) = _per_ray(rows, last, cut)
    worst = 0.0
    for k in range(rows.shape[2]):
        n = int(nrow[k])
        T = rows[:n, 4, k]
        ok = (T[0] <= times) & (times <= T[n - 1])
        assert np.array_equal(~np.isnan(val[:, 0, k].astype(np.float64)), ok) and ok.sum() >= 5
        for c, q in enumerate((0, 1, 5)):
            ref = PchipInterpolator(T, rows[:n, q, k])(times[ok])
            worst = max(worst, _eps_scale(ref, val[ok, c, k], np.abs(rows[:n, q, k]).max()))
    print(f"per-ray {fan} cut {cut} {width}: scipy - restatement {worst:.2f} eps*scale, census {P.census(lab)}, near {near.sum()}")
    assert worst <= P.SCIPY_CEILING
    assert not near.any()
    cen = P.census(lab)
    if cut == 2:
        assert set(cen) == {"two"}
    if cut == 3:
        assert set(cen) <= {"plain", "zero", "3m0", "mean", "flip", "flat"}     # both end rules meet in every interval
    if width == "f64":
        P.assert_census_floors(cen, fan, cut)


def _across(rows, last, times, nfine=100):
    nrow = P.ray_lengths(last, rows.shape[0])
    iso = P.fan_isochrones(rows, nrow, times)[0].astype(np.float64)
    return iso, [P.wavefront(iso[it, 0], iso[it, 1], iso[it, 2], nfine) for it in range(len(times))]


@pytest.mark.parametrize("fan", ["F", "I"])
def test_across_ray_stage_on_the_fans(fan, fans):
    """The wavefronts of the GPU test's traveltimes through the oracle's isochrone points: np.argsort + scipy
    (RT_bench.py:1016-1022, 1043-1044) against the restatement, the census of the rules, no tie, nothing near a threshold."""
    rows, last = fans[fan]
    times = (P.F_FAN if fan == "F" else P.I_FAN)["times"]
    iso, wfs = _across(rows, last, times)
    cen, two, both, dymin, worst = {}, 0, 0, np.inf, dict(dxdy=0.0, x_fine=0.0)
    for it, w in enumerate(wfs):
        assert not w["tie"] and not w["near"]
        if w["count"] < 2:
            continue
        ok = ~np.isnan(iso[it, 1])
        assert np.array_equal(w["ray"], np.nonzero(ok)[0][np.argsort(iso[it, 1, ok], kind="stable")])
        sp = PchipInterpolator(w["y"], w["x"])
        worst["dxdy"] = max(worst["dxdy"], _eps_scale(sp.derivative()(w["y"]), w["dxdy"], float(np.abs(w["dxdy"]).max())))
        worst["x_fine"] = max(worst["x_fine"], _eps_scale(sp(w["y_fine"]), w["x_fine"], np.abs(w["x"]).max()))
        for lab, c in P.census(w["label"]).items():
            cen[lab] = cen.get(lab, 0) + c
        two += w["count"] == 2
        both += bool(w["y"][0] < 0 < w["y"][-1])
        dymin = min(dymin, np.diff(w["y"]).min())
    print(f"across {fan}: scipy - restatement {worst}, census {cen}, two-point {two}, both signs {both}, least dy {dymin:.2e}")
    assert max(worst.values()) <= P.SCIPY_CEILING
    P.assert_census_floors(cen, fan, "across")
    if fan == "I":
        assert 2 * two >= P.I_ACROSS_TWO_POINT and 2 * both >= P.I_ACROSS_BOTH_SIGNS
    else:
        assert 0 < dymin < 1e-4
