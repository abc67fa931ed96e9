"""numpy restatement, in np.longdouble, of what rtmi_isochrones and rtmi_wavefronts (wavefront.hip, through rt_pchip.h)
restate in fp64: scipy 1.15.3's PchipInterpolator -- _find_derivatives and _edge_case, CubicHermiteSpline's power-basis
coefficients, PPoly's evaluation (a sum of powers of t - T_j, lowest first) and PPoly.derivative().  Test infrastructure.

Every function is vectorised over the evaluation points of ONE data set.  Besides the numbers it says which derivative rule
gave each of them, so that a test can prove that its inputs visit a rule:
  interior points   'mean'   Fritsch-Butland weighted harmonic mean
                    'flip'   the two neighbouring slopes differ in sign -> 0
                    'flat'   one of them is zero -> 0
  end points        'plain'  the three-point formula as it comes
                    'zero'   its sign differs from the end slope's -> 0
                    '3m0'    the two slopes differ in sign and |d| > 3 |m0| -> 3 m0
  two points        'two'    the straight line"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
LABELS = ("mean", "flip", "flat", "plain", "zero", "3m0", "two")
NEAR = 2.0 ** -40           # near_guard's relative distance


def _edge(h0, h1, m0, m1):
    """_edge_case for one end -> (d, label, near): near as near_guard defines it"""
    d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    size = (abs((2 * h0 + h1) * m0) + abs(h0 * m1)) / (h0 + h1)          # what d is the difference of
    differ = np.sign(m0) != np.sign(m1)
    if m0 == 0:                                                          # 0 under any rounding of d (m1 == 0: d is 0; else sgn(d) != 0)
        return LD(0), "zero" if m1 != 0 else "plain", False
    near = bool(abs(d) <= NEAR * size or (differ and abs(abs(d) - 3 * abs(m0)) <= NEAR * 3 * abs(m0)))
    if np.sign(d) != np.sign(m0):
        return LD(0), "zero", near
    if differ and abs(d) > 3 * abs(m0):
        return 3 * m0, "3m0", near
    return d, "plain", near


def derivatives(t, v):
    """_find_derivatives -> (d [n] longdouble, label [n], near [n]) for the strictly increasing abscissae t, n >= 2"""
    t, v = np.asarray(t, dtype=LD), np.asarray(v, dtype=LD)
    n = len(t)
    h = t[1:] - t[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (v[1:] - v[:-1]) / h
    lab = np.empty(n, dtype="U5")
    near = np.zeros(n, dtype=bool)
    if n == 2:
        lab[:] = "two"
        return np.array([m[0], m[0]]), lab, near
    flat = (m[1:] == 0) | (m[:-1] == 0)
    flip = np.sign(m[1:]) != np.sign(m[:-1])
    w1, w2 = 2 * h[1:] + h[:-1], h[1:] + 2 * h[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = 1 / ((w1 / m[:-1] + w2 / m[1:]) / (w1 + w2))
    d = np.zeros(n, dtype=LD)
    d[1:-1] = np.where(flat | flip, LD(0), mean)
    lab[1:-1] = np.where(flat, "flat", np.where(flip, "flip", "mean"))
    d[0], lab[0], near[0] = _edge(h[0], h[1], m[0], m[1])
    d[-1], lab[-1], near[-1] = _edge(h[-1], h[-2], m[-1], m[-2])
    return d, lab, near


def near_guard(t, v):
    """(first, last): whether the end rule's guard quantity at that end of the data set (t, v) lies within 2^-40 (relative) of
    its threshold -- d against 0, relative to the two products it is the difference of, and |d| against 3 |m0| where the two
    slopes differ in sign -- so that fp64 and this module may fairly take different branches there.  An end slope of exactly 0
    gives 0 under every rounding and is near nothing; neither is a two-point set, which has no end rule."""
    near = derivatives(t, v)[2]
    return bool(near[0]), bool(near[-1])


def _interval(t, q):
    """PPoly's interval of each q in [t[0], t[n-1]]: t[i] <= q < t[i+1], the last one closed on the right"""
    return np.clip(np.searchsorted(t, q, side="right") - 1, 0, len(t) - 2)


def coefficients(t, v, d, i):
    """CubicHermiteSpline's c[0..3] of the intervals i"""
    dx = t[i + 1] - t[i]
    slope = (v[i + 1] - v[i]) / dx
    tq = (d[i] + d[i + 1] - 2 * slope) / dx
    return tq / dx, (slope - d[i]) / dx - tq, d[i], v[i]


def evaluate(t, v, d, q, nu=0):
    """PPoly(c, t)(q, nu) for nu = 0, 1 through CubicHermiteSpline's coefficients; q within [t[0], t[n-1]]"""
    t, v, q = np.asarray(t, dtype=LD), np.asarray(v, dtype=LD), np.asarray(q, dtype=LD)
    i = _interval(t, q)
    c0, c1, c2, c3 = coefficients(t, v, d, i)
    s = q - t[i]
    if nu == 0:
        return c3 + c2 * s + c1 * (s * s) + c0 * (s * s * s)
    return c2 + 2 * c1 * s + 3 * c0 * (s * s)


def isochrone(T, Y, t):
    """One ray's recorded column Y [n] over its traveltimes T [n] at the times t [m], as k_isochrone and RT_bench.py:993-1001
    do: NaN unless n >= 2 and T[0] <= t <= T[n-1].  -> (values [m] longdouble, labels [m, 2]: the rules of the derivatives at
    the two ends of the evaluated interval ('' where NaN), near [m]: near_guard of an end rule that the entry used)"""
    T, Y, t = np.asarray(T, dtype=LD), np.asarray(Y, dtype=LD), np.asarray(t, dtype=LD)
    n, m = len(T), len(t)
    val = np.full(m, np.nan, dtype=LD)
    lab = np.full((m, 2), "", dtype="U5")
    near = np.zeros(m, dtype=bool)
    if n < 2:
        return val, lab, near
    ok = (T[0] <= t) & (t <= T[n - 1])
    d, dl, dn = derivatives(T, Y)
    i = _interval(T, t[ok])
    val[ok] = evaluate(T, Y, d, t[ok])
    lab[ok, 0], lab[ok, 1] = dl[i], dl[i + 1]
    near[ok] = dn[i] | dn[i + 1]
    return val, lab, near


def wavefront(x, y, angle, nfine, y_fine=None):
    """RT_bench.py:1005-1044 on one traveltime's isochrone points x, y, angle [R] (NaN: the ray does not reach it), as
    rtmi_wavefronts states it: the points that exist in a stable order of y, PCHIP x(y) through them, its derivative at
    the points (PPoly.derivative() evaluates the last one from the last interval's right end), the normal angle
    (pi/2 - arctan(dx/dy)) - pi/2, |ray angle - normal angle| of the same point, and the curve on np.linspace(y_min, y_max,
    nfine) -- or on y_fine where the caller brings its own abscissae.  Derived arrays are empty with fewer than 2 points and
    NaN throughout when two sorted neighbours have dy <= 0 (`tie`; scipy raises).  pi is the fp64 one, as on the device."""
    x, y, angle = (np.asarray(a, dtype=np.float64) for a in (x, y, angle))
    ray = np.nonzero(~np.isnan(y))[0]
    ray = ray[np.argsort(y[ray], kind="stable")]
    ys, xs = y[ray], x[ray]
    n = len(ray)
    out = dict(count=n, ray=ray, y=ys, x=xs, angle=angle[ray], tie=bool(n >= 2 and np.any(np.diff(ys) <= 0)), near=False)
    m = n if n >= 2 else 0
    nf = nfine if m else 0
    nan = np.full(m, np.nan, dtype=LD)
    out.update(dxdy=nan, normal=nan, angle_diff=nan, label=np.full(m, "", dtype="U5"),
               x_fine=np.full(nf, np.nan, dtype=LD), y_fine=np.full(nf, np.nan))
    if m == 0 or out["tie"]:
        return out
    d, lab, near = derivatives(ys, xs)
    slope = d.copy()
    slope[-1] = evaluate(ys, xs, d, ys[-1:], nu=1)[0]
    half_pi = LD(np.pi) / 2
    normal = (half_pi - np.arctan(slope)) - half_pi
    out.update(dxdy=slope, normal=normal, angle_diff=np.abs(angle[ray] - normal), label=lab, near=bool(near.any()))
    if nf:
        yf = np.linspace(ys[0], ys[-1], nfine) if y_fine is None else np.asarray(y_fine, dtype=np.float64)
        out.update(y_fine=yf, x_fine=evaluate(ys, xs, d, yf))
    return out


# (abscissae, values, the rule expected at each point): unequal spacings, negative abscissae, n = 2, 3, 4 and one longer set
RULE_SETS = [
    ([-3.0, -1.2], [0.5, 2.0], ["two", "two"]),
    ([-1.2, 7.0], [2.0, -0.25], ["two", "two"]),
    ([-2.0, -1.5, 0.7], [0.0, 1.0, 2.5], ["plain", "mean", "zero"]),
    ([-1.0, -0.3, 1.0], [0.0, 0.1, 5.0], ["zero", "mean", "plain"]),
    ([-1.0, 0.3, 1.0], [5.0, 0.1, 0.0], ["plain", "mean", "zero"]),
    ([-1.0, 0.0, 1.1], [0.0, 1.0, -9.0], ["3m0", "flip", "plain"]),
    ([-5.5, -5.4, -3.9], [2.0, -7.0, -6.5], ["plain", "flip", "3m0"]),
    ([-1.0, 0.0, 2.0], [1.0, 1.0, 3.0], ["zero", "flat", "plain"]),
    ([-1.0, 0.0, 2.0], [1.0, 1.0, 1.0], ["plain", "flat", "plain"]),
    ([-4.0, -2.5, -2.0, 1.0], [0.0, 0.0, 1.0, 3.0], ["zero", "flat", "mean", "zero"]),
    ([-4.0, -2.5, -2.0, 1.0], [0.0, 2.0, 1.0, 30.0], ["plain", "flip", "flip", "plain"]),
    ([-4.0, -2.5, -2.0, 1.0], [-1.0, -0.5, -0.4, -20.0], ["plain", "mean", "flip", "plain"]),
    ([0.1, 0.2, 0.4, 0.5], [1.0, 0.9, 0.9, -3.0], ["plain", "flat", "flat", "plain"]),
    ([0.1, 0.2, 0.4, 0.5], [1.0, 1.1, -4.0, -4.5], ["3m0", "flip", "mean", "zero"]),
    ([-9.0, -7.5, -7.0, -3.0, 0.0, 0.25, 4.0], [3.0, 2.0, 2.5, 2.5, 9.0, 9.5, -1.0],
     ["plain", "flip", "flat", "flat", "mean", "flip", "plain"]),
]

# The fans that tests/test_pchip_ref.py (oracle rows) and tests/test_gpu_wavefronts.py (device rows) both use.  F: the fisheye
# from (1, 0), whose rays circle the origin, so that x(T), y(T) turn round again and again; I: the launch conditions of the
# fixture traj_interface_op6_16, whose rays run straight (theta(T) flat) between the interface's bends.
F_FAN = dict(scen="fisheye", method=6, step=2 * np.pi / 303, max_size=700, x0=1.0, y0=0.0,
             theta=np.linspace(np.pi / 4, 3 * np.pi / 4, 64), cuts=(2, 3, 60, 79, 150), times=np.linspace(0.2, 7.2, 36))
I_FAN = dict(scen="interface", fixture="traj_interface_op6_16", method=6, y0=-2.0, cuts=(2, 3), times=np.linspace(0.5, 31, 40))
# the bound of the device against this module is 8 x the ceiling that test_pchip_ref.py asserts for scipy against this
# module, in units of eps x scale (scale: the largest magnitude of the interpolated column over the data set; for dx/dy the
# largest |dx/dy| of the wavefront)
SCIPY_CEILING = 4.0
DEVICE_BOUND = 8 * SCIPY_CEILING


# How often the rules above stand behind the numbers that the two test modules compare, counted on the oracle's rows: per-ray
# stage (fan, rec_rows cut; 0 = full record) and across-ray stage (fan, "across").  Both modules assert at least half of each,
# so that a pass cannot come from a rule going unvisited and a small change of the trajectories does not fail them.
CENSUS = {("F", 0): {"flip": 684, "zero": 2, "3m0": 3}, ("F", 3): {"zero": 6, "3m0": 6}, ("I", 0): {"flat": 554},
          ("F", "across"): {"flip": 179, "3m0": 3}, ("I", "across"): {"zero": 7, "3m0": 6, "flip": 66}}
I_ACROSS_TWO_POINT, I_ACROSS_BOTH_SIGNS = 12, 18      # wavefronts of I with two points / with y of both signs


def assert_census_floors(cen, fan, stage):
    """cen (label -> count, census()) holds at least half of what CENSUS lists for this fan and stage, if it lists any"""
    for lab, measured in CENSUS.get((fan, stage), {}).items():
        assert cen.get(lab, 0) >= (measured + 1) // 2, (fan, stage, lab, cen)


def ray_lengths(last, rec_rows):
    """rows that the isochrone stage reads of each ray: min(last row + 1, rec_rows)"""
    return np.minimum(np.asarray(last).astype(np.int64) + 1, rec_rows)


def time_list(rows, nrow, per_column=6):
    """The traveltimes at which the tests evaluate a fan's rows [rec_rows, 6, R] (nrow [R]: rows of each ray): per ray its first,
    its last and one middle recorded T exactly, the midpoints of its first and last interval, the midpoints of the two
    intervals either side of up to `per_column` interior points of each of x, y, theta whose derivative rule is 'flip' or
    'flat' (spread evenly over those the column has), and 4 equally spaced times inside the record.  Sorted, without repeats."""
    out = []
    for k in range(rows.shape[2]):
        n = int(nrow[k])
        if n < 2:
            continue
        T = rows[:n, 4, k]
        out += [T[0], T[n - 1], T[n // 2], 0.5 * (T[0] + T[1]), 0.5 * (T[n - 2] + T[n - 1])]
        out += list(np.linspace(T[0], T[n - 1], 6)[1:-1])
        if n < 3:
            continue
        for q in (0, 1, 5):
            lab = derivatives(T, rows[:n, q, k])[1]
            j = np.nonzero((lab == "flip") | (lab == "flat"))[0]
            j = j[(j > 0) & (j < n - 1)]
            if len(j) > per_column:
                j = j[np.linspace(0, len(j) - 1, per_column).astype(int)]
            out += list(0.5 * (T[j - 1] + T[j])) + list(0.5 * (T[j] + T[j + 1]))
    return np.unique(np.asarray(out, dtype=np.float64))


def fan_isochrones(rows, nrow, times):
    """isochrone() of x, y, theta of every ray of a fan -> (values [ntimes, 3, R] longdouble, labels [ntimes, 3, R, 2],
    near [ntimes, 3, R])"""
    nt, R = len(times), rows.shape[2]
    val = np.full((nt, 3, R), np.nan, dtype=LD)
    lab = np.full((nt, 3, R, 2), "", dtype="U5")
    near = np.zeros((nt, 3, R), dtype=bool)
    for k in range(R):
        n = int(nrow[k])
        for c, q in enumerate((0, 1, 5)):
            val[:, c, k], lab[:, c, k], near[:, c, k] = isochrone(rows[:n, 4, k], rows[:n, q, k], times)
    return val, lab, near


def census(labels):
    """label -> how often it occurs"""
    u, c = np.unique(labels, return_counts=True)
    return {str(a): int(b) for a, b in zip(u, c) if a}
