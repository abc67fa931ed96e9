"""GPU: first-arrival grid tables (rtmi_first_arrival_grid, rtmi_debug_grid_rows, rtmi_debug_paraxial_rows).  The device
against the numpy restatement (tests/ttgrid_ref.py) on the device's own rows, bit for bit; the synthetic edge cases; the same
bits in every schedule, under ray sorting and in every source grouping; closed-form traveltimes (vert_heterogeneous, fisheye,
the interface's refraction); the 1 M-ray fan; the per-row amplitudes against rtmi_paraxial.  Bounds are measurements on
MI355X, recorded in DESIGN.md section 11."""
import numpy as np
import pytest

import paraxial_ref as P
import ttgrid_ref as G
from conftest import LIMITS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    cache = {}

    def get(scen, dtype=0):
        if (scen, dtype) not in cache:
            F = rb.Field.build(scen, LIMITS[scen], rb.DELTA, dtype=dtype)
            cache[(scen, dtype)] = (F, P.SplineField(*F.arrays()))
        return cache[(scen, dtype)]
    yield get
    for F, _ in cache.values():
        F.close()


# scenario -> (step, source, fan, grid, max_gap)
SCEN = {
    "interface": (None, (-2.0, -2.0), (0.1, np.pi / 2 - 0.1), (-1.95, 0.1, 100, -1.95, 0.1, 60), 0.6),
    "fisheye": (2 * np.pi / 303, (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4), (-1.45, 0.05, 59, -1.45, 0.05, 59), 0.4),
    "vert_heterogeneous": (None, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (-1.95, 0.05, 140, -2.45, 0.05, 70), 0.4),
}


def setup(rb, scen):
    step, (x0, y0), fan, grid, gap = SCEN[scen]
    step = rb.DELTA_S if step is None else step
    ms = 121 if scen == "fisheye" else int(np.ceil(80 / step) + 1)
    return step, ms, x0, y0, fan, grid, gap


def batch(rb, F, scen, m, R, S=1, **kw):
    step, ms, x0, y0, (t0, t1), grid, gap = setup(rb, scen)
    th = np.linspace(t0, t1, R)
    b = rb.Batch(F, rb.METHODS[m], step, ms, LIMITS[scen], 1, np.tile(th, S), x0, y0, keep_n_ray=False, **kw)
    b.run()
    return b


def same_bits(a, b, keys=None):
    for k in keys or [k for k in a if k != "stats"]:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def relerr(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok])) / max(np.max(np.abs(b[ok])), 1e-300)) if ok.any() else 0.0


# ---------------------------------------------------------------- 1. the device against the restatement, same rows
CASES = [(s, m) for s in ("vert_heterogeneous", "fisheye", "interface") for m in range(1, 10)]


@pytest.mark.parametrize("scen,m", CASES)
def test_device_equals_the_restatement_on_the_same_rows(rb, fields, scen, m):
    F, S = fields(scen)
    *_, grid, gap = setup(rb, scen)
    b = batch(rb, F, scen, m, 96)
    dev = b.first_arrival_grid(grid, max_gap=gap, amplitude=True, stats=True)
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    pj, pk = b.paraxial_rows()
    b.close()
    J, km = G.paraxial_rows(rows, last, S)
    ref = G.from_record(rows, last, grid, max_gap=gap, amplitude=(J, km, G.record_n(rows)))
    assert dev["count"].sum() > 500
    for k in ("count", "T", "theta0", "theta", "ray", "step"):
        assert np.array_equal(dev[k], ref[k], equal_nan=True), k
    for k in ("cells", "skipped_cells", "triangles", "folded"):
        assert dev["stats"][k] == ref["stats"][k], k
    assert dev["stats"]["atomics"][0] == dev["count"].sum()
    eJ, eG = relerr(dev["J"], ref["J"]), relerr(dev["G"], ref["G"])
    ej = relerr(pj, J)
    print(f"{scen} op{m}: J {eJ:.2e} G {eG:.2e} rows J {ej:.2e} stats {dev['stats']}")
    assert eJ <= 1e-9 and eG <= 1e-9
    # kmah agrees wherever the restatement's rows agree with the device's on it (no sign change of Q2 within rounding)
    assert np.mean(dev["kmah"][dev["count"] > 0] == ref["kmah"][dev["count"] > 0]) > 0.999


# ---------------------------------------------------------------- 2. synthetic rows
def synthetic_cases():
    out = []
    h, M, rows = 0.25, 9, 9
    for skew in (0.0, 0.5, -1.0):
        m, i = np.arange(M), np.arange(rows)
        x = (m[None, :] * h + skew * i[:, None] * h).astype(np.float64)
        y = np.broadcast_to(i[:, None] * h, (rows, M)).astype(np.float64)
        out.append((x, y, y + 0.01 * x, np.full((rows, M), np.pi / 2), np.full(M, rows - 1), np.zeros(M),
                    (-3.0, h / 2, 100, 0.0, h / 2, 17), {"max_gap": 1.0}))
    u = np.linspace(-1.5, 1.5, 401)
    t = np.linspace(0.0, 1.0, 101)
    x = u[None, :] * (1 - 2 * t[:, None]) + t[:, None] * u[None, :] ** 3
    y = np.broadcast_to(t[:, None], x.shape).astype(np.float64)
    for T in (y - 0.05 * u[None, :], np.ones_like(x)):
        out.append((x, y, T, np.full(x.shape, np.pi / 2), np.full(401, 100), u, (-1.0, 0.01, 201, 0.0, 0.01, 101),
                    {"max_gap": 0.1}))
    h, M, rows = 0.1, 10, 11
    x = np.arange(M)[None, :] * h + np.where(np.arange(M) >= 5, 0.5, 0.0)[None, :] + 0 * np.arange(rows)[:, None]
    y = np.broadcast_to(np.arange(rows)[:, None] * h, (rows, M)).astype(np.float64)
    th = np.where(np.arange(M)[None, :] >= 5, np.pi / 2 - 1.0, np.pi / 2) * np.ones((rows, M))
    out.append((x.astype(np.float64), y, y.copy(), th, np.full(M, rows - 1), np.zeros(M), (0.0, 0.05, 30, 0.0, 0.05, 21),
                {"max_gap": 1.0}))
    return out


@pytest.mark.parametrize("case", range(6))
def test_debug_rows_equal_the_restatement(rb, case):
    x, y, T, th, last, th0, grid, kw = synthetic_cases()[case]
    dev = rb.debug_grid_rows(x, y, T, th, last, th0, grid, stats=True, **kw)
    ref = G.first_arrival_grid(x, y, T, th, last, grid, theta0=th0, **kw)
    same_bits(dev, ref, ["count"] + list(G.FIELDS))
    for k in ("cells", "skipped_cells", "triangles", "folded"):
        assert dev["stats"][k] == ref["stats"][k], k
    if case in (3, 4):
        assert dev["count"].max() == 3 and dev["stats"]["folded"] > 0
    if case == 5:
        assert dev["stats"]["skipped_cells"] == 10


# ---------------------------------------------------------------- 3. invariance
def test_same_bits_in_every_schedule_sorting_and_twice(rb, fields):
    F, _ = fields("interface")
    *_, grid, gap = setup(rb, "interface")
    ref = None
    for kw in ({}, {"launch_mode": "plain"}, {"launch_mode": "sliced"}, {"launch_mode": "refill"}, {"sort_rays": True}):
        b = batch(rb, F, "interface", 6, 512, S=3, **kw)
        r1 = b.first_arrival_grid(grid, fan_size=512, max_gap=gap, amplitude=True)
        r2 = b.first_arrival_grid(grid, fan_size=512, max_gap=gap, amplitude=True)
        b.close()
        same_bits(r1, r2)
        if ref is None:
            ref = r1
        same_bits(r1, ref)
    assert ref["count"].shape == (3,) + ref["count"].shape[1:] and (ref["count"] > 0).sum() > 3000


def test_traveltime_table_is_the_same_in_any_grouping(rb, fields):
    F, _ = fields("vert_heterogeneous")
    step, ms, *_ = setup(rb, "vert_heterogeneous")
    src = np.array([[-2.0, -2.0], [-1.0, -2.2], [0.0, -1.5], [1.0, -2.4], [2.0, -2.0]])
    grid = (-1.95, 0.05, 140, -2.45, 0.05, 70)
    th = np.linspace(0.05, np.pi - 0.05, 1024)
    kw = dict(thetas=th, step=step, max_size=ms, box=LIMITS["vert_heterogeneous"], amplitude=True)
    one = rb.traveltime_table(rb.op6, F, src, grid, stats=True, **kw)
    many = rb.traveltime_table(rb.op6, F, src, grid, mem_budget=2 * 1024 * one["stats"]["rec_rows"] * 60, stats=True, **kw)
    assert one["stats"]["groups"] == 1 and many["stats"]["groups"] >= 3
    same_bits(one, many)
    b = rb.Batch(F, rb.op6, step, ms, LIMITS["vert_heterogeneous"], 1, th, -1.0, -2.2, rec_rows=one["stats"]["rec_rows"],
                 keep_n_ray=False)
    b.run()
    single = b.first_arrival_grid(grid, amplitude=True)
    b.close()
    for k in single:
        assert np.array_equal(single[k][0], one[k][1], equal_nan=True), k


def test_fp32_against_fp64(rb, fields):
    out = {}
    for dt in (0, 1):
        F, _ = fields("vert_heterogeneous", dt)
        b = batch(rb, F, "vert_heterogeneous", 6, 2048)
        out[dt] = b.first_arrival_grid(SCEN["vert_heterogeneous"][3], amplitude=True)
        b.close()
    both = (out[0]["count"] > 0) & (out[1]["count"] > 0)
    assert both.sum() > 0.99 * (out[0]["count"] > 0).sum()
    e = np.max(np.abs(out[1]["T"] - out[0]["T"])[both]) / np.max(out[0]["T"][both])
    eg = np.max(np.abs(out[1]["G"] - out[0]["G"])[both]) / np.max(out[0]["G"][both])
    print(f"fp32 vs fp64: T {e:.2e} G {eg:.2e}")
    assert e <= 1e-4 and eg <= 1e-2


# ---------------------------------------------------------------- 4. physics
def grid_xy(grid):
    gx0, gdx, nx, gy0, gdy, ny = grid
    return np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)


def test_vert_heterogeneous_and_fisheye_closed_forms(rb, fields):
    F, _ = fields("vert_heterogeneous")
    b = batch(rb, F, "vert_heterogeneous", 6, 4096)
    grid = (-1.99, 0.01, 700, -2.49, 0.01, 350)
    r = b.first_arrival_grid(grid, amplitude=True)
    b.close()
    X, Y = grid_xy(grid)
    ok = (r["count"][0] > 0) & (np.hypot(X + 2, Y + 2) > 0.2)
    assert np.all(r["count"][0] <= 1)
    Tc = G.vert_T(-2.0, -2.0, X, Y)
    e = np.max(np.abs(r["T"][0] - Tc)[ok] / Tc[ok])
    Gc = 1.0 / np.sqrt(P.vert_closed_form(r["theta0"][0], X, Y) / (18.0 + 2.0 * Y))
    eg = np.max(np.abs(r["G"][0] - Gc)[ok]) / np.max(Gc[ok])
    F2, _ = fields("fisheye")
    b = batch(rb, F2, "fisheye", 6, 1024)
    grid = (-1.0, 0.02, 101, -1.0, 0.02, 101)
    f = b.first_arrival_grid(grid)
    b.close()
    X, Y = grid_xy(grid)
    okf = (f["count"][0] > 0) & (np.hypot(X - 1, Y) > 0.2)
    ef = np.max(np.abs(f["T"][0] - G.fisheye_T(1.0, 0.0, X, Y))[okf] / G.fisheye_T(1.0, 0.0, X, Y)[okf])
    print(f"vert T {e:.2e} G {eg:.2e} covered {ok.sum()}; fisheye T {ef:.2e} covered {okf.sum()}")
    assert ok.sum() > 100000 and okf.sum() > 1500
    assert e <= 2e-6 and eg <= 5e-4 and ef <= 7e-5


def refraction_T(x, y, xs=-2.0, ys=-2.0, n1=np.sqrt(2.0)):
    """min over u of n1 |src - (u, 0)| + |(u, 0) - node| (the wall y = 0), by ternary search; and the transmitted angle"""
    lo, hi = np.full(x.shape, xs), x.copy()
    f = lambda u: n1 * np.hypot(u - xs, ys) + np.hypot(x - u, y)   # noqa: E731
    for _ in range(200):
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        fa, fb = f(a), f(b)
        lo, hi = np.where(fa < fb, lo, a), np.where(fa < fb, b, hi)
    u = 0.5 * (lo + hi)
    return f(u), np.degrees(np.arctan2(np.abs(x - u), y))


def test_interface_refraction_and_no_value_from_a_skipped_cell(rb, fields):
    F, _ = fields("interface")
    b = batch(rb, F, "interface", 6, 4096)
    grid = (-1.98, 0.02, 700, -1.98, 0.02, 300)
    r = b.first_arrival_grid(grid, stats=True)
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    b.close()
    X, Y = grid_xy(grid)
    c = r["count"][0] > 0
    # below the wall, inside the direct fan's wedge (elsewhere only reflections arrive)
    ang0 = np.arctan2(Y + 2, X + 2)
    below = c & (Y < -0.1) & (np.hypot(X + 2, Y + 2) > 0.2) & (ang0 > 0.12) & (ang0 < np.pi / 2 - 0.12)
    eb = np.max(np.abs(r["T"][0] - np.sqrt(2.0) * np.hypot(X + 2, Y + 2))[below] / (np.sqrt(2.0) * np.hypot(X + 2, Y + 2))[below])
    above = c & (Y > 0.1)
    Tr, ang = refraction_T(X[above], Y[above])
    sel = ang < 80.0
    ea = np.max(np.abs(r["T"][0][above] - Tr)[sel] / Tr[sel])
    print(f"interface below {eb:.2e} ({below.sum()}), above {ea:.2e} ({sel.sum()}), skipped {r['stats']['skipped_cells']}")
    assert r["stats"]["skipped_cells"] > 0
    assert below.sum() > 20000 and sel.sum() > 10000
    assert eb <= 1e-3 and ea <= 1e-2
    # every winner's cell passes the gap rule on the device's own rows
    m = np.floor(r["ray"][0][c]).astype(np.int64)
    i = np.floor(r["step"][0][c]).astype(np.int64)
    m = np.minimum(m, 4094); i = np.minimum(i, np.minimum(last[m], last[m + 1]) - 1)
    gap, dth = G.defaults(grid)
    xa, ya, xb, yb = rows[i, 0, m], rows[i, 1, m], rows[i, 0, m + 1], rows[i, 1, m + 1]
    xc, yc, xd, yd = rows[i + 1, 0, m], rows[i + 1, 1, m], rows[i + 1, 0, m + 1], rows[i + 1, 1, m + 1]
    assert np.all(np.hypot(xb - xa, yb - ya) <= gap) and np.all(np.hypot(xd - xc, yd - yc) <= gap)
    assert np.all(np.abs(G.wrap(rows[i, 5, m + 1] - rows[i, 5, m])) <= dth)
    assert np.all(np.abs(G.wrap(rows[i + 1, 5, m + 1] - rows[i + 1, 5, m])) <= dth)


# ---------------------------------------------------------------- 5. scale
def test_million_ray_fan_onto_a_million_nodes(rb, fields):
    F, _ = fields("vert_heterogeneous")
    R = 1 << 20
    box = LIMITS["vert_heterogeneous"]
    step, ms, *_ = setup(rb, "vert_heterogeneous")
    th = np.linspace(0.05, 1.5, R)
    c = rb.Batch(F, rb.op6, step, ms, box, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, step, ms, box, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    grid = (-2.0, 7.0 / 1023, 1024, -2.5, 3.5 / 1023, 1024)
    r = b.first_arrival_grid(grid, stats=True)
    b.close()
    X, Y = grid_xy(grid)
    cov = r["count"][0] > 0
    Tc = G.vert_T(-2.0, -2.0, X, Y)
    far = cov & (np.hypot(X + 2, Y + 2) > 0.05)
    e = np.max(np.abs(r["T"][0] - Tc)[far] / Tc[far])
    # the wedge: nodes whose circle through the source leaves at 0.05 < theta0 < 1.5 and stays in the box up to the node
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = ((X ** 2 + (Y + 9) ** 2) - (4.0 + 49.0)) / (2 * (X + 2))
        t0 = np.arctan((xc + 2) / 7.0)
        rho = np.hypot(-2 - xc, 7.0)
    inside = (t0 > 0.06) & (t0 < 1.49) & (X > -1.99) & (X < 4.99) & (Y > -2.49) & (Y < 0.99) & (X > -1.95)
    inside &= (X <= xc) | (rho - 9 < 0.99)
    frac = cov[inside].mean()
    print(f"1M fan: rec_rows {rows}, covered {cov.sum()}, wedge {inside.sum()} at {frac:.5f}, T err {e:.2e}, stats {r['stats']}")
    assert np.all(r["count"][0] <= 1)
    assert e <= 2e-6
    assert frac >= 0.999


# ---------------------------------------------------------------- 6. amplitudes along every row
@pytest.mark.parametrize("scen,m,sort", [("vert_heterogeneous", 6, False), ("fisheye", 3, True), ("interface", 8, False)])
def test_row_J_at_the_last_row_is_paraxial_at_end(rb, fields, scen, m, sort):
    F, _ = fields(scen)
    b = batch(rb, F, scen, m, 300, sort_rays=sort)
    J, km = b.paraxial_rows()
    end = b.paraxial()
    last = b.d_ray()[2].astype(np.int64)
    b.close()
    k = np.arange(300)
    assert np.array_equal(J[last, k], end["J"])
    assert np.array_equal(km[last, k].astype(np.float64), end["kmah"])
    assert np.all(J[0] == 0.0)


# ---------------------------------------------------------------- 7. errors
def test_argument_and_state_errors(rb, fields):
    from raytracing_amd import _lib
    F, _ = fields("vert_heterogeneous")
    grid = SCEN["vert_heterogeneous"][3]
    b = batch(rb, F, "vert_heterogeneous", 6, 64, record_stride=4)
    with pytest.raises(_lib.RtmiError, match="record_stride"):
        b.first_arrival_grid(grid)
    b.close()
    b = batch(rb, F, "vert_heterogeneous", 6, 64)
    with pytest.raises(_lib.RtmiError, match="multiple of fan_size"):
        b.first_arrival_grid(grid, fan_size=48)
    for g in ((0, 0.1, 0, 0, 0.1, 5), (0, 0.1, 5, 0, 0.1, 0), (0, 0.0, 5, 0, 0.1, 5), (0, 0.1, 5, 0, -1.0, 5)):
        with pytest.raises(_lib.RtmiError) as e:
            b.first_arrival_grid(g)
        assert e.value.code == -1
    st, aux, ist, al = b.get_state()
    b.set_state(st, istep=ist)
    with pytest.raises(_lib.RtmiError) as e:
        b.first_arrival_grid(grid)
    assert e.value.code == -4
    b.close()
    Fa = rb.Field.build("vert_heterogeneous", LIMITS["anisotropy"], rb.DELTA)
    for m in (10, 11):
        b = rb.Batch(Fa, rb.METHODS[m], rb.DELTA_S, 2000, LIMITS["anisotropy"], 3, np.linspace(0.1, 1.4, 64), -2.0, -2.0)
        b.run()
        with pytest.raises(_lib.RtmiError, match="amplitude"):
            b.first_arrival_grid(grid, amplitude=True)
        t = b.first_arrival_grid(grid)                  # the traveltime table works for every method
        assert (t["count"] > 0).sum() > 100
        b.close()
    Fa.close()
