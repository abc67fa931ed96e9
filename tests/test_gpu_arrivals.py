"""GPU: later and most energetic arrivals on a grid (rtmi_arrival_grid, rtmi_debug_arrival_rows).  One arrival by time against
rtmi_first_arrival_grid, bit for bit; four arrivals in both orders against the numpy restatement (tests/arrival_ref.py) on the
device's own rows of the lens bed, where the fan triplicates and the strongest branch is not the first; synthetic cusps, ties and
an accordion of nine sheets; ragged fans; the same bits in every schedule, sorting and source grouping; refusals.

Every column is compared with np.array_equal, J and G included: the restatement is given the device's own per-row J and kmah
(rtmi_debug_paraxial_rows), so that nothing but the interpolation, one product, one square root and one division -- each
correctly rounded on both sides -- lies between them."""
import numpy as np
import pytest

import arrival_ref as A
import ttgrid_ref as G
from conftest import LIMITS

pytestmark = pytest.mark.gpu

COLS = A.FIELDS + A.AMPLITUDE_FIELDS


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
            if scen == "lens":
                x, y, Z, h = A.lens_samples()
                cache[(scen, dtype)] = rb.Field.from_samples(x, y, Z, h, dtype=dtype)
            else:
                cache[(scen, dtype)] = rb.Field.build(scen, LIMITS[scen], rb.DELTA, dtype=dtype)
        return cache[(scen, dtype)]
    yield get
    for F in cache.values():
        F.close()


# scenario -> (step, max_size, box, source, fan, grid, max_gap): test_gpu_ttgrid.py's cases, and the lens bed
def scenario(rb, scen):
    if scen == "lens":
        return A.LENS_STEP, A.LENS_MAX_SIZE, A.LENS_BOX, A.LENS_SOURCE, (A.LENS_THETA[0], A.LENS_THETA[-1]), A.LENS_GRID, None
    step = 2 * np.pi / 303 if scen == "fisheye" else rb.DELTA_S
    ms = 121 if scen == "fisheye" else int(np.ceil(80 / step) + 1)
    src, fan, grid, gap = {
        "interface": ((-2.0, -2.0), (0.1, np.pi / 2 - 0.1), (-1.95, 0.1, 100, -1.95, 0.1, 60), 0.6),
        "fisheye": ((1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4), (-1.45, 0.05, 59, -1.45, 0.05, 59), 0.4),
        "vert_heterogeneous": ((-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (-1.95, 0.05, 140, -2.45, 0.05, 70), 0.4)}[scen]
    return step, ms, LIMITS[scen], src, fan, grid, gap


def lens_batch(rb, F, sources=(A.LENS_SOURCE,), M=256, **kw):
    src = np.asarray(sources, dtype=np.float64)
    th = np.linspace(A.LENS_THETA[0], A.LENS_THETA[-1], M)
    b = rb.Batch(F, rb.METHODS[A.LENS_METHOD], A.LENS_STEP, A.LENS_MAX_SIZE, A.LENS_BOX, 1, np.tile(th, len(src)),
                 np.repeat(src[:, 0], M), np.repeat(src[:, 1], M), keep_n_ray=False, **kw)
    b.run()
    return b


def same_bits(a, b, keys=None):
    for k in keys or [k for k in a if k != "stats"]:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------- 1. one arrival by time is the first-arrival table
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("amplitude", [False, True])
@pytest.mark.parametrize("scen", ["vert_heterogeneous", "fisheye", "interface", "lens"])
def test_one_arrival_by_time_is_the_first_arrival_table(rb, fields, scen, amplitude, dtype):
    step, ms, box, (x0, y0), (t0, t1), grid, gap = scenario(rb, scen)
    b = rb.Batch(fields(scen, dtype), rb.op6, step, ms, box, 1, np.linspace(t0, t1, 256), x0, y0, keep_n_ray=False)
    b.run()
    first = b.first_arrival_grid(grid, max_gap=gap, amplitude=amplitude, stats=True)
    one = b.arrival_grid(grid, arrivals=1, order="time", max_gap=gap, amplitude=amplitude, stats=True)
    b.close()
    assert first["count"].sum() > 500
    assert set(one) == set(first)
    assert np.array_equal(one["count"], first["count"])
    for k in [k for k in first if k not in ("count", "stats")]:
        assert one[k].shape == (1, 1) + first[k].shape[1:]
        assert np.array_equal(one[k][:, 0], first[k], equal_nan=True), k
    for k in ("cells", "skipped_cells", "triangles", "folded", "max_gap", "max_dtheta"):
        assert one["stats"][k] == first["stats"][k], k
    assert one["stats"]["candidates"] == first["count"].sum() == one["stats"]["atomics"][0] == one["stats"]["atomics"][1]


# ---------------------------------------------------------------- 2. the lens bed, the device's own rows
@pytest.fixture(scope="module")
def lens_rows(rb, fields):
    b = lens_batch(rb, fields("lens"))
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    J, km = b.paraxial_rows()
    dev = {o: b.arrival_grid(A.LENS_GRID, arrivals=4, order=o, amplitude=True, stats=True) for o in (A.BY_TIME, A.BY_AMPLITUDE)}
    plain = b.arrival_grid(A.LENS_GRID, arrivals=4, order=A.BY_AMPLITUDE)
    b.close()
    return rows, last, (J, km, G.record_n(rows)), dev, plain


@pytest.mark.parametrize("order", [A.BY_TIME, A.BY_AMPLITUDE])
def test_lens_bed_equals_the_restatement_on_the_devices_rows(lens_rows, order):
    rows, last, amp, dev, plain = lens_rows
    ref = A.from_record(rows, last, A.LENS_GRID, arrivals=4, order=order, amplitude=amp)
    tri = ref["count"][0] == 3
    print(f"lens bed, device rows, by {order}: count histogram {np.bincount(ref['count'].ravel()).tolist()}, stats {dev[order]['stats']}")
    assert tri.sum() >= 400
    same_bits(dev[order], ref, ("count",) + COLS)
    assert dev[order]["stats"]["candidates"] == ref["count"].sum()
    if order == A.BY_AMPLITUDE:
        # the strongest is the branch through the caustic, not the first; and asking for no amplitude columns changes no order
        first = A.from_record(rows, last, A.LENS_GRID, arrivals=1, amplitude=amp)
        assert np.all(dev[order]["T"][0, 0][tri] > first["T"][0, 0][tri])
        assert np.all(dev[order]["kmah"][0, 0][tri] == 1)
        assert set(plain) == {"count"} | set(A.FIELDS)
        same_bits(plain, ref, ("count",) + A.FIELDS)


# ---------------------------------------------------------------- 3. synthetic rows
NODES = (-0.05, 0.05, 3, 0.85, 0.05, 3)             # nine nodes about (0, 0.9), inside the cusp


def cusp_cases():
    c = A.cusp_rows()
    one = np.ones(c["x"].shape)
    J, km, n = c["amplitude"]
    return {"cusp": c, "ties": dict(c, T=one, amplitude=(one, np.zeros(one.shape, dtype=np.int32), one)),
            "nan": dict(c, amplitude=(np.where(np.abs(c["theta0"])[None, :] < 0.1, np.nan, J), km, n))}


@pytest.mark.parametrize("order", [A.BY_TIME, A.BY_AMPLITUDE])
@pytest.mark.parametrize("case", ["cusp", "ties", "nan"])
def test_debug_rows_equal_the_restatement_on_a_cusp(rb, case, order):
    c = cusp_cases()[case]
    J, km, n = c["amplitude"]
    dev = rb.debug_arrival_rows(c["x"], c["y"], c["T"], c["theta"], c["last"], c["theta0"], NODES, arrivals=4, order=order, J=J, kmah=km,
                                n=n, max_gap=0.1, amplitude=True, stats=True)
    ref = A.arrival_grid(c["x"], c["y"], c["T"], c["theta"], c["last"], NODES, arrivals=4, order=order, theta0=c["theta0"],
                         amplitude=c["amplitude"], max_gap=0.1)
    same_bits(dev, ref, ("count",) + COLS)
    assert np.all(dev["count"] == 3) and dev["stats"]["folded"] > 0
    assert np.all(np.isnan(dev["T"][0, 3]))
    u = dev["theta0"][0, :3, 1, 1]                                            # the node (0, 0.9)
    ur = np.sqrt(0.8 / 0.9)
    want = {("cusp", A.BY_TIME): [ur, 0, -ur], ("ties", A.BY_TIME): [-ur, 0, ur], ("ties", A.BY_AMPLITUDE): [-ur, 0, ur],
            ("nan", A.BY_TIME): [ur, 0, -ur]}.get((case, order))
    if want is not None:
        assert np.all(np.abs(u - np.array(want)) < 1e-3)
    elif case == "cusp":
        assert abs(u[0]) < 1e-3 and dev["kmah"][0, 0, 1, 1] == 1            # |J| 0.8 against 1.6
    else:
        assert abs(u[2]) < 1e-3 and np.isnan(dev["G"][0, 2, 1, 1])          # J = NaN: c = +inf, listed last


def test_debug_rows_without_amplitude_rows(rb):
    c = A.cusp_rows()
    dev = rb.debug_arrival_rows(c["x"], c["y"], c["T"], c["theta"], c["last"], c["theta0"], NODES, arrivals=2, max_gap=0.1)
    first = rb.debug_grid_rows(c["x"], c["y"], c["T"], c["theta"], c["last"], c["theta0"], NODES, max_gap=0.1)
    assert set(dev) == set(first)
    for k in A.FIELDS:
        assert np.array_equal(dev[k][:, 0], first[k], equal_nan=True), k


def test_accordion_of_nine_sheets_keeps_the_four_earliest(rb):
    c = A.accordion_rows()
    grid = (0.11, 0.13, 6, 0.1, 0.2, 5)
    dev = rb.debug_arrival_rows(c["x"], c["y"], c["T"], c["theta"], c["last"], c["theta0"], grid, arrivals=4, stats=True)
    ref = A.arrival_grid(c["x"], c["y"], c["T"], c["theta"], c["last"], grid, arrivals=4, theta0=c["theta0"])
    same_bits(dev, ref, ("count",) + A.FIELDS)
    assert np.all(dev["count"] == 9) and dev["stats"]["candidates"] == 9 * 30
    Y = (0.1 + 0.2 * np.arange(5))[:, None] * np.ones((5, 6))
    for leg in range(4):
        assert np.max(np.abs(dev["T"][0, leg] - (leg + (Y if leg % 2 == 0 else 1.0 - Y)))) < 1e-12
    most = rb.debug_arrival_rows(c["x"], c["y"], c["T"], c["theta"], c["last"], c["theta0"], grid, arrivals=16)
    assert np.all(np.isfinite(most["T"][0, :9])) and np.all(np.isnan(most["T"][0, 9:]))
    assert np.all(np.diff(most["T"][0, :9], axis=0) > 0)


# ---------------------------------------------------------------- 4. ragged fans, several sources
SOURCES = ((0.2, 0.0), (0.2, 0.3), (0.3, -0.2))


def test_three_ragged_fans_equal_three_single_calls(rb, fields):
    """193 rays per fan: 192 ray pairs per source, 576 lanes -- two full blocks and a quarter, sources changing inside a block."""
    F = fields("lens")
    kw = dict(arrivals=4, order=A.BY_AMPLITUDE, fan_size=193, amplitude=True)
    b = lens_batch(rb, F, SOURCES, M=193)
    all3 = b.arrival_grid(A.LENS_GRID, **kw)
    b.close()
    assert all3["count"].shape[0] == 3 and (all3["count"] == 3).sum() > 300
    for s, src in enumerate(SOURCES):
        b = lens_batch(rb, F, (src,), M=193)
        one = b.arrival_grid(A.LENS_GRID, **kw)
        b.close()
        for k in one:
            assert np.array_equal(one[k][0], all3[k][s], equal_nan=True), (s, k)


# ---------------------------------------------------------------- 5. determinism
def test_same_bits_in_every_schedule_sorting_and_twice(rb, fields):
    F = fields("lens")
    ref = None
    for kw in ({}, {"launch_mode": "plain"}, {"launch_mode": "sliced"}, {"launch_mode": "refill"}, {"sort_rays": True}):
        b = lens_batch(rb, F, SOURCES, **kw)
        for order in (A.BY_TIME, A.BY_AMPLITUDE):
            r1 = b.arrival_grid(A.LENS_GRID, arrivals=4, order=order, fan_size=256, amplitude=True)
            r2 = b.arrival_grid(A.LENS_GRID, arrivals=4, order=order, fan_size=256, amplitude=True)
            same_bits(r1, r2)
            ref = ref or {}
            same_bits(r1, ref.setdefault(order, r1))
        b.close()
    assert (ref[A.BY_TIME]["count"] == 3).sum() > 400


def test_traveltime_table_with_arrivals_in_any_grouping(rb, fields):
    F = fields("lens")
    kw = dict(thetas=A.LENS_THETA, step=A.LENS_STEP, max_size=A.LENS_MAX_SIZE, box=A.LENS_BOX, amplitude=True, arrivals=2,
              order="amplitude", stats=True)
    whole = rb.traveltime_table(rb.op6, F, SOURCES, A.LENS_GRID, **kw)
    record = whole["stats"]["rec_rows"] * 60 * 256                      # bytes per source: rows, J and kmah
    single = rb.traveltime_table(rb.op6, F, SOURCES, A.LENS_GRID, mem_budget=record, **kw)
    # room for three records but not for their candidate list: the group is traced again in halves
    halved = rb.traveltime_table(rb.op6, F, SOURCES, A.LENS_GRID, mem_budget=3 * record + 16 * whole["stats"]["candidates"] // 2, **kw)
    assert whole["stats"]["groups"] == 1 and single["stats"]["groups"] == 3 and halved["stats"]["groups"] == 3
    assert whole["T"].shape == (3, 2, A.LENS_GRID[5], A.LENS_GRID[2]) and whole["count"].shape == (3, A.LENS_GRID[5], A.LENS_GRID[2])
    same_bits(whole, single)
    same_bits(whole, halved)
    b = lens_batch(rb, F, SOURCES, rec_rows=whole["stats"]["rec_rows"])
    direct = b.arrival_grid(A.LENS_GRID, arrivals=2, order="amplitude", fan_size=256, amplitude=True)
    b.close()
    same_bits(direct, whole)
    # and without `arrivals` the table is the first-arrival one
    kw.pop("arrivals"); kw.pop("order")
    first = rb.traveltime_table(rb.op6, F, SOURCES, A.LENS_GRID, **kw)
    assert first["T"].shape == (3, A.LENS_GRID[5], A.LENS_GRID[2]) and "candidates" not in first["stats"]
    assert np.array_equal(first["count"], whole["count"])


# ---------------------------------------------------------------- 6. refusals
def test_refusals(rb, fields):
    from raytracing_amd import _lib
    F = fields("lens")
    b = lens_batch(rb, F, M=64)
    for k in (0, 17, -1):
        with pytest.raises(_lib.RtmiError, match="karr") as e:
            b.arrival_grid(A.LENS_GRID, arrivals=k)
        assert e.value.code == -1
    with pytest.raises(_lib.RtmiError, match="order") as e:
        b.arrival_grid(A.LENS_GRID, order=2)
    assert e.value.code == -1
    with pytest.raises(_lib.RtmiError, match="multiple of fan_size") as e:
        b.arrival_grid(A.LENS_GRID, fan_size=48)
    assert e.value.code == -1
    assert b.arrival_grid(A.LENS_GRID, arrivals=16)["T"].shape[1] == 16
    assert set(b.arrival_grid(A.LENS_GRID, count_only=True)) == {"count"}
    b.close()
    b = lens_batch(rb, F, M=64, record_stride=4)
    with pytest.raises(_lib.RtmiError, match="record_stride") as e:
        b.arrival_grid(A.LENS_GRID)
    assert e.value.code == -1
    b.close()
    Fa = rb.Field.build("vert_heterogeneous", LIMITS["anisotropy"], rb.DELTA)
    grid = (-1.95, 0.05, 140, -2.45, 0.05, 70)
    for m in (10, 11):
        b = rb.Batch(Fa, rb.METHODS[m], rb.DELTA_S, 2000, LIMITS["anisotropy"], 3, np.linspace(0.1, 1.4, 64), -2.0, -2.0)
        b.run()
        with pytest.raises(_lib.RtmiError, match="isotropic") as e:
            b.arrival_grid(grid, order="amplitude")
        assert e.value.code == -1
        assert (b.arrival_grid(grid, arrivals=2)["count"] > 0).sum() > 100          # by time: every method
        b.close()
    Fa.close()
