"""CPU: the numpy restatement of rtmi_arrival_grid (tests/arrival_ref.py) on synthetic rows -- a cusp's three branches by time
and by amplitude, bit-equal criteria, the first slot against ttgrid_ref's winner -- and on the oracle's rows of the lens bed,
where it establishes what tests/test_gpu_arrivals.py relies on: a triplication whose strongest branch is not its first."""
import numpy as np
import pytest

import arrival_ref as A
import paraxial_ref as P
import ttgrid_ref as G

UR = np.sqrt(0.8 / 0.9)                               # the outer branches at (0, 0.9): u = +-sqrt((2t - 1) / t)
NODE = (0.0, 0.05, 1, 0.9, 0.05, 1)                   # the one node (0, 0.9)


def cusp(order, K=4, **over):
    c = dict(A.cusp_rows(), **over)
    amp = c.pop("amplitude")
    return c, amp, A.arrival_grid(c["x"], c["y"], c["T"], c["theta"], c["last"], NODE, arrivals=K, order=order, theta0=c["theta0"],
                                  amplitude=amp, max_gap=0.1)


def test_cusp_by_time_lists_the_three_branches_in_order():
    c, amp, r = cusp(A.BY_TIME)
    assert r["count"][0, 0, 0] == 3
    T, u = r["T"][0, :, 0, 0], r["theta0"][0, :, 0, 0]
    assert np.all(np.diff(T[:3]) > 0)
    assert np.all(np.abs(u[:3] - np.array([UR, 0.0, -UR])) < 1e-3)
    for k in A.FIELDS + A.AMPLITUDE_FIELDS + ("c",):
        assert np.isnan(r[k][0, 3, 0, 0]), k
    assert r["key"][0, 3, 0, 0] == -1
    first = G.first_arrival_grid(c["x"], c["y"], c["T"], c["theta"], c["last"], NODE, theta0=c["theta0"], amplitude=amp, max_gap=0.1)
    assert first["key"][0, 0, 0] == r["key"][0, 0, 0, 0]
    for k in A.FIELDS + A.AMPLITUDE_FIELDS:
        assert np.array_equal(first[k][0], r[k][0, 0], equal_nan=True), k
    assert np.array_equal(first["count"], r["count"])


def test_cusp_by_amplitude_puts_the_middle_branch_first():
    """|J| = |(1 - 2t) + 3 t u^2| at t = 0.9: 0.8 on u = 0, 1.6 on u = +-u_r; n = 1."""
    _, _, r = cusp(A.BY_AMPLITUDE)
    u, c = r["theta0"][0, :, 0, 0], r["c"][0, :, 0, 0]
    assert abs(u[0]) < 1e-3 and abs(c[0] - 0.8) < 1e-2
    assert np.all(np.abs(np.abs(u[1:3]) - UR) < 1e-3) and np.all(np.abs(c[1:3] - 1.6) < 2e-2)
    assert c[0] <= c[1] <= c[2] and np.isnan(c[3])
    assert np.array_equal(r["G"][0, :3, 0, 0], 1.0 / np.sqrt(c[:3]))
    assert r["kmah"][0, 0, 0, 0] == 1 and np.all(r["kmah"][0, 1:3, 0, 0] == 0)


@pytest.mark.parametrize("order", [A.BY_TIME, A.BY_AMPLITUDE])
def test_bit_equal_criteria_are_ordered_by_key(order):
    """T = 1 and J = 1 everywhere: every candidate has c = s / s = 1 exactly, and the key alone decides."""
    base = A.cusp_rows()
    one = np.ones(base["x"].shape)
    _, _, r = cusp(order, T=one, amplitude=(one, np.zeros(one.shape, dtype=np.int32), one))
    assert r["count"][0, 0, 0] == 3 and np.all(r["c"][0, :3, 0, 0] == 1.0)
    key = r["key"][0, :3, 0, 0]
    assert np.all(np.diff(key) > 0)
    assert np.all(np.abs(r["theta0"][0, :3, 0, 0] - np.array([-UR, 0.0, UR])) < 1e-3)     # the key grows with the ray


def test_an_unusable_amplitude_goes_last():
    """J = NaN on the rays of the middle branch: its c is +inf, it is listed after the others, and count still says 3."""
    base = A.cusp_rows()
    J, km, n = base["amplitude"]
    J = np.where(np.abs(base["theta0"])[None, :] < 0.1, np.nan, J)
    _, _, r = cusp(A.BY_AMPLITUDE, amplitude=(J, km, n))
    assert r["count"][0, 0, 0] == 3
    assert np.all(np.abs(np.abs(r["theta0"][0, :2, 0, 0]) - UR) < 1e-3)
    assert abs(r["theta0"][0, 2, 0, 0]) < 1e-3 and r["c"][0, 2, 0, 0] == np.inf and np.isnan(r["G"][0, 2, 0, 0])


def test_accordion_counts_nine_sheets_and_keeps_the_earliest():
    c = A.accordion_rows()
    grid = (0.11, 0.13, 6, 0.1, 0.2, 5)
    r = A.arrival_grid(c["x"], c["y"], c["T"], c["theta"], c["last"], grid, arrivals=4, theta0=c["theta0"])
    assert np.all(r["count"] == 9)
    Y = (0.1 + 0.2 * np.arange(5))[:, None] * np.ones((5, 6))
    for leg in range(4):
        assert np.max(np.abs(r["T"][0, leg] - (leg + (Y if leg % 2 == 0 else 1.0 - Y)))) < 1e-12


# ---------------------------------------------------------------- the lens bed on the oracle's rows
@pytest.fixture(scope="module")
def lens():
    from oracle import rt_oracle as O
    x, y, Z, h = A.lens_samples()
    F = O.Field.from_samples(x, y, Z, h)
    kw = dict(nthreads=8)
    c = O.trazar(F, A.LENS_METHOD, 1, A.LENS_STEP, A.LENS_MAX_SIZE, A.LENS_BOX, *A.LENS_SOURCE, A.LENS_THETA, record_stride=0, **kw)
    rows = int(c["d_ray"][2].max()) + 1
    o = O.trazar(F, A.LENS_METHOD, 1, A.LENS_STEP, A.LENS_MAX_SIZE, A.LENS_BOX, *A.LENS_SOURCE, A.LENS_THETA, record_stride=1,
                 rec_rows=rows, **kw)
    s, last = o["s_ray"], o["d_ray"][2].astype(np.int64)
    J, km = G.paraxial_rows(s, last, P.SplineField(*F.arrays()))
    amp = (J, km, G.record_n(s))
    return {o_: A.from_record(s, last, A.LENS_GRID, arrivals=4, order=o_, amplitude=amp) for o_ in (A.BY_TIME, A.BY_AMPLITUDE)}, rows


def test_lens_bed_folds_into_a_triplication(lens):
    r, rows = lens
    cnt = r[A.BY_TIME]["count"][0]
    hist = np.bincount(cnt.ravel(), minlength=4)
    print(f"lens bed: rec_rows {rows}, count histogram {hist.tolist()}")
    assert rows == 411
    assert hist.tolist() == [1716, 2394, 0, 551]
    assert (cnt == 3).sum() >= 400


def test_lens_bed_strongest_arrival_is_not_the_first(lens):
    r, _ = lens
    t, a = r[A.BY_TIME], r[A.BY_AMPLITUDE]
    tri = t["count"][0] == 3
    assert tri.sum() >= 400
    assert np.all(a["key"][0, 0][tri] != t["key"][0, 0][tri])
    c0, c1 = a["c"][0, 0][tri], a["c"][0, 1][tri]
    gap = 1.0 - c0 / c1
    print(f"lens bed: winner's n|J| below the runner-up's by {gap.min():.3f} at least, median {np.median(gap):.3f}")
    assert np.all(gap >= 0.01)
    assert np.all(a["kmah"][0, 0][tri] == 1)


def test_the_two_orders_hold_the_same_set(lens):
    r, _ = lens
    t, a = r[A.BY_TIME], r[A.BY_AMPLITUDE]
    assert np.array_equal(t["count"], a["count"]) and t["count"].max() <= 4
    assert np.array_equal(np.sort(t["key"], axis=1), np.sort(a["key"], axis=1))
    # the first slot by time is ttgrid_ref's table: same T where covered, NaN elsewhere
    assert np.array_equal(np.isnan(t["T"][0, 0]), t["count"][0] == 0)
