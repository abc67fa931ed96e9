"""CPU: the numpy restatement of rtmi_first_arrival_grid (tests/ttgrid_ref.py) on the oracle's trajectories against closed-form
traveltimes, and on synthetic rows against the fill, fold, tie and gap rules.  No GPU involved; these validate the rules before
the device is compared with them (tests/test_gpu_ttgrid.py)."""
import numpy as np
import pytest

import paraxial_ref as P
import ttgrid_ref as G

SIGMA = 0.05293304824724534
DELTA = SIGMA / 3
DELTA_S = SIGMA / 20
VERT_SMALL = (-2.0, 1.0, -2.5, 0.0)          # a part of vert_heterogeneous' box: fewer rows for a 4 096-ray fan
FISH = (-1.5, 1.5, -1.5, 1.5)


def trace(F, m, step, max_size, box, x0, y0, th):
    from oracle import rt_oracle as O
    c = O.trazar(F, m, 1, step, max_size, box, x0, y0, th, record_stride=0, nthreads=8)
    rows = int(c["d_ray"][2].max()) + 1
    o = O.trazar(F, m, 1, step, max_size, box, x0, y0, th, record_stride=1, rec_rows=rows, nthreads=8)
    return o["s_ray"], o["d_ray"][2].astype(np.int64)


# ---------------------------------------------------------------- synthetic rows
def lattice(M, rows, h, skew):
    m, i = np.arange(M), np.arange(rows)
    x = m[None, :] * h + skew * i[:, None] * h
    y = np.broadcast_to(i[:, None] * h, (rows, M)).astype(np.float64)
    return x.astype(np.float64), y


@pytest.mark.parametrize("skew", [0.0, 0.5, -1.0])
def test_nodes_on_shared_edges_and_vertices_count_once(skew):
    """Nodes at every vertex, edge midpoint and cell centre (on the diagonal AD) of a regular sheet: each is counted by
    exactly one triangle; only the sheet's own bottom and right boundary (not top-left) stay uncovered."""
    h, M, rows = 0.25, 9, 9
    x, y = lattice(M, rows, h, skew)
    T = y + 0.01 * x
    th = np.full((rows, M), np.pi / 2)
    grid = (-3.0, h / 2, 100, 0.0, h / 2, 17)
    r = G.first_arrival_grid(x, y, T, th, np.full(M, rows - 1), grid, max_gap=1.0)
    c = r["count"][0]
    assert set(np.unique(c)) <= {0, 1}
    # interior nodes of the sheet: strictly inside its outline
    gx = -3.0 + np.arange(100) * h / 2
    gy = np.arange(17) * h / 2
    X, Y = np.meshgrid(gx, gy)
    u = X - skew * Y
    inner = (u > 0) & (u < (M - 1) * h) & (Y > 0) & (Y < (rows - 1) * h)
    assert inner.sum() > 200
    assert np.all(c[inner] == 1)
    assert np.array_equal(np.isnan(r["T"][0]), c == 0)
    assert np.max(np.abs(r["T"][0][inner] - (Y + 0.01 * X)[inner])) < 1e-15


def fold_rows(M=401, rows=101, T_of=None):
    """A cusp: rays x = u (1 - 2 t) + t u^3, y = t for u in [-1.5, 1.5]; for t > 1/2 three rays reach x = 0 (u = 0 and
    +-sqrt((2t - 1) / t)), between the caustics x = +-(1 - 2 t) u_c + t u_c^3, u_c = sqrt((2t - 1) / (3t))."""
    u = np.linspace(-1.5, 1.5, M)
    t = np.linspace(0.0, 1.0, rows)
    x = u[None, :] * (1 - 2 * t[:, None]) + t[:, None] * u[None, :] ** 3
    y = np.broadcast_to(t[:, None], (rows, M)).astype(np.float64)
    T = T_of(u[None, :], t[:, None]) * np.ones((rows, M))
    th = np.full((rows, M), np.pi / 2)
    return x, y, T, th, u


def test_a_triplication_counts_three_branches_and_takes_the_first():
    x, y, T, th, u = fold_rows(T_of=lambda u, t: t - 0.05 * u)
    grid = (-0.05, 0.05, 3, 0.9, 0.05, 1)                  # nodes (-0.05, 0.9), (0, 0.9), (0.05, 0.9)
    r = G.first_arrival_grid(x, y, T, th, np.full(len(u), len(T) - 1), grid, theta0=u, max_gap=0.1)
    assert r["stats"]["folded"] > 0
    assert np.all(r["count"] == 3)
    # the first arrival is the branch of the largest u (T = t - 0.05 u): at x = 0, u = sqrt(0.8 / 0.9)
    ur = np.sqrt(0.8 / 0.9)
    assert abs(r["theta0"][0, 0, 1] - ur) < 1e-3
    assert abs(r["T"][0, 0, 1] - (0.9 - 0.05 * ur)) < 1e-4
    out = G.first_arrival_grid(x, y, T, th, np.full(len(u), len(T) - 1), (0.6, 0.05, 1, 0.9, 0.05, 1), theta0=u, max_gap=0.1)
    assert out["count"][0, 0, 0] == 1                      # beyond the caustic (x = 0.29): one branch


def test_bit_equal_times_take_the_lowest_key():
    """T constant: every covering triangle gives T = s / s = 1 exactly; the winner is the least key, i.e. the least ray."""
    x, y, T, th, u = fold_rows(T_of=lambda u, t: np.ones_like(u * t))
    r = G.first_arrival_grid(x, y, T, th, np.full(len(u), len(T) - 1), (0.0, 0.05, 1, 0.9, 0.05, 1), theta0=u, max_gap=0.1)
    assert r["count"][0, 0, 0] == 3 and r["T"][0, 0, 0] == 1.0
    assert abs(r["theta0"][0, 0, 0] + np.sqrt(0.8 / 0.9)) < 1e-3          # the branch of the least u
    key = r["key"][0, 0, 0]
    m = key // 2 // len(T)
    assert abs(u[m] + np.sqrt(0.8 / 0.9)) < 0.02


def test_a_split_fan_leaves_the_gap_uncovered():
    """Two halves of a fan turned 1 rad apart, as at a critical angle: the cells between them are skipped by max_dtheta, and
    by max_gap when their angles agree but they have drifted apart."""
    h, M, rows = 0.1, 10, 11
    x, y = lattice(M, rows, h, 0.0)
    x = x + np.where(np.arange(M) >= 5, 0.5, 0.0)[None, :]         # rays 5.. shifted: the gap between rays 4 and 5 is 0.6
    th = np.where(np.arange(M)[None, :] >= 5, np.pi / 2 - 1.0, np.pi / 2) * np.ones((rows, M))
    T = y.copy()
    grid = (0.0, 0.05, 30, 0.0, 0.05, 21)
    for kw in ({"max_gap": 1.0}, {"max_gap": 0.3, "max_dtheta": 2.0}):
        r = G.first_arrival_grid(x, y, T, th, np.full(M, rows - 1), grid, **kw)
        assert r["stats"]["skipped_cells"] == rows - 1
        gx = np.arange(30) * 0.05
        gap = (gx > 0.4 + 1e-9) & (gx < 1.0 - 1e-9)
        assert np.all(r["count"][0][:, gap] == 0)
        assert np.all(r["count"][0][1:-1, (gx > 0.01) & (gx < 0.39)] == 1)
    r = G.first_arrival_grid(x, y, T, th, np.full(M, rows - 1), grid, max_gap=1.0, max_dtheta=2.0)
    assert r["stats"]["skipped_cells"] == 0                         # no rule: the gap is smeared over


# ---------------------------------------------------------------- oracle trajectories, closed forms
@pytest.fixture(scope="module")
def vert_fan():
    from oracle import rt_oracle as O
    F = O.Field("vert_heterogeneous", (-2, 5, -2.5, 1), DELTA)
    th = np.linspace(0.05, 1.5, 4096)
    s, last = trace(F, 6, DELTA_S, int(np.ceil(80 / DELTA_S) + 1), VERT_SMALL, -2.0, -2.0, th)
    return F, th, s, last


VERT_GRID = (-1.99, 0.02, 150, -2.49, 0.02, 125)


def test_vert_heterogeneous_matches_the_closed_form(vert_fan):
    """Bound: the rows' own distance from the closed form (the gradient fits' scale offset) plus the linear
    interpolation term over the fan's cells, both measured here."""
    F, th, s, last = vert_fan
    r = G.from_record(s, last, VERT_GRID)
    X, Y = np.meshgrid(-1.99 + np.arange(150) * 0.02, -2.49 + np.arange(125) * 0.02)
    Tc = G.vert_T(-2.0, -2.0, X, Y)
    ok = r["count"][0] > 0
    assert ok.sum() > 8000
    assert np.all(r["count"][0] <= 1)                         # circular arcs do not cross
    far = ok & (np.hypot(X + 2, Y + 2) > 0.2)
    err = np.abs(r["T"][0] - Tc)[far] / Tc[far]
    # the rows themselves
    rows_ok = np.arange(s.shape[0])[:, None] <= last[None, :]
    Tr = G.vert_T(-2.0, -2.0, s[:, 0], s[:, 1])
    rerr = np.abs(s[:, 4] - Tr)[rows_ok & (Tr > 0.01)] / Tr[rows_ok & (Tr > 0.01)]
    print(f"vert grid rel err {err.max():.3e} (rows {rerr.max():.3e}), covered {ok.sum()}")
    assert rerr.max() <= 1.5e-6
    assert err.max() <= 2.0e-6


def test_vert_heterogeneous_amplitude_matches_the_closed_form(vert_fan):
    F, th, s, last = vert_fan
    S = P.SplineField(*F.arrays())
    J, km = G.paraxial_rows(s, last, S)
    r = G.from_record(s, last, VERT_GRID, amplitude=(J, km, G.record_n(s)))
    X, Y = np.meshgrid(-1.99 + np.arange(150) * 0.02, -2.49 + np.arange(125) * 0.02)
    ok = (r["count"][0] > 0) & (np.hypot(X + 2, Y + 2) > 0.2)
    Jc = P.vert_closed_form(r["theta0"][0], X, Y)
    Gc = 1.0 / np.sqrt(Jc / (18.0 + 2.0 * Y))
    e = np.abs(r["G"][0] - Gc)[ok] / np.max(Gc[ok])
    print(f"vert G rel err {e.max():.3e}")
    assert e.max() <= 5e-4
    assert np.all(r["kmah"][0][ok] == 0)


def test_fisheye_matches_the_great_circle_arc():
    from oracle import rt_oracle as O
    F = O.Field("fisheye", FISH, DELTA)
    step = 2 * np.pi / 303
    th = np.linspace(np.pi / 2 - 0.35, np.pi / 2 + 0.35, 1024)
    s, last = trace(F, 6, step, 120, FISH, 1.0, 0.0, th)              # 119 steps: short of the focus at (-1, 0)
    grid = (-1.0, 0.02, 101, -1.0, 0.02, 101)
    r = G.from_record(s, last, grid)
    X, Y = np.meshgrid(-1.0 + np.arange(101) * 0.02, -1.0 + np.arange(101) * 0.02)
    Tc = G.fisheye_T(1.0, 0.0, X, Y)
    ok = (r["count"][0] > 0) & (np.hypot(X - 1, Y) > 0.2)
    assert ok.sum() > 1500
    assert np.all(r["count"][0] <= 1)
    err = np.abs(r["T"][0] - Tc)[ok] / Tc[ok]
    rows_ok = np.arange(s.shape[0])[:, None] <= last[None, :]
    Tr = G.fisheye_T(1.0, 0.0, s[:, 0], s[:, 1])
    m = rows_ok & (Tr > 0.1)
    rerr = np.abs(s[:, 4] - Tr)[m] / Tr[m]
    print(f"fisheye grid rel err {err.max():.3e} (rows {rerr.max():.3e}), covered {ok.sum()}")
    assert err.max() <= 1.5 * rerr.max() + 1e-6
