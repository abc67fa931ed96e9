"""GPU: event location by grid search over device traveltime tables (rtmi_locator_*, rtmi_locate, rtmi_locate_dev; DESIGN.md
section 29).  The yardstick of every check is tests/locate_ref.py on the same arrays, compared with np.array_equal (NaN equal to
NaN): node, count, sw, obj, ref, t0, both windows, the whole of maps and the refined location.  Shapes: the grids 37 x 29,
64 x 1, 1 x 70 and 130 x 3, P in {1, 2, 7, 33, 65, 512}, E in {1, 5, 70}, and the kernel's own sizes at size - 1, size and
size + 1: the tile of 256 nodes (255, 256, 257 nodes) and the chunk of 16 events (15, 16, 17 events); the search has no staging
of stations, every P takes the same path, but two variants per chunk: one for a chunk whose 16 events have all their picks
(E = 16, the first chunks of E = 70) and one that reads a mask per station (a last chunk that is not full, missing picks).  Holes in the tables, picks that are missing or dropped by their weight, a need nobody
meets, picks offset by 1e5 s, ties, best nodes on the rim, the device-pointer form, the split of a call in two, and one case
traced through vert_heterogeneous."""
import ctypes as C

import numpy as np
import pytest

import locate_ref
from conftest import LIMITS

pytestmark = pytest.mark.gpu

KEYS = ("node", "ix", "iy", "count", "sw", "obj", "ref", "win_obj", "win_tau")
REFINED = ("x", "y", "dx", "dy", "refined")


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def grid_of(nx, ny):
    return (-2.0, 0.1, nx, -2.3, 0.125, ny)


def problem(nx, ny, P, E, seed, holes=0.0, weights=False, offset=0.0, noise=0.01):
    """random stations around a grid in a constant medium, events at random places in it, noisy picks with an origin time"""
    rng = np.random.default_rng(seed)
    grid = grid_of(nx, ny)
    X, Y = grid[0] + grid[1] * np.arange(nx), grid[3] + grid[4] * np.arange(ny)
    sx, sy = rng.uniform(X[0] - 1.0, X[-1] + 1.0, P), rng.uniform(Y[0] - 1.0, Y[-1] + 1.0, P)
    T = 1.5 * np.hypot(X[None, None, :] - sx[:, None, None], Y[None, :, None] - sy[:, None, None])
    if holes:
        T[rng.random(T.shape) < holes] = np.nan
    ex, ey = rng.uniform(X[0], X[-1] + 1e-9, E), rng.uniform(Y[0], Y[-1] + 1e-9, E)
    t = offset + rng.uniform(0.0, 5.0, E)[:, None] + 1.5 * np.hypot(ex[:, None] - sx[None, :], ey[:, None] - sy[None, :])
    t += noise * rng.standard_normal(t.shape)
    w = rng.uniform(0.5, 2.0, t.shape) if weights else None
    return grid, T, t, w


def same(got, want, keys, what=""):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


def check(rb, grid, T, t, w=None, need=None, what=""):
    """the host entry against the restatement, everything it returns"""
    want = locate_ref.locate(T, t, w=w, need=need, grid=grid)
    L = rb.Locator(T, grid)
    try:
        got, st = L.locate(t, weights=w, min_picks=need, maps=True, stats=True)
    finally:
        L.close()
    same(got, want, KEYS + REFINED + ("maps",), what)
    assert np.array_equal(got["t0_node"], want["t0"], equal_nan=True), what
    assert np.array_equal(got["t0"], want["t0_refined"], equal_nan=True), what
    c = want["cov"]
    assert np.array_equal(got["cov"], np.stack([c[:, 0], c[:, 1], c[:, 1], c[:, 2]], axis=1).reshape(-1, 2, 2), equal_nan=True), what
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got["rms"], np.sqrt(want["obj"]), equal_nan=True)
    # the window is the map's 3 x 3 slice
    ny, nx = T.shape[1:]
    for e in range(len(t)):
        ix, iy = got["ix"][e], got["iy"][e]
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                inside = got["node"][e] >= 0 and 0 <= iy + j < ny and 0 <= ix + i < nx
                m = got["maps"][e, iy + j, ix + i] if inside else np.nan
                assert np.array_equal(got["win_obj"][e, j + 1, i + 1], m, equal_nan=True), (what, e, j, i)
    assert st["triples"] == len(t) * T.size
    valid = np.isfinite(t) if w is None else np.isfinite(t) & np.isfinite(w) & (w > 0)
    assert st["contributing"] == int((valid[:, :, None, None] & np.isfinite(T)[None]).sum())
    return got, want


# ---------------------------------------------------------------- 1. shapes
SHAPES = [  # nx, ny, P, E, weights
    (37, 29, 7, 70, False), (37, 29, 33, 5, True), (37, 29, 1, 70, False), (37, 29, 512, 1, True), (37, 29, 65, 70, True),
    (64, 1, 1, 1, False), (64, 1, 2, 17, True), (1, 70, 65, 16, False), (1, 70, 7, 15, True), (130, 3, 512, 5, False),
    (130, 3, 2, 70, True), (255, 1, 7, 16, False), (256, 1, 7, 17, True), (257, 1, 33, 15, False), (16, 16, 2, 5, False),
]


@pytest.mark.parametrize("nx,ny,P,E,weights", SHAPES)
def test_every_output_has_the_restatements_bits(rb, nx, ny, P, E, weights):
    grid, T, t, w = problem(nx, ny, P, E, seed=nx + 7 * ny + 13 * P + E, weights=weights)
    got, _ = check(rb, grid, T, t, w)
    assert (got["node"] >= 0).all() and (got["count"] == P).all()
    if nx >= 3 and ny >= 3 and P >= 7:
        assert got["refined"].any()


# ---------------------------------------------------------------- 2. holes
@pytest.mark.parametrize("need_all", [True, False])
def test_tables_with_holes(rb, need_all):
    """5 % NaN in every table: with need absent only the nodes all stations cover are candidates, with need = P - 2 more are"""
    P, E = 33, 17
    grid, T, t, w = problem(37, 29, P, E, seed=3, holes=0.05, weights=not need_all)
    need = None if need_all else np.full(E, P - 2, dtype=np.int32)
    got, want = check(rb, grid, T, t, w, need)
    assert (got["node"] >= 0).all()
    assert np.isinf(got["maps"]).any() and np.isfinite(got["maps"]).any()
    assert (got["count"] == P).all() if need_all else ((got["count"] >= P - 2).all() and (got["count"] < P).any())
    assert np.isinf(got["win_obj"]).any() or not need_all     # a hole next to a best node shows as +inf in its window


def test_a_table_that_is_nan_everywhere_and_a_need_nobody_meets(rb):
    P, E = 7, 5
    grid, T, t, w = problem(37, 29, P, E, seed=4)
    T[2] = np.nan
    got, _ = check(rb, grid, T, t, None, None, "need absent")              # need = 7 valid picks, but at most 6 contribute
    assert (got["node"] == -1).all() and (got["count"] == 0).all() and np.isinf(got["maps"]).all()
    for k in ("sw", "obj", "t0", "x", "y", "rms", "win_obj", "win_tau", "cov", "ref"):
        assert np.isnan(got[k]).all(), k
    got, _ = check(rb, grid, T, t, None, np.array([6, 6, 7, 0, 1], dtype=np.int32), "need given")
    assert list(got["node"] >= 0) == [True, True, False, True, True] and list(got["count"][[0, 1, 3, 4]]) == [6] * 4


# ---------------------------------------------------------------- 3. picks
def test_missing_picks_and_weights_that_drop_picks(rb):
    P, E = 7, 18
    grid, T, t, w = problem(37, 29, P, E, seed=5, weights=True)
    rng = np.random.default_rng(6)
    t[rng.random(t.shape) < 0.2] = np.nan
    t[3] = np.nan                                            # an event with no valid pick
    t[:, 0][::2] = np.nan                                    # ref is then not station 0's pick
    check(rb, grid, T, t, None, None, "NaN picks")
    for k, bad in enumerate((0.0, -1.0, np.nan, np.inf)):
        w[k::4][rng.random(w[k::4].shape) < 0.3] = bad
    w[5] = 0.0                                               # every pick of the event dropped by its weight
    got, _ = check(rb, grid, T, t, w, None, "weights")
    assert got["node"][3] == -1 and got["node"][5] == -1 and (np.delete(got["node"], [3, 5]) >= 0).all()
    # a pick that its weight drops is a pick that is missing
    t2 = np.where(np.isfinite(w) & (w > 0), t, np.nan)
    w2 = np.where(np.isfinite(w) & (w > 0), w, 1.0)
    L = rb.Locator(T, grid)
    a, b = L.locate(t, weights=w, maps=True), L.locate(t2, weights=w2, maps=True)
    L.close()
    same(a, b, KEYS + REFINED + ("maps", "t0", "cov"))


def test_no_weights_is_weights_of_one(rb):
    """Equal here because 1 * d = d and (1 * u) * u = u * u exactly, and a sum of n ones is n: a property of the weight 1.0, not
    of the entry -- any other constant weight rounds differently."""
    grid, T, t, _ = problem(37, 29, 7, 17, seed=7, holes=0.02)
    need = np.full(17, 5, dtype=np.int32)
    L = rb.Locator(T, grid)
    a, b = L.locate(t, min_picks=need, maps=True), L.locate(t, weights=np.ones_like(t), min_picks=need, maps=True)
    L.close()
    same(a, b, KEYS + REFINED + ("maps", "t0", "cov"))
    check(rb, grid, T, t, np.ones_like(t), need)


def test_picks_offset_by_1e5_seconds(rb):
    """Exact picks of 16 nodes, then the same picks with 1e5 s added.  Adding 1e5 rounds a pick by at most half an ulp of 1e5,
    7.3e-12 s; the reference pick is taken out before anything is squared, so a residual at the true node is at most a few of
    those roundings, below 1e-10 s, and the objective, a mean of their squares, below 1e-20 s^2 -- where the one-pass form
    would leave 1e10 * 2^-53 = 1e-6 s^2 of cancellation noise.  The same node wins, and the origin time moves by 1e5 to 1e-9 s."""
    grid, T, _, _ = problem(37, 29, 7, 1, seed=8)
    rng = np.random.default_rng(8)
    ix, iy = rng.integers(1, 36, 16), rng.integers(1, 28, 16)
    near = rng.uniform(0.0, 5.0, 16)[:, None] + T[:, iy, ix].T
    far = near + 1e5
    got, _ = check(rb, grid, T, far, None)
    base, _ = check(rb, grid, T, near, None)
    assert np.array_equal(got["ix"], ix) and np.array_equal(got["iy"], iy) and np.array_equal(base["node"], got["node"])
    assert (got["obj"] < 1e-20).all() and (base["obj"] < 1e-20).all()
    assert np.abs((got["t0_node"] - 1e5) - base["t0_node"]).max() < 1e-9


def test_negative_need_is_refused_and_the_handle_stays_usable(rb):
    from raytracing_amd import _lib
    grid, T, t, _ = problem(16, 16, 2, 5, seed=9)
    L = rb.Locator(T, grid)
    with pytest.raises(_lib.RtmiError, match=r"rtmi_locate: need\[3\] is negative"):
        L.locate(t, min_picks=np.array([1, 1, 1, -1, 1]))
    assert (L.locate(t)["node"] >= 0).all()
    L.close()
    with pytest.raises(RuntimeError, match="closed"):
        L.locate(t)


# ---------------------------------------------------------------- 4. ties and rims
def test_mirror_symmetric_stations_tie_to_the_least_node(rb):
    """Two stations mirrored in the grid's middle row (the second table is the first one upside down, bit for bit) and events on
    that axis, the same pick at both stations: every node of the middle row fits exactly, obj = +0.0, and the least index among
    them wins -- twice in a row with the same bits.  With two stations a node and its mirror image add the same two terms in
    the other order, so the whole map is mirror-symmetric in its bits."""
    nx, ny = 37, 29
    grid = grid_of(nx, ny)
    X, Y = grid[0] + grid[1] * np.arange(nx), grid[3] + grid[4] * np.arange(ny)
    T = np.empty((2, ny, nx))
    T[0] = 1.5 * np.hypot(X[None, :] - 0.3, Y[:, None] - (Y[ny // 2] + 1.1))
    T[1] = T[0][::-1]
    t = np.array([[2.0, 2.0], [1e5 + 0.7, 1e5 + 0.7], [-3.25, -3.25]])
    for w in (None, np.array([[2.0, 2.0], [0.25, 0.25], [8.0, 8.0]])):   # powers of two: (w d + w d) / (w + w) is d exactly
        got, _ = check(rb, grid, T, t, w)
        L = rb.Locator(T, grid)
        again = [L.locate(t, weights=w, maps=True) for _ in range(2)]
        L.close()
        for a in again:
            same(a, got, KEYS + REFINED + ("maps", "t0", "cov"))
        for e in range(len(t)):
            m = got["maps"][e]
            assert np.array_equal(m, m[::-1])
            assert (m[ny // 2] == 0.0).all() and (np.delete(m, ny // 2, axis=0) > 0.0).all()
            assert got["node"][e] == (ny // 2) * nx and got["ix"][e] == 0 and got["obj"][e] == 0.0 and got["refined"][e] == 0


def test_best_node_on_each_rim_and_in_a_corner(rb):
    nx, ny = 37, 29
    grid, T, _, _ = problem(nx, ny, 7, 1, seed=10)
    nodes = [(0, 12), (nx - 1, 12), (17, 0), (17, ny - 1), (0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx - 1, 0)]
    t = np.stack([4.0 + T[:, iy, ix] for ix, iy in nodes])   # exact picks of a rim node: obj = 0 there
    got, _ = check(rb, grid, T, t)
    for e, (ix, iy) in enumerate(nodes):
        assert (got["ix"][e], got["iy"][e]) == (ix, iy) and got["refined"][e] == 0
        out = np.array([[not (0 <= iy + j < ny and 0 <= ix + i < nx) for i in (-1, 0, 1)] for j in (-1, 0, 1)])
        assert np.array_equal(np.isnan(got["win_obj"][e]), out) and np.array_equal(np.isnan(got["win_tau"][e]), out)
        assert got["x"][e] == grid[0] + ix * grid[1] and got["y"][e] == grid[3] + iy * grid[4] and np.isnan(got["cov"][e]).all()
        assert got["t0"][e] == got["t0_node"][e]


# ---------------------------------------------------------------- 5. entry forms
@pytest.mark.parametrize("weights", [False, True])
def test_device_pointers_and_the_split_of_a_call(rb, torch, weights):
    P, E = 33, 70
    grid, T, t, w = problem(37, 29, P, E, seed=11, holes=0.03, weights=weights)
    need = np.full(E, P - 3, dtype=np.int32)
    L = rb.Locator(T, grid)
    whole = L.locate(t, weights=w, min_picks=need, maps=True)
    dev = "cuda:0"
    d = L.locate_device(torch.from_numpy(t).to(dev), None if w is None else torch.from_numpy(w).to(dev),
                        torch.from_numpy(need).to(dev), maps=True)
    assert d["maps"].is_cuda
    d["maps"] = d["maps"].cpu().numpy()
    same(d, whole, KEYS + REFINED + ("maps", "t0", "cov"), "locate_device")
    # chunking must not show: 70 events in one call are two calls of 35
    halves = [L.locate(t[a:a + 35], weights=None if w is None else w[a:a + 35], min_picks=need[a:a + 35], maps=True) for a in (0, 35)]
    for k in KEYS + REFINED + ("maps", "t0", "cov"):
        assert np.array_equal(np.concatenate([h[k] for h in halves]), whole[k], equal_nan=True), k
    # refine=False reports the node's own values; a scalar min_picks is the array of it
    plain = L.locate(t, weights=w, min_picks=P - 3, refine=False)
    same(plain, whole, KEYS)
    assert np.array_equal(plain["t0"], whole["t0_node"]) and not plain["refined"].any() and np.isnan(plain["cov"]).all()
    assert np.array_equal(plain["x"], grid[0] + whole["ix"] * grid[1])
    with pytest.raises(ValueError, match="on a GPU"):
        L.locate_device(torch.from_numpy(t))
    L.close()


def test_from_table_takes_slot_zero(rb):
    grid, T, t, _ = problem(16, 16, 3, 5, seed=12)
    T4 = np.stack([T, T + 1.0], axis=1)
    a, b = rb.Locator.from_table({"T": T}, grid), rb.Locator.from_table({"T": T4}, grid)
    same(a.locate(t), b.locate(t), KEYS + REFINED)
    a.close()
    b.close()


# ---------------------------------------------------------------- 6. traced tables, picks by another path
def test_traced_tables_locate_two_point_picks(rb):
    """vert_heterogeneous, op6.  Tables: traveltime_table from 16 stations on the lines x = 4 and x = -1.5 onto a 71 x 57 grid.
    Picks: two_point from 8 off-grid events to the stations on both lines, a path that never sees the tables.  The located node is
    within one cell of the truth on both axes; the refined error and the origin-time error are printed (DESIGN.md section 29
    records them; no tighter bound is set here)."""
    box = LIMITS["vert_heterogeneous"]
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    grid = (-1.0, 0.065, 71, -2.2, 0.05, 57)
    ys = np.linspace(-2.1, 0.5, 8)
    kw = dict(step=rb.DELTA_S, max_size=ms, box=box)
    right = rb.traveltime_table(rb.op6, F, np.stack([np.full(8, 4.0), ys], axis=1), grid,
                                thetas=np.linspace(np.pi / 2 + 0.02, 3 * np.pi / 2 - 0.02, 1024), **kw)
    left = rb.traveltime_table(rb.op6, F, np.stack([np.full(8, -1.5), ys], axis=1), grid,
                               thetas=np.linspace(-np.pi / 2 + 0.02, np.pi / 2 - 0.02, 1024), **kw)
    T = np.concatenate([right["T"], left["T"]])
    assert np.isfinite(T).mean() > 0.9
    rng = np.random.default_rng(13)
    ev = np.stack([rng.uniform(-0.3, 2.9, 8), rng.uniform(-1.9, 0.2, 8)], axis=1)
    origin = rng.uniform(10.0, 20.0, 8)
    to_right = rb.two_point(rb.op6, F, ev, (1.0, 0.0, 4.0), ys, thetas=np.linspace(-1.5, 1.5, 512), **kw)
    to_left = rb.two_point(rb.op6, F, ev, (1.0, 0.0, -1.5), ys, thetas=np.linspace(np.pi - 1.5, np.pi + 1.5, 512), **kw)
    first = lambda r: np.where(r["count"] > 0, r["T"][:, :, 0], np.nan)          # noqa: E731
    t = origin[:, None] + np.concatenate([first(to_right), first(to_left)], axis=1)
    assert (np.isfinite(t).sum(axis=1) >= 12).all()
    L = rb.Locator.from_table({"T": T}, grid)
    got = L.locate(t, min_picks=10)
    L.close()
    F.close()
    cx, cy = (ev[:, 0] - grid[0]) / grid[1], (ev[:, 1] - grid[3]) / grid[4]
    node_err = max(np.abs(got["ix"] - cx).max(), np.abs(got["iy"] - cy).max())
    ref_err = max((np.abs(got["x"] - ev[:, 0]) / grid[1]).max(), (np.abs(got["y"] - ev[:, 1]) / grid[4]).max())
    print(f"traced case: node {node_err:.3f} cell, refined {ref_err:.4f} cell ({int(got['refined'].sum())} of 8 refined), "
          f"t0 {np.abs(got['t0'] - origin).max():.3e} s, rms {got['rms'].max():.3e} s")
    assert (got["node"] >= 0).all()
    assert node_err <= 1.0
