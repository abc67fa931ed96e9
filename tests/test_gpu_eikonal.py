"""GPU: the eikonal continuation of traveltime tables (rtmi_eikonal_fill, rtmi_eikonal_fill_dev, traveltime_table(fill="eikonal");
DESIGN.md section 34).  The yardstick is tests/eikonal_ref.py, the serial sweeps in Python floats, and every comparison is bit
for bit on T, rounds, converged and filled, NaN positions included.  Shapes: a corridor that winds against the sweeps and needs
seven rounds (asserted in tests/test_eikonal_ref.py), with and without a cap on the rounds; the grids 1 x 1, 1 x 70, 70 x 1,
5 x 70, 64 x 64 and 65 x 63 (diagonals of 1, 5, 63 and 64 nodes in a block of one wave), 80 x 80 (two waves, the last not full) and
100 x 90, which is over the LDS path's 7 710 nodes, each on the LDS path where it fits and on the global path; 300 x 260 on the
global path, whose diagonals of 260 nodes make the 256 lanes stride; seeds in every state; the device-pointer form; repeated
runs; the split of a call over its sources; an absent table; and one case traced through vert_heterogeneous, which no table
without the continuation passes."""
import ctypes as C
import functools

import numpy as np
import pytest

import eikonal_ref as R
from conftest import LIMITS

pytestmark = pytest.mark.gpu


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


def same(got, want, what=""):
    assert R.same_bits(got["T"], want["T"]), f"{what}: T differs at {int((~np.isclose(got['T'], want['T'], rtol=0, atol=0, equal_nan=True)).sum())} nodes"
    assert np.array_equal(got["rounds"], want["rounds"]), (what, got["rounds"], want["rounds"])
    assert np.array_equal(got["converged"], want["converged"]), (what, got["converged"], want["converged"])
    assert got["filled"].dtype == np.uint8 and np.array_equal(got["filled"], want["filled"]), what


def check_stats(st, want, path):
    assert st["path"] == path and st["filled"] == int(want["filled"].sum()) and st["changes"] == want["changes"]
    assert st["rounds_max"] == int(want["rounds"].max()) and st["free_nodes"] == st["filled"] + st["unreached"]
    assert st["kernel_ms"] > 0.0


# ------------------------------------------------------------------------------------------------- the several-round medium
CORRIDOR_GRID = (0.0, 1.0, 31, 0.0, 1.0, 27)


@functools.lru_cache(maxsize=None)
def corridor(max_rounds=0):
    n, (ix, iy) = R.winding_corridor()
    src = np.array([[ix + 0.25, iy - 0.125], [15.0, 13.0], [29.0 - 0.5, 1.0 + 0.375]])       # the outer end, the middle, a far corner
    ns = np.array([1.0, 1.0, 1.0])
    return n, src, ns, R.solve(CORRIDOR_GRID, n, src, ns, max_rounds=max_rounds)


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_that_needs_several_rounds(rb, global_path):
    n, src, ns, want = corridor()
    assert want["rounds"][0] == 7 and (want["rounds"] >= 3).all() and want["converged"].all()
    got = rb.eikonal_fill(n, src, CORRIDOR_GRID, n_src=ns, stats=True, _global_path=global_path)
    same(got, want, "corridor")
    check_stats(got["stats"], want, "global" if global_path else "lds")


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_under_a_cap_of_one_round(rb, global_path):
    n, src, ns, want = corridor(max_rounds=1)
    assert (want["rounds"] == 1).all() and not want["converged"].any()
    got = rb.eikonal_fill(n, src, CORRIDOR_GRID, n_src=ns, max_rounds=1, _global_path=global_path)
    same(got, want, "corridor, max_rounds 1")
    assert not R.same_bits(got["T"], corridor()[3]["T"])


# --------------------------------------------------------------------------------------------------------------- shapes
def smooth_problem(nx, ny, S, seed):
    """a smooth medium with a slow lens, spacings that differ, sources inside the grid and off its nodes"""
    rng = np.random.default_rng(seed)
    grid = (-2.0, 0.1, nx, -2.3, 0.125, ny)
    X, Y = R.nodes(grid)
    cx, cy = X.mean(), Y.mean()
    n = 1.0 + 0.05 * (X - X.min()) + 0.6 * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (0.1 * max(nx, ny)) ** 2)
    src = np.stack([rng.uniform(X.min(), X.max() + 1e-9, S), rng.uniform(Y.min(), Y.max() + 1e-9, S)], axis=1)
    ns = 1.0 + 0.05 * (src[:, 0] - X.min()) + 0.6 * np.exp(-((src[:, 0] - cx) ** 2 + (src[:, 1] - cy) ** 2) / (0.1 * max(nx, ny)) ** 2)
    return grid, n, src, ns


SHAPES = [(1, 1), (1, 70), (70, 1), (5, 70), (64, 64), (65, 63), (80, 80), (100, 90)]


@functools.lru_cache(maxsize=None)
def shape_case(nx, ny):
    grid, n, src, ns = smooth_problem(nx, ny, 2, 100 * nx + ny)
    return grid, n, src, ns, R.solve(grid, n, src, ns)


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_where_lane_wave_and_block_loops_can_go_wrong(rb, nx, ny, global_path):
    grid, n, src, ns, want = shape_case(nx, ny)
    assert want["filled"].all() and want["converged"].all()
    got = rb.eikonal_fill(n, src, grid, n_src=ns, stats=True, _global_path=global_path)
    same(got, want, f"{nx} x {ny}")
    check_stats(got["stats"], want, "global" if global_path or nx * ny * 17 > 128 * 1024 else "lds")


def test_grid_over_the_lds_capacity_with_striding_lanes(rb):
    """300 x 260: 78 000 nodes against the LDS path's 7 710, and diagonals of 260 nodes for 256 lanes"""
    grid, n, src, ns = smooth_problem(300, 260, 2, 7)
    want = R.solve(grid, n, src, ns)
    got = rb.eikonal_fill(n, src, grid, n_src=ns, stats=True)
    same(got, want, "300 x 260")
    check_stats(got["stats"], want, "global")


# ------------------------------------------------------------------------------------------------------ seeds in every state
@functools.lru_cache(maxsize=None)
def seeded_case():
    rng = np.random.default_rng(23)
    grid, n, src, ns = smooth_problem(37, 29, 3, 5)
    n = n.copy()
    n[8:15, 20] = n[8, 20:27] = n[14, 20:27] = n[8:15, 26] = 0.0         # a sealed pocket behind obstacles ...
    n[3, 3], n[4, 3], n[20, 30] = np.nan, -2.0, np.inf                    # ... and obstacles of every kind
    X, Y = R.nodes(grid)
    T = np.empty((3,) + n.shape)
    for s in range(3):
        exact = 1.1 * np.hypot(X - src[s, 0], Y - src[s, 1])
        u = rng.random(n.shape)
        T[s] = np.where(u < 0.3, exact, np.where(u < 0.6, np.nan, np.where(u < 0.8, np.inf, -np.inf)))
        T[s, 8, 22], T[s, 3, 3] = 5.0, -np.inf                            # obstacles with inputs: they are their outputs
        T[s, 9:14, 21:26] = np.nan                                       # the pocket's inside: unreachable
    T[2, 11, 23] = 0.25                                                   # ... but for the source that has a seed in there
    return grid, n, src, ns, T, R.solve(grid, n, src, ns, T=T)


@pytest.mark.parametrize("global_path", [False, True])
def test_seeds_obstacles_and_a_sealed_pocket(rb, global_path):
    grid, n, src, ns, T, want = seeded_case()
    assert np.isnan(want["T"][:2, 9:14, 21:26]).all() and np.isfinite(want["T"][2, 9:14, 21:26]).all()
    keep = T.copy()
    got = rb.eikonal_fill(n, src, grid, T, n_src=ns, stats=True, _global_path=global_path)
    same(got, want, "seeded")
    assert R.same_bits(T, keep)                                           # the caller's table is not modified by the host form
    seeded = np.isfinite(T) & np.isfinite(n) & (n > 0)
    assert R.same_bits(got["T"][seeded], T[seeded]) and not got["filled"][seeded].any()
    assert got["stats"]["unreached"] > 0


def test_device_form_repeated_runs_and_split_over_sources(rb, torch):
    grid, n, src, ns, T, want = seeded_case()
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    for rep in range(2):
        d_T = up(T)
        got = rb.eikonal_fill_device(up(n), up(src), grid, d_T, n_src=up(ns))
        assert got["T"] is d_T and got["filled"].dtype == torch.uint8
        same({"T": d_T.cpu().numpy(), "rounds": got["rounds"], "converged": got["converged"], "filled": got["filled"].cpu().numpy()},
             want, f"device form, run {rep}")
    # S = 5 in one call against five calls of one source
    grid, n, src, ns = smooth_problem(41, 23, 5, 77)
    whole = rb.eikonal_fill(n, src, grid, n_src=ns)
    for s in range(5):
        one = rb.eikonal_fill(n, src[s:s + 1], grid, n_src=ns[s:s + 1])
        same(one, {k: whole[k][s:s + 1] for k in ("T", "rounds", "converged", "filled")}, f"source {s} alone")
    same(whole, R.solve(grid, n, src, ns), "five sources")


def test_absent_table_is_a_table_of_nan(rb, torch):
    from raytracing_amd import _lib
    grid, n, src, ns = smooth_problem(33, 21, 2, 9)
    want = R.solve(grid, n, src, ns)
    same(rb.eikonal_fill(n, src, grid, n_src=ns), want, "T=None")
    same(rb.eikonal_fill(n, src, grid, np.full((2, 21, 33), np.nan), n_src=ns), want, "T all NaN")
    dev = torch.device("cuda:0")
    got = rb.eikonal_fill_device(torch.as_tensor(n, device=dev), torch.as_tensor(src, device=dev), grid, None,
                                 n_src=torch.as_tensor(ns, device=dev))
    assert R.same_bits(got["T"].cpu().numpy(), want["T"])
    # the C entry with a null T: no table comes back, rounds and filled are those of the all-NaN input
    rounds = np.zeros((2, 2), dtype=np.int32)
    filled = np.zeros((2, 21, 33), dtype=np.uint8)
    ep = rb.eikonal_params(grid)
    _lib.check(_lib.lib().rtmi_eikonal_fill(C.byref(ep), _lib.dptr(n), 2, _lib.dptr(src), _lib.dptr(ns), None,
                                            rounds.ctypes.data_as(_lib._ip), filled.ctypes.data_as(C.POINTER(C.c_uint8)), None))
    assert np.array_equal(rounds[:, 0], want["rounds"]) and np.array_equal(rounds[:, 1], want["converged"])
    assert np.array_equal(filled, want["filled"])
    # a source off the grid without a table: no seed, no round
    off = rb.eikonal_fill(n, [[40.0, 0.0]], grid, n_src=[1.0])
    assert np.isnan(off["T"]).all() and off["rounds"][0] == 0 and off["converged"][0] == 1 and not off["filled"].any()


def test_device_form_refuses_host_memory(rb, torch):
    from raytracing_amd import _lib
    grid, n, src, ns = smooth_problem(9, 7, 1, 1)
    ep = rb.eikonal_params(grid)
    rc = _lib.lib().rtmi_eikonal_fill_dev(C.byref(ep), n.ctypes.data, 1, src.ctypes.data, ns.ctypes.data, None, None, None, None)
    assert rc == -1 and b"d_n is not memory" in _lib.lib().rtmi_last_error()
    with pytest.raises(ValueError, match="on a GPU"):
        rb.eikonal_fill_device(torch.as_tensor(n), torch.as_tensor(src), grid, n_src=torch.as_tensor(ns))


# ---------------------------------------------------------------------------------------------------------- the traced case
TRACED_GRID = (-1.0, 0.065, 71, -2.2, 0.05, 57)
# the largest error of a filled node against the closed form, as a fraction of the tables' largest T: the restatement on the
# device's own unfilled tables gives FILLED_ERROR_MEASURED; the bound is that figure rounded up to one digit
FILLED_ERROR_MEASURED = 7.594e-2
FILLED_ERROR_BOUND = 8e-2


def test_traced_tables_completed_and_located_in_a_shadow(rb):
    """vert_heterogeneous, op6, 16 stations on the lines x = 4 and x = -1.5 as in test_traced_tables_locate_two_point_picks, on
    its 71 x 57 grid, but each with a fan of 0.05 .. 1.5 rad only, measured from the horizontal towards the grid (mirrored for the
    stations on x = 4): most of each table is NaN.  traveltime_table(fill="eikonal") leaves no NaN, keeps the covered nodes' bits,
    is the restatement's completion bit for bit, and lies within a bound of the closed form at the filled nodes.  An event at a
    node that the unfilled tables leave uncovered for at least one station, with picks from the closed form: the locator over
    the filled tables counts all 16 picks there and finds it within one cell; over the unfilled tables that node is no candidate
    for 16 picks, and with fewer asked for the count is smaller.  The filled nodes' error is large here by design of the case:
    most filled nodes lie behind the wedge, where the continuation bends round its edge and the true first arrival is a direct ray
    that was not shot (shoot the full fan)."""
    box = LIMITS["vert_heterogeneous"]
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    grid = TRACED_GRID
    ys = np.linspace(-2.1, 0.5, 8)
    kw = dict(step=rb.DELTA_S, max_size=ms, box=box)
    fan = np.linspace(0.05, 1.5, 512)
    st_right, st_left = np.stack([np.full(8, 4.0), ys], axis=1), np.stack([np.full(8, -1.5), ys], axis=1)
    stations = np.concatenate([st_right, st_left])
    plain = [rb.traveltime_table(rb.op6, F, st_right, grid, thetas=(np.pi - fan)[::-1].copy(), **kw),
             rb.traveltime_table(rb.op6, F, st_left, grid, thetas=fan, **kw)]
    full = [rb.traveltime_table(rb.op6, F, st_right, grid, thetas=(np.pi - fan)[::-1].copy(), fill="eikonal", **kw),
            rb.traveltime_table(rb.op6, F, st_left, grid, thetas=fan, fill="eikonal", **kw)]
    # fill=None is the call without the argument, bit for bit
    none = rb.traveltime_table(rb.op6, F, st_left, grid, thetas=fan, fill=None, **kw)
    assert sorted(none) == sorted(plain[1]) and "filled" not in none
    for k in none:
        assert none[k].dtype == plain[1][k].dtype and np.array_equal(none[k], plain[1][k], equal_nan=True), k
    # every column but T is the unfilled table's; T is complete, and the covered nodes keep their bits
    for p, f in zip(plain, full):
        assert sorted(f) == sorted(list(p) + ["filled"])
        for k in p:
            if k != "T":
                assert np.array_equal(f[k], p[k], equal_nan=True), k
    T0, T1 = np.concatenate([p["T"] for p in plain]), np.concatenate([f["T"] for f in full])
    filled = np.concatenate([f["filled"] for f in full])
    covered = np.isfinite(T0)
    assert 0.05 < covered.mean() < 0.9
    assert np.isfinite(T1).all()
    assert R.same_bits(T1[covered], T0[covered]) and np.array_equal(filled == 1, ~covered)
    assert (np.concatenate([f["count"] for f in full])[~covered] == 0).all()
    # the restatement on the device's own unfilled tables, with the field's own samples
    X, Y = R.nodes(grid)
    n = F.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(X.shape)
    ns = F.n_gradient(stations[:, 0], stations[:, 1])[0]
    want = R.solve(grid, n, stations, ns, T=T0)
    assert R.same_bits(T1, want["T"]) and np.array_equal(filled, want["filled"])
    truth = np.stack([R.gradient_truth(X, Y, sx, sy) for sx, sy in stations])
    err = float(np.max(np.abs(want["T"] - truth)[filled == 1]) / truth.max())
    err_covered = float(np.max(np.abs(T0 - truth)[covered]) / truth.max())
    print(f"traced case: {int(filled.sum())} of {filled.size} nodes filled, error at the filled nodes {err:.3e} of the largest T "
          f"({truth.max():.4f} s), at the covered nodes {err_covered:.3e}")
    # an event at a node in the shadow of at least one station: the interior node with the fewest such stations, the first of them
    holes = (~covered).sum(axis=0)
    inner = np.zeros(holes.shape, dtype=bool)
    inner[5:-5, 5:-5] = True
    cand = np.where(inner & (holes >= 1), holes, 99)
    iy, ix = np.unravel_index(np.argmin(cand), cand.shape)
    assert 1 <= holes[iy, ix] < 99
    ex, ey = grid[0] + ix * grid[1], grid[3] + iy * grid[4]
    picks = 12.5 + np.array([[float(R.gradient_truth(ex, ey, sx, sy)) for sx, sy in stations]])
    L1 = rb.Locator.from_table({"T": T1}, grid)
    got = L1.locate(picks)
    L1.close()
    L0 = rb.Locator.from_table({"T": T0}, grid)
    old = L0.locate(picks, maps=True)
    old_any = L0.locate(picks, min_picks=1)
    L0.close()
    F.close()
    print(f"traced case: event at node ({ix}, {iy}), uncovered for {int(holes[iy, ix])} stations; filled tables: node "
          f"({int(got['ix'][0])}, {int(got['iy'][0])}) count {int(got['count'][0])} rms {got['rms'][0]:.3e} s t0 {got['t0'][0]:.4f}; "
          f"unfilled: node {int(old['node'][0])} count {int(old['count'][0])}; with min_picks 1: node ({int(old_any['ix'][0])}, "
          f"{int(old_any['iy'][0])}) count {int(old_any['count'][0])}")
    assert got["count"][0] == 16 and abs(int(got["ix"][0]) - ix) <= 1 and abs(int(got["iy"][0]) - iy) <= 1
    # the unfilled tables: with all 16 picks asked for the event's node is no candidate, and the answer, if there is one, lies
    # elsewhere; with fewer asked for, fewer contribute
    assert not np.isfinite(old["maps"][0, iy, ix])
    assert old["node"][0] < 0 or max(abs(int(old["ix"][0]) - ix), abs(int(old["iy"][0]) - iy)) > 1
    assert old_any["count"][0] < 16
    assert err <= FILLED_ERROR_BOUND
