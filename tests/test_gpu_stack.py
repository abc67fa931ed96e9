"""GPU: pick-free detection and location by stacking station traces (rtmi_locate_stack, rtmi_locate_stack_dev; DESIGN.md section
30).  The yardstick of every check is tests/stack_ref.py on the same arrays, compared with np.array_equal (NaN equal to NaN): peak,
peak_node, best, best_m, the whole volume, every field of every event, the count of contributing triples.  Shapes: the grids
37 x 29, 64 x 1, 1 x 70 and 130 x 3, P in {1, 2, 7, 33}, nt in {2, 3, 64, 300}, M in {1, 15, 16, 17, 70}, and the kernel's own
sizes at size - 1, size and size + 1: the tile of 256 nodes (255, 256, 257 nodes), the chunk of 16 scan indices (15, 16, 17), and
the split of the scan: on a 16 x 1 grid every chunk is a part of its own (M = 16: one part, 17 and 18: two, 33: three), and a
scan of 393 221 indices is long enough that a block walks several chunks.  With and without weights."""
import ctypes as C

import numpy as np
import pytest

import stack_ref
from conftest import LIMITS

pytestmark = pytest.mark.gpu

TILE, CHUNK = 256, 16             # stack.hip's kTile and kChunk
EVENT_KEYS = ("m", "node", "ix", "iy", "count", "value", "t0_node", "win", "x", "y", "t0", "dx", "dy", "dm", "refined")
SERIES = ("peak", "peak_node", "best", "best_m", "volume")


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


def problem(nx, ny, P, nt, M, seed, holes=0.0, gaps=0.1, weights=False, offset=1e5):
    """Random stations around a grid in a constant medium, random traces with gaps; the trace axis covers the middle 70 % of the
    times o + T the scan asks for, so that reads fall before the first sample, inside, and past the last one."""
    rng = np.random.default_rng(seed)
    grid = grid_of(nx, ny)
    X, Y = grid[0] + grid[1] * np.arange(nx), grid[3] + grid[4] * np.arange(ny)
    sx, sy = rng.uniform(X[0] - 1.0, X[-1] + 1.0, P), rng.uniform(Y[0] - 1.0, Y[-1] + 1.0, P)
    T = 1.5 * np.hypot(X[None, None, :] - sx[:, None, None], Y[None, :, None] - sy[:, None, None])
    if holes:
        T[rng.random(T.shape) < holes] = np.nan
    od = 0.013
    total = np.nanmax(T) + M * od
    o0 = offset + 3.0
    ct0, cdt = o0 + 0.15 * total, 0.7 * total / (nt - 1)
    c = rng.uniform(0.0, 1.0, (P, nt))
    if gaps:
        c[rng.random(c.shape) < gaps] = np.nan
    w = rng.uniform(0.5, 2.0, P) if weights else None
    return grid, T, c, w, (ct0, cdt, o0, od, M)


def same(got, want, keys, what=""):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


def check(rb, grid, T, c, w, axes, need=0, threshold=-np.inf, min_sep=2, max_events=5, what=""):
    """the host entry against the restatement, everything it returns"""
    ct0, cdt, o0, od, M = axes
    want = stack_ref.stack(T, c, ct0, cdt, o0, od, M, w=w, need=need, threshold=threshold, min_sep=min_sep, max_events=max_events, grid=grid)
    L = rb.Locator(T, grid)
    try:
        got, st = L.stack(c, cdt, t0=ct0, scan=(o0, od, M), weights=w, min_stations=need or None, threshold=threshold, min_sep=min_sep,
                          max_events=max_events, maps=True, volume=True, stats=True)
    finally:
        L.close()
    same(got, want, SERIES + EVENT_KEYS, what)
    assert st["triples"] == M * T.size and st["contributing"] == want["contributing"] and st["truncated"] == want["truncated"], (what, st)
    return got, want, st


# ---------------------------------------------------------------- 1. shapes
SHAPES = [  # nx, ny, P, nt, M, weights
    (37, 29, 7, 300, 70, False), (37, 29, 33, 64, 17, True), (37, 29, 1, 3, 16, False), (37, 29, 2, 2, 15, True),
    (64, 1, 1, 2, 1, False), (64, 1, 2, 64, 17, True), (1, 70, 33, 300, 16, False), (1, 70, 7, 3, 15, True),
    (130, 3, 7, 64, 70, False), (130, 3, 2, 300, 1, True), (255, 1, 7, 64, 16, False), (256, 1, 7, 64, 17, True),
    (257, 1, 33, 64, 15, False), (257, 2, 2, 300, 33, True),
]


@pytest.mark.parametrize("nx,ny,P,nt,M,weights", SHAPES)
def test_every_output_has_the_restatements_bits(rb, nx, ny, P, nt, M, weights):
    grid, T, c, w, axes = problem(nx, ny, P, nt, M, seed=nx + 7 * ny + 13 * P + nt + 31 * M, weights=weights, gaps=0.1 if nt > 3 else 0.0)
    got, want, st = check(rb, grid, T, c, w, axes, need=1)
    assert (want["n"] > 0).any() and (want["n"] < P).any()               # reads fall inside and outside the traces
    assert np.isfinite(got["peak"]).any()


@pytest.mark.parametrize("M,parts,weights", [(15, 1, True), (16, 1, False), (17, 2, True), (18, 2, False), (33, 3, True)])
def test_scan_split_into_parts_of_whole_chunks(rb, M, parts, weights):
    """16 nodes are one tile, so the scan alone fills the device: every chunk of 16 scan indices is a part of its own"""
    grid, T, c, w, axes = problem(16, 1, 7, 64, M, seed=M, weights=weights)
    _, _, st = check(rb, grid, T, c, w, axes, need=3, max_events=M, min_sep=0)
    assert st["parts"] == parts == -(-M // CHUNK)


def test_a_block_that_walks_several_chunks(rb):
    """A scan of 24 577 chunks on one tile: more chunks than the blocks the search aims at, so every block walks several, and
    the two buffers of its reduction are reused"""
    M = CHUNK * 24576 + 5
    grid, T, c, w, _ = problem(16, 1, 2, 64, 70, seed=2)
    span = np.nanmax(T) + 3.0
    o0, od = 1e5, span / M
    axes = (o0 + 0.2 * span, 0.6 * span / 63, o0, od, M)
    _, _, st = check(rb, grid, T, c, w, axes, need=1, min_sep=1000, max_events=4)
    assert 1 <= st["parts"] <= (M + CHUNK - 1) // CHUNK // 3


# ---------------------------------------------------------------- 2. exact hits and ties
def dyadic(M=17, o_shift=0):
    """Everything on a grid of 1 / 64 s, times offset by 1e5 s: f is an integer, 0 and nt - 1 among its values"""
    nx, ny, P, nt = 37, 29, 3, 32
    grid = grid_of(nx, ny)
    x = np.arange(nx * ny).reshape(ny, nx)
    T = np.stack([((x * 7 + r * 13) % 40) / 64.0 for r in range(P)])
    ct0 = 1e5
    o0 = ct0 - 8 / 64.0 + o_shift / 64.0
    return grid, T, np.ones((P, nt)), (ct0, 1 / 64.0, o0, 1 / 64.0, M)


def test_exact_hits_and_ties_go_to_the_least_index(rb):
    grid, T, c, axes = dyadic()
    ct0, cdt, o0, od, M = axes
    f = ((o0 + od * np.arange(M))[:, None, None, None] + T[None] - ct0) / cdt
    assert (f == np.round(f)).all() and (f == 0).any() and (f == 31).any() and (f < 0).any() and (f > 31).any()
    got, want, _ = check(rb, grid, T, c, None, axes, need=1, max_events=M, min_sep=0)
    n = ((f >= 0) & (f < 31)).sum(axis=1)                                        # f = nt - 1 exactly is left out
    assert np.array_equal(want["n"], n)
    cand = n >= 1
    assert np.array_equal(got["volume"], np.where(cand, 1.0, -np.inf))           # constant traces: every S is 1
    first = lambda a, axis: np.where(a.any(axis=axis), a.argmax(axis=axis), -1)  # noqa: E731
    assert np.array_equal(got["peak_node"], first(cand.reshape(M, -1), 1)) and np.array_equal(got["best_m"], first(cand, 0))
    assert list(got["m"]) == list(np.flatnonzero(cand.reshape(M, -1).any(axis=1)))    # all tied: ascending m
    # weights that are powers of two keep every S at 1
    gw, _, _ = check(rb, grid, T, c, np.array([2.0, 0.5, 4.0]), axes, need=1, max_events=M, min_sep=0)
    same(gw, got, ("volume", "peak", "peak_node", "best", "best_m", "m", "node"))


def test_a_scan_split_over_two_calls_is_one_call(rb):
    grid, T, c, _ = dyadic()
    rng = np.random.default_rng(1)
    c = rng.uniform(0.0, 1.0, c.shape)
    whole_axes = dyadic(M=34)[3]
    whole, _, _ = check(rb, grid, T, c, None, whole_axes, need=2)
    a, _, _ = check(rb, grid, T, c, None, dyadic(M=17)[3], need=2)
    b, _, _ = check(rb, grid, T, c, None, dyadic(M=17, o_shift=17)[3], need=2)
    for k in ("peak", "peak_node", "volume"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k], equal_nan=True), k
    later = (b["best_m"] >= 0) & ((a["best_m"] < 0) | (b["best"] > a["best"]))
    assert np.array_equal(np.where(later, b["best"], a["best"]), whole["best"])
    assert np.array_equal(np.where(later, b["best_m"] + 17, a["best_m"]), whole["best_m"])


# ---------------------------------------------------------------- 3. exclusions
def test_holes_gaps_and_a_station_out_for_part_of_the_scan(rb):
    P, M = 7, 70
    grid, T, c, w, axes = problem(37, 29, P, 300, M, seed=21, holes=0.05, gaps=0.1)
    c[3, :150] = np.nan                                       # station 3 has no data for the first half of the traces
    got, want, _ = check(rb, grid, T, c, None, axes, need=P - 2)
    assert np.isneginf(got["volume"]).any() and np.isfinite(got["volume"]).any()
    assert (want["n"] < P - 2).any() and (want["n"] == P).any()
    got, want, _ = check(rb, grid, T, c, None, axes, need=0, what="need absent")   # every station must contribute
    assert (want["n"][got["volume"] > -np.inf] == P).all()


def test_weights_that_drop_stations_and_needs(rb):
    P, M = 7, 33
    grid, T, c, _, axes = problem(37, 29, P, 64, M, seed=22, gaps=0.05)
    w = np.array([1.0, 0.0, 2.0, -1.0, np.nan, np.inf, 0.5])
    got, want, _ = check(rb, grid, T, c, w, axes, need=0, what="need absent: the three valid stations")
    assert want["n"].max() == 3 and np.isfinite(got["peak"]).any()
    # a dropped station is a station that is not there
    keep = np.array([0, 2, 6])
    L = rb.Locator(T[keep], grid)
    ct0, cdt, o0, od, _ = axes
    sub = L.stack(c[keep], cdt, t0=ct0, scan=(o0, od, M), weights=w[keep], maps=True, volume=True)
    L.close()
    same(sub, got, SERIES)
    got2, _, _ = check(rb, grid, T, c, w, axes, need=2, what="need below the valid count")
    assert np.isfinite(got2["volume"]).sum() > np.isfinite(got["volume"]).sum()
    none, _, _ = check(rb, grid, T, c, w, axes, need=4, what="a need nobody meets")
    assert np.isneginf(none["peak"]).all() and (none["peak_node"] == -1).all() and (none["best_m"] == -1).all()
    assert np.isneginf(none["best"]).all() and np.isneginf(none["volume"]).all() and len(none["m"]) == 0
    allbad, _, _ = check(rb, grid, T, c, np.zeros(P), axes, need=0, what="no valid station")
    assert (allbad["peak_node"] == -1).all()


# ---------------------------------------------------------------- 4. consistency
@pytest.mark.parametrize("nx,ny", [(64, 1), (1, 70), (37, 29)])
def test_windows_projections_and_the_device_form(rb, torch, nx, ny):
    P, M = 7, 17
    grid, T, c, w, axes = problem(nx, ny, P, 64, M, seed=31 + nx, weights=True, holes=0.02)
    ct0, cdt, o0, od, _ = axes
    got, want, _ = check(rb, grid, T, c, w, axes, need=3, threshold=-np.inf, min_sep=0, max_events=M)
    assert list(np.sort(got["m"])) == list(range(M))                             # every scan index is an event: both ends too
    V = got["volume"]
    for k in range(M):
        m, ix, iy = got["m"][k], got["ix"][k], got["iy"][k]
        for d in (-1, 0, 1):
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    inside = 0 <= m + d < M and 0 <= iy + j < ny and 0 <= ix + i < nx
                    v = V[m + d, iy + j, ix + i] if inside else np.nan
                    assert np.array_equal(got["win"][k, d + 1, j + 1, i + 1], v, equal_nan=True), (k, d, j, i)
        assert got["value"][k] == got["peak"][m] == V[m].max() and got["node"][k] == got["peak_node"][m] == V[m].argmax()
    assert not np.isnan(V).any()
    assert np.array_equal(got["peak"], V.reshape(M, -1).max(axis=1)) and np.array_equal(got["best"], V.max(axis=0))
    assert np.array_equal(got["best_m"], np.where(np.isfinite(V).any(axis=0), V.argmax(axis=0), -1))
    dev = "cuda:0"
    L = rb.Locator(T, grid)
    d = L.stack_device(torch.from_numpy(c).to(dev), cdt, t0=ct0, scan=(o0, od, M), weights=torch.from_numpy(w).to(dev), min_stations=3,
                       threshold=-np.inf, min_sep=0, max_events=M, maps=True, volume=True)
    for k in SERIES:
        assert d[k].is_cuda
        d[k] = d[k].cpu().numpy()
    same(d, got, SERIES + EVENT_KEYS, "stack_device")
    plain = L.stack(c, cdt, t0=ct0, scan=(o0, od, M), weights=w, min_stations=3, threshold=-np.inf, max_events=3, refine=False)
    assert "best" not in plain and "volume" not in plain
    assert np.array_equal(plain["t0"], plain["t0_node"]) and not plain["refined"].any() and np.array_equal(plain["x"], grid[0] + plain["ix"] * grid[1])
    with pytest.raises(ValueError, match="on a GPU"):
        L.stack_device(torch.from_numpy(c), cdt, t0=ct0, scan=(o0, od, M))
    with pytest.raises(TypeError, match="float64"):
        L.stack_device(torch.from_numpy(c).to(dev).float(), cdt, t0=ct0, scan=(o0, od, M))
    L.close()


def test_refusals_that_need_a_handle(rb):
    from raytracing_amd import _lib
    grid, T, c, _, axes = problem(130, 32, 1, 8, 4, seed=5)                      # 4 160 nodes: 17 tiles
    ct0, cdt, o0, od, _ = axes
    L = rb.Locator(T, grid)
    with pytest.raises(_lib.RtmiError, match=r"rtmi_locate_stack: M is over 2\^31 - 17, or more than 2\^31 \(tile of 256 nodes, chunk of 16"):
        sp = L._stack_params("t", 8, cdt, ct0, (o0, od, 2 ** 31 - 17), None, 0.0, 0, 0)
        buf, ibuf, nev = (C.c_double * 8)(), (C.c_int32 * 8)(), C.c_int64(0)
        _lib.check(_lib.lib().rtmi_locate_stack(L._h, C.byref(sp), _lib.dptr(np.ascontiguousarray(c)), None, buf, ibuf, None, None, None,
                                                None, C.byref(nev), None))
    with pytest.raises(_lib.RtmiError, match="rtmi_locate_stack: need is negative"):
        L.stack(c, cdt, t0=ct0, scan=(o0, od, 4), min_stations=-1)
    assert np.isfinite(L.stack(c, cdt, t0=ct0, scan=(o0, od, 4), min_stations=1)["peak"]).any()     # the handle stays usable
    L.close()
    with pytest.raises(RuntimeError, match="closed"):
        L.stack(c, cdt, t0=ct0, scan=(o0, od, 4))


# ---------------------------------------------------------------- 5. traced tables, arrival times by another path
def test_traced_tables_stack_finds_planted_events(rb):
    """vert_heterogeneous, op6, the stations and grid of test_traced_tables_locate_two_point_picks.  Traces: Gaussian pulses at the
    two_point arrival times of three off-grid events, a path that never sees the tables.  Every output has the restatement's
    bits, exactly the three events are found, each node within 1.5 cells of the truth; the distances are printed (DESIGN.md
    section 30 records them)."""
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
    ev = np.array([[0.43, -1.37], [2.21, -0.52], [1.32, -0.11]])
    to_right = rb.two_point(rb.op6, F, ev, (1.0, 0.0, 4.0), ys, thetas=np.linspace(-1.5, 1.5, 512), **kw)
    to_left = rb.two_point(rb.op6, F, ev, (1.0, 0.0, -1.5), ys, thetas=np.linspace(np.pi - 1.5, np.pi + 1.5, 512), **kw)
    F.close()
    first = lambda r: np.where(r["count"] > 0, r["T"][:, :, 0], np.nan)          # noqa: E731
    tt = np.concatenate([first(to_right), first(to_left)], axis=1)               # [event, station]
    assert (np.isfinite(tt).sum(axis=1) >= 12).all()
    tmax = float(np.nanmax(T))
    cdt = od = tmax / 200.0
    sigma = 4.0 * cdt
    origin = 50.0 + tmax * np.array([0.31, 1.13, 1.87])
    M, nt, ct0, o0 = 460, 700, 50.0, 50.0
    t = ct0 + cdt * np.arange(nt)
    rng = np.random.default_rng(13)
    with np.errstate(invalid="ignore"):
        pulses = np.exp(-0.5 * ((t[None, None, :] - (origin[:, None] + tt)[:, :, None]) / sigma) ** 2)
    c = np.nan_to_num(pulses).sum(axis=0) + 0.02 * np.abs(rng.standard_normal((16, nt)))
    args = dict(threshold=0.9, min_sep=60, max_events=10)
    want = stack_ref.stack(T, c, ct0, cdt, o0, od, M, need=10, grid=grid, **args)
    L = rb.Locator.from_table({"T": T}, grid)
    got, st = L.stack(c, cdt, t0=ct0, scan=(o0, od, M), min_stations=10, maps=True, volume=True, stats=True, **args)
    L.close()
    same(got, want, SERIES + EVENT_KEYS)
    assert st["contributing"] == want["contributing"]
    print(f"traced case: {len(got['m'])} events, values {got['value']}, counts {got['count']}, stations with an arrival {np.isfinite(tt).sum(axis=1)}")
    assert len(got["m"]) == 3
    k = np.array([int(np.argmin(np.abs(got["t0_node"] - o))) for o in origin])
    assert sorted(k) == [0, 1, 2]
    cx, cy = (ev[:, 0] - grid[0]) / grid[1], (ev[:, 1] - grid[3]) / grid[4]
    node_d = np.hypot(got["ix"][k] - cx, got["iy"][k] - cy)
    ref_d = np.hypot((got["x"][k] - ev[:, 0]) / grid[1], (got["y"][k] - ev[:, 1]) / grid[4])
    print(f"traced case: node {node_d} cells, refined {ref_d} cells, t0 {np.abs(got['t0'][k] - origin)} s (od {od:.4f} s), "
          f"refined flags {got['refined'][k]}")
    assert (node_d <= 1.5).all()
