"""GPU: robust event location by equal differential time (rtmi_locate_edt, rtmi_locate_edt_dev).  Every
output is compared with the numpy restatement tests/edt_ref.py bit for bit: the device adds and multiplies in the header's
order, exp is one text on both sides, and the reductions are exact minima.  The shapes are the smallest at which the kernels
can go wrong: one full tile, 255 and 257 nodes, five tiles with a partial last one; 2, 3, 7 and 33 stations; 1, 16, 17 and 35
events, so a full chunk, a partial last chunk and several chunks; with and without weights, which are different kernels."""
import ctypes as C

import numpy as np
import pytest

import edt_ref
import locate_ref
from conftest import LIMITS

pytestmark = pytest.mark.gpu

KEYS = ("node", "ix", "iy", "count", "npairs", "value", "ref", "share_sum", "win_val", "win_tau")
REFINED = ("x", "y", "dx", "dy", "refined")
SIGMA = 0.05


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
    """random stations around a grid in a constant medium, events at random places in it, noisy picks with an origin time;
    weights are 1 / sigma^2 of pick errors between 0.02 and 0.1 s"""
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
    w = 1.0 / rng.uniform(0.02, 0.1, t.shape) ** 2 if weights else None
    return grid, T, t, w


def same(got, want, keys, what=""):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


def contributing_pairs(T, t, w):
    valid = np.isfinite(t) if w is None else np.isfinite(t) & np.isfinite(w) & (w > 0)
    n = (valid[:, :, None, None] & np.isfinite(T)[None]).sum(axis=1).astype(np.int64)
    return int((n * (n - 1) // 2).sum())


def check(rb, grid, T, t, sigma=SIGMA, w=None, need=None, what=""):
    """the host entry against the restatement, everything it returns, with maps, share and resid asked for and with none of them"""
    want = edt_ref.locate(T, t, sigma, w=w, need=need, grid=grid)
    L = rb.Locator(T, grid)
    try:
        got, st = L.locate_edt(t, sigma, weights=w, min_picks=need, maps=True, shares=True, stats=True)
        bare = L.locate_edt(t, sigma, weights=w, min_picks=need)
    finally:
        L.close()
    same(got, want, KEYS + REFINED + ("maps", "share", "resid"), what)
    assert np.array_equal(got["t0_node"], want["t0"], equal_nan=True), what
    assert np.array_equal(got["t0"], want["t0_refined"], equal_nan=True), what
    same(bare, got, KEYS + REFINED + ("t0", "t0_node"), what + " without maps, share and resid")
    assert "maps" not in bare and "share" not in bare
    # the window is the map's 3 x 3 slice
    ny, nx = T.shape[1:]
    for e in range(len(t)):
        ix, iy = got["ix"][e], got["iy"][e]
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                inside = got["node"][e] >= 0 and 0 <= iy + j < ny and 0 <= ix + i < nx
                m = got["maps"][e, iy + j, ix + i] if inside else np.nan
                assert np.array_equal(got["win_val"][e, j + 1, i + 1], m, equal_nan=True), (what, e, j, i)
    P = T.shape[0]
    assert st["triples"] == len(t) * T[0].size * (P * (P - 1) // 2)
    assert st["contributing"] == contributing_pairs(T, t, w)
    fin = got["maps"][np.isfinite(got["maps"])]
    assert ((fin >= 0.0) & (fin <= 1.0)).all()
    return got, want


# ---------------------------------------------------------------- 1. shapes
SHAPES = [  # nx, ny, P, E: every grid, every P and every E of the list above at least once
    (16, 16, 2, 1), (16, 16, 7, 17), (17, 15, 3, 16), (17, 15, 33, 1), (257, 1, 7, 35), (257, 1, 2, 16),
    (37, 29, 33, 35), (37, 29, 3, 17), (37, 29, 7, 16),
    (16, 16, 65, 17), (17, 15, 129, 1),          # 2 080 and 8 256 pairs: the pair index and the staged layout well past 33 stations
]


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("nx,ny,P,E", SHAPES)
def test_every_output_has_the_restatements_bits(rb, nx, ny, P, E, weights):
    grid, T, t, w = problem(nx, ny, P, E, seed=nx + 7 * ny + 13 * P + E, weights=weights)
    got, _ = check(rb, grid, T, t, SIGMA if not weights else 0.01, w)
    assert (got["node"] >= 0).all() and (got["count"] == P).all() and (got["npairs"] == P * (P - 1) // 2).all()
    assert np.isfinite(got["share"]).all() and np.isfinite(got["resid"]).all()
    if nx >= 3 and ny >= 3 and P >= 7 and E >= 16:
        assert got["refined"].any()


def test_share_and_resid_each_alone(rb):
    """the C entry with share but no resid, and with resid but no share"""
    from raytracing_amd import _lib
    grid, T, t, _ = problem(17, 15, 7, 17, seed=21)
    want = edt_ref.locate(T, t, SIGMA)
    L = rb.Locator(T, grid)
    ep = _lib.EdtParams()
    ep.sigma = SIGMA
    for which in ("share", "resid"):
        res = (_lib.EdtResult * 17)()
        out = np.full((17, 7), -1.0)
        args = (_lib.dptr(out), None) if which == "share" else (None, _lib.dptr(out))
        _lib.check(_lib.lib().rtmi_locate_edt(L._h, C.byref(ep), 17, _lib.dptr(t), None, None, res, *args, None, None))
        assert np.array_equal(out, want[which], equal_nan=True), which
        assert np.array_equal(np.frombuffer(res, dtype=np.dtype(_lib.EdtResult))["value"], want["value"])
    L.close()


# ---------------------------------------------------------------- 2. holes
@pytest.mark.parametrize("need_all", [True, False])
def test_tables_with_holes(rb, need_all):
    """5 % NaN in every table: with need absent only the nodes all stations cover are candidates, with need = P - 2 more are"""
    P, E = 33, 17
    grid, T, t, w = problem(37, 29, P, E, seed=3, holes=0.05, weights=not need_all)
    need = None if need_all else np.full(E, P - 2, dtype=np.int32)
    got, want = check(rb, grid, T, t, SIGMA if need_all else 0.01, w, need)
    assert (got["node"] >= 0).all()
    assert np.isinf(got["maps"]).any() and np.isfinite(got["maps"]).any()
    assert (got["count"] == P).all() if need_all else ((got["count"] >= P - 2).all() and (got["count"] < P).any())
    assert need_all or np.isnan(got["share"]).any()           # a station with a hole at the best node has no share there


def test_a_table_that_is_nan_everywhere_and_needs_from_two_to_above_p(rb):
    P, E = 7, 8
    grid, T, t, w = problem(37, 29, P, E, seed=4)
    T[2] = np.nan
    got, _ = check(rb, grid, T, t, need=None, what="need absent: all 7, and station 2 never contributes")
    assert (got["node"] == -1).all() and (got["count"] == 0).all() and (got["npairs"] == 0).all()
    assert np.isnan(got["share"]).all() and np.isnan(got["resid"]).all() and np.isnan(got["t0"]).all()
    need = np.array([0, 1, 2, 3, 6, 7, 8, 100], dtype=np.int32)
    got, _ = check(rb, grid, T, t, need=need, what="need 0 .. 100")
    assert (got["node"][:5] >= 0).all() and (got["count"][:5] == 6).all() and (got["npairs"][:5] == 15).all()
    assert (got["node"][5:] == -1).all()
    assert np.isnan(got["share"][:5, 2]).all() and np.isfinite(np.delete(got["share"][:5], 2, axis=1)).all()
    # one station: never a candidate
    got, _ = check(rb, grid, T[:1], t[:, :1])
    assert (got["node"] == -1).all()


# ---------------------------------------------------------------- 3. picks
@pytest.mark.parametrize("weights", [False, True])
def test_missing_picks_beside_a_full_chunk(rb, weights):
    """35 events: the first chunk has every pick (the all-picks variant), in the second one event misses picks, one has none and
    one has a single pick (the masked variant), and with weights some of them drop picks in the third"""
    P, E = 7, 35
    grid, T, t, w = problem(37, 29, P, E, seed=5, weights=weights)
    t[20, [1, 4]] = np.nan
    t[21] = np.nan
    t[22, 1:] = np.inf
    if weights:
        w[33, 0], w[33, 3], w[34, 6], w[32, 2] = 0.0, -1.0, np.nan, np.inf
    need = np.full(E, 4, dtype=np.int32)
    got, _ = check(rb, grid, T, t, 0.02 if weights else SIGMA, w, need)
    assert got["count"][20] == 5 and got["node"][21] == -1 and got["node"][22] == -1 and (got["count"][:16] == P).all()
    assert np.isnan(got["share"][20, [1, 4]]).all() and np.isfinite(got["share"][20, [0, 2, 3, 5, 6]]).all()
    if weights:
        assert got["count"][33] == 5 and got["count"][34] == 6 and got["count"][32] == 6 and np.isnan(got["share"][33, [0, 3]]).all()
    # with need absent an event wants all its valid picks
    got, _ = check(rb, grid, T, t, 0.02 if weights else SIGMA, w)
    assert got["count"][20] == 5 and got["node"][22] == -1


def test_a_pick_shifted_by_1e3_seconds_is_cut_and_an_event_whose_every_pair_is_cut(rb):
    P, E = 7, 17
    grid, T, t, _ = problem(37, 29, P, E, seed=6, noise=0.002)
    bad = np.arange(E) % P
    t[np.arange(E), bad] += 1e3
    t[16] = 100.0 * np.arange(P)                              # every pair of event 16 is far beyond the cut at every node
    got, _ = check(rb, grid, T, t, 0.01)
    assert (got["share"][np.arange(16), bad[:16]] == 0.0).all()          # z < -700: +0.0 exactly, pair by pair
    assert (got["share"][:16] >= 0.0).all() and (got["share"][:16].max(axis=1) > 0.0).all()
    assert (got["value"][:16] > 0.0).all() and (got["value"][:16] <= 15.0 / 21.0).all()
    assert got["value"][16] == 0.0 and np.isnan(got["t0"][16]) and np.isnan(got["t0_node"][16]) and got["share_sum"][16] == 0.0
    assert got["node"][16] == 0 and (got["maps"][16] == 0.0).all() and (got["share"][16] == 0.0).all() and np.isnan(got["resid"][16]).all()


@pytest.mark.parametrize("weights", [False, True])
def test_picks_offset_by_1e5_seconds(rb, weights):
    P, E = 7, 17
    grid, T, t, w = problem(37, 29, P, E, seed=7, weights=weights, offset=1e5)
    got, _ = check(rb, grid, T, t, 0.02, w)
    base, _ = check(rb, grid, T, t - 1e5, 0.02, w)
    assert (got["node"] >= 0).all() and np.abs((got["t0_node"] - 1e5) - base["t0_node"]).max() < 1e-6


def test_refusals_name_the_argument_and_the_handle_stays_usable(rb):
    from raytracing_amd import _lib
    grid, T, t, w = problem(16, 16, 2, 5, seed=9, weights=True)
    L = rb.Locator(T, grid)
    with pytest.raises(_lib.RtmiError, match=r"rtmi_locate_edt: need\[3\] is negative"):
        L.locate_edt(t, SIGMA, min_picks=np.array([1, 1, 1, -1, 1]))
    for sigma in (0.0, -0.1, np.nan, np.inf):
        with pytest.raises(_lib.RtmiError, match=r"rtmi_locate_edt: sigma must be finite and > 0"):
            L.locate_edt(t, sigma)
    for sigma in (-0.1, np.nan, np.inf):
        with pytest.raises(_lib.RtmiError, match=r"rtmi_locate_edt: sigma must be finite and >= 0"):
            L.locate_edt(t, sigma, weights=w)
    res = (_lib.EdtResult * 5)()
    assert _lib.lib().rtmi_locate_edt(L._h, None, 5, _lib.dptr(t), None, None, res, None, None, None, None) == -1
    assert b"rtmi_locate_edt: null ep" in _lib.lib().rtmi_last_error()
    assert (L.locate_edt(t, SIGMA)["node"] >= 0).all() and (L.locate_edt(t, 0.0, weights=w)["node"] >= 0).all()
    L.close()
    with pytest.raises(RuntimeError, match="closed"):
        L.locate_edt(t, SIGMA)


# ---------------------------------------------------------------- 4. ties and rims
def test_mirror_symmetric_stations_tie_to_the_least_node(rb):
    """Two stations mirrored in the grid's middle row (the second table is the first one upside down, bit for bit), the same pick
    at both: every node of the middle row has u = 0, k = 1 and value 1.0 exactly, and the least index among them wins."""
    nx, ny = 37, 29
    grid = grid_of(nx, ny)
    X, Y = grid[0] + grid[1] * np.arange(nx), grid[3] + grid[4] * np.arange(ny)
    T = np.empty((2, ny, nx))
    T[0] = 1.5 * np.hypot(X[None, :] - 0.3, Y[:, None] - (Y[ny // 2] + 1.1))
    T[1] = T[0][::-1]
    t = np.array([[2.0, 2.0], [1e5 + 0.7, 1e5 + 0.7], [-3.25, -3.25]])
    for w in (None, np.array([[200.0, 200.0], [25.0, 25.0], [800.0, 800.0]])):
        got, _ = check(rb, grid, T, t, 0.03, w)
        for e in range(len(t)):
            m = got["maps"][e]
            assert np.array_equal(m, m[::-1])
            assert (m[ny // 2] == 1.0).all() and (np.delete(m, ny // 2, axis=0) < 1.0).all()
            assert got["node"][e] == (ny // 2) * nx and got["ix"][e] == 0 and got["value"][e] == 1.0 and got["refined"][e] == 0


def test_best_node_on_each_rim_and_in_a_corner(rb):
    nx, ny = 37, 29
    grid, T, _, _ = problem(nx, ny, 7, 1, seed=10)
    nodes = [(0, 12), (nx - 1, 12), (17, 0), (17, ny - 1), (0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx - 1, 0)]
    t = np.stack([4.0 + T[:, iy, ix] for ix, iy in nodes])   # near-exact picks of a rim node
    got, _ = check(rb, grid, T, t, 0.02)
    for e, (ix, iy) in enumerate(nodes):
        assert (got["ix"][e], got["iy"][e]) == (ix, iy) and got["refined"][e] == 0
        out = np.array([[not (0 <= iy + j < ny and 0 <= ix + i < nx) for i in (-1, 0, 1)] for j in (-1, 0, 1)])
        assert np.array_equal(np.isnan(got["win_val"][e]), out) and np.array_equal(np.isnan(got["win_tau"][e]), out)
        assert got["x"][e] == grid[0] + ix * grid[1] and got["y"][e] == grid[3] + iy * grid[4]
        assert got["t0"][e] == got["t0_node"][e] and abs(got["t0"][e] - 4.0) < 1e-9


# ---------------------------------------------------------------- 5. entry forms
@pytest.mark.parametrize("weights", [False, True])
def test_device_pointers_and_the_split_of_a_call(rb, torch, weights):
    P, E = 33, 35
    grid, T, t, w = problem(37, 29, P, E, seed=11, holes=0.03, weights=weights)
    sigma = 0.01 if weights else SIGMA
    need = np.full(E, P - 3, dtype=np.int32)
    L = rb.Locator(T, grid)
    whole = L.locate_edt(t, sigma, weights=w, min_picks=need, maps=True, shares=True)
    dev = "cuda:0"
    d = L.locate_edt_device(torch.from_numpy(t).to(dev), sigma, None if w is None else torch.from_numpy(w).to(dev),
                            torch.from_numpy(need).to(dev), maps=True, shares=True)
    for k in ("maps", "share", "resid"):
        assert d[k].is_cuda
        d[k] = d[k].cpu().numpy()
    every = KEYS + REFINED + ("maps", "share", "resid", "t0", "t0_node")
    same(d, whole, every, "locate_edt_device")
    bare = L.locate_edt_device(torch.from_numpy(t).to(dev), sigma, None if w is None else torch.from_numpy(w).to(dev),
                               torch.from_numpy(need).to(dev))
    same(bare, whole, KEYS + REFINED + ("t0",), "locate_edt_device without maps and shares")
    # chunking must not show: 35 events in one call are calls of 16, 16 and 3
    parts = [L.locate_edt(t[a:b], sigma, weights=None if w is None else w[a:b], min_picks=need[a:b], maps=True, shares=True)
             for a, b in ((0, 16), (16, 32), (32, 35))]
    for k in every:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k], equal_nan=True), k
    # refine=False reports the node's own values; a scalar min_picks is the array of it
    plain = L.locate_edt(t, sigma, weights=w, min_picks=P - 3, refine=False)
    same(plain, whole, KEYS)
    assert np.array_equal(plain["t0"], whole["t0_node"]) and not plain["refined"].any()
    assert np.array_equal(plain["x"], grid[0] + whole["ix"] * grid[1])
    with pytest.raises(ValueError, match="on a GPU"):
        L.locate_edt_device(torch.from_numpy(t), sigma)
    L.close()


def test_a_weighted_call_walked_in_several_groups_of_chunks(rb):
    """70 events are five chunks; two chunks per group make three groups, the last a partial one, of a staging buffer of a few
    kilobytes; one chunk per group makes five.  The same bits as the call in one group."""
    P, E = 7, 70
    grid, T, t, w = problem(37, 29, P, E, seed=12, weights=True)
    t[40, 2] = np.nan
    L = rb.Locator(T, grid)
    one, st1 = L.locate_edt(t, 0.01, weights=w, maps=True, shares=True, stats=True)
    assert st1["groups"] == 1
    for per, groups in ((2, 3), (1, 5), (5, 1), (64, 1)):
        many, st = L.locate_edt(t, 0.01, weights=w, maps=True, shares=True, stats=True, _chunks_per_group=per)
        assert st["groups"] == groups
        same(many, one, KEYS + REFINED + ("maps", "share", "resid", "t0", "t0_node"), f"{per} chunks per group")
    from raytracing_amd import _lib
    with pytest.raises(_lib.RtmiError, match=r"reserved\[0\] must be >= 0"):
        L.locate_edt(t, 0.01, weights=w, _chunks_per_group=-1)
    L.close()
    want = edt_ref.locate(T, t, 0.01, w=w, grid=grid)
    same(one, want, KEYS + REFINED + ("maps", "share", "resid"))


# ---------------------------------------------------------------- 6. traced tables, picks by another path, one of them wrong
def test_traced_tables_locate_two_point_picks_with_one_pick_shifted(rb):
    """vert_heterogeneous, op6; the field, stations, grid and events of test_gpu_locate's traced case.  One of the 16 picks of each
    event is shifted by +0.02 s, or by the first of its doublings at which the least-squares restatement leaves the truth's cell
    for some event; sigma is the tables' median traveltime across one cell.  Every event is bit-equal to the restatement, the EDT
    node is within one cell of the truth and the shifted station holds the least share.  DESIGN.md section 31 records the
    printed figures."""
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
    clean = origin[:, None] + np.concatenate([first(to_right), first(to_left)], axis=1)
    F.close()
    assert (np.isfinite(clean).sum(axis=1) >= 12).all()
    with np.errstate(invalid="ignore"):
        across = np.concatenate([np.abs(np.diff(T, axis=2)).ravel(), np.abs(np.diff(T, axis=1)).ravel()])
    sigma = float(np.median(across[np.isfinite(across)]))
    bad = np.array([np.flatnonzero(np.isfinite(clean[e]))[(5 * e) % 12] for e in range(8)])
    cx, cy = (ev[:, 0] - grid[0]) / grid[1], (ev[:, 1] - grid[3]) / grid[4]
    err = lambda o: np.maximum(np.abs(o["ix"] - cx), np.abs(o["iy"] - cy))       # noqa: E731
    shift = 0.02
    while True:
        t = clean.copy()
        t[np.arange(8), bad] += shift
        l2 = locate_ref.locate(T, t, need=np.full(8, 10))
        print(f"shift {shift:.2f} s: least squares node error {err(l2).max():.3f} cell, {int((err(l2) > 1.0).sum())} of 8 beyond one cell")
        if (err(l2) > 1.0).any() or shift >= 1.0:
            break
        shift *= 2.0
    assert (err(l2) > 1.0).any()
    need = np.full(8, 10, dtype=np.int32)
    want = edt_ref.locate(T, t, sigma, need=need, grid=grid)
    L = rb.Locator.from_table({"T": T}, grid)
    got = L.locate_edt(t, sigma, min_picks=need, maps=True, shares=True)
    L.close()
    same(got, want, KEYS + REFINED + ("maps", "share", "resid"))
    share = np.where(np.isnan(got["share"]), np.inf, got["share"])
    ratio = share[np.arange(8), bad] / np.nanmax(got["share"], axis=1)
    ref_err = np.maximum(np.abs(got["x"] - ev[:, 0]) / grid[1], np.abs(got["y"] - ev[:, 1]) / grid[4])
    print(f"traced case, sigma {sigma:.4e} s, shift {shift:.2f} s: EDT node {err(got).max():.3f} cell, refined {ref_err.max():.3f} cell "
          f"({int(got['refined'].sum())} of 8 refined), t0 {np.abs(got['t0_node'] - origin).max():.3e} s, shifted share / greatest "
          f"{ratio.max():.3e}; least squares {err(l2).max():.3f} cell")
    assert (got["node"] >= 0).all()
    assert err(got).max() <= 1.0
    assert (np.argmin(share, axis=1) == bad).all()
