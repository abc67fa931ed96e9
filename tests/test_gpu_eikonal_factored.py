"""GPU: the source-factored scheme of the eikonal fill (scheme="factored": rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED in
rtmi_eikonal_fill, rtmi_eikonal_fill_dev, a self-filled EikonalTomography and traveltime_table(fill="eikonal"); DESIGN.md section
39).  The yardstick is tests/eikonal_factored_ref.py, the serial sweeps in Python floats, and every comparison is bit for bit on
T, rounds, converged and filled, NaN positions included.  Shapes: the grids 1 x 1, 1 x 70, 70 x 1, 5 x 70, 64 x 64 and 65 x 63
(diagonals of 1, 5, 63 and 64 nodes in a block of one wave) and 80 x 80 (two waves, the last not full), each on the LDS path where
it fits and on the global path; 300 x 260 under a cap of two rounds, whose diagonals of 260 nodes make the 256 lanes stride; the
71 x 57 gradient medium with a source on a node, one off the nodes and one off the grid with a seeded wedge, in one call and in
three; the corridor that winds against the sweeps; seeds in every state; an obstacle's n_src; the device-pointer form and
repeated runs; scheme 0 through the same entry; a self-filled tomography handle; and the traced case of section 34."""
import ctypes as C
import functools

import numpy as np
import pytest

import eikonal_factored_ref as F
import eikonal_ref as R
import eikonal_tomo_ref as E
from conftest import LIMITS
from test_eikonal_ref import launch_angle
from test_gpu_eikonal import TRACED_GRID, check_stats, same, seeded_case, shape_case, smooth_problem

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


# --------------------------------------------------------------------------------------------------------------- shapes
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 70), (64, 64), (65, 63), (80, 80)]


@functools.lru_cache(maxsize=None)
def factored_shape(nx, ny):
    grid, n, src, ns = smooth_problem(nx, ny, 2, 100 * nx + ny)
    return grid, n, src, ns, F.solve(grid, n, src, ns)


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_where_lane_wave_and_block_loops_can_go_wrong(rb, nx, ny, global_path):
    grid, n, src, ns, want = factored_shape(nx, ny)
    print(f"{nx} x {ny}: rounds {want['rounds'].tolist()}, converged {want['converged'].tolist()}")
    assert want["filled"].all()
    got = rb.eikonal_fill(n, src, grid, n_src=ns, stats=True, scheme="factored", _global_path=global_path)
    same(got, want, f"{nx} x {ny}")
    # no table of T0: the LDS rule is the plain scheme's, 17 bytes per node
    check_stats(got["stats"], want, "global" if global_path or nx * ny * 17 > 128 * 1024 else "lds")
    if nx * ny >= 70:
        assert not R.same_bits(want["T"], shape_case(nx, ny)[4]["T"])         # and it is no copy of the plain result


def test_grid_over_the_lds_capacity_with_striding_lanes(rb):
    """300 x 260 under max_rounds = 2: 78 000 nodes against the LDS path's 7 710, and diagonals of 260 nodes for 256 lanes.  The
    cap keeps the restatement to seconds; converged is 0, and the bits are defined all the same."""
    grid, n, src, ns = smooth_problem(300, 260, 1, 7)
    want = F.solve(grid, n, src, ns, max_rounds=2)
    assert want["rounds"].tolist() == [2] and want["converged"].tolist() == [0] and want["filled"].all()
    got = rb.eikonal_fill(n, src, grid, n_src=ns, max_rounds=2, stats=True, scheme="factored")
    same(got, want, "300 x 260")
    check_stats(got["stats"], want, "global")


# ---------------------------------------------------------------------------------------------------- the gradient medium
@functools.lru_cache(maxsize=None)
def gradient_case():
    """71 x 57, n = 1 / (18 + 2 y): a source on node (20, 30), one off the nodes, and one off the grid whose table is the closed
    form on the launch angles 0.05 .. 1.5 (the other two have no table)"""
    g = F.GRIDS[71]
    X, Y, n = F.gradient_medium(g)
    src = np.array([[g[0] + 20 * g[1], g[3] + 30 * g[4]], F.SOURCES[1], [-2.31, -2.03]])
    ns = 1.0 / (18.0 + 2.0 * src[:, 1])
    T = np.full((3,) + n.shape, np.nan)
    th = launch_angle(X, Y, src[2, 0], src[2, 1])
    T[2] = np.where((th >= 0.05) & (th <= 1.5), R.gradient_truth(X, Y, src[2, 0], src[2, 1]), np.nan)
    return g, n, src, ns, T, F.solve(g, n, src, ns, T=T)


@pytest.mark.parametrize("global_path", [False, True])
def test_gradient_medium_three_sources_in_one_call_and_in_three(rb, global_path):
    g, n, src, ns, T, want = gradient_case()
    assert want["converged"].all() and want["filled"][:2].all() and 0 < want["filled"][2].sum() < n.size
    assert F.t0(g, 20, 30, src[0, 0], src[0, 1], ns[0])[3] == 0.0          # the first source sits on its node to the bit
    print(f"gradient medium: rounds {want['rounds'].tolist()}")
    whole = rb.eikonal_fill(n, src, g, T, n_src=ns, stats=True, scheme="factored", _global_path=global_path)
    same(whole, want, "three sources")
    check_stats(whole["stats"], want, "global" if global_path else "lds")
    for s in range(3):
        one = rb.eikonal_fill(n, src[s:s + 1], g, T[s:s + 1], n_src=ns[s:s + 1], scheme="factored", _global_path=global_path)
        same(one, {k: want[k][s:s + 1] for k in ("T", "rounds", "converged", "filled")}, f"source {s} alone")
    X, Y = R.nodes(g)
    truth = R.gradient_truth(X, Y, src[1, 0], src[1, 1])
    assert np.max(np.abs(whole["T"][1] - truth)) / truth.max() <= 3e-3      # 2.161e-3 (tests/test_eikonal_factored_ref.py)


# ------------------------------------------------------------------------------------------------- the several-round medium
CORRIDOR_GRID = (0.0, 1.0, 31, 0.0, 1.0, 27)


@functools.lru_cache(maxsize=None)
def corridor():
    n, (ix, iy) = R.winding_corridor()
    src = np.array([[ix + 0.25, iy - 0.125], [15.0, 13.0], [29.0 - 0.5, 1.0 + 0.375]])       # the outer end, the middle, a far corner
    ns = np.array([1.0, 1.0, 1.0])
    return n, src, ns, F.solve(CORRIDOR_GRID, n, src, ns)


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_that_needs_several_rounds(rb, global_path):
    n, src, ns, want = corridor()
    assert want["rounds"][0] == 7 and (want["rounds"] >= 3).all() and want["converged"].all()
    got = rb.eikonal_fill(n, src, CORRIDOR_GRID, n_src=ns, stats=True, scheme="factored", _global_path=global_path)
    same(got, want, "corridor")
    check_stats(got["stats"], want, "global" if global_path else "lds")


# ------------------------------------------------------------------------------------------------------ seeds in every state
@functools.lru_cache(maxsize=None)
def factored_seeded():
    grid, n, src, ns, T, _ = seeded_case()
    return grid, n, src, ns, T, F.solve(grid, n, src, ns, T=T)


@pytest.mark.parametrize("global_path", [False, True])
def test_seeds_obstacles_and_a_sealed_pocket(rb, global_path):
    grid, n, src, ns, T, want = factored_seeded()
    assert np.isnan(want["T"][:2, 9:14, 21:26]).all() and np.isfinite(want["T"][2, 9:14, 21:26]).all()
    keep = T.copy()
    got = rb.eikonal_fill(n, src, grid, T, n_src=ns, stats=True, scheme="factored", _global_path=global_path)
    same(got, want, "seeded")
    assert R.same_bits(T, keep)
    seeded = np.isfinite(T) & np.isfinite(n) & (n > 0)
    assert R.same_bits(got["T"][seeded], T[seeded]) and not got["filled"][seeded].any()
    assert got["stats"]["unreached"] > 0 and not R.same_bits(want["T"], seeded_case()[5]["T"])


def test_an_obstacle_n_src_has_the_bits_of_plain(rb):
    grid, n, src, ns, T, _ = seeded_case()
    bad = np.array([0.0, np.nan, -1.0])
    want = R.solve(grid, n, src, bad, T=T)
    assert (want["rounds"] >= 2).all()
    same(F.solve(grid, n, src, bad, T=T), want, "the restatement")
    for global_path in (False, True):
        same(rb.eikonal_fill(n, src, grid, T, n_src=bad, scheme="factored", _global_path=global_path), want, "obstacle n_src")


def test_device_form_and_repeated_runs(rb, torch):
    grid, n, src, ns, T, want = factored_seeded()
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    for rep in range(2):
        d_T = up(T)
        got = rb.eikonal_fill_device(up(n), up(src), grid, d_T, n_src=up(ns), scheme="factored")
        assert got["T"] is d_T and got["filled"].dtype == torch.uint8
        same({"T": d_T.cpu().numpy(), "rounds": got["rounds"], "converged": got["converged"], "filled": got["filled"].cpu().numpy()},
             want, f"device form, run {rep}")
    a = rb.eikonal_fill(n, src, grid, T, n_src=ns, scheme="factored")
    same(rb.eikonal_fill(n, src, grid, T, n_src=ns, scheme="factored"), a, "two runs of the host form")


def test_scheme_0_keeps_the_plain_bits(rb):
    grid, n, src, ns, want = shape_case(65, 63)
    for global_path in (False, True):
        same(rb.eikonal_fill(n, src, grid, n_src=ns, scheme="plain", _global_path=global_path), want, "scheme plain")
    same(rb.eikonal_fill(n, src, grid, n_src=ns), want, "no scheme")
    assert rb.eikonal_params(grid).scheme == 0


# ------------------------------------------------------------------------------------------- a self-filled tomography handle
def test_self_filled_tomography_handle(rb):
    """71 x 57, two sources and eight receivers in the gradient medium.  The factored handle's tables are eikonal_fill's, and its
    residual against closed-form picks is smaller than the plain handle's: the restatements alone give an rms of 5.08e-4 s against
    3.55e-3 s at these receivers (seven times; asserted below on the restatement, then on the device)."""
    g = F.GRIDS[71]
    X, Y, n = F.gradient_medium(g)
    src = np.array(F.SOURCES)
    ns = 1.0 / (18.0 + 2.0 * src[:, 1])
    rec = np.array([E.at(g, u, v) for u, v in [(60.5, 50.25), (10.0, 50.0), (65.0, 5.5), (35.25, 28.5), (69.5, 30.0), (5.5, 30.5),
                                               (50.0, 55.0), (20.75, 10.5)]])
    picks = np.array([[float(R.gradient_truth(x, y, sx, sy)) for x, y in rec] for sx, sy in src]).reshape(-1)
    ridx, rw, _ = E.cells(g, rec)
    rms = {}
    for scheme, code in (("plain", F.PLAIN), ("factored", F.FACTORED)):
        want = F.solve(g, n, src, ns, scheme=code)
        res_want = np.array([picks[s * 8 + k] - E.sample(want["T"][s].reshape(-1), ridx[k], rw[k]) for s in range(2) for k in range(8)])
        fill = rb.eikonal_fill(n, src, g, n_src=ns, scheme=scheme)
        same(fill, want, scheme)
        h = rb.EikonalTomography(n, src, g, rec, n_src=ns, scheme=scheme)
        try:
            tab = h.table()
            assert R.same_bits(tab["T"], fill["T"]) and np.array_equal(tab["filled"], fill["filled"]) and tab["live"].all()
            res = h.residual(picks)
            assert R.same_bits(res, res_want)
            # the products linearise the plain update about the table they are given: they run, and are finite
            y = h.apply(np.full(n.shape, 1e-3))
            assert np.isfinite(y).all()
            if scheme == "factored":
                # re-linearising fills again with the handle's scheme
                h.relinearise(n * 1.01, ns * 1.01)
                again = rb.eikonal_fill(n * 1.01, src, g, n_src=ns * 1.01, scheme="factored")
                assert R.same_bits(h.table()["T"], again["T"])
        finally:
            h.close()
        rms[scheme] = (float(np.sqrt(np.mean(res_want ** 2))), float(np.sqrt(np.mean(res ** 2))))
    print(f"residual rms: plain {rms['plain'][1]:.3e} s, factored {rms['factored'][1]:.3e} s")
    assert rms["factored"][0] < 0.25 * rms["plain"][0] and rms["factored"][1] < 0.25 * rms["plain"][1]
    # the default is the plain scheme, and a handle with a fill_result takes no scheme
    with pytest.raises(ValueError, match="fill_result"):
        rb.EikonalTomography(n, src, g, rec, n_src=ns, fill_result=fill, scheme="factored")


# ---------------------------------------------------------------------------------------------------------- the traced case
def test_traced_tables_completed_by_the_factored_scheme(rb):
    """Section 34's traced case, the eight stations on x = -1.5 with fans of 0.05 .. 1.5 rad: fill_scheme="factored" keeps every
    covered node's bits and every other column, and the filled nodes are the restatement's on the device's own unfilled table"""
    box = LIMITS["vert_heterogeneous"]
    Fd = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    try:
        ms = int(np.ceil(80 / rb.DELTA_S) + 1)
        grid = TRACED_GRID
        stations = np.stack([np.full(8, -1.5), np.linspace(-2.1, 0.5, 8)], axis=1)
        kw = dict(thetas=np.linspace(0.05, 1.5, 512), step=rb.DELTA_S, max_size=ms, box=box)
        bare = rb.traveltime_table(rb.op6, Fd, stations, grid, **kw)
        full = rb.traveltime_table(rb.op6, Fd, stations, grid, fill="eikonal", fill_scheme="factored", stats=True, **kw)
        plain = rb.traveltime_table(rb.op6, Fd, stations, grid, fill="eikonal", **kw)
        X, Y = R.nodes(grid)
        n = Fd.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(X.shape)
        ns = Fd.n_gradient(stations[:, 0], stations[:, 1])[0]
    finally:
        Fd.close()
    for k in bare:
        if k != "T":
            assert np.array_equal(full[k], bare[k], equal_nan=True), k
    covered = np.isfinite(bare["T"])
    assert 0.05 < covered.mean() < 0.9 and np.isfinite(full["T"]).all()
    assert R.same_bits(full["T"][covered], bare["T"][covered]) and np.array_equal(full["filled"] == 1, ~covered)
    want = F.solve(grid, n, stations, ns, T=bare["T"])
    assert R.same_bits(full["T"], want["T"]) and np.array_equal(full["filled"], want["filled"])
    assert full["stats"]["eikonal"]["rounds_max"] == int(want["rounds"].max())
    assert not R.same_bits(full["T"], plain["T"]) and R.same_bits(plain["T"], R.solve(grid, n, stations, ns, T=bare["T"])["T"])
    truth = np.stack([R.gradient_truth(X, Y, sx, sy) for sx, sy in stations])
    err = [float(np.max(np.abs(t - truth)[full["filled"] == 1]) / truth.max()) for t in (plain["T"], full["T"])]
    print(f"traced case: {int(full['filled'].sum())} nodes filled in {want['rounds'].tolist()} rounds; error at the filled nodes "
          f"{err[0]:.3e} plain, {err[1]:.3e} factored, of the largest T")
