"""GPU: launch angle, direction and spreading at eikonal-filled nodes (rtmi_eikonal_attributes, its _dev form and
traveltime_table(fill_attributes=True)).  The yardstick is tests/eikonal_attr_ref.py, the serial sweeps in
Python floats over the restatement's own fill, and every comparison is bit for bit on theta0, px, py, J, G, rounds and converged,
with NaN compared by place.  Shapes: section 35's grids 1 x 1, 1 x 70, 70 x 1, 5 x 70, 64 x 64, 65 x 63 and 100 x 90 (over the LDS
path's 7 710 nodes), each on the LDS path where it fits and on the global path; 300 x 260, whose diagonals of 260 nodes make the
256 lanes stride.  Cases: the corridor, which needs more than three rounds, with and without a cap; obstacles of every kind with
NaN and infinite launch angles among the seeds; a table seeded with the closed-form launch angle everywhere but two discs, one
of them across the +-pi cut of the interior source, in both conventions of the angle; null dir, J and G in turn; the
device-pointer form; the split of a call over its sources; and vert_heterogeneous traced and completed end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import eikonal_attr_ref as A
import eikonal_lin_ref as L
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


def seeds_in(fill, seed):
    """theta0, J and G at every node as the rays would leave them; only the seeds' and the dead nodes' are read or kept"""
    rng = np.random.default_rng(seed)
    shape = fill["T"].shape
    return {"theta0": rng.uniform(-3.1, 3.1, shape), "J": rng.uniform(0.1, 2.0, shape), "G": rng.uniform(0.1, 2.0, shape)}


def same(got, want, what=""):
    k = A.same(got, want)
    assert k is None, f"{what}: {k} differs" + ("" if k in ("rounds", "converged") else
                                                 f" at {int((~(got[k] == want[k]) & ~(np.isnan(got[k]) & np.isnan(want[k]))).sum())} nodes")


def check_stats(st, nets, want, path):
    assert st["path"] == path and st["changes"] == want["changes"] and st["rounds_max"] == int(want["rounds"].max())
    assert st["free_nodes"] == st["filled"] == sum(len(net.free) + net.cls.count(L.BALL) for net in nets) and st["unreached"] == 0
    assert st["kernel_ms"] > 0.0


def both(rb, grid, n, src, ns, fill, nets, ins, what, global_path, path=None, max_rounds=0):
    """the device's attributes of one case against the restatement's; the device's theta is arctan2 of its own direction"""
    want = A.solve(grid, n, src, ns, fill, **ins, nets=nets, max_rounds=max_rounds)
    got = rb.eikonal_attributes(n, src, grid, fill["T"], fill["filled"], **ins, n_src=ns, stats=True, max_rounds=max_rounds,
                                _global_path=global_path)
    same(got, want, what)
    written = np.array([net.cls for net in nets]).reshape(fill["T"].shape) >= L.FREE
    assert np.array_equal(np.isnan(got["theta"]), ~written | np.isnan(got["px"]))
    assert L.same_but_nan(got["theta"][written], np.arctan2(got["py"], got["px"])[written])
    if path:
        check_stats(got["stats"], nets, want, path)
    return want


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


SHAPES = [(1, 1), (1, 70), (70, 1), (5, 70), (64, 64), (65, 63), (100, 90)]
LDS_NODES = 128 * 1024 // 17


@functools.lru_cache(maxsize=None)
def shape_case(nx, ny, S=2):
    grid, n, src, ns = smooth_problem(nx, ny, S, 100 * nx + ny)
    return L.filled((grid, n, src, ns, None))


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_where_lane_wave_and_block_loops_can_go_wrong(rb, nx, ny, global_path):
    grid, n, src, ns, fill, nets = shape_case(nx, ny)
    assert fill["filled"].all() and fill["converged"].all()
    want = both(rb, grid, n, src, ns, fill, nets, {}, f"{nx} x {ny}", global_path, "global" if global_path or nx * ny > LDS_NODES else "lds")
    assert np.isfinite(want["theta0"]).all() and want["converged"].all()


def test_grid_over_the_lds_capacity_with_striding_lanes(rb):
    """300 x 260: 78 000 nodes against the LDS path's 7 710, and diagonals of 260 nodes for 256 lanes"""
    grid, n, src, ns, fill, nets = shape_case(300, 260, 1)
    both(rb, grid, n, src, ns, fill, nets, {}, "300 x 260", False, "global")


# ------------------------------------------------------------------------------------------------- the several-round medium
@functools.lru_cache(maxsize=None)
def named(name):
    return L.filled(getattr(L, name)())


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_with_three_sources_and_under_a_cap_of_one_round(rb, global_path):
    grid, n, src, ns, fill, nets = named("corridor_case")
    want = both(rb, grid, n, src, ns, fill, nets, {}, "corridor", global_path, "global" if global_path else "lds")
    assert (want["rounds"] > 3).all() and want["converged"].all() and np.isfinite(want["theta0"]).all()
    cap = both(rb, grid, n, src, ns, fill, nets, {}, "corridor, max_rounds 1", global_path, max_rounds=1)
    assert (cap["rounds"] == 1).all() and not cap["converged"].any() and np.isnan(cap["theta0"]).any()


# ------------------------------------------------------------------------------------------ obstacles, a pocket, bad seeds
@pytest.mark.parametrize("global_path", [False, True])
def test_walls_with_nan_and_infinite_launch_angles_among_the_seeds(rb, global_path):
    grid, n, src, ns, fill, nets = named("walls_case")
    cls = np.array([net.cls for net in nets]).reshape(fill["T"].shape)
    assert all(set(c.reshape(-1)) == {L.DEAD, L.SEED, L.FREE, L.BALL} for c in cls)
    ins = seeds_in(fill, 5)
    for s in range(len(src)):
        seeds = np.argwhere(cls[s] == L.SEED)
        for (j, i), bad in zip(seeds[:3], (np.nan, np.inf, -np.inf)):
            ins["theta0"][s, j, i] = bad
    want = both(rb, grid, n, src, ns, fill, nets, ins, "walls", global_path)
    keep = cls <= L.SEED
    for k in ("theta0", "J", "G"):
        assert L.same_but_nan(want[k][keep], ins[k][keep])
    assert np.isinf(want["theta0"][keep]).sum() == 2 * len(src) and np.isfinite(want["theta0"][cls >= L.FREE]).any()


# --------------------------------------------------------------------------------------------------------- the seeded discs
@functools.lru_cache(maxsize=None)
def discs():
    """the gradient medium's table, exact but for the disc of section 35 and a second one left of the interior source, where that
    source's launch angles are about +-pi"""
    grid, n, src, ns, T, th, Jc = A.seeded_disc((71, 57), holes=((3.0, -1.0, 0.49), (0.0, -0.8, 0.25)))
    fill = R.solve(grid, n, src, ns, T=T)
    return grid, n, src, ns, fill, L.nets(grid, n, src, ns, fill), th, Jc


def gather_wraps(want):
    """per source the free nodes with two parents whose launch angles differ by more than pi"""
    out = []
    for s, net in enumerate(want["nets"]):
        v, nx, c = want["theta0"][s].reshape(-1), net.nx, 0
        for x in net.free:
            p = net.par[x]
            if p & L.XPARENT and p & L.YPARENT:
                c += abs(v[x + nx if p & L.YNORTH else x - nx] - v[x + 1 if p & L.XEAST else x - 1]) > np.pi
        out.append(c)
    return out


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("global_path", [False, True])
def test_seeded_discs_with_the_cut_across_free_nodes(rb, global_path, shifted):
    grid, n, src, ns, fill, nets, th, Jc = discs()
    assert all(len(net.free) > 300 and net.cls.count(L.SEED) > 3000 for net in nets)
    seeds = fill["filled"] == 0
    th = np.where(shifted & (th < 0.0), th + 2.0 * np.pi, th)              # (-pi, pi], or [0, 2 pi)
    ins = {"theta0": np.where(seeds, th, np.nan), "J": np.where(seeds, Jc, np.nan), "G": np.where(seeds, 1.0 / np.sqrt(n[None] * Jc), np.nan)}
    want = both(rb, grid, n, src, ns, fill, nets, ins, f"discs, shifted {shifted}", global_path)
    assert np.isfinite(want["theta0"]).all() and R.same_bits(want["theta0"][seeds], th[seeds])
    # wrap fires in the gathers of the interior source, whichever the convention, and the result is the angle modulo 2 pi
    assert gather_wraps(want)[1] > 5
    err = np.abs((want["theta0"] - th + np.pi) % (2.0 * np.pi) - np.pi)[~seeds]
    assert err.max() < 5e-2


# ------------------------------------------------------------------------------------------------------------ null outputs
def test_null_dir_J_and_G_in_turn(rb):
    from raytracing_amd import _lib
    grid, n, src, ns, fill, nets = named("walls_case")
    ins = seeds_in(fill, 6)
    want = A.solve(grid, n, src, ns, fill, **ins, nets=nets)
    S, (ny, nx) = len(src), n.shape
    u8 = C.POINTER(C.c_uint8)
    T, filled = np.ascontiguousarray(fill["T"]), np.ascontiguousarray(fill["filled"], dtype=np.uint8)
    for skip in ("dir", "J", "G", "all"):
        th, J, G = ins["theta0"].copy(), ins["J"].copy(), ins["G"].copy()
        d = np.full((S, 2, ny, nx), np.nan)
        rounds = np.zeros((S, 2), dtype=np.int32)
        ptr = lambda name, a: None if skip in (name, "all") else _lib.dptr(a)      # noqa: E731
        ep = rb.eikonal_params(grid)
        _lib.check(_lib.lib().rtmi_eikonal_attributes(C.byref(ep), _lib.dptr(n), S, _lib.dptr(src), _lib.dptr(ns), _lib.dptr(T),
                                                      filled.ctypes.data_as(u8), _lib.dptr(th), ptr("dir", d), ptr("J", J), ptr("G", G),
                                                      rounds.ctypes.data_as(_lib._ip), None))
        got = {"theta0": th, "px": d[:, 0], "py": d[:, 1], "J": J, "G": G, "rounds": rounds[:, 0], "converged": rounds[:, 1]}
        keys = [k for k in A.KEYS if skip != "all" and k != skip and not (skip == "dir" and k in ("px", "py"))] or ["theta0"]
        assert A.same(got, want, keys) is None, (skip, A.same(got, want, keys))
        # what was not asked for was not written
        if skip in ("dir", "all"):
            assert np.isnan(d).all()
        if skip in ("J", "all"):
            assert R.same_bits(J, ins["J"])
        if skip in ("G", "all"):
            assert R.same_bits(G, ins["G"])


# ------------------------------------------------------------------------------------------------------- the device form
def test_device_form_repeated_runs_and_split_over_sources(rb, torch):
    grid, n, src, ns, fill, nets = named("walls_case")
    ins = seeds_in(fill, 8)
    want = A.solve(grid, n, src, ns, fill, **ins, nets=nets)
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    host = lambda res: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}     # noqa: E731
    d_T, d_filled = up(fill["T"]), up(fill["filled"])
    for rep in range(2):
        d_in = {k: up(v) for k, v in ins.items()}
        got = rb.eikonal_attributes_device(up(n), up(src), grid, d_T, d_filled, **d_in, n_src=up(ns))
        assert all(got[k].is_cuda for k in A.KEYS + ("theta",)) and got["theta0"] is d_in["theta0"] and got["G"] is d_in["G"]
        same(host(got), want, f"device form, run {rep}")
    assert R.same_bits(d_T.cpu().numpy(), fill["T"])                         # the table is read, not written
    with pytest.raises(ValueError, match="on a GPU"):
        rb.eikonal_attributes_device(torch.as_tensor(n), up(src), grid, d_T, d_filled, n_src=up(ns))
    # S = 5 in one call against five calls of one source
    grid, n, src, ns, fill, nets = shape_case(41, 23, 5)
    whole = rb.eikonal_attributes(n, src, grid, fill["T"], fill["filled"], n_src=ns)
    for s in range(5):
        one = rb.eikonal_attributes(n, src[s:s + 1], grid, fill["T"][s:s + 1], fill["filled"][s:s + 1], n_src=ns[s:s + 1])
        same(one, {k: whole[k][s:s + 1] for k in A.KEYS + ("rounds", "converged")}, f"source {s} alone")
    same(whole, A.solve(grid, n, src, ns, fill, nets=nets), "five sources")


# ---------------------------------------------------------------------------------------------------------- the traced case
TRACED_GRID = (-1.0, 0.065, 71, -2.2, 0.05, 57)
# The distance of the filled nodes from the closed forms, the restatement's figures on the device's own tables rounded up to one
# digit.  They are large by design of the case, as section 34's for T: most filled nodes lie outside the
# wedge, where the continuation bends round its edge and carries the edge ray's launch angle, while the true first arrival is a
# direct ray that was not shot: the carried angle is the edge ray's and G, a diffraction's, is near 0 where the closed form's is
# not.  theta0: the median and the largest |error| in rad; G: the median relative error
TRACED_MEASURED = (3.572e-1, 1.512, 7.921e-1)
TRACED_BOUNDS = (4e-1, 2.0, 8e-1)


def test_traced_tables_completed_with_attributes_end_to_end(rb):
    """vert_heterogeneous, op6, four stations on each of the lines x = 4 and x = -1.5 of section 34's traced case, on its 71 x 57
    grid, each with a fan of 0.05 .. 1.5 rad only, with amplitude=True.  fill_attributes=True leaves the covered nodes' bits in
    every column, gives every filled node a finite theta0, theta and G and every node a finite position_slope, is the
    restatement on the device's own tables bit for bit, lies within the recorded distance of the closed forms, and lets an
    anti-aliased, angle-binned, amplitude-weighted Kirchhoff handle use more pairs than the same table without it."""
    box = LIMITS["vert_heterogeneous"]
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    grid = TRACED_GRID
    ys = np.linspace(-2.1, 0.5, 4)
    kw = dict(step=rb.DELTA_S, max_size=ms, box=box, amplitude=True, fill="eikonal")
    fan = np.linspace(0.05, 1.5, 512)
    st_right, st_left = np.stack([np.full(4, 4.0), ys], axis=1), np.stack([np.full(4, -1.5), ys], axis=1)
    stations = np.concatenate([st_right, st_left])
    sides = ((st_right, (np.pi - fan)[::-1].copy()), (st_left, fan))
    plain = [rb.traveltime_table(rb.op6, F, st, grid, thetas=th, **kw) for st, th in sides]
    full = [rb.traveltime_table(rb.op6, F, st, grid, thetas=th, fill_attributes=True, stats=True, **kw) for st, th in sides]
    stats = [f.pop("stats") for f in full]
    assert all("eikonal_attributes" in st and st["eikonal_attributes"]["rounds_max"] >= 1 for st in stats)
    cat = lambda tabs, k: np.concatenate([t[k] for t in tabs])       # noqa: E731
    filled = cat(full, "filled") == 1
    assert np.array_equal(cat(plain, "filled") == 1, filled) and 0.1 < filled.mean() < 0.95
    # the same keys; T, count, ray and step as without the flag; covered nodes keep every column's bits
    for p, f in zip(plain, full):
        assert sorted(p) == sorted(f)
        for k in p:
            m = slice(None) if k in ("T", "count", "ray", "step", "filled") else (f["filled"] == 0)
            assert p[k].dtype == f[k].dtype and np.array_equal(p[k][m], f[k][m], equal_nan=True), k
    for k in ("theta0", "theta", "J", "G"):
        assert np.isnan(cat(plain, k)[filled]).all() and np.isfinite(cat(full, k)[~filled]).all(), k
    assert np.isfinite(cat(full, "theta0")).all() and np.isfinite(cat(full, "theta")).all() and np.isfinite(cat(full, "G")).all()
    assert (cat(full, "kmah")[filled] == 0).all()
    n_st = F.n_gradient(stations[:, 0], stations[:, 1])[0]
    for f, sl in zip(full, (slice(0, 4), slice(4, 8))):
        assert np.isfinite(rb.position_slope(f, n_st[sl], direction=(0.0, 1.0))).all()
    # the restatement on the device's own tables, with the field's own samples
    X, Y = R.nodes(grid)
    n = F.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(X.shape)
    fill = {"T": cat(full, "T"), "filled": cat(full, "filled")}
    want = A.solve(grid, n, stations, n_st, fill, theta0=cat(plain, "theta0"), J=cat(plain, "J"), G=cat(plain, "G"))
    for k in ("theta0", "J", "G"):
        assert L.same_but_nan(cat(full, k), want[k]), k
    assert L.same_but_nan(cat(full, "theta")[filled], np.arctan2(want["py"], want["px"])[filled])
    # the closed forms
    th_c = np.stack([A.gradient_theta0(X, Y, sx, sy) for sx, sy in stations])
    G_c = 1.0 / np.sqrt(n[None] * np.stack([A.gradient_J(X, Y, sx, sy) for sx, sy in stations]))
    e = np.abs((want["theta0"] - th_c + np.pi) % (2.0 * np.pi) - np.pi)
    ge = np.abs(want["G"] - G_c) / G_c
    ec = np.abs((cat(plain, "theta0") - th_c + np.pi) % (2.0 * np.pi) - np.pi)[~filled]
    gc = (np.abs(cat(plain, "G") - G_c) / G_c)[~filled]
    got = (float(np.median(e[filled])), float(e[filled].max()), float(np.median(ge[filled])))
    spikes = float((want["G"][filled] > 3.0 * G_c[filled]).mean())
    print(f"traced case: {int(filled.sum())} of {filled.size} nodes filled; at the filled nodes theta0 median {got[0]:.3e} largest "
          f"{got[1]:.3e} rad, G median {got[2]:.3e}, G over three times the closed form at {spikes:.3e} of them; at the covered "
          f"nodes theta0 median {np.median(ec):.3e} largest {ec.max():.3e} rad, G median {np.median(gc):.3e}")
    # for the record, not asserted: the filled nodes whose true launch angle the fan holds (beyond the rays' ends, in rejected gaps)
    lo, hi = np.where(np.arange(8) < 4, np.pi - 1.5, 0.05)[:, None, None], np.where(np.arange(8) < 4, np.pi - 0.05, 1.5)[:, None, None]
    inside = filled & (th_c >= lo) & (th_c <= hi)
    if inside.any():
        print(f"traced case: {int(inside.sum())} filled nodes inside the wedge: theta0 median {np.median(e[inside]):.3e} largest "
              f"{e[inside].max():.3e} rad, G median {np.median(ge[inside]):.3e}")
    # the Kirchhoff handle: every pair of the four stations of each side
    counts = []
    for tabs in (plain, full):
        tab = {k: cat(tabs, k) for k in ("T", "theta0", "theta", "G")}
        isrc, irec = [a.reshape(-1) for a in np.meshgrid(np.arange(8), np.arange(8))]
        op = rb.Kirchhoff.from_table(tab, isrc, irec, 256, 0.004, amplitude=True, nbin=4, dopen=0.5,
                                     antialias=dict(n_at_positions=n_st, direction=(0.0, 1.0), asrc=0.5, arec=0.5))
        try:
            counts.append(op.migrate(np.zeros((len(isrc), 256)), stats=True)[1]["contributing"])
        finally:
            op.close()
    F.close()
    print(f"traced case: contributing pairs {counts[0]} without the attributes, {counts[1]} with them")
    assert counts[1] > counts[0] > 0
    assert all(g <= b for g, b in zip(got, TRACED_BOUNDS)), (got, TRACED_BOUNDS)
