"""GPU: the factored update linearised (linearise="factored", rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED_LIN; DESIGN.md
section 40).  The yardstick is tests/eikonal_factored_lin_ref.py, the serial sweeps in Python floats over the restatement's own
factored fill, and every comparison is bit for bit on dT, lam, g, g_src, rounds and converged.  Shapes: the grids of
tests/test_gpu_eikonal_lin.py -- 1 x 1, 1 x 70, 70 x 1, 5 x 70, 64 x 64, 65 x 63 and 100 x 90, each on the LDS path where it fits and
on the global path -- and 300 x 260, whose rows and diagonals make the 256 lanes stride, under a cap of two rounds so that the
restatement stays quick (a capped sweep's bits are defined as any other's); the corridor with three sources, also under a cap of
one round; the walls with dT_seed; a source exactly on a node and an obstacle's n_src; the device-pointer forms, two runs, five
sources against five calls; the batched entries at every chunk width; schemes 0 and 1 through the same entries, which give
tests/eikonal_lin_ref.py's bits; and the tomography handle: both products, relinearise, and one LSQR step against the plain
handle's."""
import ctypes as C
import functools

import numpy as np
import pytest

import eikonal_factored_lin_ref as FL
import eikonal_factored_ref as F
import eikonal_lin_ref as L
import eikonal_ref as R
import eikonal_tomo_ref as E

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


def inputs(n, S, seed):
    """dn [ny, nx], dn_src [S], dT_seed and r [S, ny, nx]: normal draws, dn scaled by n where n is a number"""
    rng = np.random.default_rng(seed)
    ok = np.isfinite(n)
    dn = np.where(ok, 0.1 * np.where(ok, n, 0.0) * rng.standard_normal(n.shape), rng.standard_normal(n.shape))
    return dn, 0.1 * rng.standard_normal(S), rng.standard_normal((S,) + n.shape), rng.standard_normal((S,) + n.shape)


def same_tangent(got, want, what=""):
    assert R.same_bits(got["dT"], want["dT"]), f"{what}: dT differs at {int((got['dT'] != want['dT']).sum())} nodes"
    assert np.array_equal(got["rounds"], want["rounds"]), (what, got["rounds"], want["rounds"])
    assert np.array_equal(got["converged"], want["converged"]), (what, got["converged"], want["converged"])


def same_adjoint(got, want, what=""):
    for k in ("lam", "g", "g_src"):
        assert R.same_bits(got[k], want[k]), f"{what}: {k} differs at {int((got[k] != want[k]).sum())} places"
    assert np.array_equal(got["rounds"], want["rounds"]), (what, got["rounds"], want["rounds"])
    assert np.array_equal(got["converged"], want["converged"]), (what, got["converged"], want["converged"])


def check_stats(st, nets, want, path):
    assert st["path"] == path and st["changes"] == want["changes"] and st["rounds_max"] == int(want["rounds"].max())
    assert st["free_nodes"] == st["filled"] == sum(len(net.free) + net.cls.count(L.BALL) for net in nets) and st["unreached"] == 0
    assert st["kernel_ms"] > 0.0


def both(rb, grid, n, src, ns, fill, nets, seed, what, global_path, path=None, use_seed=False, max_rounds=0):
    """the device's factored tangent and adjoint of one case against the restatement's"""
    dn, dns, sd, r = inputs(n, len(src), seed)
    sd = sd if use_seed else None
    want_t, want_a = FL.tangent(nets, dn, dns, sd, max_rounds=max_rounds), FL.adjoint(nets, r, max_rounds=max_rounds)
    kw = dict(n_src=ns, stats=True, max_rounds=max_rounds, _global_path=global_path, linearise="factored")
    got_t = rb.eikonal_tangent(n, src, grid, fill, dn, dn_src=dns, dT_seed=sd, **kw)
    got_a = rb.eikonal_adjoint(n, src, grid, fill, r, **kw)
    same_tangent(got_t, want_t, what + ", tangent")
    same_adjoint(got_a, want_a, what + ", adjoint")
    if path:
        check_stats(got_t["stats"], nets, want_t, path)
        check_stats(got_a["stats"], nets, want_a, path)
    return want_t, want_a


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


@functools.lru_cache(maxsize=None)
def shape_case(nx, ny, S=2):
    grid, n, src, ns = smooth_problem(nx, ny, S, 100 * nx + ny)
    return FL.filled((grid, n, src, ns, None))


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_where_lane_wave_and_block_loops_can_go_wrong(rb, nx, ny, global_path):
    grid, n, src, ns, fill, _, nets = shape_case(nx, ny)
    assert fill["filled"].all() and fill["converged"].all()
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, nx + ny, f"{nx} x {ny}", global_path,
                          "global" if global_path or nx * ny * 26 > 128 * 1024 else "lds")
    assert want_t["converged"].all() and want_a["converged"].all()
    if nx * ny > 70:
        assert (want_a["g_src"] != 0.0).all() and (want_t["rounds"] > 3).any()


def test_grid_over_the_lds_capacity_with_striding_lanes(rb):
    """300 x 260: 78 000 nodes against the LDS path's 5 041; diagonals of 260 nodes and, in the g_src pass, 260 rows for 256
    lanes.  The table is the device's factored fill (held to the restatement in tests/test_gpu_eikonal_factored.py) and the
    sweeps are capped at two rounds: the restatement's ten rounds of 78 000 nodes would take a quarter of a minute"""
    grid, n, src, ns = smooth_problem(300, 260, 1, 30260)
    fill = rb.eikonal_fill(n, src, grid, n_src=ns, scheme="factored")
    assert fill["converged"].all() and fill["filled"].all()
    nets = FL.nets(grid, n, src, ns, fill)
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 7, "300 x 260", False, "global", max_rounds=2)
    assert not want_t["converged"].any() and not want_a["converged"].any() and want_a["g_src"][0] != 0.0


# ------------------------------------------------------------------------------------------------- the several-round medium
@functools.lru_cache(maxsize=None)
def named(name):
    return FL.filled(getattr(L, name)())


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_with_three_sources_and_under_a_cap_of_one_round(rb, global_path):
    grid, n, src, ns, fill, _, nets = named("corridor_case")
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 3, "corridor", global_path, "global" if global_path else "lds")
    assert (want_t["rounds"] > 3).all() and (want_a["rounds"] > 3).all() and want_t["converged"].all() and want_a["converged"].all()
    cap_t, cap_a = both(rb, grid, n, src, ns, fill, nets, 3, "corridor, max_rounds 1", global_path, max_rounds=1)
    assert (cap_t["rounds"] == 1).all() and not cap_t["converged"].any() and not cap_a["converged"].any()
    assert not R.same_bits(cap_t["dT"], want_t["dT"]) and not R.same_bits(cap_a["lam"], want_a["lam"])


# ------------------------------------------------------------------------------------------ obstacles, a pocket, seeds
@pytest.mark.parametrize("global_path", [False, True])
def test_walls_with_dT_seed(rb, global_path):
    grid, n, src, ns, fill, _, nets = named("walls_case")
    cls = np.array([net.cls for net in nets]).reshape(fill["T"].shape)
    assert all(set(c.reshape(-1)) == {L.DEAD, L.SEED, L.FREE, L.BALL} for c in cls) and (cls[:, 9:14, 31:35] == L.DEAD).all()
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 5, "walls", global_path, use_seed=True)
    assert (want_t["dT"][cls == L.DEAD] == 0).all() and (want_a["lam"][cls == L.DEAD] == 0).all()
    _, _, sd, _ = inputs(n, len(src), 5)
    assert R.same_bits(want_t["dT"][cls == L.SEED], sd[cls == L.SEED])


@functools.lru_cache(maxsize=None)
def fallback_case():
    """41 x 23 with three sources: one exactly on a node with no ball, so that the node is free with rr == 0; one with an
    obstacle's n_src, seeded by a few nodes of a table; one ordinary, with a seed for the call without a ball"""
    grid, n, _, _ = smooth_problem(41, 23, 1, 4123)
    X, Y = R.nodes(grid)
    src = np.array([[X[11, 17], Y[11, 17]], [0.33, -0.71], [1.07, -1.9]])
    ns = np.array([n[11, 17], -1.0, 1.3])
    T = np.full((3,) + n.shape, np.nan)
    T[0, 11, 16], T[0, 10, 17] = 0.11, 0.13             # seeds beside the first source's node
    T[1, 5, 5:9], T[2, 3, 30] = 0.5, 0.2
    return grid, n, src, ns, T


@pytest.mark.parametrize("global_path", [False, True])
def test_source_on_a_node_and_an_obstacles_n_src(rb, global_path):
    grid, n, src, ns, T = fallback_case()
    for ball, s_on_node_free in ((-1.0, True), (2.0, False)):
        fill = F.solve(grid, n, src, ns, T=T, ball=ball)
        assert fill["converged"].all()
        nets, plain = FL.nets(grid, n, src, ns, fill, ball), L.nets(grid, n, src, ns, fill, ball)
        x = 11 * 41 + 17
        assert (nets[0].cls[x] == L.FREE) == s_on_node_free
        if s_on_node_free:                                       # rr == 0: the plain coefficients and no share of g_src
            assert nets[0].csrc[x] == 0.0 and (nets[0].ca[x], nets[0].cb[x], nets[0].cs[x]) == (plain[0].ca[x], plain[0].cb[x], plain[0].cs[x])
            assert nets[0].par[x] != 0
        assert not any(nets[1].csrc) and nets[1].ca == plain[1].ca                           # the obstacle's n_src: every node plain
        dn, dns, sd, r = inputs(n, 3, 12)
        kw = dict(n_src=ns, ball=ball, _global_path=global_path, linearise="factored")
        same_tangent(rb.eikonal_tangent(n, src, grid, fill, dn, dn_src=dns, dT_seed=sd, **kw), FL.tangent(nets, dn, dns, sd), f"ball {ball}")
        got = rb.eikonal_adjoint(n, src, grid, fill, r, **kw)
        same_adjoint(got, FL.adjoint(nets, r), f"ball {ball}")
        assert got["g_src"][1] == 0.0 and got["g_src"][2] != 0.0


def test_device_forms_repeated_runs_and_split_over_sources(rb, torch):
    grid, n, src, ns, fill, _, nets = named("walls_case")
    dn, dns, sd, r = inputs(n, len(src), 8)
    want_t, want_a = FL.tangent(nets, dn, dns, sd), FL.adjoint(nets, r)
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    d_fill = {"T": up(fill["T"]), "filled": up(fill["filled"])}
    host = lambda res: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}     # noqa: E731
    for rep in range(2):
        got = rb.eikonal_tangent_device(up(n), up(src), grid, d_fill, up(dn), n_src=up(ns), dn_src=up(dns), dT_seed=up(sd),
                                        linearise="factored")
        assert got["dT"].is_cuda
        same_tangent(host(got), want_t, f"device form, run {rep}")
        got = rb.eikonal_adjoint_device(up(n), up(src), grid, d_fill, up(r), n_src=up(ns), linearise="factored")
        assert got["lam"].is_cuda and got["g"].is_cuda and got["g_src"].is_cuda
        same_adjoint(host(got), want_a, f"device form, run {rep}")
    assert R.same_bits(d_fill["T"].cpu().numpy(), fill["T"])                 # the tables are read, not written
    # S = 5 in one call against five calls of one source
    grid, n, src, ns, fill, _, nets = shape_case(41, 23, 5)
    dn, dns, sd, r = inputs(n, 5, 9)
    kw = dict(linearise="factored")
    whole_t = rb.eikonal_tangent(n, src, grid, fill, dn, n_src=ns, dn_src=dns, **kw)
    whole_a = rb.eikonal_adjoint(n, src, grid, fill, r, n_src=ns, **kw)
    for s in range(5):
        one = {k: v[s:s + 1] for k, v in fill.items() if k in ("T", "filled")}
        got = rb.eikonal_tangent(n, src[s:s + 1], grid, one, dn, n_src=ns[s:s + 1], dn_src=dns[s:s + 1], **kw)
        same_tangent(got, {k: whole_t[k][s:s + 1] for k in ("dT", "rounds", "converged")}, f"source {s} alone")
        got = rb.eikonal_adjoint(n, src[s:s + 1], grid, one, r[s:s + 1], n_src=ns[s:s + 1], **kw)
        same_adjoint(got, {k: whole_a[k][s:s + 1] for k in ("lam", "g", "g_src", "rounds", "converged")}, f"source {s} alone")
    same_tangent(whole_t, FL.tangent(nets, dn, dns), "five sources")
    same_adjoint(whole_a, FL.adjoint(nets, r), "five sources")


# ------------------------------------------------------------------------------------------------------ several columns
#        K, the forced chunk width (0: the call's own choice): whole chunks, a partial chunk, one column, two chunks
MULTI = [(1, 0), (3, 0), (3, 4), (4, 4), (4, 0), (8, 8), (8, 4), (8, 0)]


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("K,width", MULTI)
def test_multi_column_c_is_the_single_call(rb, torch, K, width, global_path):
    grid, n, src, ns, fill, _, nets = shape_case(41, 23, 5)
    src, ns = src[:3], ns[:3]
    fill = {k: fill[k][:3] for k in ("T", "filled")}
    rng = np.random.default_rng(50 + K)
    dn, dns = 0.1 * rng.standard_normal((K,) + n.shape), 0.1 * rng.standard_normal((K, 3))
    sd, r = rng.standard_normal((K, 3) + n.shape), rng.standard_normal((K, 3) + n.shape)
    kw = dict(n_src=ns, _global_path=global_path, linearise="factored")
    mt = rb.eikonal_tangent_multi(n, src, grid, fill, dn, dn_src=dns, dT_seed=sd, _width=width, **kw)
    ma = rb.eikonal_adjoint_multi(n, src, grid, fill, r, _width=width, **kw)
    for c in range(K):
        one = rb.eikonal_tangent(n, src, grid, fill, dn[c], dn_src=dns[c], dT_seed=sd[c], **kw)
        same_tangent({k: mt[k][c] for k in ("dT", "rounds", "converged")}, one, f"K {K}, width {width}, column {c}")
        one = rb.eikonal_adjoint(n, src, grid, fill, r[c], **kw)
        same_adjoint({k: ma[k][c] for k in ("lam", "g", "g_src", "rounds", "converged")}, one, f"K {K}, width {width}, column {c}")
    # the last column against the restatement, and the device-pointer forms against the host forms
    same_tangent({k: mt[k][K - 1] for k in ("dT", "rounds", "converged")}, FL.tangent(nets[:3], dn[K - 1], dns[K - 1], sd[K - 1]), "twin")
    same_adjoint({k: ma[k][K - 1] for k in ("lam", "g", "g_src", "rounds", "converged")}, FL.adjoint(nets[:3], r[K - 1]), "twin")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")     # noqa: E731
    d_fill = {"T": up(fill["T"]), "filled": up(fill["filled"])}
    dkw = dict(n_src=up(ns), _global_path=global_path, _width=width, linearise="factored")
    dt = rb.eikonal_tangent_multi_device(up(n), up(src), grid, d_fill, up(dn), dn_src=up(dns), dT_seed=up(sd), **dkw)
    da = rb.eikonal_adjoint_multi_device(up(n), up(src), grid, d_fill, up(r), **dkw)
    assert R.same_bits(dt["dT"].cpu().numpy(), mt["dT"]) and np.array_equal(dt["rounds"], mt["rounds"])
    for k in ("lam", "g", "g_src"):
        assert R.same_bits(da[k].cpu().numpy(), ma[k]), k
    assert np.array_equal(da["rounds"], ma["rounds"]) and np.array_equal(da["converged"], ma["converged"])


# ---------------------------------------------------------------------------------- the other schemes keep their bits
def raw_tangent_adjoint(rb, scheme, grid, n, src, ns, fill, dn, dns, r, global_path):
    """rtmi_eikonal_tangent and rtmi_eikonal_adjoint with ep->scheme set to `scheme` as a number, which the Python layer does not
    offer for 1"""
    from raytracing_amd import _lib
    ep = rb.eikonal_params(grid, _global_path=global_path)
    ep.scheme = scheme
    S = len(src)
    T, filled = np.ascontiguousarray(fill["T"]), np.ascontiguousarray(fill["filled"], dtype=np.uint8)
    u8 = filled.ctypes.data_as(C.POINTER(C.c_uint8))
    dT, lam, g, g_src = np.zeros(T.shape), np.zeros(T.shape), np.zeros(T.shape), np.zeros(S)
    rt, ra = np.zeros((S, 2), dtype=np.int32), np.zeros((S, 2), dtype=np.int32)
    d = _lib.dptr
    src, ns, n, dn, dns, r = (np.ascontiguousarray(a, dtype=np.float64) for a in (src, ns, n, dn, dns, r))
    _lib.check(_lib.lib().rtmi_eikonal_tangent(C.byref(ep), d(n), S, d(src), d(ns), d(T), u8, d(dn), d(dns), None, d(dT),
                                               rt.ctypes.data_as(_lib._ip), None))
    _lib.check(_lib.lib().rtmi_eikonal_adjoint(C.byref(ep), d(n), S, d(src), d(ns), d(T), u8, d(r), d(lam), d(g), d(g_src),
                                               ra.ctypes.data_as(_lib._ip), None))
    return ({"dT": dT, "rounds": rt[:, 0].copy(), "converged": rt[:, 1].copy()},
            {"lam": lam, "g": g, "g_src": g_src, "rounds": ra[:, 0].copy(), "converged": ra[:, 1].copy()})


@pytest.mark.parametrize("global_path", [False, True])
def test_schemes_0_and_1_give_the_plain_linearisation_of_the_same_table(rb, global_path):
    grid, n, src, ns, fill, plain, nets = named("gradient_case")
    dn, dns, _, r = inputs(n, len(src), 21)
    want_t, want_a = L.tangent(plain, dn, dns), L.adjoint(plain, r)
    for scheme in (0, 1):
        got_t, got_a = raw_tangent_adjoint(rb, scheme, grid, n, src, ns, fill, dn, dns, r, global_path)
        same_tangent(got_t, want_t, f"scheme {scheme}")
        same_adjoint(got_a, want_a, f"scheme {scheme}")
    got_t, got_a = raw_tangent_adjoint(rb, 3, grid, n, src, ns, fill, dn, dns, r, global_path)
    same_tangent(got_t, FL.tangent(nets, dn, dns), "scheme 3")
    same_adjoint(got_a, FL.adjoint(nets, r), "scheme 3")
    assert not R.same_bits(got_t["dT"], want_t["dT"]) and (got_t["rounds"] > want_t["rounds"]).all()
    # and the Python layer's default is the plain one
    same_tangent(rb.eikonal_tangent(n, src, grid, fill, dn, n_src=ns, dn_src=dns, _global_path=global_path), want_t, "default")
    same_adjoint(rb.eikonal_adjoint(n, src, grid, fill, r, n_src=ns, _global_path=global_path), want_a, "default")


# ------------------------------------------------------------------------------------------------------ the handle
TOMO_SOURCES = (0, 2, 5, 7)         # of eikonal_lin_ref.tomography_case's eight: the restatement's step on all eight takes 8 s


@functools.lru_cache(maxsize=None)
def handle_case():
    grid, n0, n_true, src, rec, idx, w = L.tomography_case()
    src, idx, w = src[list(TOMO_SOURCES)], idx[list(TOMO_SOURCES)], w[list(TOMO_SOURCES)]
    pts = np.stack([grid[0] + (rec % grid[2]) * grid[1], grid[3] + (rec // grid[2]) * grid[4]], axis=1)      # the receiver nodes
    ns = lambda n: (n.reshape(-1)[idx] * w).sum(axis=1)             # noqa: E731
    return grid, n0, n_true, src, rec, pts, ns


def restated(grid, n, src, ns, pts):
    """eikonal_tomo_ref's handle on the restatement's factored fill, with the factored networks"""
    fill = F.solve(grid, n, src, ns)
    op = E.Operator(grid, n, src, ns, fill, pts)
    op.nets = FL.nets(grid, n, src, ns, fill)
    return op


def test_handle_products_are_the_restatements_and_relinearise_keeps_the_mode(rb):
    grid, n0, n_true, src, rec, pts, ns = handle_case()
    op = restated(grid, n0, src, ns(n0), pts)
    rng = np.random.default_rng(17)
    dn, y = rng.standard_normal(op.nn), rng.standard_normal(op.S * op.R)
    T = rb.EikonalTomography(n0, src, grid, pts, n_src=ns(n0), scheme="factored", linearise="factored")
    P = rb.EikonalTomography(n0, src, grid, pts, n_src=ns(n0), scheme="factored")
    assert L.same_but_nan(T.table()["T"], op.fill["T"]) and R.same_bits(T.table()["T"], P.table()["T"])      # the same fill
    want_y, want_G = op.apply(dn), op.transpose(y)
    assert R.same_bits(T.apply(dn), want_y) and R.same_bits(T.transpose(y).reshape(-1), want_G)
    assert not R.same_bits(P.apply(dn), want_y) and not R.same_bits(P.transpose(y).reshape(-1), want_G)
    # several columns through the handle
    Y = T.matmat(np.stack([dn, 2.0 * dn, -dn]).reshape(3, op.ny, op.nx))
    assert R.same_bits(Y[0], want_y) and R.same_bits(Y[2], T.apply(-dn))
    G = T.rmatmat(np.stack([y, -y]))
    assert R.same_bits(G[0].reshape(-1), want_G) and R.same_bits(G[1], T.transpose(-y))
    # a handle on tables the caller filled with the factored scheme
    Q = rb.EikonalTomography(n0, src, grid, pts, n_src=ns(n0), fill_result=op.fill, linearise="factored")
    assert R.same_bits(Q.apply(dn), want_y) and R.same_bits(Q.transpose(y).reshape(-1), want_G)
    Q.close()
    # relinearise: the factored fill and the factored linearisation of the new medium
    T.relinearise(n_true, ns(n_true))
    op2 = restated(grid, n_true, src, ns(n_true), pts)
    assert L.same_but_nan(T.table()["T"], op2.fill["T"])
    assert R.same_bits(T.apply(dn), op2.apply(dn)) and R.same_bits(T.transpose(y).reshape(-1), op2.transpose(y))
    T.close(), P.close()


def test_one_lsqr_step_reproduces_the_restatements_ratio_and_beats_the_plain_handles(rb):
    """The step of tests/test_eikonal_factored_lin_ref.py on four of its sources.  Both sides run the same 40 iterations of
    LSQR in fp64 on Jacobians that agree to rounding (1e-13), the restatement's by scipy on a dense matrix, so the ratios agree
    far below the 1e-6 asked here, which is what tests/test_gpu_eikonal_tomo.py asks of the same kind of pair"""
    grid, n0, n_true, src, rec, pts, ns = handle_case()
    rms = lambda r: float(np.sqrt(np.mean(r * r)))                  # noqa: E731
    at = lambda T: T.reshape(len(src), -1)[:, rec].reshape(-1)      # noqa: E731
    data = at(rb.eikonal_fill(n_true, src, grid, n_src=ns(n_true), scheme="factored")["T"])
    ratios = {}
    for linearise in ("factored", "plain"):
        T = rb.EikonalTomography(n0, src, grid, pts, n_src=ns(n0), scheme="factored", linearise=linearise)
        r0 = data - at(T.table()["T"])
        out = T.lsqr(r0, L.TOMO_ITERS, damp=L.TOMO_DAMP)
        n1 = n0 + out["x"]
        r1 = data - at(rb.eikonal_fill(n1, src, grid, n_src=ns(n1), scheme="factored")["T"])
        ratios[linearise] = rms(r1) / rms(r0)
        T.close()
    before, after, _ = FL.tomography_step("factored", TOMO_SOURCES)
    print(f"LSQR step on the device: factored {ratios['factored']:.6e} (the restatement {after / before:.6e}), plain {ratios['plain']:.6e}")
    assert abs(ratios["factored"] - after / before) <= 1e-6 * (after / before)
    assert ratios["factored"] < ratios["plain"]
