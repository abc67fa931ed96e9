"""GPU: several right-hand sides through the linearised eikonal fill in one call (rtmi_eikonal_tangent_multi,
rtmi_eikonal_adjoint_multi and their _dev forms), and, in the second half of the file, through the products
and the solver of the tomography handle on it.  The yardstick is the single entry on the same column in
the same process, compared as bytes (NaN by place: a NaN's payload is the processor's) on dT, lam, g, g_src, rounds and converged;
at the small shapes tests/eikonal_lin_ref.py, the serial sweeps in Python floats, is a yardstick too.  A batched result is never
compared with another batched result alone.  The compiled chunk widths are 1, 4 and 8.  A call chooses among them from K, S and
the device's CUs (the widest that K fills and that still leaves a workgroup per CU), which at a test's few sources is always 1; so
the tests force the width (ep->reserved[1], on which no result depends) to the widest that K fills, and K = 1, 2, 3, 4, 5, 8, 9
covers every width alone, each with a partial last chunk, and more than one chunk; the call's own choice is checked on 128 sources.  Grids: 1 x 1, 1 x 70,
13 x 11; 65 x 63, which is on the LDS path at width 1 (26 bytes per node of 128 KiB) and on the global path at widths 4 and 8; 50 x
40, on the LDS path at widths 1 and 4 and on the global path at 8; 300 x 260, over LDS at every width and with diagonals longer than
the block."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9)


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


def width(K):
    return 8 if K >= 8 else 4 if K >= 4 else 1


def path(nx, ny, K, global_path):
    return "global" if global_path or nx * ny * (8 * width(K) + 18) > 128 * 1024 else "lds"


def columns(n, S, K, seed):
    """dn [K, ny, nx], dn_src [K, S], dT_seed and r [K, S, ny, nx]: normal draws, dn scaled by n where n is a number"""
    rng = np.random.default_rng(seed)
    ok = np.isfinite(n)
    dn = np.where(ok, 0.1 * np.where(ok, n, 0.0), 1.0) * rng.standard_normal((K,) + n.shape)
    return dn, 0.1 * rng.standard_normal((K, S)), rng.standard_normal((K, S) + n.shape), rng.standard_normal((K, S) + n.shape)


def same(a, b):
    return L.same_but_nan(a, b)


def against_singles(rb, grid, n, src, ns, fill, cols, what, global_path=False, use_src=True, use_seed=False, max_rounds=0, want_path=None,
                    forced=None):
    """the batched tangent and adjoint of `cols`, at the chunk width `forced` (None: the widest that K fills; 0: the call's own
    choice), against one single call per column; returns the single calls' results"""
    dn, dns, sd, r = cols
    K = len(dn)
    kw = dict(n_src=ns, stats=True, max_rounds=max_rounds, _global_path=global_path)
    w = width(K) if forced is None else forced
    got_t = rb.eikonal_tangent_multi(n, src, grid, fill, dn, dn_src=dns if use_src else None, dT_seed=sd if use_seed else None, _width=w, **kw)
    got_a = rb.eikonal_adjoint_multi(n, src, grid, fill, r, _width=w, **kw)
    singles_t, singles_a = [], []
    for c in range(K):
        one_t = rb.eikonal_tangent(n, src, grid, fill, dn[c], dn_src=dns[c] if use_src else None, dT_seed=sd[c] if use_seed else None, **kw)
        one_a = rb.eikonal_adjoint(n, src, grid, fill, r[c], **kw)
        assert same(got_t["dT"][c], one_t["dT"]), f"{what}: dT of column {c} of {K}"
        for k in ("lam", "g", "g_src"):
            assert same(got_a[k][c], one_a[k]), f"{what}: {k} of column {c} of {K}"
        for got, one in ((got_t, one_t), (got_a, one_a)):
            assert np.array_equal(got["rounds"][c], one["rounds"]), (what, c, got["rounds"][c], one["rounds"])
            assert np.array_equal(got["converged"][c], one["converged"]), (what, c, got["converged"][c], one["converged"])
        singles_t.append(one_t)
        singles_a.append(one_a)
    for got, singles in ((got_t, singles_t), (got_a, singles_a)):
        st = got["stats"]
        assert st["changes"] == sum(s["stats"]["changes"] for s in singles), what
        assert st["free_nodes"] == st["filled"] == sum(s["stats"]["free_nodes"] for s in singles), what
        assert st["rounds_max"] == max(s["stats"]["rounds_max"] for s in singles) and st["kernel_ms"] > 0.0
        if want_path:
            assert st["path"] == want_path, (what, st["path"], want_path)
    return singles_t, singles_a


# ------------------------------------------------------------------------------------------------------------------- shapes
def smooth_problem(nx, ny, S, seed):
    """a smooth medium with a slow lens, spacings that differ, sources inside the grid and off its nodes"""
    rng = np.random.default_rng(seed)
    grid = (-2.0, 0.1, nx, -2.3, 0.125, ny)
    X, Y = R.nodes(grid)
    cx, cy = X.mean(), Y.mean()
    lens = lambda x, y: 1.0 + 0.05 * (x - X.min()) + 0.6 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (0.1 * max(nx, ny)) ** 2)   # noqa: E731
    src = np.stack([rng.uniform(X.min(), X.max() + 1e-9, S), rng.uniform(Y.min(), Y.max() + 1e-9, S)], axis=1)
    return grid, lens(X, Y), src, lens(src[:, 0], src[:, 1])


_FILLS = {}


def device_case(rb, nx, ny, S):
    """a smooth problem with the device's own fill, once per shape"""
    key = (nx, ny, S)
    if key not in _FILLS:
        grid, n, src, ns = smooth_problem(nx, ny, S, 100 * nx + ny)
        fill = rb.eikonal_fill(n, src, grid, n_src=ns)
        assert fill["converged"].all() and fill["filled"].all()
        _FILLS[key] = (grid, n, src, ns, {"T": fill["T"], "filled": fill["filled"]})
    return _FILLS[key]


SHAPES = [(1, 1), (1, 70), (13, 11), (50, 40), (65, 63)]


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_width_alone_with_a_partial_chunk_and_in_several_chunks(rb, nx, ny, global_path):
    grid, n, src, ns, fill = device_case(rb, nx, ny, 2)
    for K in KS:
        cols = columns(n, 2, K, 1000 * K + nx)
        against_singles(rb, grid, n, src, ns, fill, cols, f"{nx} x {ny}, K {K}", global_path, use_src=K % 2 == 1, use_seed=K % 3 == 0,
                        want_path=path(nx, ny, K, global_path))
    assert path(65, 63, 1, False) == "lds" and path(65, 63, 4, False) == "global"
    assert path(50, 40, 4, False) == "lds" and path(50, 40, 8, False) == "global"


def test_the_calls_own_choice_of_width(rb, torch):
    """50 x 40 is on the LDS path at widths 1 and 4 and on the global path at 8, so the path shows the width the call chose"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid, n, src, ns, fill = device_case(rb, 50, 40, 2)
    # two sources: even single columns leave CUs idle, width 1
    against_singles(rb, grid, n, src, ns, fill, columns(n, 2, 9, 1), "50 x 40, 2 sources, the call's choice", forced=0, want_path="lds")
    S = 128
    grid, n, src, ns, fill = device_case(rb, 50, 40, S)
    for K in (8, 16):
        want = max([1] + [w for w in (1, 4, 8) if w <= K and -(-K // w) * S >= cus])
        cols = columns(n, S, K, K)
        got_t = rb.eikonal_tangent_multi(n, src, grid, fill, cols[0], n_src=ns, stats=True)
        got_a = rb.eikonal_adjoint_multi(n, src, grid, fill, cols[3], n_src=ns, stats=True)
        assert got_t["stats"]["path"] == got_a["stats"]["path"] == ("global" if want == 8 else "lds"), (K, cus, want)
        for c in (0, K - 1):
            one_t = rb.eikonal_tangent(n, src, grid, fill, cols[0][c], n_src=ns)
            one_a = rb.eikonal_adjoint(n, src, grid, fill, cols[3][c], n_src=ns)
            assert same(got_t["dT"][c], one_t["dT"]) and same(got_a["g"][c], one_a["g"]) and same(got_a["g_src"][c], one_a["g_src"])
            assert np.array_equal(got_t["rounds"][c], one_t["rounds"]) and np.array_equal(got_a["rounds"][c], one_a["rounds"])


@pytest.mark.parametrize("K", [3, 5, 9])
def test_grid_over_the_lds_capacity_with_striding_lanes(rb, K):
    """300 x 260: over LDS at every width, and diagonals of 260 nodes for 256 lanes"""
    grid, n, src, ns, fill = device_case(rb, 300, 260, 1)
    against_singles(rb, grid, n, src, ns, fill, columns(n, 1, K, K), f"300 x 260, K {K}", want_path="global")


def test_small_shape_against_the_restatement(rb):
    grid, n, src, ns = smooth_problem(13, 11, 2, 7)
    grid, n, src, ns, fill, nets = L.filled((grid, n, src, ns, None))
    dn, dns, sd, r = columns(n, 2, 5, 11)
    got_t = rb.eikonal_tangent_multi(n, src, grid, fill, dn, n_src=ns, dn_src=dns)
    got_a = rb.eikonal_adjoint_multi(n, src, grid, fill, r, n_src=ns)
    for c in range(5):
        want_t, want_a = L.tangent(nets, dn[c], dns[c]), L.adjoint(nets, r[c])
        assert R.same_bits(got_t["dT"][c], want_t["dT"]) and np.array_equal(got_t["rounds"][c], want_t["rounds"])
        for k in ("lam", "g", "g_src"):
            assert R.same_bits(got_a[k][c], want_a[k]), (k, c)
        assert np.array_equal(got_a["rounds"][c], want_a["rounds"]) and np.array_equal(got_a["converged"][c], want_a["converged"])


# ------------------------------------------------------------------------------------------------- the several-round medium
@functools.lru_cache(maxsize=None)
def named(name):
    return L.filled(getattr(L, name)())


def corridor_columns(n, nets, K=5):
    """column 0 all zeros, column 1 with a NaN in r at each source's latest node of the corridor, the others random"""
    dn, dns, sd, r = columns(n, len(nets), K, 3)
    dn[0], dns[0], r[0] = 0.0, 0.0, 0.0
    far = [max((x for x in net.free if n.reshape(-1)[x] == 1.0), key=lambda x: net.T[x]) for net in nets]
    for s, x in enumerate(far):
        r[1, s].reshape(-1)[x] = np.nan
    return dn, dns, sd, r


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_chunk_of_a_zero_column_random_columns_and_a_nan(rb, global_path):
    """one chunk (K = 5 makes a chunk of 4 and one of 1) whose columns need different numbers of rounds"""
    grid, n, src, ns, fill, nets = named("corridor_case")
    cols = corridor_columns(n, nets)
    st, sa = against_singles(rb, grid, n, src, ns, fill, cols, "corridor", global_path)
    # the test does not degenerate: the zero column is clean in its first round, the others need more than three, and the NaN spreads
    assert (st[0]["rounds"] == 1).all() and (sa[0]["rounds"] == 1).all() and (st[2]["rounds"] > 3).all() and (sa[2]["rounds"] > 3).all()
    assert all(s["converged"].all() for s in st + sa) and np.isnan(sa[1]["lam"]).sum(axis=(1, 2)).min() > 100
    # against the restatement too
    want = L.adjoint(nets, cols[3][1])
    got = rb.eikonal_adjoint_multi(n, src, grid, fill, cols[3], n_src=ns, _global_path=global_path)
    assert L.same_but_nan(got["lam"][1], want["lam"]) and np.array_equal(got["rounds"][1], want["rounds"])
    # under a cap of one round the zero column reports clean and the others do not
    ct, ca = against_singles(rb, grid, n, src, ns, fill, cols, "corridor, max_rounds 1", global_path, max_rounds=1)
    for one in (ct, ca):
        assert (one[0]["rounds"] == 1).all() and one[0]["converged"].all()
        assert all((o["rounds"] == 1).all() and not o["converged"].any() for o in one[1:])
    assert not same(ct[2]["dT"], st[2]["dT"]) and not same(ca[2]["lam"], sa[2]["lam"])


@pytest.mark.parametrize("global_path", [False, True])
def test_obstacles_of_every_kind_with_a_sealed_pocket_and_seeds(rb, global_path):
    grid, n, src, ns, fill, nets = named("walls_case")
    cols = columns(n, len(src), 9, 5)
    st, sa = against_singles(rb, grid, n, src, ns, fill, cols, "walls", global_path, use_seed=True)
    want_t, want_a = L.tangent(nets, cols[0][8], cols[1][8], cols[2][8]), L.adjoint(nets, cols[3][8])
    assert R.same_bits(st[8]["dT"], want_t["dT"]) and R.same_bits(sa[8]["g"], want_a["g"]) and R.same_bits(sa[8]["g_src"], want_a["g_src"])


def test_two_columns_swapped_and_two_runs(rb):
    grid, n, src, ns, fill, nets = named("walls_case")
    dn, dns, sd, r = columns(n, len(src), 8, 6)
    kw = dict(n_src=ns)
    t1 = rb.eikonal_tangent_multi(n, src, grid, fill, dn, dn_src=dns, dT_seed=sd, **kw)
    a1 = rb.eikonal_adjoint_multi(n, src, grid, fill, r, **kw)
    one_t = rb.eikonal_tangent(n, src, grid, fill, dn[6], dn_src=dns[6], dT_seed=sd[6], **kw)
    one_a = rb.eikonal_adjoint(n, src, grid, fill, r[6], **kw)
    p = np.array([0, 6, 2, 3, 4, 5, 1, 7])
    t2 = rb.eikonal_tangent_multi(n, src, grid, fill, dn[p], dn_src=dns[p], dT_seed=sd[p], **kw)
    a2 = rb.eikonal_adjoint_multi(n, src, grid, fill, r[p], **kw)
    assert same(t2["dT"][1], one_t["dT"]) and same(a2["g"][1], one_a["g"]) and same(a2["g_src"][1], one_a["g_src"])
    assert same(t2["dT"], t1["dT"][p]) and same(a2["lam"], a1["lam"][p]) and np.array_equal(a2["rounds"], a1["rounds"][p])
    t3 = rb.eikonal_tangent_multi(n, src, grid, fill, dn, dn_src=dns, dT_seed=sd, **kw)
    a3 = rb.eikonal_adjoint_multi(n, src, grid, fill, r, **kw)
    assert same(t3["dT"][6], one_t["dT"]) and same(t3["dT"], t1["dT"])
    assert all(same(a3[k], a1[k]) for k in ("lam", "g", "g_src")) and same(a3["lam"][6], one_a["lam"])


def test_device_forms_and_host_pointers_refused(rb, torch):
    from raytracing_amd import _lib
    grid, n, src, ns, fill, nets = named("walls_case")
    S, K = len(src), 5
    dn, dns, sd, r = columns(n, S, K, 8)
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    d_fill = {"T": up(fill["T"]), "filled": up(fill["filled"])}
    got_t = rb.eikonal_tangent_multi_device(up(n), up(src), grid, d_fill, up(dn), n_src=up(ns), dn_src=up(dns), dT_seed=up(sd))
    got_a = rb.eikonal_adjoint_multi_device(up(n), up(src), grid, d_fill, up(r), n_src=up(ns))
    assert got_t["dT"].is_cuda and got_a["lam"].is_cuda and got_a["g"].is_cuda and got_a["g_src"].is_cuda
    for c in range(K):
        one_t = rb.eikonal_tangent(n, src, grid, fill, dn[c], n_src=ns, dn_src=dns[c], dT_seed=sd[c])
        one_a = rb.eikonal_adjoint(n, src, grid, fill, r[c], n_src=ns)
        assert same(got_t["dT"][c].cpu().numpy(), one_t["dT"]) and np.array_equal(got_t["rounds"][c], one_t["rounds"])
        for k in ("lam", "g", "g_src"):
            assert same(got_a[k][c].cpu().numpy(), one_a[k]), (k, c)
        assert np.array_equal(got_a["rounds"][c], one_a["rounds"]) and np.array_equal(got_a["converged"][c], one_a["converged"])
    assert R.same_bits(d_fill["T"].cpu().numpy(), fill["T"])                 # the tables are read, not written
    with pytest.raises(ValueError, match="on a GPU"):
        rb.eikonal_adjoint_multi_device(up(n), up(src), grid, d_fill, torch.as_tensor(r), n_src=up(ns))
    # host memory handed to the _dev entries themselves is refused by name
    lib = _lib.lib()
    ep = rb.eikonal_params(grid, 2.0, 0, False)
    d = {k: up(v) for k, v in dict(n=n, src=src, ns=ns, dn=dn, r=r).items()}
    out = torch.zeros((K, S) + n.shape, dtype=torch.float64, device=dev)
    host = np.zeros((K, S) + n.shape)
    rc = lib.rtmi_eikonal_tangent_multi_dev(C.byref(ep), d["n"].data_ptr(), S, d["src"].data_ptr(), d["ns"].data_ptr(),
                                            d_fill["T"].data_ptr(), d_fill["filled"].data_ptr(), K, dn.ctypes.data, None, None,
                                            out.data_ptr(), None, None)
    assert rc == -1 and b"d_dn is not memory" in lib.rtmi_last_error()
    rc = lib.rtmi_eikonal_adjoint_multi_dev(C.byref(ep), d["n"].data_ptr(), S, d["src"].data_ptr(), d["ns"].data_ptr(),
                                            d_fill["T"].data_ptr(), d_fill["filled"].data_ptr(), K, d["r"].data_ptr(), host.ctypes.data,
                                            None, None, None, None)
    assert rc == -1 and b"d_lam is not memory" in lib.rtmi_last_error()


# ================================================================================= the handle: products, solver, Python
# (rtmi_eikonal_tomo_apply_multi, _transpose_multi, their _dev forms, _lsqr_multi, _set_column_group).  The yardstick is the single
# entry on the same column of the same handle; at 13 x 11 the restatements (tests/eikonal_tomo_ref.py, tests/lsqr_weighted_ref.py) too.
import eikonal_tomo_ref as E          # noqa: E402
import lsqr_weighted_ref as LW        # noqa: E402


def shape_problem(name):
    """section 36's sources and receivers on a smooth medium, without the restatement's fill: the handle fills its own"""
    grid = E.SHAPE_GRIDS[name]
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = R.nodes(grid)
    med = lambda x, y: 1.0 + 0.25 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2)      # noqa: E731
    src = [E.at(grid, 1.0, 2.0), E.at(grid, nx / 2 - 0.3, ny / 2 - 0.6), [gx0 - 0.6 * gdx, gy0 - 0.7 * gdy]]
    if name == "65x63":
        src += [E.at(grid, 50.4, 10.2), E.at(grid, 7.7, 55.5)]
    src = np.array(src)
    return grid, med(X, Y), src, med(src[:, 0], src[:, 1]), E.shape_receivers(grid)


def product_columns(T, K, seed):
    """X [K, ny nx]; Y [K, S R] with a NaN at every dead row, and column 1, where there is one, at 1e308 on every live row"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K, T.ny * T.nx))
    Y = rng.standard_normal((K, T.S * T.R))
    Y[:, T.table()["live"].reshape(-1) == 0] = np.nan
    if K > 1:
        Y[1] = np.where(np.isnan(Y[1]), np.nan, 1e308)                      # the adjoint sums several of them: not finite
    return X, Y


def products_against_singles(T, K, seed, what):
    X, Y = product_columns(T, K, seed)
    got_y, got_G = T.matmat(X), T.rmatmat(Y)
    assert got_y.shape == (K, T.S * T.R) and got_G.shape == (K, T.ny, T.nx)
    for c in range(K):
        assert R.same_bits(got_y[c], T.apply(X[c])), f"{what}: y of column {c} of {K}"
        assert same(got_G[c], T.transpose(Y[c])), f"{what}: G of column {c} of {K}"
    if K > 1:
        assert not np.isfinite(T.transpose(Y[1])).all() and np.isfinite(got_G[0]).all(), what
    return X, Y, got_y, got_G


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("name", ["13x11", "65x63"])
def test_products_on_the_handle_column_by_column(rb, name, global_path):
    grid, n, src, ns, rec = shape_problem(name)
    for w in (1, 4, 8):                                                     # the sweeps' chunk width, forced: see the head of the file
        T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, _global_path=global_path, _width=w)
        for K in [K for K in KS if width(K) == w]:
            products_against_singles(T, K, 40 + K, f"{name}, K {K}")
        T.close()


def test_products_with_dead_rows_against_the_restatement_and_the_column_group(rb, torch):
    grid, n, src, ns, rec, op, _ = E.solver_case()
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, _width=8)
    dead = ~op.live.reshape(-1)
    assert dead.any() and np.array_equal(T.table()["live"].reshape(-1) == 0, dead)
    b0 = T.info()["bytes_device"]
    X, Y, y8, G8 = products_against_singles(T, 8, 51, "solver case, the default group")
    b8 = T.info()["bytes_device"]
    assert b8 > b0                                                         # the work tables grew, and the handle counts them
    for c in (0, 7):
        assert R.same_bits(y8[c], op.apply(X[c])) and R.same_bits(G8[c].reshape(-1), op.transpose(np.where(dead, 0.0, Y[c])))
    assert not y8[:, dead].any()
    # groups of 3: 3 + 3 + 2 columns, against the single calls again
    T.set_column_group(3)
    products_against_singles(T, 8, 51, "solver case, groups of 3")
    assert T.info()["bytes_device"] == b8
    T.set_column_group(0)
    # the device forms
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")     # noqa: E731
    dy, dG = T.matmat_device(up(X)), T.rmatmat_device(up(Y))
    assert dy.is_cuda and dG.is_cuda
    for c in range(8):
        assert R.same_bits(dy[c].cpu().numpy(), T.apply(X[c])) and same(dG[c].cpu().numpy(), T.transpose(Y[c]))
    from raytracing_amd import _lib
    with pytest.raises(_lib.RtmiError, match="cg must be in") as e:
        T.set_column_group(-1)
    assert e.value.code == -1
    rc = _lib.lib().rtmi_eikonal_tomo_apply_multi_dev(T._open(), 8, X.ctypes.data, dy.data_ptr(), None)
    assert rc == -1 and b"d_dn is not memory" in _lib.lib().rtmi_last_error()
    T.close()


def test_a_sweep_that_is_not_clean_names_the_sweep_the_source_and_the_column(rb):
    from raytracing_amd import _lib
    cgrid, cn, csrc, cns, _ = L.corridor_case()
    fill = rb.eikonal_fill(cn, csrc, cgrid, n_src=cns)
    crec = np.array([E.at(cgrid, 3.5, 3.25), E.at(cgrid, 27.0, 23.5), E.at(cgrid, 15.5, 13.0)])
    T = rb.EikonalTomography(cn, csrc, cgrid, crec, n_src=cns, fill_result=fill, max_rounds=1)
    rows, lib = len(csrc) * len(crec), _lib.lib()
    X = np.ones((3, cn.size))
    X[0] = 0.0                                                             # a zero column is clean in its first round
    y = np.full((3, rows), np.nan)
    rc = lib.rtmi_eikonal_tomo_apply_multi(T._open(), 3, _lib.dptr(X), _lib.dptr(y), None)
    msg = lib.rtmi_last_error().decode()
    assert rc == -4 and re.search(r"the tangent sweep of source \d, column 1 did not converge within max_rounds", msg), msg
    assert np.isnan(y).all()
    Y = np.ones((3, rows)) * (T.table()["live"].reshape(-1) != 0)
    Y[:2] = 0.0
    G = np.full((3, cn.size), np.nan)
    rc = lib.rtmi_eikonal_tomo_transpose_multi(T._open(), 3, _lib.dptr(Y), _lib.dptr(G), None)
    msg = lib.rtmi_last_error().decode()
    assert rc == -4 and "the adjoint sweep of source " in msg and ", column 2 did not converge within max_rounds" in msg, msg
    assert np.isnan(G).all()
    T.close()


# ------------------------------------------------------------------------------------------------------------ the solver
ITER, DAMP, BTOL = 6, 1e-3, 0.15
REGS = [None, ((0.02, 0.03), None), ((0.02, 0.03), (0.004, 0.005))]


@functools.lru_cache(maxsize=None)
def solver_columns():
    """right-hand sides that stop differently in the single solver: a consistent one (btol), a random one (iter_lim), zeros (itn
    0), one at 1.5e308 (its norm is out of range: RTMI_LSQR_RANGE), the residual of the picks, another random one"""
    grid, n, src, ns, rec, op, picks = E.solver_case()
    live = op.live.reshape(-1)
    rng = np.random.default_rng(5)
    xt = np.zeros(op.nn)
    xt[60], xt[75] = 0.05, -0.03
    cons = np.where(live, op.apply(xt), 0.0)
    return np.stack([cons, rng.standard_normal(live.size) * live, np.zeros(live.size), 1.5e308 * live, op.residual(picks),
                     rng.standard_normal(live.size) * live])


def solver_options(op, picks, K, which):
    rng = np.random.default_rng(23)
    live = op.live.reshape(-1)
    if which == "plain":
        return {}
    wr = rng.uniform(0.5, 2.0, live.size) * live
    wr[np.isnan(picks)] = 0.0
    dc = rng.uniform(0.5, 2.0, op.nn)
    dc[40] = 0.0
    dc[~np.isfinite(op.n.reshape(-1))] = 0.0
    if which == "shared":
        return dict(row_weight=wr, col_scale=dc, x0=0.01 * rng.standard_normal(op.nn))
    # per-column weights that drop half the live rows
    w = np.stack([wr * (rng.random(live.size) < 0.5) for _ in range(K)])
    assert all(0 < np.count_nonzero(w[c]) < live.sum() for c in range(K))
    return dict(row_weight=w)


def same_solve(got, one, what):
    assert (got["istop"], got["itn"]) == (one["istop"], one["itn"]), (what, got["istop"], got["itn"], one["istop"], one["itn"])
    assert same(got["x"], one["x"]) and R.same_bits(got["history"], one["history"]), what
    for k in ("r1norm", "r2norm", "anorm", "arnorm"):
        assert same(got[k], one[k]), (what, k, got[k], one[k])


@pytest.mark.parametrize("reg", REGS, ids=["noreg", "d1", "d1d2"])
@pytest.mark.parametrize("options", ["plain", "shared", "percolumn"])
def test_solver_columns_that_stop_differently_match_the_single_solver(rb, options, reg):
    from raytracing_amd import _lib
    grid, n, src, ns, rec, op, picks = E.solver_case()
    rhs = solver_columns()
    K = len(rhs)
    d1, d2 = reg if reg else (None, None)
    kw = dict(damp=DAMP, btol=BTOL, smooth=d1, smooth2=d2, history=True)
    opts = solver_options(op, picks, K, options)
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, _width=4)         # six columns: a chunk of 4 and a partial one
    got = T.lsqr_multi(rhs, ITER, **kw, **opts)
    ones = []
    for c in range(K):
        o = dict(opts)
        if options == "percolumn":
            o["row_weight"] = opts["row_weight"][c]
        ones.append(T.lsqr(rhs[c], ITER, **kw, **o))
        same_solve(got[c], ones[c], f"{options}, column {c}")
    stops = [(o["istop"], o["itn"]) for o in ones]
    assert stops[3] == (_lib.LSQR_RANGE, 0) and (options == "shared" or stops[2] == (0, 0)), stops     # with x0 the zero column is - A x0
    if options == "plain":
        # the call holds a column that btol stops, columns that run to iter_lim, a zero one and one out of range
        assert stops[0][0] == 1 and stops[0][1] < ITER and stops[1] == (7, ITER), stops
        mv, rmv, nr = op.stacked(d1, d2)
        for c in (0, 1, 4):
            want = LW.lsqr_weighted(mv, rmv, np.r_[rhs[c], np.zeros(nr)], ITER, damp=DAMP, btol=BTOL)
            assert (got[c]["istop"], got[c]["itn"]) == (want["istop"], want["itn"]) and R.same_bits(got[c]["x"].reshape(-1), want["x"])
            assert R.same_bits(got[c]["history"], want["history"][:want["itn"]])
    T.close()


def test_solver_history_from_a_nan_filled_buffer_and_refusals(rb):
    from raytracing_amd import _lib
    grid, n, src, ns, rec, op, picks = E.solver_case()
    rhs = np.ascontiguousarray(solver_columns())
    K, rows, lib = len(rhs), op.S * op.R, _lib.lib()
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    lp = _lib.LsqrParams()
    lp.iter_lim, lp.damp, lp.atol, lp.btol = ITER, DAMP, 0.0, BTOL
    x, hist, st = np.empty((K, op.nn)), np.full((K, ITER, 4), np.nan), (_lib.LsqrStats * K)()
    assert lib.rtmi_eikonal_tomo_lsqr_multi(T._open(), C.byref(lp), None, None, K, 0, _lib.dptr(rhs), _lib.dptr(x), _lib.dptr(hist), st) == 0
    for c in range(K):
        one = T.lsqr(rhs[c], ITER, damp=DAMP, btol=BTOL, history=True)
        assert st[c].itn == one["itn"] and R.same_bits(hist[c, :one["itn"]], one["history"]) and same(x[c], one["x"].reshape(-1))
        assert not hist[c, one["itn"]:].any() and not np.isnan(hist[c]).any()
    assert len({st[c].itn for c in range(K)}) >= 3
    # a non-zero weight on a dead row in column 2 is refused by number
    live = op.live.reshape(-1)
    w = np.ones((K, rows)) * live
    dead = int(np.flatnonzero(~live)[0])
    w[2, dead] = 0.5
    with pytest.raises(_lib.RtmiError, match=f"row_weight is not zero on dead row {dead} of column 2") as e:
        T.lsqr_multi(rhs, 3, row_weight=w)
    assert e.value.code == -1
    with pytest.raises(_lib.RtmiError, match=f"row_weight is not zero on dead row {dead}") as e:
        T.lsqr_multi(rhs, 3, row_weight=np.ones(rows))
    bad = rhs.copy()
    bad[4, 0] = np.inf
    with pytest.raises(_lib.RtmiError, match="rhs has a value that is not finite in column 4"):
        T.lsqr_multi(bad, 3)
    T.close()


# ---------------------------------------------------------------------------------------------------------------- Python
def test_recover_bootstrap_and_seventy_columns(rb):
    grid, n, src, ns, rec, op, picks = E.solver_case()
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    kw = dict(iter_lim=4, damp=DAMP, smooth=(0.02, 0.03))
    models = np.concatenate([rb.checkerboard(T.ny, T.nx, 3, 0.02)[None], rb.spikes(T.ny, T.nx, [(5, 4), (2, 9)], 0.05)])
    models[:, ~np.isfinite(n)] = 0.0
    xs, outs = T.recover(models, **kw)
    assert xs.shape == models.shape and len(outs) == 3
    for c in range(3):
        one = T.lsqr(T.apply(models[c]), **kw)
        assert R.same_bits(xs[c], one["x"]) and (outs[c]["istop"], outs[c]["itn"]) == (one["istop"], one["itn"]) and np.abs(xs[c]).max() > 0
    # bootstrap: the mean and the ddof-1 deviation of the single solves under the same weights
    rhs = T.residual(picks)
    mean, std, reps = T.bootstrap(rhs, 5, 77, results=True, **kw)
    live = T.table()["live"].reshape(-1) != 0
    w = rb.bootstrap_weights(rhs.size, 5, 77) * live[None, :]
    singles = np.stack([T.lsqr(rhs, row_weight=w[k], **kw)["x"] for k in range(5)])
    assert all(R.same_bits(reps[k]["x"], singles[k]) for k in range(5))
    assert R.same_bits(mean, singles.mean(axis=0)) and R.same_bits(std, singles.std(axis=0, ddof=1)) and std.max() > 0
    # K = 70: the products in groups of 64, the solver in groups of 64 and of 3
    rng = np.random.default_rng(70)
    X = rng.standard_normal((70, T.ny, T.nx))
    Y = T.matmat(X)
    G = T.rmatmat(Y)
    singles = [T.lsqr(Y[c], 2, damp=DAMP) for c in range(70)]
    for c in range(70):
        assert R.same_bits(Y[c], T.apply(X[c])) and R.same_bits(G[c], T.transpose(Y[c]))
    for group in (None, 3):
        outs = T.lsqr_multi(Y, 2, damp=DAMP, group=group)
        assert len(outs) == 70 and all(R.same_bits(outs[c]["x"], singles[c]["x"]) and outs[c]["itn"] == singles[c]["itn"] for c in range(70))
    T.close()
