"""GPU: the linearised eikonal fill (rtmi_eikonal_tangent, rtmi_eikonal_adjoint, their _dev forms and eikonal_operator; DESIGN.md
section 35).  The yardstick is tests/eikonal_lin_ref.py, the serial sweeps in Python floats over the restatement's own fill, and
every comparison is bit for bit on dT, lam, g, g_src, rounds and converged.  Shapes: the grids 1 x 1, 1 x 70, 70 x 1, 5 x 70,
64 x 64 and 65 x 63 (diagonals of 1, 5, 63 and 64 nodes in a block of one wave) and 100 x 90, which is over the LDS path's 5 041
nodes, each on the LDS path where it fits and on the global path; 300 x 260, whose diagonals of 260 nodes make the 256 lanes
stride; the corridor, which needs more than three rounds (asserted in tests/test_eikonal_lin_ref.py), with and without a cap;
obstacles of every kind with a sealed pocket; a table seeded everywhere but a disc, with dT_seed; the device-pointer forms;
repeated runs; the split of a call over its sources; a NaN in r; and one damped LSQR step of tomography through
eikonal_operator."""
import ctypes as C
import functools

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_ref as R

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
    """the device's tangent and adjoint of one case against the restatement's"""
    dn, dns, sd, r = inputs(n, len(src), seed)
    sd = sd if use_seed else None
    want_t, want_a = L.tangent(nets, dn, dns, sd, max_rounds=max_rounds), L.adjoint(nets, r, max_rounds=max_rounds)
    kw = dict(n_src=ns, stats=True, max_rounds=max_rounds, _global_path=global_path)
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
    return L.filled((grid, n, src, ns, None))


@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_shapes_where_lane_wave_and_block_loops_can_go_wrong(rb, nx, ny, global_path):
    grid, n, src, ns, fill, nets = shape_case(nx, ny)
    assert fill["filled"].all() and fill["converged"].all()
    both(rb, grid, n, src, ns, fill, nets, nx + ny, f"{nx} x {ny}", global_path,
         "global" if global_path or nx * ny * 26 > 128 * 1024 else "lds")


def test_grid_over_the_lds_capacity_with_striding_lanes(rb):
    """300 x 260: 78 000 nodes against the LDS path's 5 041, and diagonals of 260 nodes for 256 lanes"""
    grid, n, src, ns, fill, nets = shape_case(300, 260, 1)
    both(rb, grid, n, src, ns, fill, nets, 7, "300 x 260", False, "global")


# ------------------------------------------------------------------------------------------------- the several-round medium
@functools.lru_cache(maxsize=None)
def named(name):
    return L.filled(getattr(L, name)())


@pytest.mark.parametrize("global_path", [False, True])
def test_corridor_with_three_sources_and_under_a_cap_of_one_round(rb, global_path):
    grid, n, src, ns, fill, nets = named("corridor_case")
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 3, "corridor", global_path, "global" if global_path else "lds")
    assert (want_t["rounds"] > 3).all() and (want_a["rounds"] > 3).all() and want_t["converged"].all() and want_a["converged"].all()
    cap_t, cap_a = both(rb, grid, n, src, ns, fill, nets, 3, "corridor, max_rounds 1", global_path, max_rounds=1)
    assert (cap_t["rounds"] == 1).all() and not cap_t["converged"].any() and not cap_a["converged"].any()
    assert not R.same_bits(cap_t["dT"], want_t["dT"]) and not R.same_bits(cap_a["lam"], want_a["lam"])


# ------------------------------------------------------------------------------------------ obstacles, a pocket, seeds
@pytest.mark.parametrize("global_path", [False, True])
def test_obstacles_of_every_kind_with_a_sealed_pocket(rb, global_path):
    grid, n, src, ns, fill, nets = named("walls_case")
    cls = np.array([net.cls for net in nets]).reshape(fill["T"].shape)
    assert all(set(c.reshape(-1)) == {L.DEAD, L.SEED, L.FREE, L.BALL} for c in cls) and (cls[:, 9:14, 31:35] == L.DEAD).all()
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 5, "walls", global_path, use_seed=True)
    assert (want_t["dT"][cls == L.DEAD] == 0).all() and (want_a["lam"][cls == L.DEAD] == 0).all()


@pytest.mark.parametrize("global_path", [False, True])
def test_table_seeded_everywhere_but_a_disc_with_dT_seed(rb, global_path):
    grid, n, src, ns, fill, nets = named("disc_case")
    assert all(net.cls.count(L.SEED) > 3000 and len(net.free) > 200 for net in nets)
    want_t, want_a = both(rb, grid, n, src, ns, fill, nets, 6, "disc", global_path, use_seed=True)
    seeds = np.array([net.cls for net in nets]).reshape(fill["T"].shape) == L.SEED
    _, _, sd, _ = inputs(n, len(src), 6)
    assert R.same_bits(want_t["dT"][seeds], sd[seeds]) and np.abs(want_a["lam"][seeds]).max() > 1.0


def test_device_forms_repeated_runs_and_split_over_sources(rb, torch):
    grid, n, src, ns, fill, nets = named("walls_case")
    dn, dns, sd, r = inputs(n, len(src), 8)
    want_t, want_a = L.tangent(nets, dn, dns, sd), L.adjoint(nets, r)
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)     # noqa: E731
    d_fill = {"T": up(fill["T"]), "filled": up(fill["filled"])}
    host = lambda res: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}     # noqa: E731
    for rep in range(2):
        got = rb.eikonal_tangent_device(up(n), up(src), grid, d_fill, up(dn), n_src=up(ns), dn_src=up(dns), dT_seed=up(sd))
        assert got["dT"].is_cuda
        same_tangent(host(got), want_t, f"device form, run {rep}")
        got = rb.eikonal_adjoint_device(up(n), up(src), grid, d_fill, up(r), n_src=up(ns))
        assert got["lam"].is_cuda and got["g"].is_cuda and got["g_src"].is_cuda
        same_adjoint(host(got), want_a, f"device form, run {rep}")
    assert R.same_bits(d_fill["T"].cpu().numpy(), fill["T"])                 # the tables are read, not written
    with pytest.raises(ValueError, match="on a GPU"):
        rb.eikonal_adjoint_device(torch.as_tensor(n), up(src), grid, d_fill, up(r), n_src=up(ns))
    # S = 5 in one call against five calls of one source
    grid, n, src, ns, fill, nets = shape_case(41, 23, 5)
    dn, dns, sd, r = inputs(n, 5, 9)
    whole_t = rb.eikonal_tangent(n, src, grid, fill, dn, n_src=ns, dn_src=dns)
    whole_a = rb.eikonal_adjoint(n, src, grid, fill, r, n_src=ns)
    for s in range(5):
        one = {k: v[s:s + 1] for k, v in fill.items() if k in ("T", "filled")}
        got = rb.eikonal_tangent(n, src[s:s + 1], grid, one, dn, n_src=ns[s:s + 1], dn_src=dns[s:s + 1])
        same_tangent(got, {k: whole_t[k][s:s + 1] for k in ("dT", "rounds", "converged")}, f"source {s} alone")
        got = rb.eikonal_adjoint(n, src[s:s + 1], grid, one, r[s:s + 1], n_src=ns[s:s + 1])
        same_adjoint(got, {k: whole_a[k][s:s + 1] for k in ("lam", "g", "g_src", "rounds", "converged")}, f"source {s} alone")
    same_tangent(whole_t, L.tangent(nets, dn, dns), "five sources")
    same_adjoint(whole_a, L.adjoint(nets, r), "five sources")


@pytest.mark.parametrize("global_path", [False, True])
def test_nan_in_r_ends_within_the_cap_and_clean(rb, global_path):
    """a NaN spreads down its parents and, compared by its bits, stops changing: the sweeps end clean.  A NaN's payload is the
    processor's, so NaN is compared by place and every other value by its bits"""
    grid, n, src, ns, fill, nets = named("corridor_case")
    _, _, _, r = inputs(n, len(src), 4)
    # at the corridor's latest node: the NaN reaches all its ancestors, round by round
    far = [max((x for x in net.free if n.reshape(-1)[x] == 1.0), key=lambda x: net.T[x]) for net in nets]
    for s, x in enumerate(far):
        r[s].reshape(-1)[x] = np.nan
    want = L.adjoint(nets, r)
    got = rb.eikonal_adjoint(n, src, grid, fill, r, n_src=ns, _global_path=global_path)
    assert got["converged"].all() and (got["rounds"] < 64).all()
    assert np.array_equal(got["rounds"], want["rounds"]) and np.array_equal(got["converged"], want["converged"])
    assert np.isnan(want["lam"]).sum(axis=(1, 2)).min() > 100 and (want["rounds"] > 3).all()
    for k in ("lam", "g", "g_src"):
        assert L.same_but_nan(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------- the operator, end to end
# The rms traveltime residual after one damped LSQR step as a fraction of the residual before it: the restatement's own step, with
# its Jacobian as a dense matrix, gives 4.712e-2 (tests/test_eikonal_lin_ref.py); the bound is that figure
# rounded up to one digit
TOMOGRAPHY_FRACTION_BOUND = 5e-2


def test_one_lsqr_step_through_the_operator_cuts_the_residual(rb):
    grid, n0, n_true, src, rec, idx, w = L.tomography_case()
    ridx, rw = rb.eikonal_source_weights(src, grid)
    assert np.array_equal(ridx, idx) and np.array_equal(rw, w)

    def solve(n, ns):
        f = rb.eikonal_fill(n, src, grid, n_src=ns)
        assert f["converged"].all() and f["filled"].all()
        return f["T"], (n, ns, f)

    ops = []

    def jacobian(state):
        ops.append(rb.eikonal_operator(state[0], src, grid, state[2], rec, n_src=state[1]))
        return ops[-1]

    before, after, step = L.tomography_step(solve, jacobian)
    print(f"tomography step on the device: rms residual {before:.4e} -> {after:.4e} s, fraction {after / before:.4e}")
    # the operator's two halves are each other's transposes, and the step is the anomaly's size, not noise
    A = ops[0]
    assert A.shape == (len(src) * len(rec), n0.size)
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    lhs, rhs = float(np.dot(A.matvec(x), y)), float(np.dot(x, A.rmatvec(y)))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert 0.3 < np.abs(step).max() / np.abs(n_true - n0).max() < 3.0
    assert after <= TOMOGRAPHY_FRACTION_BOUND * before
