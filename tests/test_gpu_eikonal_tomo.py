"""GPU: first-arrival eikonal tomography on the device (rtmi_eikonal_tomo_*) against the restatement
(tests/eikonal_tomo_ref.py), bit for bit: both products, the residual and the live rows on grids with cells, of one column and of
one row, on the LDS and the global path of the sweeps; dead rows behind walls, with a NaN planted where the transpose must not
read; the device-pointer forms, two runs, and one handle against one handle per source; re-linearisation against a new handle; the
solver against the restated loop with every option and regulariser; every refusal; and tomography with receivers off the nodes,
one step and Gauss-Newton."""
import ctypes as C

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_ref as R
import eikonal_tomo_ref as E
import lsqr_weighted_ref as LW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


def vectors(op, seed):
    rng = np.random.default_rng(seed)
    dn = rng.standard_normal(op.nn)
    y = rng.standard_normal(op.S * op.R)
    picks = rng.standard_normal(op.S * op.R) + 2.0
    picks[1] = np.nan
    planted = y.copy()
    planted[~op.live.reshape(-1)] = np.nan                    # a read of a dead row's entry would show
    return dn, y, planted, picks


def check_against(T, op, seed):
    """a handle's products, residual and live rows against the restated operator, bit for bit"""
    dn, y, planted, picks = vectors(op, seed)
    info = T.info()
    assert info["rows"] == op.S * op.R and info["live_rows"] == int(op.live.sum()) and list(info["live_per_source"]) == list(op.live_per)
    assert np.array_equal(T.table()["live"] != 0, op.live)
    assert R.same_bits(T.apply(dn), op.apply(dn))
    G = T.transpose(planted)
    assert G.shape == (op.ny, op.nx) and R.same_bits(G.reshape(-1), op.transpose(y))
    assert R.same_bits(T.residual(picks), op.residual(picks))


# ------------------------------------------------------------------------------------------------ 1. grids and paths
@pytest.mark.parametrize("global_path", [False, True])
@pytest.mark.parametrize("name", list(E.SHAPE_GRIDS))
def test_products_residual_and_live_rows_match_the_restatement(rb, name, global_path):
    grid, n, src, ns, rec, op = E.shape_case(name)
    assert len(src) == (5 if name == "65x63" else 3) and list(op.inside[:3]) == [True, True, False] and 7 <= len(rec) <= 9
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, _global_path=global_path)
    info = T.info()
    assert info["self_filled"] and info["path"] == ("global" if global_path else "lds")
    assert L.same_but_nan(T.table()["T"], op.fill["T"])
    check_against(T, op, 11)
    T.close()


# ------------------------------------------------------------------------------------------------ 2. walls
def test_dead_rows_behind_walls(rb):
    grid, n, src, ns, fill, rec, op = E.walls()
    assert (~op.live).any(axis=1).all() and op.live.any(axis=1).all()
    for global_path in (False, True):
        T = rb.EikonalTomography(n, src, grid, rec, n_src=ns, fill_result=fill, _global_path=global_path)
        assert not T.info()["self_filled"]
        check_against(T, op, 13)
        dn = vectors(op, 13)[0]
        y = T.apply(dn)
        assert not y[~op.live.reshape(-1)].any() and not np.signbit(y[~op.live.reshape(-1)]).any()
        T.close()


# ------------------------------------------------------------------------------------------------ 3. forms and determinism
def test_device_forms_two_runs_and_one_handle_per_source(rb):
    import torch
    grid, n, src, ns, rec, op = E.shape_case("13x11")
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    dn, y, _, picks = vectors(op, 17)
    dev = torch.device("cuda")
    up = lambda a: torch.as_tensor(a, device=dev)         # noqa: E731
    host = (T.apply(dn), T.transpose(y), T.residual(picks))
    device = (T.apply_device(up(dn)), T.transpose_device(up(y)), T.residual_device(up(picks)))
    again = (T.apply(dn), T.transpose(y), T.residual(picks))
    for a, b, c in zip(host, device, again):
        assert R.same_bits(a.reshape(-1), b.cpu().numpy().reshape(-1)) and R.same_bits(a, c)
    parts = []
    for s in range(len(src)):
        P = rb.EikonalTomography(n, src[s:s + 1], grid, rec, n_src=ns[s:s + 1])
        ys = y.reshape(len(src), -1)[s]
        assert R.same_bits(P.apply(dn), host[0].reshape(len(src), -1)[s])
        assert R.same_bits(P.residual(picks.reshape(len(src), -1)[s]), host[2].reshape(len(src), -1)[s])
        one = E.Operator(grid, n, src[s:s + 1], ns[s:s + 1], {"T": op.fill["T"][s:s + 1], "filled": op.fill["filled"][s:s + 1]}, rec)
        Gs = P.transpose(ys)
        assert R.same_bits(Gs.reshape(-1), one.transpose(ys))
        parts.append(Gs.reshape(-1))
        P.close()
    # the whole is the ordered sum of the sources' g, then the sources' own terms: the restatement from its parts
    Gref, gs, gsrc = op.transpose(y, parts=True)
    assert R.same_bits(host[1].reshape(-1), op.reduce(gs, gsrc)) and R.same_bits(host[1].reshape(-1), Gref)
    assert R.same_bits(parts[2], gs[2])                       # a source outside the grid adds nothing of its own
    T.close()
    # with every source outside the grid a part's G is its g, and the whole is their sum in increasing s
    gx0, gdx, nx, gy0, gdy, ny = grid
    out = np.array([[gx0 - 0.5 * gdx, gy0 + 3.3 * gdy], [gx0 + 6.2 * gdx, gy0 - 0.7 * gdy], [gx0 + (nx - 0.4) * gdx, gy0 + 8.1 * gdy]])
    W = rb.EikonalTomography(n, out, grid, rec, n_src=ns)
    Gw = W.transpose(y).reshape(-1)
    acc = np.zeros(op.nn)
    for s in range(3):
        P = rb.EikonalTomography(n, out[s:s + 1], grid, rec, n_src=ns[s:s + 1])
        acc = acc + P.transpose(y.reshape(3, -1)[s]).reshape(-1)
        P.close()
    assert W.info()["live_rows"] == 3 * len(rec) and R.same_bits(Gw, acc) and np.abs(Gw).max() > 0
    W.close()


# ------------------------------------------------------------------------------------------------ 4. re-linearisation
def test_relinearise_is_a_new_handle(rb):
    from raytracing_amd import _lib
    grid, n, src, ns, rec, op, _ = E.solver_case()
    X, Y = R.nodes(grid)
    n2 = n * (1.0 + 0.1 * np.exp(-((X - 2.0) ** 2 + Y ** 2)))
    n2[6, 7], n2[7, 3] = 1.3, np.nan                                   # the obstacle moves: other rows die
    dn, y, _, _ = vectors(op, 19)
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    check_against(T, op, 19)
    for n_src2 in (ns * 1.01, None):
        T.relinearise(n2, n_src2)
        want = n_src2
        if want is None:                                               # inside: sample(n2, src); outside: the value it had
            want = np.array([E.sample(n2.reshape(-1), op.sidx[s], op.sw[s]) if op.inside[s] else (ns * 1.01)[s] for s in range(len(src))])
        F = rb.EikonalTomography(n2, src, grid, rec, n_src=want)
        a, b = T.table(), F.table()
        assert L.same_but_nan(a["T"], b["T"]) and np.array_equal(a["filled"], b["filled"]) and np.array_equal(a["live"], b["live"])
        assert list(T.info()["live_per_source"]) == list(F.info()["live_per_source"]) and not np.array_equal(a["live"] != 0, op.live)
        planted = y.copy()
        planted[a["live"].reshape(-1) == 0] = np.nan
        assert R.same_bits(T.apply(dn), F.apply(dn)) and R.same_bits(T.transpose(planted), F.transpose(planted))
        ref = E.Operator(grid, n2, src, want, R.solve(grid, n2, src, want), rec)
        assert R.same_bits(T.apply(dn), ref.apply(dn)) and np.array_equal(a["live"] != 0, ref.live)
        F.close()
    # the device form, back to the first medium: the first handle's bits again
    import torch
    T.relinearise_device(torch.as_tensor(n, device="cuda"), torch.as_tensor(ns, device="cuda"))
    check_against(T, op, 19)
    T.close()
    G = rb.EikonalTomography(n, src, grid, rec, n_src=ns, fill_result=op.fill)
    with pytest.raises(_lib.RtmiError, match="re-linearised") as e:
        G.relinearise(n2)
    assert e.value.code == -4
    with pytest.raises(_lib.RtmiError, match="re-linearised") as e:
        G.relinearise_device(torch.as_tensor(n2, device="cuda"))
    assert e.value.code == -4
    check_against(G, op, 19)                                           # and the handle is as it was
    G.close()


# ------------------------------------------------------------------------------------------------ 5. the solver
ITER, DAMP = 5, 1e-3


def solver_options(op, picks):
    """row_weight with zeros at the dead rows and the absent pick, col_scale with a zero, x0"""
    rng = np.random.default_rng(23)
    wr = rng.uniform(0.5, 2.0, op.S * op.R)
    wr[~op.live.reshape(-1)] = 0.0
    wr[np.isnan(picks)] = 0.0
    dc = rng.uniform(0.5, 2.0, op.nn)
    dc[40] = 0.0
    dc[~np.isfinite(op.n.reshape(-1))] = 0.0
    x0 = 0.01 * rng.standard_normal(op.nn)
    return wr, dc, x0


@pytest.mark.parametrize("reg", [None, ((0.02, 0.03), None), ((0.02, 0.03), (0.004, 0.005))], ids=["noreg", "d1", "d1d2"])
@pytest.mark.parametrize("options", [False, True], ids=["plain", "options"])
def test_solver_matches_the_restated_loop(rb, options, reg):
    grid, n, src, ns, rec, op, picks = E.solver_case()
    rhs = op.residual(picks)
    assert not rhs[~op.live.reshape(-1)].any() and rhs[op.R + 1] == 0.0
    d1, d2 = reg if reg else (None, None)
    wr, dc, x0 = solver_options(op, picks) if options else (None, None, None)
    mv, rmv, nr = op.stacked(d1, d2)
    want = LW.lsqr_weighted(mv, rmv, np.r_[rhs, np.zeros(nr)], ITER, wr=wr, dc=dc, x0=x0, ndata=op.S * op.R, damp=DAMP)
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    assert R.same_bits(T.residual(picks), rhs)
    out = T.lsqr(rhs, ITER, damp=DAMP, row_weight=wr, col_scale=dc, x0=x0, smooth=d1, smooth2=d2, history=True, stats=True)
    assert (out["istop"], out["itn"]) == (want["istop"], want["itn"]) and out["itn"] == ITER
    assert R.same_bits(out["history"], want["history"]) and R.same_bits(out["x"].reshape(-1), want["x"])
    assert out["stats"]["operator_ms"] > 0 and out["stats"]["vector_ms"] > 0 and np.abs(out["x"]).max() > 0
    if options:
        assert out["x"].reshape(-1)[40] == x0[40]
        frozen = T.lsqr(rhs, ITER, damp=DAMP, row_weight=wr, col_scale=np.zeros(op.nn), x0=x0, smooth=d1, smooth2=d2)
        assert R.same_bits(frozen["x"].reshape(-1), x0)
    T.close()


def test_solver_refusals_and_scipy(rb):
    from scipy.sparse.linalg import lsqr
    from raytracing_amd import _lib
    grid, n, src, ns, rec, op, picks = E.solver_case()
    T = rb.EikonalTomography(n, src, grid, rec, n_src=ns)
    rhs = T.residual(picks)
    # with lo and reg null the solver is scipy's on the same operator (the tolerance of tests/test_gpu_tomo.py)
    sc = lsqr(T.as_linear_operator(), rhs, damp=DAMP, atol=0.0, btol=0.0, conlim=0.0, iter_lim=10)
    out = T.lsqr(rhs, 10, damp=DAMP)
    fit, fit_ref = float(np.linalg.norm(T.apply(out["x"]) - rhs)), float(np.linalg.norm(T.apply(sc[0]) - rhs))
    print(f"|A x - rhs| {fit:.9e} here, {fit_ref:.9e} scipy, |rhs| {np.linalg.norm(rhs):.3e}")
    assert out["itn"] == sc[2] == 10 and abs(fit - fit_ref) <= 1e-6 * fit_ref and fit < 0.5 * np.linalg.norm(rhs)
    wr = np.ones(op.S * op.R)
    for kw, word in ((dict(row_weight=wr), "row_weight is not zero on dead row 3"), (dict(damp=-1.0), "damp"),
                     (dict(smooth=(-1.0, 0.0)), "reg.d1"), (dict(col_scale=np.full(op.nn, np.nan)), "col_scale")):
        with pytest.raises(_lib.RtmiError, match=word) as e:
            T.lsqr(rhs, 3, **kw)
        assert e.value.code == -1
    bad = rhs.copy()
    bad[0] = np.inf
    with pytest.raises(_lib.RtmiError, match="rhs has a value that is not finite"):
        T.lsqr(bad, 3)
    T.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_with_their_messages_and_nothing_written(rb):
    import torch
    from raytracing_amd import _lib
    grid, n, src, ns, rec, op = E.shape_case("13x11")
    gx0, gdx, nx, gy0, gdy, ny = grid
    with pytest.raises(_lib.RtmiError, match="receiver 1 is not finite or lies outside the grid") as e:
        rb.EikonalTomography(n, src, grid, [rec[0], [gx0 + nx * gdx, gy0]], n_src=ns)
    assert e.value.code == -1
    with pytest.raises(_lib.RtmiError, match="R must be >= 1"):
        rb.EikonalTomography(n, src, grid, np.zeros((0, 2)), n_src=ns)
    lib = _lib.lib()
    ep = rb.eikonal_params(grid)
    h = C.c_void_p(0x1234)
    T1 = np.ascontiguousarray(op.fill["T"])
    assert lib.rtmi_eikonal_tomo_create(C.byref(ep), _lib.dptr(np.ascontiguousarray(n)), len(src), _lib.dptr(np.ascontiguousarray(src)),
                                        _lib.dptr(np.ascontiguousarray(ns)), _lib.dptr(T1), None, len(rec),
                                        _lib.dptr(np.ascontiguousarray(rec)), C.byref(h)) == -1
    assert "exactly one of T and filled is null" in lib.rtmi_last_error().decode() and h.value is None
    # a sweep that cannot converge: the corridor within one round
    cgrid, cn, csrc, cns, _ = L.corridor_case()
    fill = rb.eikonal_fill(cn, csrc, cgrid, n_src=cns)
    assert fill["converged"].all()
    crec = np.array([E.at(cgrid, 3.5, 3.25), E.at(cgrid, 27.0, 23.5), E.at(cgrid, 15.5, 13.0)])
    ok = rb.EikonalTomography(cn, csrc, cgrid, crec, n_src=cns, fill_result=fill)
    assert ok.info()["live_rows"] > 0 and np.abs(ok.apply(np.ones(cn.size))).max() > 0
    ok.close()
    T = rb.EikonalTomography(cn, csrc, cgrid, crec, n_src=cns, fill_result=fill, max_rounds=1)
    dev = torch.device("cuda")
    y = torch.full((len(csrc) * len(crec),), 7.0, dtype=torch.float64, device=dev)
    G = torch.full((cn.shape[0], cn.shape[1]), 7.0, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.RtmiError, match="the tangent sweep of source . did not converge within max_rounds") as e:
        T.apply_device(torch.ones(cn.size, dtype=torch.float64, device=dev), out=y)
    assert e.value.code == -4 and bool((y == 7.0).all())
    with pytest.raises(_lib.RtmiError, match="the adjoint sweep of source . did not converge within max_rounds") as e:
        T.transpose_device(torch.ones(len(csrc) * len(crec), dtype=torch.float64, device=dev), out=G)
    assert e.value.code == -4 and bool((G == 7.0).all())
    with pytest.raises(_lib.RtmiError, match="did not converge") as e:
        T.lsqr(np.ones(len(csrc) * len(crec)) * T.table()["live"].reshape(-1), 3)
    assert e.value.code == -4
    T.close()
    with pytest.raises(_lib.RtmiError, match="the fill of source . did not converge within max_rounds") as e:
        rb.EikonalTomography(cn, csrc, cgrid, crec, n_src=cns, max_rounds=1)
    assert e.value.code == -4


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_tomography_with_receivers_off_the_nodes_one_step_and_gauss_newton(rb):
    """Measured: one step takes the rms residual from 1.4348e-03 to 6.69e-05 (fraction 0.047, the restatement's figure); three
    Gauss-Newton iterations go on to the figures that DESIGN.md section 36 records"""
    grid, n0, n_true, src, _, idx, w = L.tomography_case()
    pts = E.tomography_receivers()
    ns = lambda n: (n.reshape(-1)[idx] * w).sum(axis=1)             # noqa: E731
    rms = lambda r: float(np.sqrt(np.mean(r * r)))                  # noqa: E731
    truth = rb.EikonalTomography(n_true, src, grid, pts, n_src=ns(n_true))
    data = -truth.residual(np.zeros(len(src) * len(pts)))           # the tables of the truth at the receivers
    truth.close()
    T = rb.EikonalTomography(n0, src, grid, pts, n_src=ns(n0))
    assert T.info()["live_rows"] == len(src) * len(pts)
    r0 = T.residual(data)
    out = T.lsqr(r0, L.TOMO_ITERS, damp=L.TOMO_DAMP)
    n1 = n0 + out["x"]
    ridx, rw, _ = E.cells(grid, pts)
    T1 = rb.eikonal_fill(n1, src, grid, n_src=ns(n1))["T"].reshape(len(src), -1)
    r1 = data - np.array([E.sample(T1[s], ridx[k], rw[k]) for s in range(len(src)) for k in range(len(pts))])
    print(f"off-node tomography on the device: rms residual {rms(r0):.6e} -> {rms(r1):.6e}, fraction {rms(r1) / rms(r0):.4f}")
    assert rms(r1) <= E.TOMO_BOUND * rms(r0)
    gn = T.gauss_newton(data, 3, iter_lim=L.TOMO_ITERS, damp=L.TOMO_DAMP)
    print("gauss_newton: rms residual " + " -> ".join(f"{v:.6e}" for v in gn["rms"]))
    assert len(gn["rms"]) == 4 and (np.diff(gn["rms"]) < 0).all() and gn["rms"][-1] < rms(r1)
    assert abs(gn["rms"][0] - rms(r0)) <= 1e-12 * rms(r0) and abs(gn["rms"][1] - rms(r1)) <= 1e-6 * rms(r1)
    T.close()
