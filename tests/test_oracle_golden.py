"""CPU: the oracle (oracle/rt_oracle.c) against golden vectors captured from the reference
(oracle/gen_golden.py).  This is what pins the oracle; the GPU parity tests then compare against it."""
import numpy as np
import pytest

from conftest import LIMITS, golden, sub_rows, traj_fixtures, traj_inputs
from oracle import rt_oracle as O


@pytest.mark.parametrize("scen", ["interface", "fisheye", "vert_heterogeneous"])
def test_field_build_matches_reference(scen, consts, oracle_fields):
    g = golden(f"field_{scen}")
    F = oracle_fields(scen)
    assert (F.qx, F.qy) == (int(g["qx"]), int(g["qy"]))
    x, y, Z, cdy, cdx = F.arrays()
    # genZ axes (numpy.linspace) bit for bit
    assert np.array_equal(x[:4], g["x_head"]) and np.array_equal(x[-4:], g["x_tail"])
    assert np.array_equal(y[:4], g["y_head"]) and np.array_equal(y[-4:], g["y_tail"])
    # FITPACK's interior knots are x[2:-2] (not-a-knot)
    assert np.array_equal(g["tx"][4:-4], x[2:-2]) and np.array_equal(g["ty"][4:-4], y[2:-2])
    qy, qx = Z.shape
    for name, arr in (("Z", Z), ("cdy", cdy), ("cdx", cdx)):
        for tag, blk in (("c00", arr[:8, :8]), ("c11", arr[-8:, -8:]),
                         ("mid", arr[qy // 2:qy // 2 + 8, qx // 2:qx // 2 + 8])):
            # the reference's BITS: numpy's array exp (SVML, np_exp in rt_oracle.c) for the interface samples, np.gradient's
            # stencil, FITPACK regrid's Givens QR (regrid_interp) for the coefficients
            assert np.array_equal(blk, g[f"{name}_{tag}"]), (name, tag)


@pytest.mark.parametrize("scen", ["interface", "fisheye", "vert_heterogeneous"])
def test_lu_solver_is_close_but_not_the_references_bits(scen, consts):
    """What rounds 1-2 solved the collocation system with (banded LU): the same spline to 4e-15, not the same bits --
    which is what moved interface x op3/4/5 by 2e-7 (test_trajectory_matches_reference now passes at 0 there)."""
    g = golden(f"field_{scen}")
    O.set_field_solver(1)
    try:
        F = O.Field(scen, LIMITS[scen], consts["DELTA"])
    finally:
        O.set_field_solver(0)
    _, _, Z, cdy, cdx = F.arrays()
    qy, qx = Z.shape
    differs = False
    for name, arr in (("cdy", cdy), ("cdx", cdx)):
        blk = arr[qy // 2:qy // 2 + 8, qx // 2:qx // 2 + 8]
        assert np.abs(blk - g[f"{name}_mid"]).max() <= 4e-15 * max(np.abs(arr).max(), 1e-300)
        differs |= not np.array_equal(blk, g[f"{name}_mid"])
    assert differs


def test_np_exp_restatement_equals_numpy_here():
    """np_exp (rt_oracle.c) against this host's np.exp -- only where numpy dispatches float64 exp to SVML (AVX512_SKX
    builds, as in the container the fixtures were made in); elsewhere np.exp is another function and there is nothing to
    compare (the fixtures above pin np_exp either way)."""
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    if not feat.get("AVX512_SKX"):
        pytest.skip("numpy does not use SVML's exp on this CPU")
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-707, 707, 2_000_000), rng.uniform(-2, 2, 500_000), np.arange(-700, 700, 1 / 16.0),
                        -np.linspace(-5, 7, 681) / 0.005])
    with np.errstate(over="ignore"):
        ref = np.exp(x)
    ok = np.abs(x) < 707.7                      # beyond: SVML's scalar fall-back, restated as libm exp (immaterial for n)
    assert np.array_equal(O.np_exp(x)[ok], ref[ok])


@pytest.mark.parametrize("scen", ["interface", "fisheye", "vert_heterogeneous"])
def test_n_gradient_matches_reference(scen, oracle_fields):
    g = golden(f"field_{scen}")
    F = oracle_fields(scen)
    n, gx, gy = F.n_gradient(g["px"], g["py"])
    # 1 024 random points per grid: the reference's bits (same coefficients, fpbisp/fpbspl operation by operation)
    assert np.array_equal(n, g["n"]) and np.array_equal(gx, g["gx"]) and np.array_equal(gy, g["gy"])


@pytest.mark.parametrize("m", range(1, 12))
def test_single_step_matches_reference(m, oracle_fields):
    g = golden("step_methods")
    F = oracle_fields("vert_heterogeneous")
    out = O.single_step(F, m, 3 if m >= 10 else 1, float(g["step"]), g[f"st{m}"], g[f"hist{m}"])
    ref = g[f"out{m}"]
    # numpy's scalar pow differs from x*x by <= 1 ulp; everything else is bit-exact
    assert np.max(np.abs(out - ref) / np.maximum(np.abs(ref), 1e-3)) < 2e-15
    if True:
        with O.variant("pow"):
            Fp = O.Field("vert_heterogeneous", LIMITS["vert_heterogeneous"], float(golden("constants")["DELTA"]))
            outp = O.single_step(Fp, m, 3 if m >= 10 else 1, float(g["step"]), g[f"st{m}"], g[f"hist{m}"])
        assert np.array_equal(outp, ref)          # the reference-faithful build: its bits


@pytest.fixture(scope="module")
def pow_fields(consts):
    """Fields of the reference-faithful build (SQ() = libm pow(x, 2.0), like numpy's scalar x**2)."""
    cache = {}

    def get(scen):
        key = "vert_heterogeneous" if scen == "anisotropy" else scen
        if key not in cache:
            with O.variant("pow"):
                cache[key] = O.Field(key, LIMITS[key], consts["DELTA"])
        return cache[key]
    return get


@pytest.mark.parametrize("build", ["default", "pow"])
@pytest.mark.parametrize("name,scen,m", traj_fixtures())
def test_trajectory_matches_reference(name, scen, m, build, oracle_fields, pow_fields):
    """Every trajectory fixture captured from the reference -- all 11 methods, all four scenarios, 31 fixtures -- with both
    builds of the oracle:
      * "pow" build (squares like numpy's scalar x**2): the reference's BITS -- every recorded row, d_ray, step counts -- on
        every fixture (numpy's SVML exp and arctan2, FITPACK's Givens QR, glibc's sin/cos are all restated);
      * "default" build (x*x, what the device reproduces): <= 1e-15 (measured: 0 on 27 fixtures, <= 2.2e-16 on four) -- the
        whole cost of that one deviation."""
    t = golden("traj_" + name)
    F = (pow_fields if build == "pow" else oracle_fields)(scen)
    x0, y0, th = traj_inputs(t, scen)
    r = O.trazar(F, m, float(t["gamma"]), float(t["step"]), int(t["max_size"]), t["box"], x0, y0, th, record_stride=1,
                 nthreads=4)
    assert r["s_ray"].shape == (int(t["max_size"]), 6, len(th))
    assert np.array_equal(r["d_ray"][2], t["d_ray"][2]), "last written row per ray"
    strided, last = sub_rows(r["s_ray"], r["d_ray"], int(t["stride"]))
    if build == "pow":
        assert np.array_equal(strided, t["strided"]) and np.array_equal(last, t["last"]) and np.array_equal(r["d_ray"], t["d_ray"])
    else:
        assert np.abs(strided - t["strided"]).max() < 1e-15 and np.abs(last - t["last"]).max() < 1e-15
        assert np.abs(r["d_ray"][:2] - t["d_ray"][:2]).max() < 1e-12
    # rows after termination stay zero (Q7)
    k = int(np.argmin(r["d_ray"][2])); i = int(r["d_ray"][2, k])
    assert i + 1 >= r["s_ray"].shape[0] or not r["s_ray"][i + 1:, :, k].any()


def test_np_arctan2_restatement_equals_numpy_here():
    """np_arctan2 (rt_oracle.c: SVML __svml_atan28_ha with VRCP14PD as a table) against this host's np.arctan2, bit for bit --
    where numpy dispatches to SVML (AVX512_SKX, as in the container the fixtures were made in)."""
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    if not feat.get("AVX512_SKX"):
        pytest.skip("numpy does not use SVML's arctan2 on this CPU")
    rng = np.random.default_rng(12)
    N = 500_000
    y = np.concatenate([rng.normal(0, 1, N), rng.uniform(-0.1, 0.1, N), rng.normal(0, 1, N) * 10.0 ** rng.uniform(-30, 30, N),
                        [0.0, -0.0, 1.0, -1.0, 0.0, np.inf]])
    x = np.concatenate([rng.normal(0, 1, N), rng.normal(0, 1, N), rng.normal(0, 1, N) * 10.0 ** rng.uniform(-30, 30, N),
                        [1.0, -1.0, 0.0, 0.0, 0.0, -np.inf]])
    assert np.array_equal(O.np_arctan2(y, x).view(np.uint64), np.arctan2(y, x).view(np.uint64))


def test_reference_anchor_values(oracle_fields):
    """SURVEY.md 8c anchors (vert, op6, default DELTA_S), measured on the reference."""
    t = golden("traj_vert_op6")
    F = oracle_fields("vert_heterogeneous")
    n, gx, gy = F.n_gradient(-2.0, -2.0)
    assert n[0] == 0.07142864686293911 and abs(gy[0] - (-0.01021203672272615)) < 1e-17
    assert list(t["d_ray"][2, [0, 15, 30]]) == [1006, 2938, 1134]
    r = O.trazar(F, 6, 1, float(t["step"]), int(t["max_size"]), t["box"], -2.0, -2.0, t["theta"], record_stride=0)
    fin = r["final"]
    assert abs(fin[0, 15] - 5.001510180773436) < 1e-12 and abs(fin[1, 15] - 0.8968279249636953) < 1e-12
    assert abs(fin[8, 0] - 0.19494379134524772) < 1e-13


def test_threads_do_not_change_results(oracle_fields):
    F = oracle_fields("vert_heterogeneous")
    th = np.linspace(0, np.pi / 2, 64)
    a = O.trazar(F, 6, 1, 0.002646652412362267, 30228, LIMITS["vert_heterogeneous"], -2.0, -2.0, th, record_stride=0)
    b = O.trazar(F, 6, 1, 0.002646652412362267, 30228, LIMITS["vert_heterogeneous"], -2.0, -2.0, th, record_stride=0,
                 nthreads=4)
    assert np.array_equal(a["final"], b["final"]) and a["steps"] == b["steps"]


@pytest.mark.parametrize("scen", ["interface", "fisheye", "vert_heterogeneous"])
def test_delta_s_sweep_matches_reference(scen, oracle_fields):
    """search_delta (RT_bench.py:950-958) over every 10th DELTA_S candidate of the calibration sweep: the
    oracle at other step sizes / max_size values than the default, reduced with the reference's three metrics."""
    from raytracing_amd import rt_bench as rb
    g = golden(f"sweep_{scen}_op6")
    choice = {"interface": "1", "fisheye": "2", "vert_heterogeneous": "3"}[scen]
    gam, R, th, pos_x, s, xi, xs, yi, ys, op_if, op_fish, _, _ = rb.constants(choice)
    F = oracle_fields(scen)
    for i, ref in zip(g["sel"], g["results"]):
        step, div = float(g["all_options"][i]), g["all_divisors"][i] + 1
        ms = int(rb.N * div) if op_fish else int(np.ceil(s / step) + 1)
        x0, y0 = (1.0, 0.0) if op_fish else (pos_x[:R], -2.0)
        r = O.trazar(F, 6, gam, step, ms, (xi, xs, yi, ys), x0, y0, th[:R], record_stride=1)
        if op_if:
            e = rb.snell_errors(r["s_ray"], r["d_ray"], th)
            assert abs(np.mean(e) - ref[0]) < 1e-7 and abs(np.max(e) - ref[1]) < 1e-7
        elif op_fish:
            assert abs(rb.closure_error(r["s_ray"]) - ref[0]) < 1e-9
        else:
            assert abs(rb.moment_cv(r["s_ray"], R) - ref[0]) < 1e-9


def _state_at(r, k, method):
    """state9 (and op7's hist4) of trajectory r at row k: what rtmi_batch_set_state takes (d_ray holds dist_real, dist_sim)."""
    fin, d = r["final"], r["d_ray"]
    st9 = np.concatenate([fin[:6], d[1:2], d[0:1], fin[8:9]])
    hist4 = None
    if method == 7:
        s = r["s_ray"]
        prev = lambda j: s[j, :2] if j >= 0 else np.zeros_like(s[0, :2])      # state_init's history is zeros before row 0
        hist4 = np.concatenate([prev(k - 2), prev(k - 1)])
    return st9, hist4


@pytest.mark.parametrize("name,scen,m", traj_fixtures())
def test_trazar_from_state_continues_bit_for_bit(name, scen, m, oracle_fields):
    """rto_trazar_from_state, the reference for runs continued from a caller-set state (rtmi_batch_set_state): a run stopped at
    row k (max_size = k + 1) and continued from its final state is the unsplit run, bit for bit -- rows k+1 .., final, d_ray and
    the step total -- for every method on every trajectory fixture's rays; at rows inside op7's bootstrap (1, 2, 3) and after
    some rays have left the box (only the live ones are continued)."""
    t = golden("traj_" + name)
    F = oracle_fields(scen)
    x0, y0, th = traj_inputs(t, scen)
    gam, step, ms, box = float(t["gamma"]), float(t["step"]), int(t["max_size"]), t["box"]
    R = len(th)
    rows = int(t["d_ray"][2].max()) + 2
    full = O.trazar(F, m, gam, step, ms, box, x0, y0, th, record_stride=1, rec_rows=rows, nthreads=4)
    d2 = full["d_ray"][2]
    ks = [2, 3, 200] + ([1] if m == 7 else [])
    if d2.min() + 7 < d2.max():                               # a k after some rays have ended (all fixtures but one-ray ones)
        ks.append(int(d2.min()) + 7)
    for k in ks:
        part = O.trazar(F, m, gam, step, k + 1, box, x0, y0, th, record_stride=1, rec_rows=k + 1, nthreads=4)
        live = np.flatnonzero(d2 > k)
        assert len(live) > 0
        st9, hist4 = _state_at(part, k, m)
        st9 = st9[:, live]
        hist4 = hist4[:, live] if hist4 is not None else None
        cont = O.trazar_from_state(F, m, gam, step, ms, box, st9, hist4, k, record_stride=1, rec_rows=rows, nthreads=4)
        assert not cont["s_ray"][:k + 1].any(), "rows at or before istep are not the continuation's"
        assert np.array_equal(cont["s_ray"][k + 1:], full["s_ray"][k + 1:, :, live]), f"k={k}"
        assert np.array_equal(cont["final"], full["final"][:, live]) and np.array_equal(cont["d_ray"], full["d_ray"][:, live])
        assert cont["steps"] == int(d2[live].sum())


def test_trazar_from_state_edges(oracle_fields):
    """istep = max_size - 1: no step, final is the state given; istep = max_size - 2: exactly one; a state outside the box
    takes exactly one step (the reference tests the box after the step, :878)."""
    F = oracle_fields("vert_heterogeneous")
    box = LIMITS["vert_heterogeneous"]
    st9 = np.zeros((9, 3))
    st9[:3] = [[0.5, 0.7, 9.0], [-1.0, -0.5, -1.0], [0.3, 1.1, 0.2]]         # the third ray lies outside the box
    st9[3:6] = np.stack(F.n_gradient(st9[0], st9[1]))
    st9[6:] = [[1.0], [1.2], [0.3]]
    ms = 50
    r = O.trazar_from_state(F, 6, 1, 0.01, ms, box, st9, None, [ms - 1, ms - 2, 5], record_stride=1)
    assert np.array_equal(r["d_ray"][2], [ms - 1, ms - 1, 6])
    assert np.array_equal(r["final"][:6, 0], st9[:6, 0]) and r["final"][8, 0] == st9[8, 0]
    assert r["d_ray"][0, 0] == st9[7, 0] and r["d_ray"][1, 0] == st9[6, 0]
    assert not r["s_ray"][:, :, 0].any() and r["s_ray"][ms - 1, 0, 1] == r["final"][0, 1]
    one = O.single_step(F, 6, 1, 0.01, np.concatenate([st9[:6], np.ones((1, 3))]).T)
    assert np.array_equal(r["final"][:6, 1:].T, one[1:])
    assert r["final"][0, 2] > box[1] and r["s_ray"][6, 0, 2] == r["final"][0, 2] and not r["s_ray"][7:, :, 2].any()
