"""GPU: Kirchhoff migration and modelling from traveltime tables (rtmi_kirchhoff_*, rt_bench.Kirchhoff).  Migration against the
numpy restatement (tests/kirchhoff_ref.py) bit for bit, on closed-form tables and on the device's own; modelling against the
restatement's CSR matrix, the same bits twice and in any trace order; adjointness; imaging a scatterer end to end from
traveltime_table's tables; least-squares migration through scipy's LSQR.  Bounds and their measured values: DESIGN.md 14."""
import numpy as np
import pytest

import kirchhoff_ref as K
from conftest import LIMITS

pytestmark = pytest.mark.gpu

SCEN = "vert_heterogeneous"


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def field(rb):
    F = rb.Field.build(SCEN, LIMITS[SCEN], rb.DELTA)
    yield F
    F.close()


def table(rb, F, pos_x, grid, rays, amplitude):
    src = np.stack([pos_x, np.full(len(pos_x), K.POS_Y)], axis=1)
    return rb.traveltime_table(rb.op6, F, src, grid, thetas=np.linspace(0.05, np.pi - 0.05, rays), step=rb.DELTA_S,
                               max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=LIMITS[SCEN], amplitude=amplitude)


@pytest.fixture(scope="module")
def closed():
    isrc, irec = K.geometry()
    return {"T": K.closed_T(), "theta": K.closed_theta(), "isrc": isrc, "irec": irec, "nt": K.NT}


@pytest.fixture(scope="module")
def small(rb, field):
    """the device's own tables: 12 positions, a 256-ray fan, amplitudes, an 80 x 40 grid"""
    grid = (-1.0, 0.0625, 80, -2.0, 0.0625, 40)
    tab = table(rb, field, K.POS_X[::4], grid, 256, True)
    isrc, irec = K.geometry(12, 4)
    return {"T": tab["T"], "theta": tab["theta"], "G": tab["G"], "isrc": isrc, "irec": irec, "nt": K.NT}


@pytest.fixture(scope="module")
def survey(rb, field):
    """the standard positions and grid from traveltime_table: a 1 024-ray fan at DELTA_S"""
    tab = table(rb, field, K.POS_X, K.GRID, 1024, False)
    isrc, irec = K.geometry()
    return {"T": tab["T"], "theta": tab["theta"], "isrc": isrc, "irec": irec, "nt": K.NT}


# (nbin, amp, w, holes)
CASES = [(0, False, False, False), (0, True, True, False), (6, False, False, False), (6, True, True, True), (0, False, True, True),
         (6, True, False, False)]


def inputs(tabs, case, seed):
    """-> (kwargs of the restatement, data, model)"""
    nbin, amp, w, holes = case
    rng = np.random.default_rng(seed)
    T, th = tabs["T"], tabs["theta"]
    A = (tabs["G"] if "G" in tabs else 0.5 + rng.random(T.shape)) if amp else None
    if holes:
        T, th = K.with_holes(T, rng), K.with_holes(th, rng)
        A = None if A is None else K.with_holes(A, rng)
    N = len(tabs["isrc"])
    kw = dict(amp=A, theta=th if nbin else None, w=rng.standard_normal(N) if w else None, nbin=nbin, dopen=K.DOPEN if nbin else None)
    return T, kw, rng.standard_normal((N, tabs["nt"])), rng.standard_normal((max(nbin, 1),) + T.shape[1:])


def operator(rb, T, tabs, kw, order=None):
    isrc, irec, w = tabs["isrc"], tabs["irec"], kw["w"]
    if order is not None:
        isrc, irec, w = isrc[order], irec[order], None if w is None else w[order]
    return rb.Kirchhoff(T, isrc, irec, tabs["nt"], K.DT, t0=K.T0, amp=kw["amp"], theta=kw["theta"], weights=w, nbin=kw["nbin"],
                        dopen=kw["dopen"])


# ---------------------------------------------------------------- 4, 5. the device against the restatement
@pytest.mark.parametrize("which", ["closed", "small"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_migrate_bit_for_bit_and_model_against_the_matrix(rb, request, which, case):
    tabs = request.getfixturevalue(which)
    T, kw, d, m = inputs(tabs, CASES[case], 100 + case)
    nbin = kw["nbin"]
    ref, cnt = K.migrate(T, tabs["isrc"], tabs["irec"], d, K.DT, K.T0, **kw)
    L = K.matrix(T, tabs["isrc"], tabs["irec"], tabs["nt"], K.DT, K.T0, **kw)
    op = operator(rb, T, tabs, kw)
    img, st = op.migrate(d, stats=True)
    assert img.shape == ((nbin,) + T.shape[1:] if nbin else T.shape[1:])
    assert np.array_equal(img.reshape(ref.shape), ref), f"{np.max(np.abs(img.reshape(ref.shape) - ref)):.3e}"
    assert st["contributing"] == cnt and st["pairs"] == len(tabs["isrc"]) * T[0].size
    assert 0 < cnt and (cnt < st["pairs"] or not CASES[case][3])
    # model
    dm, sm = op.model(m, stats=True)
    dref = (L @ m.reshape(-1)).reshape(dm.shape)
    e = np.max(np.abs(dm - dref)) / np.max(np.abs(dref))
    assert sm["contributing"] == cnt
    again = op.model(m)
    assert np.array_equal(dm, again)
    # the traces in a random order: the model's rows keep their bits, the image moves by rounding only
    order = np.random.default_rng(5).permutation(len(tabs["isrc"]))
    opp = operator(rb, T, tabs, kw, order)
    dp = opp.model(m)
    ip = opp.migrate(d[order])
    ei = np.max(np.abs(ip - img)) / np.max(np.abs(img))
    op.close(); opp.close()
    print(f"{which} {CASES[case]}: contributing {cnt} of {st['pairs']}, model against the matrix {e:.2e}, scale_exp {sm['scale_exp']}, "
          f"migrate under a permutation {ei:.2e}, kernel ms migrate {st['kernel_ms']:.3f} model {sm['kernel_ms']:.3f}")
    assert e <= 1e-12
    assert np.array_equal(dp, dm[order])
    assert ei <= 1e-12


# ---------------------------------------------------------------- 6. adjointness
@pytest.mark.parametrize("nbin", [0, 6])
def test_adjointness_on_the_device(rb, closed, nbin):
    T, kw, d, m = inputs(closed, (nbin, True, True, True), 11 + nbin)
    op = operator(rb, T, closed, kw)
    lhs = float(op.model(m).reshape(-1) @ d.reshape(-1))
    rhs = float(m.reshape(-1) @ op.migrate(d).reshape(-1))
    op.close()
    L = K.matrix(T, closed["isrc"], closed["irec"], closed["nt"], K.DT, K.T0, **kw)
    scale = float(np.abs(d.reshape(-1)) @ (abs(L) @ np.abs(m.reshape(-1))))
    print(f"nbin {nbin}: <Lm, d> {lhs:.12e} <m, L^T d> {rhs:.12e}, |diff| / sum|terms| {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs - rhs) <= 1e-12 * scale


# ---------------------------------------------------------------- 7. imaging end to end
def test_imaging_a_scatterer_from_the_devices_tables(rb, survey, closed):
    ix, iy = K.SCATTERER
    cover = np.isfinite(survey["T"]).mean(axis=(1, 2))
    print("covered share of nodes per table:", np.round(cover, 4), f"min {cover.min():.4f}")
    assert np.all(np.isfinite(survey["T"][:, iy, ix])), "a table does not cover the scatterer's node"
    data = K.scatterer_data(survey["isrc"], survey["irec"])
    N = len(survey["isrc"])
    op = rb.Kirchhoff.from_table(survey, survey["isrc"], survey["irec"], K.NT, K.DT)
    img = op.migrate(data)
    op.close()
    ref, _ = K.migrate(closed["T"], closed["isrc"], closed["irec"], data, K.DT)
    py, px = np.unravel_index(np.argmax(np.abs(img)), img.shape)
    e = np.nanmax(np.abs(survey["T"] - closed["T"]))
    print(f"peak at {(px, py)}, I / N {img[iy, ix] / N:.6f}, on closed-form tables {ref[0, iy, ix] / N:.6f}, tables against the "
          f"closed form {e:.2e}")
    assert (px, py) == (ix, iy)
    assert abs(img[iy, ix] / N - ref[0, iy, ix] / N) <= 1e-3


# ---------------------------------------------------------------- 8. least-squares migration
def test_least_squares_migration_through_lsqr(rb, survey):
    from scipy.sparse.linalg import lsqr
    L = K.matrix(survey["T"], survey["isrc"], survey["irec"], K.NT, K.DT)
    d = L @ K.lsm_model().reshape(-1)
    op = rb.Kirchhoff.from_table(survey, survey["isrc"], survey["irec"], K.NT, K.DT)
    xd = lsqr(op.as_linear_operator(), d, atol=0, btol=0, iter_lim=10)[0]
    op.close()
    xr = lsqr(L, d, atol=0, btol=0, iter_lim=10)[0]
    rd = float(np.linalg.norm(L @ xd - d) / np.linalg.norm(d))
    rr = float(np.linalg.norm(L @ xr - d) / np.linalg.norm(d))
    print(f"LSQR, 10 iterations: residual ratio on the device {rd:.8f}, with the restatement's matrix {rr:.8f}")
    assert abs(rd - rr) <= 1e-6 * rr
    assert rd < 0.3


# ---------------------------------------------------------------- the handle
def test_closed_handle_and_windows_of_a_long_trace(rb):
    """nt above the 4 096 samples a block holds at a time: the trace is modelled in windows, the same operator"""
    rng = np.random.default_rng(3)
    T = 0.5 + 2.4 * rng.random((3, 6, 50))
    isrc = np.array([0, 0, 1, 2], dtype=np.int32); irec = np.array([1, 2, 2, 0], dtype=np.int32)
    nt = 9000
    op = rb.Kirchhoff(T, isrc, irec, nt, 0.001)
    m = rng.standard_normal(T.shape[1:])
    d = rng.standard_normal((4, nt))
    L = K.matrix(T, isrc, irec, nt, 0.001)
    ref, cnt = K.migrate(T, isrc, irec, d, 0.001)
    dm, st = op.model(m, stats=True)
    assert np.array_equal(op.migrate(d), ref[0])
    assert st["contributing"] == cnt
    assert np.max(np.abs(dm.reshape(-1) - L @ m.reshape(-1))) <= 1e-12 * np.max(np.abs(dm))
    op.close()
    with pytest.raises(RuntimeError, match="closed"):
        op.migrate(d)
