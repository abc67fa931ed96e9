"""GPU: traveltime sensitivity kernels (rtmi_traveltime_perturb, rtmi_traveltime_backproject).  The device against the numpy
restatement (tests/sensitivity_ref.py) on the device's own rows; A Z and A 1 against the recorded traveltimes and chord sums;
adjointness; the same bits of A^T under every schedule, ray sorting and ray order; fp32; Fermat's principle on two-point
arrivals; one Gauss-Newton step of crosswell tomography; the 1 M-ray fan.  Bounds and measurements: DESIGN.md section 12."""
import numpy as np
import pytest

import sensitivity_ref as S
from conftest import LIMITS

pytestmark = pytest.mark.gpu

VERT_BOX = LIMITS["vert_heterogeneous"]


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    cache = {}

    def get(scen, dtype=None):
        key = (scen, dtype)
        if key not in cache:
            kw = {} if dtype is None else {"dtype": dtype}
            cache[key] = rb.Field.build(scen, LIMITS[scen], rb.DELTA, **kw)
        return cache[key]
    yield get
    for F in cache.values():
        F.close()


# scenario -> (step, launch point, fan, line)
SCEN = {
    "interface": (None, (-2.0, -2.0), (2 * np.pi / 60, np.pi / 2), (0.0, 1.0, 1.0)),
    "fisheye": (2 * np.pi / 303, (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4), (0.0, 1.0, 0.3)),
    "vert_heterogeneous": (None, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
    "anisotropy": (None, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
}


def batch(rb, F, scen, m, R, **kw):
    step, (x0, y0), fan, _ = SCEN[scen]
    step = rb.DELTA_S if step is None else step
    ms = rb.N * 304 if scen == "fisheye" else int(np.ceil(80 / step) + 1)
    th = kw.pop("thetas", np.linspace(*fan, R))
    gamma = 3.0 if scen == "anisotropy" else 1.0
    c = rb.Batch(F, rb.METHODS[m], step, ms, LIMITS[scen], gamma, th, x0, y0, record_stride=0)
    c.run()
    rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.METHODS[m], step, ms, LIMITS[scen], gamma, th, x0, y0, rec_rows=rows, **kw)
    b.run()
    return b


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(b)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(a[ok] - b[ok])) / max(np.max(np.abs(b[ok])), 1e-300))


CASES = [(s, m) for s in ("interface", "fisheye", "vert_heterogeneous") for m in range(1, 10)] + \
        [("anisotropy", 10), ("anisotropy", 11)]


# ---------------------------------------------------------------- 5. the device against the restatement
@pytest.mark.parametrize("scen,m", CASES)
def test_device_matches_the_restatement(rb, fields, scen, m):
    F = fields(scen)
    R = 512
    b = batch(rb, F, scen, m, R)
    s = b.rows()
    d = b.d_ray()
    last = d[2].astype(np.int64)
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    line = SCEN[scen][3]
    gamma = 3.0 if scen == "anisotropy" else 1.0
    M = S.matrices(s, last, ax, ay, line=line, kmax=4, method=m, gamma=gamma)
    rng = np.random.default_rng(m)
    dz = rng.standard_normal(Z.shape)
    dev = b.traveltime_perturb(dz, line=line, kmax=4)
    ref = S.perturb(M, dz)
    assert np.array_equal(dev["count"], M["count"])
    e_end, e_line = relerr(dev["end"], ref["end"]), relerr(dev["line"], ref["line"])
    dev0 = b.traveltime_perturb(dz)
    assert np.array_equal(dev0["end"], dev["end"])
    # identities 1 and 2 on the device's rows
    zt = b.traveltime_perturb(Z, line=line, kmax=4)
    T_end = s[last, 4, np.arange(R)]
    e_T = max(relerr(zt["end"], T_end), relerr(zt["line"], b.crossings(line, kmax=4)["T"]))
    e_1 = relerr(b.traveltime_perturb(np.ones_like(Z))["end"], d[1]) if m < 10 else 0.0
    # A^T
    we = rng.standard_normal(R)
    wl = rng.standard_normal((4, R))
    g = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=4)
    wl_ref = np.where(np.arange(4)[:, None] < np.maximum(M["count"], 0)[None, :], wl, 0.0)
    gr = S.backproject(M, we, wl_ref).reshape(Z.shape)
    e_g = float(np.max(np.abs(g - gr)) / np.max(np.abs(gr)))
    g0 = b.traveltime_backproject(w_end=we)
    gr0 = S.backproject(M, we).reshape(Z.shape)
    e_g0 = float(np.max(np.abs(g0 - gr0)) / np.max(np.abs(gr0)))
    b.close()
    print(f"{scen} op{m}: A end {e_end:.2e} line {e_line:.2e}; A Z - T {e_T:.2e}; A 1 - chord sum {e_1:.2e}; "
          f"A^T {e_g:.2e}, end only {e_g0:.2e}")
    assert e_end <= 1e-13 and e_line <= 1e-13
    assert e_T <= 1e-12 and e_1 <= 1e-12
    assert e_g <= 1e-12 and e_g0 <= 1e-12


# ---------------------------------------------------------------- 6. adjointness
@pytest.mark.parametrize("scen,m", [("vert_heterogeneous", 6), ("interface", 2), ("anisotropy", 11)])
def test_adjointness(rb, fields, scen, m):
    F = fields(scen)
    R = 1024
    b = batch(rb, F, scen, m, R)
    line = SCEN[scen][3]
    rng = np.random.default_rng(7)
    Z = F.arrays()[2]
    dz = rng.standard_normal(Z.shape)
    d = b.traveltime_perturb(dz, line=line, kmax=3)
    we = rng.standard_normal(R)
    wl = rng.standard_normal((3, R))
    g = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=3)
    b.close()
    lhs = np.dot(d["end"], we) + np.nansum(d["line"] * wl)
    rhs = float(np.dot(dz.ravel(), g.ravel()))
    scale = np.sum(np.abs(d["end"] * we)) + np.nansum(np.abs(d["line"] * wl))
    print(f"{scen} op{m}: <A dZ, w> - <dZ, A^T w> = {abs(lhs - rhs) / scale:.2e} relative")
    assert abs(lhs - rhs) <= 1e-12 * scale


# ---------------------------------------------------------------- 7. reproducibility
def test_backprojection_bits_do_not_depend_on_schedule_sorting_or_order(rb, fields):
    F = fields("vert_heterogeneous")
    R = 4096
    line = SCEN["vert_heterogeneous"][3]
    rng = np.random.default_rng(11)
    we = rng.standard_normal(R)
    wl = rng.standard_normal((2, R))
    ref = None
    for mode in ("plain", "sliced", "refill", "auto"):
        for sort in (False, True):
            b = batch(rb, F, "vert_heterogeneous", 6, R, launch_mode=mode, sort_rays=sort)
            g1 = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=2)
            g2 = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=2)
            b.close()
            assert np.array_equal(g1, g2), (mode, sort)
            if ref is None:
                ref = g1
            assert np.array_equal(g1, ref), (mode, sort)
    perm = rng.permutation(R)
    th = np.linspace(*SCEN["vert_heterogeneous"][2], R)
    b = batch(rb, F, "vert_heterogeneous", 6, R, thetas=th[perm])
    gp = b.traveltime_backproject(w_end=we[perm], w_line=wl[:, perm], line=line, kmax=2)
    b.close()
    assert np.array_equal(gp, ref)


# ---------------------------------------------------------------- 8. fp32
def test_fp32_against_fp64(rb, fields):
    R = 2048
    line = SCEN["vert_heterogeneous"][3]
    out = {}
    for dt in (rb.F64, rb.F32):
        F = fields("vert_heterogeneous", dt)
        b = batch(rb, F, "vert_heterogeneous", 6, R)
        Z = F.arrays()[2]
        d = b.traveltime_perturb(Z, line=line, kmax=2)
        g = b.traveltime_backproject(w_end=np.ones(R))
        out[dt] = (d, g, b.d_ray()[1])
        b.close()
    (d64, g64, _), (d32, g32, _) = out[rb.F64], out[rb.F32]
    e_end = float(np.max(np.abs(d32["end"] - d64["end"])) / np.max(np.abs(d64["end"])))
    e_g = float(np.max(np.abs(g32 - g64)) / np.max(np.abs(g64)))
    print(f"fp32 vs fp64, {R} rays: A Z at the ends {e_end:.2e}, A^T 1 {e_g:.2e}")
    assert e_end <= 1e-3 and e_g <= 1e-1


# ---------------------------------------------------------------- 9. Fermat on two_point
def bump(x, y, cx, cy, w):
    X_, Y_ = np.meshgrid(x, y)
    return np.exp(-((X_ - cx) ** 2 + (Y_ - cy) ** 2) / (2 * w * w))


def crosswell(rb, F, **kw):
    src = np.stack([np.full(8, -1.5), np.linspace(-2.2, 0.6, 8)], axis=1)
    ru = np.linspace(-2.3, 0.8, 32)
    return rb.two_point(rb.op6, F, src, (1.0, 0.0, 4.0), ru, thetas=np.linspace(-1.5, 3.0, 512), step=rb.DELTA_S,
                        max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=VERT_BOX, **kw)


def test_fermat_on_two_point_arrivals(rb, fields):
    F = fields("vert_heterogeneous")
    x, y, Z = F.arrays()[:3]
    dz = bump(x, y, 1.0, -1.0, 0.6) * Z
    eps = 1e-4
    r0 = crosswell(rb, F, sensitivity=True)
    sens = r0["sensitivity"]
    ad = sens.matvec(dz)
    Ts = []
    for sgn in (1.0, -1.0):
        Fp = rb.Field.from_samples(x, y, Z + sgn * eps * dz, rb.DELTA)
        Ts.append(crosswell(rb, Fp))
        Fp.close()
    sens.close()
    s_, j, a = sens.index.T
    one = (r0["count"][s_, j] == 1) & (Ts[0]["count"][s_, j] == 1) & (Ts[1]["count"][s_, j] == 1) & (a == 0)
    fd = (Ts[0]["T"][s_, j, a] - Ts[1]["T"][s_, j, a]) / (2 * eps)
    assert one.sum() >= 128
    err = float(np.max(np.abs(fd[one] - ad[one])) / np.max(np.abs(ad[one])))
    print(f"two_point Fermat: {one.sum()} arrivals, central difference vs sensitivity {err:.2e}")
    assert err <= 2e-3                   # measured 4.6e-4 on MI355X


# ---------------------------------------------------------------- 10. one Gauss-Newton step
def test_crosswell_gauss_newton_step(rb, fields):
    from scipy.sparse.linalg import LinearOperator, lsqr
    F = fields("vert_heterogeneous")
    x, y, Z0 = F.arrays()[:3]
    Zt = Z0 * (1 + 0.01 * bump(x, y, 1.0, -1.0, 0.7))
    Ft = rb.Field.from_samples(x, y, Zt, rb.DELTA)
    obs = crosswell(rb, Ft)
    Ft.close()
    F0 = rb.Field.from_samples(x, y, Z0, rb.DELTA)
    r0 = crosswell(rb, F0, sensitivity=True)
    sens = r0["sensitivity"]
    s_, j, a = sens.index.T
    use = (r0["count"][s_, j] == 1) & (obs["count"][s_, j] == 1) & (a == 0)
    rows = np.nonzero(use)[0]
    res0 = obs["T"][s_[rows], j[rows], 0] - r0["T"][s_[rows], j[rows], 0]

    def mv(v):
        return sens.matvec(v)[rows]

    def rmv(r):
        w = np.zeros(sens.shape[0])
        w[rows] = r
        return sens.rmatvec(w)
    op = LinearOperator((len(rows), sens.shape[1]), matvec=mv, rmatvec=rmv, dtype=np.float64)
    dz = lsqr(op, res0, damp=1e-3, iter_lim=30)[0].reshape(Z0.shape)
    sens.close()
    F0.close()
    F1 = rb.Field.from_samples(x, y, Z0 + dz, rb.DELTA)
    r1 = crosswell(rb, F1)
    F1.close()
    ok = r1["count"][s_[rows], j[rows]] >= 1                # the updated model's first arrival (slot 0)
    res1 = obs["T"][s_[rows], j[rows], 0][ok] - r1["T"][s_[rows], j[rows], 0][ok]
    m0, m1 = np.sqrt(np.mean(res0 ** 2)), np.sqrt(np.mean(res1 ** 2))
    print(f"crosswell: {len(rows)} arrivals, RMS misfit {m0:.3e} -> {m1:.3e} ({m1 / m0:.3f}), {ok.sum()} re-traced")
    assert ok.sum() >= 0.9 * len(rows)
    assert m1 <= 0.2 * m0


# ---------------------------------------------------------------- 11. the 1 M-ray fan
def test_million_ray_record(rb, fields):
    F = fields("vert_heterogeneous")
    R = 1 << 20
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.0, np.pi / 2, R)
    c = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1, th, -2.0, -2.0, record_stride=0)
    c.run()
    rows = int(c.d_ray()[2].max()) + 1
    c.close()
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1, th, -2.0, -2.0, rec_rows=rows, keep_n_ray=False)
    b.run()
    Z = F.arrays()[2]
    T = b.final()[8]
    walked = float(np.sum(b.d_ray()[2]) + R)             # rows read: x and y, 16 bytes each
    d = b.traveltime_perturb(Z, stats=True)
    e_T = float(np.max(np.abs(d["end"] - T) / np.abs(T)))
    dl = b.traveltime_perturb(Z, line=(1.0, 0.0, 4.0), kmax=1, stats=True)
    w = np.ones(R)
    g, st = b.traveltime_backproject(w_end=w, stats=True)
    g2, st2 = b.traveltime_backproject(w_end=w, w_line=np.ones((1, R)), line=(1.0, 0.0, 4.0), kmax=1, stats=True)
    b.close()
    # <Z, A^T 1> against sum(A Z): the fp64 host sum of the same contributions, in another order
    lhs = float(np.sum(d["end"]))
    rhs = float(np.dot(Z.ravel(), g.ravel()))
    e_adj = abs(lhs - rhs) / abs(lhs)
    floor = 16 * walked
    print(f"1 M rays, {rows} rows: A Z - T {e_T:.2e} per ray; <Z, A^T 1> - sum A Z {e_adj:.2e}; A {d['stats']['kernel_ms']:.2f} ms "
          f"(line {dl['stats']['kernel_ms']:.2f} ms), A^T {st['kernel_ms']:.2f} ms, {st['atomics']} atomics, scale 2^{st['scale_exp']} "
          f"(line {st2['kernel_ms']:.2f} ms, {st2['atomics']} atomics); x, y bytes {floor / 1e9:.1f} GB")
    assert e_T <= 1e-12
    assert e_adj <= 1e-12
