"""GPU: receiver-line crossings (rtmi_crossings) against the numpy restatement on the oracle's rows, and two-point ray tracing
(rtmi_two_point) against exact geometry, against fresh batches at the reported launch angles, and against the oracle.

The receiver angle theta of a crossing goes through atan2, the device's on one side and numpy's on the other: that column is
compared to 2 ulp, every other one bit for bit."""
import numpy as np
import pytest

import crossing_ref as X
from conftest import LIMITS

pytestmark = pytest.mark.gpu

NTHREADS = 16
VERT_BOX = LIMITS["vert_heterogeneous"]
IFACE_BOX = LIMITS["interface"]


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    from oracle import rt_oracle as O
    cache = {}

    def get(scen):
        key = "vert_heterogeneous" if scen == "anisotropy" else scen
        if key not in cache:
            cache[key] = (rb.Field.build(key, LIMITS[key], rb.DELTA), O.Field(key, LIMITS[key], rb.DELTA))
        return cache[key]
    yield get
    for g, _ in cache.values():
        g.close()


def ulp_close(a, b, n=2):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b))))))


def same_crossings(dev, cnt, out):
    """dev: Batch.crossings' dict; (cnt, out): crossing_ref's."""
    assert np.array_equal(dev["count"], cnt)
    for q, k in enumerate(X.FIELDS):
        if k == "theta":
            assert ulp_close(dev[k], out[:, q]), k
        else:
            assert np.array_equal(dev[k], out[:, q], equal_nan=True), k


def relerr(a, b):
    """per quantity (row), relative to that quantity's largest magnitude: bench.parity_relerr's measure"""
    return float(max(np.max(np.abs(a[q] - b[q])) / max(np.max(np.abs(b[q])), 1e-300) for q in range(len(a))))


def max_size_of(rb, scen):
    return rb.N * 304 if scen == "fisheye" else int(np.ceil(80 / rb.DELTA_S) + 1)


# scenario -> (step, launch point, fan, lines: horizontal, vertical, 30 degrees, a box edge)
def _line30(px, py):
    a = np.radians(30.0)
    return (-np.sin(a), np.cos(a), -np.sin(a) * px + np.cos(a) * py)


SCEN = {
    "interface": (None, (-2.0, -2.0), (2 * np.pi / 60, np.pi / 2),
                  [(0.0, 1.0, 1.0), (1.0, 0.0, 5.0), _line30(2.0, 0.0), (0.0, 1.0, 4.0)]),
    "fisheye": (2 * np.pi / 303, (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4),
                [(0.0, 1.0, 0.3), (1.0, 0.0, -0.2), _line30(0.0, 0.0), (1.0, 0.0, 1.5)]),
    "vert_heterogeneous": (None, (-2.0, -2.0), (0.0, np.pi / 2),
                           [(0.0, 1.0, -1.0), (1.0, 0.0, 2.0), _line30(0.0, -1.0), (0.0, 1.0, 1.0)]),
    "anisotropy": (None, (-2.0, -2.0), (0.0, np.pi / 2),
                   [(0.0, 1.0, -1.0), (1.0, 0.0, 2.0), _line30(0.0, -1.0), (0.0, 1.0, 1.0)]),
}
CASES = [(s, m, ro) for s in ("interface", "fisheye", "vert_heterogeneous") for (m, ro) in ((3, False), (6, True), (9, False))]
CASES += [("anisotropy", 11, False)]


@pytest.mark.parametrize("scen,m,ro", CASES)
def test_crossings_equal_the_restatement_on_the_oracles_rows(rb, fields, scen, m, ro):
    from oracle import rt_oracle as O
    F, OF = fields(scen)
    step, (x0, y0), (t0, t1), lines = SCEN[scen]
    step = rb.DELTA_S if step is None else step
    gam = 3.0 if scen == "anisotropy" else 1.0
    ms = max_size_of(rb, scen)
    box = LIMITS["vert_heterogeneous" if scen == "anisotropy" else scen]
    th = np.linspace(t0, t1, 40)
    b = rb.Batch(F, rb.METHODS[m], step, ms, box, gam, th, x0, y0, reference_order=ro, keep_n_ray=False)
    b.run()
    o = O.trazar(OF, m, gam, step, ms, box, x0, y0, th, record_stride=1, nthreads=NTHREADS)
    last = o["d_ray"][2].astype(np.int64)
    assert np.array_equal(b.d_ray()[2], o["d_ray"][2])
    for line in lines:
        for kmax in (1, 4):
            cnt, out = X.crossings(o["s_ray"], last, line, kmax)
            same_crossings(b.crossings(line, kmax), cnt, out)
    b.close()


def test_crossings_in_the_callers_order_with_sort_rays_and_fp32(rb, fields):
    F, _ = fields("vert_heterogeneous")
    ms = max_size_of(rb, "vert_heterogeneous")
    th = np.random.default_rng(5).permutation(np.linspace(0.0, np.pi / 2, 300))
    line = (1.0, 0.0, 2.0)
    ref = rb.Batch(F, rb.op3, rb.DELTA_S, ms, VERT_BOX, 1, th, -2.0, -2.0, keep_n_ray=False)
    ref.run()
    srt = rb.Batch(F, rb.op3, rb.DELTA_S, ms, VERT_BOX, 1, th, -2.0, -2.0, keep_n_ray=False, sort_rays=True)
    srt.run()
    a, c = ref.crossings(line), srt.crossings(line)
    for k in a:
        assert np.array_equal(a[k], c[k], equal_nan=True), k
    rows, last = ref.rows(), ref.d_ray()[2].astype(np.int64)
    same_crossings(a, *X.crossings(rows, last, line))
    # fp32 batches: the kernel reads fp32 rows and computes in fp64, like the restatement on the same rows
    F32 = rb.Field.build("vert_heterogeneous", VERT_BOX, rb.DELTA, rb.F32)
    b32 = rb.Batch(F32, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1, th[:64], -2.0, -2.0, keep_n_ray=False)
    b32.run()
    rows32 = b32.rows()                     # fp32 rows widened to fp64: exact, the values the kernel computes with
    same_crossings(b32.crossings(line), *X.crossings(rows32, b32.d_ray()[2].astype(np.int64), line))
    from raytracing_amd import _lib
    # a strided record is refused
    bs = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1, th[:8], -2.0, -2.0, record_stride=16)
    bs.run()
    with pytest.raises(_lib.RtmiError) as e:
        bs.crossings(line)
    assert e.value.code == -1
    for x in (ref, srt, b32, bs, F32):
        x.close()


# ---------------------------------------------------------------- two-point
def vert_exact(xs, ys, xr, yr):
    """Rays of v = 18 + 2 y are circular arcs centred on y = -9: (launch angle, traveltime, apex x, apex y)."""
    xc = ((xr ** 2 - xs ** 2) + (yr + 9) ** 2 - (ys + 9) ** 2) / (2 * (xr - xs))
    th0 = np.arctan2(xc - xs, ys + 9)
    vs, vr = 18 + 2 * ys, 18 + 2 * yr
    T = 0.5 * np.arccosh(1 + 4 * ((xr - xs) ** 2 + (yr - ys) ** 2) / (2 * vs * vr))
    return th0, T, xc, -9 + np.hypot(xs - xc, ys + 9)


def tp_kw(rb, step=None, **kw):
    step = rb.DELTA_S if step is None else step
    d = dict(step=step, max_size=int(np.ceil(80 / step) + 1), box=VERT_BOX, thetas=np.linspace(0.05, 1.5, 512))
    d.update(kw)
    return d


def test_vert_heterogeneous_matches_the_circular_arcs(rb, fields):
    F, _ = fields("vert_heterogeneous")
    yr = np.linspace(-2.4, 0.9, 64)
    errs = {}
    for step in (rb.DELTA_S, rb.DELTA_S / 2):
        r = rb.two_point(rb.op6, F, [(-2.0, -2.0)], (1.0, 0.0, 4.0), yr, **tp_kw(rb, step), stats=True)
        th0, T, xc, ya = vert_exact(-2.0, -2.0, 4.0, yr)
        blocked = (xc > -2.0) & (xc < 4.0) & (ya > 1.0)
        assert np.array_equal(r["count"][0], np.where(blocked, 0, 1))
        assert (r["nbad"][0] == 0).all()
        ok = ~blocked
        assert (np.abs(r["residual"][0, ok, 0]) <= 1e-10).all()
        errs[step] = (np.max(np.abs(r["T"][0, ok, 0] - T[ok]) / T[ok]), np.max(np.abs(r["theta0"][0, ok, 0] - th0[ok])))
        print(f"DELTA_S {step:.3e}: max rel T error {errs[step][0]:.3e}, max launch angle error {errs[step][1]:.3e}, "
              f"stats {r['stats']}")
    e1, e2 = errs[rb.DELTA_S], errs[rb.DELTA_S / 2]
    # Measured on MI355X: T 1.055e-6 relative and launch angle 3.077e-4 at DELTA_S, 1.050e-6 and 3.077e-4 at DELTA_S / 2.  The
    # error does not shrink with the step, so it is not the step method's; every arrival is within tol of its receiver, so it
    # is not the solver's either.  Bounds: twice the measurement.  That halving DELTA_S does not reduce it is pinned too.
    assert e1[0] <= 2.2e-6 and e1[1] <= 6.2e-4
    assert e2[0] <= 2.2e-6 and e2[1] <= 6.2e-4
    # the box top y = 1 as the receiver line: crossings on the final step; u = -x
    xr = np.linspace(-1.0, 4.5, 24)
    r = rb.two_point(rb.op6, F, [(-2.0, -2.0)], (0.0, 1.0, 1.0), -xr[::-1], **tp_kw(rb))
    xr = xr[::-1]
    th0, T, xc, _ = vert_exact(-2.0, -2.0, xr, 1.0)
    reach = xc >= xr                       # on the rising part of its arc: a ray through (x_r, 1) that falls there left before
    assert np.array_equal(r["count"][0], reach.astype(np.int32))
    assert np.max(np.abs(r["T"][0, reach, 0] - T[reach]) / T[reach]) <= 1e-5
    assert np.max(np.abs(r["theta0"][0, reach, 0] - th0[reach])) <= 5e-4       # measured: 2.5e-4, the same offset as on x = 4


def fresh_check(rb, F, m, src, line, r, kmax=4, **bkw):
    """Every converged arrival == a fresh batch's crossing at the reported launch angle, bit for bit."""
    S, J, A = r["T"].shape
    n = 0
    for s in range(S):
        conv = r["status"][s] == 1
        th = r["theta0"][s][conv]
        if not len(th):
            continue
        b = rb.Batch(F, rb.METHODS[m], bkw["step"], bkw["max_size"], bkw["box"], 1, th,
                     src[s][0], src[s][1], reference_order=bkw.get("reference_order", False), retrace=bkw.get("retrace", True))
        b.run()
        d = b.crossings(line, kmax)
        b.close()
        for q, k in enumerate(("u", "x", "y", "T", "theta")):
            got = r[k][s][conv]
            hit = (d["u"] == r["u"][s][conv][None, :])
            assert hit.any(axis=0).all(), "no crossing of the fresh ray has the arrival's u"
            c = np.argmax(hit, axis=0)
            assert np.array_equal(d[k][c, np.arange(len(th))], got), k
        n += len(th)
    return n


@pytest.mark.parametrize("m,retrace", [(6, True), (6, False), (3, True)])
def test_arrivals_are_fresh_batch_crossings_and_follow_snell(rb, fields, m, retrace):
    F, _ = fields("interface")
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    # op3's curvature advancement divides a cancelled difference of sines by a small curvature: u(theta) moves in
    # steps far above 1e-10 between neighbouring angles, so at the default tol its brackets end STALLED (measured: 0 converged)
    kw = dict(step=rb.DELTA_S, max_size=ms, box=IFACE_BOX, thetas=np.linspace(0.03, 1.5, 512), retrace=retrace,
              tol=1e-10 if m == 6 else 1e-7)
    n = rb.SCENARIOS["interface"](0.0, -2.0) * 1.0          # sqrt 2 below the wall
    # reflection: the line y = -2 through the source (the box bottom; u = -x)
    xr = np.linspace(0.5, 15.0, 32)
    r = rb.two_point(rb.METHODS[m], F, [(-2.0, -2.0)], (0.0, 1.0, -2.0), -xr[::-1], **kw)
    xr = xr[::-1]
    assert fresh_check(rb, F, m, [(-2.0, -2.0)], (0.0, 1.0, -2.0), r, **kw) > 0
    tot = (xr + 2.0) > 4.0 + 0.5                             # beyond the critical distance (45 degrees), with a margin
    c = r["count"][0] > 0
    sel = tot & c
    assert sel.sum() >= 10
    T_mirror = n * np.hypot(xr + 2.0, 4.0)
    eT = np.abs(r["T"][0, sel, 0] - T_mirror[sel])
    eA = np.abs(r["theta"][0, sel, 0] + np.arctan2(4.0, xr[sel] + 2.0))
    print(f"op{m} retrace={retrace} reflection: {sel.sum()} receivers, max |T - mirror T| {eT.max():.3e}, max angle error {eA.max():.3e}")
    assert eT.max() <= 8 * rb.SIGMA and eA.max() <= 0.05     # a wall of thickness ~SIGMA turns the ray below y = 0
    # refraction: y = 3 above the wall
    xr = np.linspace(0.0, 15.0, 32)
    r = rb.two_point(rb.METHODS[m], F, [(-2.0, -2.0)], (0.0, 1.0, 3.0), -xr[::-1], **kw)
    xr = xr[::-1]
    assert fresh_check(rb, F, m, [(-2.0, -2.0)], (0.0, 1.0, 3.0), r, **kw) > 0
    sel = r["count"][0] > 0
    assert sel.sum() >= 10
    t1 = r["theta0"][0, sel, 0]
    t2 = np.arccos(np.clip(np.sqrt(2.0) * np.cos(t1), -1, 1))
    x_pred = -2.0 + 2.0 / np.tan(t1) + 3.0 / np.tan(t2)
    T_pred = np.sqrt(2.0) * 2.0 / np.sin(t1) + 3.0 / np.sin(t2)
    eX = np.abs(x_pred - xr[sel]); eT = np.abs(r["T"][0, sel, 0] - T_pred); eA = np.abs(r["theta"][0, sel, 0] - t2)
    print(f"op{m} retrace={retrace} refraction: {sel.sum()} receivers, max x error {eX.max():.3e}, T {eT.max():.3e}, angle {eA.max():.3e}")
    assert eT.max() <= 8 * rb.SIGMA and eA.max() <= 0.05


@pytest.mark.parametrize("m,ro", [(3, False), (9, False), (6, True), (6, False)])
def test_arrivals_against_the_oracle(rb, fields, m, ro):
    from oracle import rt_oracle as O
    F, OF = fields("vert_heterogeneous")
    # op9's golden-section searches make u(theta) step by more than 1e-10 between neighbouring angles (measured: 4 of 16
    # brackets STALLED at the default tol)
    kw = tp_kw(rb, reference_order=ro, thetas=np.linspace(0.05, 1.5, 128), tol=1e-7 if m == 9 else 1e-10)
    line = (1.0, 0.0, 4.0)
    r = rb.two_point(rb.METHODS[m], F, [(-2.0, -2.0)], line, np.linspace(-2.4, 0.9, 16), **kw)
    conv = r["status"][0] == 1
    th = r["theta0"][0][conv]
    assert len(th) == 16
    o = O.trazar(OF, m, 1.0, kw["step"], kw["max_size"], VERT_BOX, -2.0, -2.0, th, record_stride=1, nthreads=NTHREADS)
    cnt, out = X.crossings(o["s_ray"], o["d_ray"][2].astype(np.int64), line, 4)
    assert (cnt >= 1).all()
    ref = {k: out[0, q] for q, k in enumerate(X.FIELDS)}
    if m == 6 and not ro:
        got = np.stack([r[k][0][conv] for k in ("u", "x", "y", "T", "theta")])
        want = np.stack([ref[k] for k in ("u", "x", "y", "T", "theta")])
        assert relerr(got, want) <= 1e-9
        return
    for k in ("u", "x", "y", "T"):
        assert np.array_equal(r[k][0][conv], ref[k]), k
    assert ulp_close(r["theta"][0][conv], ref["theta"])


def lens_field(rb, O):
    """A low-velocity Gaussian lens in a uniform medium, as samples on the vert_heterogeneous grid."""
    x, y = O.Field("vert_heterogeneous", VERT_BOX, rb.DELTA).arrays()[:2]
    Xg, Yg = np.meshgrid(x, y)
    Z = 1.0 + 0.3 * np.exp(-((Xg - 0.5) ** 2 + (Yg + 0.75) ** 2) / 0.3 ** 2)
    return rb.Field.from_samples(x, y, Z, rb.DELTA), O.Field.from_samples(x, y, Z, rb.DELTA)


def test_multipath_behind_a_lens(rb):
    from oracle import rt_oracle as O
    F, OF = lens_field(rb, O)
    src, line = (-1.5, -0.75), (1.0, 0.0, 4.0)
    ms = 4000
    th = np.linspace(-0.5, 0.5, 65536)
    ru = np.linspace(-2.3, 0.8, 48)
    r = rb.two_point(rb.op6, F, [src], line, ru, thetas=th, step=rb.DELTA_S, max_size=ms, box=VERT_BOX, max_arrivals=8,
                     mem_budget=64 << 30)
    # brute force over the same fan: sign changes of u - u_j between neighbouring rays, per crossing index
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, VERT_BOX, 1, th, src[0], src[1], keep_n_ray=False)
    b.run()
    d = b.crossings(line, 4)
    b.close()
    brute = np.zeros(len(ru), dtype=np.int64)
    for c in range(4):
        ok = np.minimum(d["count"][:-1], d["count"][1:]) > c
        lo = np.fmin(d["u"][c, :-1], d["u"][c, 1:])[ok]
        hi = np.fmax(d["u"][c, :-1], d["u"][c, 1:])[ok]
        brute += ((lo[None, :] <= ru[:, None]) & (ru[:, None] < hi[None, :])).sum(axis=1)
    print(f"lens: arrivals per receiver {r['count'][0].tolist()}, not converged {int(r['nbad'][0].sum())}")
    assert r["count"][0].max() >= 3
    assert np.array_equal(r["count"][0] + r["nbad"][0], brute)
    assert np.array_equal(r["count"][0], brute)
    conv = r["status"][0] == 1
    o = O.trazar(OF, 6, 1.0, rb.DELTA_S, ms, VERT_BOX, src[0], src[1], r["theta0"][0][conv], record_stride=1, nthreads=NTHREADS)
    cnt, out = X.crossings(o["s_ray"], o["d_ray"][2].astype(np.int64), line, 4)
    n = int(conv.sum())
    c = np.argmin(np.abs(np.nan_to_num(out[:, 0], nan=np.inf) - r["u"][0][conv][None, :]), axis=0)   # the oracle's crossing
    got = np.stack([r[k][0][conv] for k in ("u", "x", "y", "T")])
    want = np.stack([out[c, q, np.arange(n)] for q in range(4)])
    assert relerr(got, want) <= 1e-9
    F.close()


def test_sources_are_independent_and_output_deterministic(rb, fields):
    F, _ = fields("vert_heterogeneous")
    src = [(-2.0, -2.3 + 0.2 * k) for k in range(8)]
    kw = tp_kw(rb, thetas=np.linspace(0.0, 1.5, 256))
    ru = np.linspace(-2.4, 0.9, 32)
    line = (1.0, 0.0, 4.0)
    allr = rb.two_point(rb.op6, F, src, line, ru, **kw, stats=True)
    assert allr["stats"]["groups"] == 1
    again = rb.two_point(rb.op6, F, src, line, ru, **kw)
    small = rb.two_point(rb.op6, F, src, line, ru, **kw, mem_budget=48 * 256 * allr["stats"]["rec_rows"] * 3, stats=True)
    assert small["stats"]["groups"] >= 3
    keys = [k for k in allr if k != "stats"]
    for k in keys:
        assert np.array_equal(allr[k], again[k], equal_nan=True), k
        assert np.array_equal(allr[k], small[k], equal_nan=True), k
    for s in range(8):
        one = rb.two_point(rb.op6, F, [src[s]], line, ru, **kw)
        for k in keys:
            assert np.array_equal(allr[k][s], one[k][0], equal_nan=True), k
    assert (allr["count"] >= 1).sum() > 100
