"""GPU: the step methods and the post-trace kernels on caller-sampled beds (tests/sampled_beds.py): unpadded grids whose boxes
reach past them (rows in the not-a-knot rim cells and off the grid), unequal spacings, plateaus of equal samples, ragged batch
sizes with partly filled tail waves, dead starts, truncated rays and short records.  Reference-order methods against the oracle's
bits; fused op1/2/6/8 against the oracle at REL on every ray; fp32; rtmi_crossings / rtmi_paraxial / rtmi_first_arrival_grid /
rtmi_traveltime_perturb / _backproject against the restatements on the device's own rows; the constant medium's closed forms."""
import functools
import re

import numpy as np
import pytest

import crossing_ref as X
import paraxial_ref as P
import sensitivity_ref as S
import ttgrid_ref as G
from sampled_beds import BEDS, RAGGED
from test_gpu_parity import REL, relerr
from test_gpu_two_point import same_crossings

pytestmark = pytest.mark.gpu

NAMES = sorted(BEDS)
# (method, gamma, reference_order): every method that steps in the reference's operation order
REF_ORDER = [(3, 1.0, False), (4, 1.0, False), (5, 1.0, False), (7, 1.0, False), (9, 1.0, False), (10, 0.3, False),
             (11, 3.0, False), (1, 1.0, True), (2, 1.0, True), (6, 1.0, True), (8, 1.0, True)]
GAMMA = {10: 0.3, 11: 3.0}


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

    def get(name, dtype=0):
        if (name, dtype) not in cache:
            x, y, Z, delta, _ = BEDS[name].fields()
            cache[(name, dtype)] = rb.Field.from_samples(x, y, Z, delta, dtype)
        return cache[(name, dtype)]
    yield get
    for F in cache.values():
        F.close()


@functools.lru_cache(maxsize=None)
def oracle_field(name):
    from oracle import rt_oracle as O
    x, y, Z, delta, _ = BEDS[name].fields()
    return O.Field.from_samples(x, y, Z, delta)


def oracle(name, m, x0, y0, th, rec_rows=None, max_size=None):
    from oracle import rt_oracle as O
    bed = BEDS[name]
    return O.trazar(oracle_field(name), m, GAMMA.get(m, 1.0), bed.step, max_size or bed.max_size, bed.box, x0, y0, th,
                    record_stride=1, rec_rows=rec_rows, nthreads=16)


def batch(rb, F, name, m, x0, y0, th, max_size=None, **kw):
    bed = BEDS[name]
    b = rb.Batch(F, rb.METHODS[m], bed.step, max_size or bed.max_size, bed.box, GAMMA.get(m, 1.0), th, x0, y0, **kw)
    b.run()
    return b


def bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def short_rows(name):
    return BEDS[name].max_size // 2          # below the longest ray of every bed


# ---------------------------------------------------------------- 1. reference-order methods: the oracle's bits
@pytest.mark.parametrize("m,gam,ro", REF_ORDER)
@pytest.mark.parametrize("name", NAMES)
def test_reference_order_is_the_oracles_bits(rb, fields, name, m, gam, ro):
    bed = BEDS[name]
    for R in RAGGED:
        x0, y0, th = bed.launches(R, 10 * m + R)
        rec = short_rows(name) if R == 65 else None
        o = oracle(name, m, x0, y0, th, rec_rows=rec)
        b = batch(rb, fields(name), name, m, x0, y0, th, rec_rows=rec or 0, reference_order=ro)
        d, fin, s = b.d_ray(), b.final(), b.rows()
        b.close()
        assert bits(d, o["d_ray"]) and bits(fin, o["final"]) and bits(s, o["s_ray"]), (R, np.sum(d[2] != o["d_ray"][2]))
        if R == 333:
            off, rim = bed.edge_counts(s, d[2])
            trunc = int(np.sum(d[2] == bed.max_size - 1))
            print(f"{name} op{m}{' ref' if ro else ''}: {off} rows off the grid, {rim} in rim cells, {trunc} truncated; bits equal")
            assert off > 1000 and rim > 500 and trunc > 0


@pytest.mark.parametrize("mode", ["sliced", "refill"])
@pytest.mark.parametrize("m,ro", [(3, False), (9, False), (6, True), (11, False)])
@pytest.mark.parametrize("name", NAMES)
def test_schedules_with_sorted_rays_are_the_oracles_bits(rb, fields, name, m, ro, mode):
    bed = BEDS[name]
    x0, y0, th = bed.launches(333, 500 + m)
    rec = short_rows(name)
    o = oracle(name, m, x0, y0, th, rec_rows=rec)
    b = batch(rb, fields(name), name, m, x0, y0, th, rec_rows=rec, reference_order=ro, launch_mode=mode, sort_rays=True,
              slice_steps=37)
    d, fin, s = b.d_ray(), b.final(), b.rows()
    b.close()
    assert bits(d, o["d_ray"]) and bits(fin, o["final"]) and bits(s, o["s_ray"])


# ---------------------------------------------------------------- 2. fused op1/2/6/8 (re-trace on): REL on every ray
@pytest.mark.parametrize("m", [1, 2, 6, 8])
@pytest.mark.parametrize("name", NAMES)
def test_fused_methods_hold_the_north_star_on_every_ray(rb, fields, name, m):
    bed = BEDS[name]
    worst, retraced = 0.0, 0
    for R in RAGGED:
        x0, y0, th = bed.launches(R, 20 * m + R)
        o = oracle(name, m, x0, y0, th)
        b = batch(rb, fields(name), name, m, x0, y0, th)
        d, fin, s, st = b.d_ray(), b.final(), b.rows(), b.stats()
        b.close()
        bad = np.flatnonzero(d[2] != o["d_ray"][2])
        assert bad.size == 0, f"R {R}: step counts differ on rays {bad[:8]}"
        err = max(relerr(fin, o["final"]), relerr(d[:2], o["d_ray"][:2]), relerr(s, o["s_ray"]))
        worst, retraced = max(worst, err), retraced + st["retraced"]
        assert st["retrace_overflow"] == 0
    print(f"{name} op{m}: largest relative error {worst:.2e}, {retraced} rays re-traced")
    assert worst < REL


def test_layers_field_build_line_and_retrace(rb, monkeypatch, capfd):
    """The field-build line of RTMI_DEBUG for the layered bed, and the default runs' re-trace counts.  Measured: 0 of 1 536 cells
    flat and 0 steep.  A cell is flat when every gradient-spline coefficient is below 2^-80 of the grid's largest, and the
    not-a-knot fits ring about 0.27x per cell away from each step, so a layer needs some 42 cells of equal rows before one of
    its cells qualifies; steep needs lambda * (shorter side) >= 40, which 65 rows reach only for a contrast of about 80 %.  So
    no ray here is handed to the re-trace, and test_fused_methods_hold_the_north_star_on_every_ray holds the fused forms at REL
    on this bed without it."""
    bed = BEDS["layers"]
    x, y, Z, delta, _ = bed.fields()
    monkeypatch.setenv("RTMI_DEBUG", "1")
    F = rb.Field.from_samples(x, y, Z, delta)
    monkeypatch.delenv("RTMI_DEBUG")
    err = capfd.readouterr().err
    hit = re.search(r"field (\d+) x (\d+): (\d+) of (\d+) cells flat, (\d+) steep", err)
    assert hit, err
    assert (int(hit.group(1)), int(hit.group(2)), int(hit.group(4))) == (25, 65, 24 * 64)
    print(f"layers: {hit.group(3)} of {hit.group(4)} cells flat, {hit.group(5)} steep")
    for m in (1, 2, 6, 8):
        x0, y0, th = bed.launches(333, 20 * m + 333)
        b = batch(rb, F, "layers", m, x0, y0, th, record_stride=0)
        st = b.stats()
        b.close()
        print(f"layers op{m}: {st['retraced']} rays re-traced")
        assert st["retrace_overflow"] == 0
    F.close()


# ---------------------------------------------------------------- 3. fp32 fields
@pytest.mark.parametrize("name", NAMES)
def test_fp32_fields_track_fp64(rb, fields, name):
    """test_fp32_path_tracks_fp64's bounds: step counts at most one apart, the same on > 98 % of rays, end points within 2e-5"""
    bed = BEDS[name]
    x0, y0, th = bed.launches(333, 77)
    a = batch(rb, fields(name, 0), name, 6, x0, y0, th, record_stride=0)
    b = batch(rb, fields(name, 1), name, 6, x0, y0, th, record_stride=0)
    fa, fb, da, db = a.final(), b.final(), a.d_ray(), b.d_ray()
    a.close(); b.close()
    assert np.max(np.abs(da[2] - db[2])) <= 1
    same = da[2] == db[2]
    err = np.abs(fa[:2] - fb[:2])[:, same].max()
    print(f"{name} fp32: same step count on {same.sum()}/333 rays, end points {err:.2e}")
    assert same.mean() > 0.98 and err < 2e-5


# ---------------------------------------------------------------- 4. post-trace kernels on the device's own rows
def nan_relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok])) / max(np.max(np.abs(b[ok])), 1e-300)) if ok.any() else 0.0


# (R, sort_rays, rec_rows cut short)
POST = [(333, True, False), (65, True, True), (63, False, False), (1, False, False)]


@pytest.mark.parametrize("R,srt,short", POST)
@pytest.mark.parametrize("name", NAMES)
def test_post_trace_kernels_equal_the_restatements(rb, fields, name, R, srt, short):
    bed = BEDS[name]
    F = fields(name)
    x0, y0, th = bed.launches(R, 900 + R)
    rec = short_rows(name) if short else bed.max_size
    b = batch(rb, F, name, 6, x0, y0, th, rec_rows=rec, sort_rays=srt)
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    line = bed.line
    for kmax in (1, 4):
        same_crossings(b.crossings(line, kmax), *X.crossings(rows, last, line, kmax))
    dev = b.paraxial(line, kmax=3)
    cnt, atl, end = P.paraxial(rows, last, P.SplineField(*F.arrays()), line=line, kmax=3)
    assert np.array_equal(dev["count"], cnt)
    ee = max(nan_relerr(dev[k], end[q]) for q, k in enumerate(P.FIELDS[:6]))
    el = max(nan_relerr(dev["at_line"][k], atl[:, q]) for q, k in enumerate(P.FIELDS[:6]))
    assert ee <= 1e-10 and el <= 1e-10
    assert np.array_equal(dev["kmah"], end[6], equal_nan=True)
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    M = S.matrices(rows, last, ax, ay, line=line, kmax=4, method=6)
    rng = np.random.default_rng(R)
    dz = rng.standard_normal(Z.shape)
    d = b.traveltime_perturb(dz, line=line, kmax=4)
    ref = S.perturb(M, dz)
    assert np.array_equal(d["count"], M["count"])
    e_end, e_line = nan_relerr(d["end"], ref["end"]), nan_relerr(d["line"], ref["line"])
    we, wl = rng.standard_normal(R), rng.standard_normal((4, R))
    g = b.traveltime_backproject(w_end=we, w_line=wl, line=line, kmax=4)
    wl_ref = np.where(np.arange(4)[:, None] < np.maximum(M["count"], 0)[None, :], wl, 0.0)
    wl_ref[:, M["count"] < 0] = 0.0
    gr = S.backproject(M, np.where(np.isfinite(ref["end"]), we, 0.0), wl_ref).reshape(Z.shape)
    e_g = float(np.max(np.abs(g - gr)) / max(np.max(np.abs(gr)), 1e-300))
    b.close()
    off, rim = bed.edge_counts(rows, last)
    print(f"{name} R {R} sort {srt} rec {rec}: {off} rows off the grid, {rim} in rim cells; paraxial end {ee:.1e} line {el:.1e}; "
          f"A end {e_end:.1e} line {e_line:.1e}; A^T {e_g:.1e}")
    assert e_end <= 1e-13 and e_line <= 1e-13 and e_g <= 1e-12


def out_grid(bed):
    """an output grid over the whole box, past the field grid, hx != hy"""
    xi, xs, yi, ys = bed.box
    return (xi + 0.01, (xs - xi - 0.02) / 120, 121, yi + 0.01, (ys - yi - 0.02) / 90, 91)


@pytest.mark.parametrize("name", NAMES)
def test_first_arrival_grid_equals_the_restatement(rb, fields, name):
    bed = BEDS[name]
    F = fields(name)
    th, xs, ys = bed.fan(512, (bed.x[len(bed.x) // 2], bed.y[len(bed.y) // 3]))
    b = batch(rb, F, name, 6, xs, ys, th, keep_n_ray=False)
    grid = out_grid(bed)
    dev = b.first_arrival_grid(grid, amplitude=True, stats=True)
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    b.close()
    J, km = G.paraxial_rows(rows, last, P.SplineField(*F.arrays()))
    ref = G.from_record(rows, last, grid, amplitude=(J, km, G.record_n(rows)))
    gx0, gdx, nx, gy0, gdy, ny = grid
    X2, Y2 = np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)
    covered_off = int(((dev["count"][0] > 0) & bed.off_grid(X2, Y2)).sum())
    print(f"{name}: {int((dev['count'] > 0).sum())} nodes covered, {covered_off} of them off the field grid")
    assert covered_off > 100
    for k in ("count", "T", "theta0", "theta", "ray", "step"):
        assert np.array_equal(dev[k], ref[k], equal_nan=True), k
    for k in ("cells", "skipped_cells", "triangles", "folded"):
        assert dev["stats"][k] == ref["stats"][k], k
    assert nan_relerr(dev["J"], ref["J"]) <= 1e-9 and nan_relerr(dev["G"], ref["G"]) <= 1e-9
    assert np.mean(dev["kmah"][dev["count"] > 0] == ref["kmah"][dev["count"] > 0]) > 0.999


# ---------------------------------------------------------------- 5. the constant medium's closed forms
# bounds about twice what the oracle gives on this bed: the angle's drift from the launch angle, and |T / (1.5 coef L) - 1|
ANGLE = {7: 5e-12, 9: 2e-5, 11: 2e-5}
TRAVEL = {9: 1e-11, 11: 5e-5}


@pytest.mark.parametrize("m", range(1, 12))
def test_constant_medium_closed_forms(rb, fields, m):
    bed = BEDS["const"]
    F = fields("const")
    x0, y0, th = bed.launches(333, 40 + m)
    b = batch(rb, F, "const", m, x0, y0, th)
    s, d = b.rows(), b.d_ray()
    last = d[2].astype(np.int64)
    R = len(th)
    ang, tb = ANGLE.get(m, 1e-15), TRAVEL.get(m, 2.5e-14)
    coef = S._coef(th, m, GAMMA.get(m, 1.0))
    L = np.zeros(R)
    for k in range(R):
        p = s[:last[k] + 1, :, k]
        dth = np.abs(np.angle(np.exp(1j * (p[:, 5] - th[k]))))
        L[k] = np.sum(np.hypot(np.diff(p[:, 0]), np.diff(p[:, 1])))
        dist = np.abs(-np.sin(th[k]) * (p[:, 0] - x0[k]) + np.cos(th[k]) * (p[:, 1] - y0[k]))
        assert dth.max() <= ang, (k, dth.max())
        assert dist.max() <= 2 * L[k] * ang + 1e-13, (k, dist.max())
        if L[k] > 0:
            assert abs(p[-1, 4] / (1.5 * coef[k] * L[k]) - 1.0) <= tb, (k, p[-1, 4] / (1.5 * coef[k] * L[k]) - 1.0)
    g = b.traveltime_backproject(w_end=np.ones(R))
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    M = S.matrices(s, last, ax, ay, method=m, gamma=GAMMA.get(m, 1.0))
    gr = S.backproject(M, np.ones(R)).reshape(Z.shape)
    assert np.max(np.abs(g - gr)) <= 1e-12 * np.max(gr)
    if m < 10:
        # A^T 1: every row's chord weights, and they sum to the chord lengths of all rays
        assert abs(g.sum() - L.sum()) <= 1e-12 * L.sum()
        par = b.paraxial()
        ok = L > 0
        assert np.max(np.abs(par["J"][ok] - L[ok]) / L[ok]) <= 1e-13                 # J = s in a homogeneous medium
        assert np.max(np.abs(par["G"][ok] * np.sqrt(1.5 * L[ok]) - 1.0)) <= 1e-13
        assert np.all(par["kmah"] == 0)
    b.close()
    # the grid table far off the field grid: T = 1.5 coef |p - s| (op10 / op11: the anisotropy factor along each ray)
    fth, xs, ys = bed.fan(4096, (0.5, 0.5))
    f = batch(rb, F, "const", m, xs, ys, fth, keep_n_ray=False)
    grid = (-2.9, 0.05, 131, -2.9, 0.07, 95)
    r = f.first_arrival_grid(grid)
    f.close()
    gx0, gdx, nx, gy0, gdy, ny = grid
    X2, Y2 = np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)
    Tc = 1.5 * np.hypot(X2 - xs, Y2 - ys) * S._coef(np.arctan2(Y2 - ys, X2 - xs), m, GAMMA.get(m, 1.0))
    ok = (r["count"][0] > 0) & bed.off_grid(X2, Y2) & (Tc > 0.3)
    err = np.max(np.abs(r["T"][0] - Tc)[ok] / Tc[ok])
    print(f"const op{m}: grid T off the field grid {err:.2e} over {ok.sum()} nodes")
    # linear interpolation across a fan cell of width dth: (dth^2 / 8) |d2T/dtheta2| / T, i.e. the anisotropy factor's own
    # curvature (max |coef''| / coef: 10.1 at gamma 0.3, 8.0 at gamma 3), on top of the isotropic bound
    tt, h = np.linspace(-np.pi, np.pi, 20001), 1e-4
    c = lambda t: S._coef(t, m, GAMMA.get(m, 1.0))                          # noqa: E731
    curv = np.max(np.abs(c(tt + h) - 2 * c(tt) + c(tt - h)) / (h * h) / c(tt))
    assert ok.sum() > 8000 and err <= 1e-6 + curv * (2 * np.pi / 4096) ** 2 / 8 + (0 if m not in (9, 11) else 2 * tb)
