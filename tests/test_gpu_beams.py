"""GPU: Gaussian beam summation (rtmi_gaussian_beams, Batch.gaussian_beams, rt_bench.beam_table).  The device against the numpy
restatement (tests/beam_ref.py) on the device's own rows; a constant medium against the Hankel function; vert_heterogeneous
against the library's ray-theory Green's function; the fisheye focus, where ray theory is infinite, and the caustic phase past
it; the same bits in every schedule, under ray sorting, twice in a row and in every source grouping; fp32 against fp64.  Bounds
are measurements on MI355X, recorded in DESIGN.md section 13.  Every restatement case here has a footprint wider than its grid
and the default cutoff, max_width and edge_taper; tests/test_gpu_beam_edges.py holds the device to the restatement where the
tiles, the caps, the cutoff, the frequency groups and the record's length decide something."""
import numpy as np
import pytest
from scipy.special import hankel1

import beam_ref as B
import paraxial_ref as P
from conftest import LIMITS
from sampled_beds import BEDS

pytestmark = pytest.mark.gpu


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
            if name in BEDS:
                x, y, Z, delta, _ = BEDS[name].fields()
                F = rb.Field.from_samples(x, y, Z, delta, dtype)
            else:
                F = rb.Field.build(name, LIMITS[name], rb.DELTA, dtype=dtype)
            cache[(name, dtype)] = (F, P.SplineField(*F.arrays()))
        return cache[(name, dtype)]
    yield get
    for F, _ in cache.values():
        F.close()


# name -> (step, max_size, box, source, fan (first, last), grid, omegas, eps)
SCEN = {
    "vert_heterogeneous": (None, 8.0, LIMITS["vert_heterogeneous"], (-2.0, -2.0), (0.05, np.pi / 2 - 0.05),
                           (-1.9, 0.1, 24, -2.4, 0.1, 24), (300.0, 700.0), 28.0),
    "fisheye": (2 * np.pi / 303, 121, LIMITS["fisheye"], (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4),
                (-1.2, 0.1, 24, -1.2, 0.1, 24), (60.0, 150.0), 4.0),
    "interface": (None, 8.0, LIMITS["interface"], (-2.0, -2.0), (0.1, np.pi / 2 - 0.1), (-1.9, 0.1, 24, -1.9, 0.1, 24),
                  (40.0, 90.0), 2.0),
    "rim8": (0.02, 200, BEDS["rim8"].box, (0.5, 1.5), (np.pi - 0.05, -np.pi + 0.05), (-1.0, 0.1, 24, 0.3, 0.1, 24),
             (40.0, 90.0), 1.0),
}


def setup(rb, name):
    step, ms, box, src, fan, grid, om, eps = SCEN[name]
    step = rb.DELTA_S if step is None else step
    ms = ms if isinstance(ms, int) else int(np.ceil(ms / step)) + 1
    return step, ms, box, src, fan, grid, om, eps


def batch(rb, F, name, m, R, S=1, dtype=None, **kw):
    step, ms, box, (x0, y0), (t0, t1), *_ = setup(rb, name)
    th = np.linspace(t0, t1, R)
    b = rb.Batch(F, rb.METHODS[m], step, ms, box, 1, np.tile(th, S), x0, y0, keep_n_ray=False, **kw)
    b.run()
    return b, np.tile(th, S)


def rel_to_max(a, b):
    """per source and frequency: max |a - b| / max |b|, the largest of them"""
    return max(float(np.max(np.abs(a[s, q] - b[s, q])) / np.max(np.abs(b[s, q])))
               for s in range(a.shape[0]) for q in range(a.shape[1]))


# ---------------------------------------------------------------- 1. the device against the restatement, same rows
CASES = [(s, m) for s in ("vert_heterogeneous", "fisheye", "interface", "rim8") for m in range(1, 10)]


@pytest.mark.parametrize("name,m", CASES)
def test_device_equals_the_restatement_on_the_same_rows(rb, fields, name, m):
    F, S = fields(name)
    *_, grid, om, eps = setup(rb, name)
    b, th = batch(rb, F, name, m, 64)
    u, st = b.gaussian_beams(grid, om, eps, stats=True)
    rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
    b.close()
    ref = B.gaussian_beams(rows, last, S, th, 64, grid, om, eps)
    err = rel_to_max(u, ref)
    print(f"{name} op{m}: {err:.2e} max|u| {np.abs(u).max():.3e} stats {st}")
    assert st["pairs_inside"] > 1000          # capped steps are fine: the restatement caps q_max the same way
    assert np.isfinite(u).all()
    assert err <= 1e-10


# ---------------------------------------------------------------- 2. a constant medium against the Hankel function
def test_constant_medium_matches_the_hankel_function(rb):
    ax = np.linspace(-4.0, 4.0, 81)
    F = rb.Field.from_samples(ax, ax, np.ones((81, 81)), 0.1)
    th = np.linspace(-0.6, np.pi / 2 + 0.6, 301)
    b = rb.Batch(F, rb.op1, rb.DELTA_S, int(np.ceil(6.0 / rb.DELTA_S)) + 1, (-4.0, 4.0, -4.0, 4.0), 1, th, 0.0, 0.0,
                 keep_n_ray=False)
    b.run()
    grid = (0.0, 0.1, 31, 0.0, 0.1, 31)
    X, Y = B.nodes(grid)
    r, a = np.hypot(X, Y), np.arctan2(Y, X)
    sel = (r >= 1.0) & (r <= 3.0) & (a >= 0.1) & (a <= np.pi / 2 - 0.1)
    worst = {}
    for omega, eps in ((200.0, 1.0), (800.0, 4.0)):
        u = b.gaussian_beams(grid, [omega], eps)[0, 0]
        ref = 0.25j * hankel1(0, omega * r[sel])
        worst[omega] = float(np.max(np.abs(u[sel] - ref) / np.abs(ref)))
    b.close(); F.close()
    print(f"constant medium: worst relative difference {worst}")
    assert worst[200.0] <= 1e-2 and worst[800.0] <= 1e-3


# ---------------------------------------------------------------- 3. vert_heterogeneous against ray theory
def test_vert_heterogeneous_matches_the_ray_theory_greens_function(rb, fields):
    F, _ = fields("vert_heterogeneous")
    n0 = float(F.n_gradient(-2.0, -2.0)[0][0])
    omega, eps = 2 * np.pi / (0.05 * n0), 4.0 / n0
    t0, t1 = 0.05, np.pi / 2 - 0.05
    box = LIMITS["vert_heterogeneous"]
    th = np.linspace(t0, t1, 257)
    b = rb.Batch(F, rb.op6, rb.DELTA_S, int(np.ceil(80 / rb.DELTA_S)) + 1, box, 1, th, -2.0, -2.0, keep_n_ray=False)
    b.run()
    grid = (-1.95, 0.05, 140, -2.45, 0.05, 70)
    u, st = b.gaussian_beams(grid, [omega], eps, stats=True)
    u = u[0, 0]
    tab = b.first_arrival_grid(grid, max_gap=0.4, amplitude=True)
    q1max = float(np.nanmax(np.abs(b.paraxial()["Q1"])))
    b.close()
    T, G, J, th0 = tab["T"][0], tab["G"][0], tab["J"][0], tab["theta0"][0]
    rt = B.ray_theory(T, G, 0.0, omega)
    X, Y = B.nodes(grid)
    aw = np.sqrt(2.0 / (omega * eps))                                  # the beam's angular width
    hw = np.sqrt(2.0 * ((J / n0) ** 2 + (eps * q1max) ** 2) / (omega * eps))   # half-width, with the largest Q1 of the fan
    edge = np.minimum.reduce([X - box[0], box[1] - X, Y - box[2], box[3] - Y])
    with np.errstate(invalid="ignore"):
        sel = ((tab["count"][0] == 1) & (omega * T >= 200.0) & (th0 >= t0 + 3 * aw) & (th0 <= t1 - 3 * aw) & (edge >= 3 * hw))
    err = np.abs(u[sel] - rt[sel]) / np.abs(rt[sel])
    med, p90 = float(np.median(err)), float(np.percentile(err, 90))
    print(f"vert_heterogeneous: omega {omega:.1f} eps {eps:.2f}: {sel.sum()} nodes, median {med:.3e}, p90 {p90:.3e}, "
          f"max {err.max():.3e}; stats {st}")
    assert sel.sum() > 500
    assert med <= 1e-2 and p90 <= 5e-2


# ---------------------------------------------------------------- 4. the fisheye focus
def test_fisheye_focus_is_finite_and_the_caustic_retards_the_phase(rb, fields):
    F, _ = fields("fisheye")
    eps, c0 = 4.0, np.pi / 2
    th = np.linspace(c0 - 0.35, c0 + 0.35, 141)
    # a quarter of the reference's fisheye step: at 2 pi / 303 the rows' own second-order error (the recorded spreading against
    # the rays' geometry) leaves a floor of ~0.9 % in both medians that does not fall with omega
    ms, tail = 1200, 160
    b = rb.Batch(F, rb.op6, 2 * np.pi / (4 * 303), ms, LIMITS["fisheye"], 1, th, 1.0, 0.0, keep_n_ray=False)
    b.run()
    grid = (-1.45, 0.025, 117, -1.45, 0.025, 117)
    tab = b.first_arrival_grid(grid, max_gap=0.4, amplitude=True)
    X, Y = B.nodes(grid)
    d_src, d_foc = np.hypot(X - 1.0, Y), np.hypot(X + 1.0, Y)
    res = {}
    for omega in (400.0, 1600.0):
        u = b.gaussian_beams(grid, [omega], eps)[0, 0]
        assert np.isfinite(u).all()
        aw = np.sqrt(2.0 / (omega * eps))
        T, G, th0, step = tab["T"][0], tab["G"][0], tab["theta0"][0], tab["step"][0]
        with np.errstate(invalid="ignore"):
            ok = ((tab["count"][0] == 1) & (th0 >= c0 - 0.35 + 3 * aw) & (th0 <= c0 + 0.35 - 3 * aw) & (d_src > 0.3) &
                  (d_foc > 0.3) & (step <= ms - 1 - tail))
        before, after = ok & (Y > 0), ok & (Y < 0)
        rel = lambda sel, k: np.abs(u[sel] - B.ray_theory(T[sel], G[sel], k, omega)) / np.abs(B.ray_theory(T[sel], G[sel], k, omega))
        res[omega] = (float(np.median(rel(before, 0))), float(np.median(rel(after, 1))), float(np.median(rel(after, 0))),
                      int(before.sum()), int(after.sum()))
        away = np.where(d_src > 0.3, np.abs(u), 0.0)
        iy, ix = np.unravel_index(np.argmax(away), away.shape)
        res[omega] += (float(X[iy, ix]), float(Y[iy, ix]))
    b.close()
    print(f"fisheye: omega -> (median before, after kmah 1, after kmah 0, nodes before, after, peak x, y): {res}")
    mb, ma, m0, nb, na, px, py = res[1600.0]
    assert nb > 200 and na > 200
    assert np.hypot(px + 1.0, py) <= 0.025 * 1.0001
    assert mb <= 1e-2 and ma <= 0.1 and m0 >= 1.0
    assert res[400.0][0] >= 2 * mb and res[400.0][1] >= 2 * ma


# ---------------------------------------------------------------- 5. the same bits everywhere
def test_same_bits_in_every_schedule_sorting_rerun_and_grouping(rb, fields):
    F, _ = fields("vert_heterogeneous")
    step, ms, box, _, (t0, t1), grid, om, eps = setup(rb, "vert_heterogeneous")
    th = np.linspace(t0, t1, 64)
    src = np.array([(-2.0, -2.0), (-1.5, -2.2), (-1.0, -1.8)])
    S, M = len(src), len(th)
    ref = None
    for mode in ("auto", "refill", "sliced", "plain"):
        for sort in (False, True):
            b = rb.Batch(F, rb.op6, step, ms, box, 1, np.tile(th, S), np.repeat(src[:, 0], M), np.repeat(src[:, 1], M),
                         keep_n_ray=False, launch_mode=mode, sort_rays=sort)
            b.run()
            for _ in range(2):
                u = b.gaussian_beams(grid, om, eps, fan_size=M)
                if ref is None:
                    ref = u
                assert np.array_equal(u.view(np.float64), ref.view(np.float64)), (mode, sort)
            b.close()
    for budget in (0, 1):                       # one group; one source per group
        u = rb.beam_table(rb.op6, F, src, grid, om, thetas=th, eps=eps, step=step, max_size=ms, box=box, mem_budget=budget)
        assert np.array_equal(u.view(np.float64), ref.view(np.float64)), budget
    assert np.abs(ref).max() > 0


# ---------------------------------------------------------------- 6. fp32 records
def test_fp32_against_fp64(rb, fields):
    out = []
    for dt in (0, 1):
        F, _ = fields("vert_heterogeneous", dt)
        *_, grid, om, eps = setup(rb, "vert_heterogeneous")
        b, _ = batch(rb, F, "vert_heterogeneous", 6, 128)
        out.append(b.gaussian_beams(grid, om, eps))
        b.close()
    err = rel_to_max(out[1], out[0])
    print(f"fp32 against fp64: {err:.3e}")
    assert err <= 1e-2


# ---------------------------------------------------------------- the batch rules
def test_batch_rules(rb, fields):
    from raytracing_amd import _lib
    F, _ = fields("vert_heterogeneous")
    step, ms, box, (x0, y0), (t0, t1), grid, om, eps = setup(rb, "vert_heterogeneous")
    th = np.linspace(t0, t1, 16)
    b = rb.Batch(F, rb.op6, step, ms, box, 1, th[::-1], x0, y0, keep_n_ray=False)      # decreasing angles are monotone too
    b.run()
    assert np.isfinite(b.gaussian_beams(grid, om, eps)).all()
    with pytest.raises(_lib.RtmiError) as e:
        b.gaussian_beams(grid, om, eps, fan_size=3)
    assert e.value.code == -1
    b.close()
    b = rb.Batch(F, rb.op6, step, ms, box, 1, np.r_[th[:8], th[7:15]], x0, y0, keep_n_ray=False)
    b.run()
    with pytest.raises(_lib.RtmiError, match="monotone") as e:
        b.gaussian_beams(grid, om, eps)
    assert e.value.code == -1
    b.close()
    b = rb.Batch(F, rb.op10, step, ms, box, 1, th, x0, y0, keep_n_ray=False)
    b.run()
    with pytest.raises(_lib.RtmiError) as e:
        b.gaussian_beams(grid, om, eps)
    assert e.value.code == -1
    b.close()
    b = rb.Batch(F, rb.op6, step, ms, box, 1, th, x0, y0, keep_n_ray=False)
    b.step(3)
    st9 = b.get_state()[0]
    b.set_state(st9, istep=np.full(16, 3, dtype=np.int32))
    with pytest.raises(_lib.RtmiError) as e:
        b.gaussian_beams(grid, om, eps)
    assert e.value.code == -4
    b.close()
