"""CPU: the oracle and the numpy restatements on caller-sampled beds (tests/sampled_beds.py), where rows lie in the rim cells
and off the grid: the oracle's lookup against scipy at the clamped arguments, A Z = T and A 1 = chord sums of
tests/sensitivity_ref.py for op1..op11, the tube matrix's determinant, the grid table of a constant medium against its closed
form, and the spreading across the grid's edge against finite differences of neighbouring rays.  No GPU involved; the device
tests (tests/test_gpu_sampled_fields.py) lean on these."""
import functools

import numpy as np
import pytest

import crossing_ref as X
import paraxial_ref as P
import sensitivity_ref as S
import ttgrid_ref as G
from sampled_beds import BEDS

GAMMA = {10: 0.3, 11: 3.0}


@functools.lru_cache(maxsize=None)
def oracle_field(name):
    from oracle import rt_oracle as O
    x, y, Z, delta, _ = BEDS[name].fields()
    return O.Field.from_samples(x, y, Z, delta)


def trace(name, m, R=333, seed=7):
    from oracle import rt_oracle as O
    bed = BEDS[name]
    x0, y0, th = bed.launches(R, seed)
    o = O.trazar(oracle_field(name), m, GAMMA.get(m, 1.0), bed.step, bed.max_size, bed.box, x0, y0, th, record_stride=1,
                 nthreads=16)
    return o, o["d_ray"][2].astype(np.int64)


@pytest.mark.parametrize("name", sorted(BEDS))
def test_oracle_lookup_clamps_like_scipy(name):
    bed = BEDS[name]
    OF = oracle_field(name)
    rng = np.random.default_rng(5)
    xi, xs, yi, ys = bed.box
    x, y = bed.x, bed.y
    px = np.r_[rng.uniform(xi, xs, 10000), rng.uniform(x[0] - 0.3, x[-1] + 0.3, 10000)]
    py = np.r_[rng.uniform(yi, ys, 10000), rng.uniform(y[0] - 0.3, y[-1] + 0.3, 10000)]
    off, rim = bed.off_grid(px, py), bed.in_rim(px, py)
    assert off.sum() > 1000 and rim.sum() > 1000
    ref = P.SplineField(*OF.arrays())(px, py)[:3]
    got = OF.n_gradient(px, py)
    for q, (a, b) in enumerate(zip(got, ref)):
        scale = max(np.max(np.abs(b)), 1.0)
        assert np.max(np.abs(a - b)) <= 1e-13 * scale, q


@pytest.mark.parametrize("m", range(1, 12))
@pytest.mark.parametrize("name", sorted(BEDS))
def test_A_Z_and_A_1_on_the_beds(name, m):
    bed = BEDS[name]
    o, last = trace(name, m)
    s = o["s_ray"]
    off, rim = bed.edge_counts(s, last)
    assert off > 1000 and rim > 500
    assert np.any(last == bed.max_size - 1)                              # some rays truncated
    x, y, Z = oracle_field(name).arrays()[:3]
    ax, ay = S.axes(x, y)
    M = S.matrices(s, last, ax, ay, line=bed.line, kmax=4, method=m, gamma=GAMMA.get(m, 1.0))
    d = S.perturb(M, Z)
    R = s.shape[2]
    T = s[last, 4, np.arange(R)]
    assert np.max(np.abs(d["end"] - T)) <= 1e-12 * np.max(np.abs(T))
    ok = np.isfinite(d["line"])
    assert ok.sum() >= 50
    Tl = M["crossings"][:, 3]
    assert np.array_equal(ok, np.isfinite(Tl))
    assert np.max(np.abs(d["line"][ok] - Tl[ok])) <= 1e-12 * np.max(np.abs(Tl[ok]))
    if m < 10:
        chord = o["d_ray"][1]
        assert np.max(np.abs(S.perturb(M, np.ones_like(Z))["end"] - chord)) <= 1e-12 * np.max(chord)


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("name", sorted(BEDS))
def test_tube_matrix_has_determinant_one(name, m):
    bed = BEDS[name]
    o, last = trace(name, m)
    _, atl, end = P.paraxial(o["s_ray"], last, P.SplineField(*oracle_field(name).arrays()), line=bed.line, kmax=2)
    det = end[0] * end[3] - end[2] * end[1]
    assert np.max(np.abs(det - 1.0)) <= 1e-12
    d2 = atl[:, 0] * atl[:, 3] - atl[:, 2] * atl[:, 1]
    assert np.isfinite(d2).sum() >= 50 and np.nanmax(np.abs(d2 - 1.0)) <= 1e-12


CONST_GRID = (-2.9, 0.05, 131, -2.9, 0.07, 95)          # runs far past the field grid [0, 1]^2; hx != hy


def test_const_grid_table_is_the_distance_off_the_field_grid():
    """T = 1.5 |p - s| from a 4 096-ray fan; the bound is test_fisheye_matches_the_great_circle_arc's (1.5 x the rows' own
    error + 1e-6: the linear interpolation across the fan's cells)."""
    from oracle import rt_oracle as O
    bed = BEDS["const"]
    th, xs, ys = bed.fan(4096, (0.5, 0.5))
    o = O.trazar(oracle_field("const"), 6, 1, bed.step, 400, bed.box, xs, ys, th, record_stride=1, nthreads=16)
    s, last = o["s_ray"], o["d_ray"][2].astype(np.int64)
    r = G.from_record(s, last, CONST_GRID)
    gx0, gdx, nx, gy0, gdy, ny = CONST_GRID
    X2, Y2 = np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)
    Tc = 1.5 * np.hypot(X2 - xs, Y2 - ys)
    ok = (r["count"][0] > 0) & bed.off_grid(X2, Y2) & (Tc > 0.3)
    assert ok.sum() > 8000
    live = np.arange(s.shape[0])[:, None] <= last[None, :]
    Tr = 1.5 * np.hypot(s[:, 0] - xs, s[:, 1] - ys)
    m = live & (Tr > 0.3)
    rerr = np.max(np.abs(s[:, 4] - Tr)[m] / Tr[m])
    err = np.max(np.abs(r["T"][0] - Tc)[ok] / Tc[ok])
    print(f"const grid rel err {err:.2e} (rows {rerr:.2e}), {ok.sum()} nodes off the field grid")
    assert err <= 1.5 * rerr + 1e-6


# ---------------------------------------------------------------- spreading across the grid's edge
H = 1e-5


def spread_field(kind, ext):
    """hx = hy = delta = 0.05 (np.gradient's spacing is the grid's: no g / grad n offset on the grid).  'samples' is the field of
    test_dgrad_equals_scipys_derivatives_of_the_fits; 'plateau' the same with y frozen above y = 1, so that its last ten rows of
    samples are equal along y and past the top edge the clamped field is consistent (g = grad n).  ext = 1 carries the grid on
    to y = 3.5 with the same formula."""
    x = -1.0 + 0.05 * np.arange(61)
    y = -0.5 + 0.05 * np.arange(41 + 40 * ext)
    X2, Y2 = np.meshgrid(x, y)
    Yc = np.minimum(Y2, 1.0) if kind == "plateau" else Y2
    return x, y, 1.0 + 0.3 * np.sin(2 * X2) * np.cos(3 * Yc) + 0.1 * X2 * Yc, 0.05


@functools.lru_cache(maxsize=None)
def spread_trace(kind, ext, R=512):
    from oracle import rt_oracle as O
    x, y, Z, delta = spread_field(kind, ext)
    F = O.Field.from_samples(x, y, Z, delta)
    th = np.linspace(np.pi / 2 - 0.5, np.pi / 2 + 0.5, R)
    o = O.trazar(F, 6, 1, 0.005, 2000, (-3.0, 4.0, -0.49, 3.5), 0.5, -0.4, np.concatenate([th, th + H, th - H]),
                 record_stride=1, nthreads=16)
    return P.SplineField(*F.arrays()), o["s_ray"], o["d_ray"][2].astype(np.int64)


def spread_errors(kind, ext, yline, R=512):
    """|du/dtheta0 - J / (n.t)| / max |J / (n.t)| at the first crossing of y = yline (op6, a fan from (0.5, -0.4))"""
    Sf, s, last = spread_trace(kind, ext)
    line = (0.0, 1.0, yline)
    _, atl, _ = P.paraxial(s[:, :, :R], last[:R], Sf, line=line, kmax=1)
    c, cr = X.crossings(s, last, line, 1)
    c, u = c.reshape(3, R), cr[0, 0].reshape(3, R)
    nt = np.sin(cr[0, 4][:R])
    pred = atl[0, 4] / nt
    keep = (c.min(axis=0) >= 1) & (np.abs(nt) > 0.2)
    return np.abs((u[1] - u[2]) / (2 * H) - pred)[keep] / np.max(np.abs(pred[keep]))


# line -> (samples clamped, plateau clamped): measured (median, max)
SPREAD = {2.5: ((2.14e-2, 0.186), (1.34e-4, 0.136)), 3.0: ((2.66e-2, 0.326), (1.01e-3, 0.167))}


@pytest.mark.parametrize("yline", sorted(SPREAD))
def test_spreading_past_the_grid_edge(yline):
    """Receiver lines 1 and 1.5 units past the top of the grid (y = 1.5), each field traced on its grid (the lines off it: the
    lookup clamps y) and on the grid carried on to y = 3.5 (the lines on it).  Measured (median, max):

      field    line   clamped           carried on
      samples  2.5    2.1e-2, 0.19      4.3e-5, 7.2e-2
      samples  3.0    2.7e-2, 0.33      7.4e-5, 3.4e-2
      plateau  2.5    1.3e-4, 0.14      1.3e-4, 0.14
      plateau  3.0    1.0e-3, 0.17      1.0e-3, 0.17
      (both, inside at y = 0.9: 2.8e-4, 5.3e-4)

    Past the edge the clamped 'samples' field freezes n along y while its frozen dn/dy fit still bends the rays: g is not
    grad n there, and the paraxial system assumes g = grad n.  'plateau' differs from it only in that g = grad n
    holds at the edge (its samples stop varying in y below it): there the clamped run is the carried-on one and the gap is gone.
    The propagator and the restatement's clamp are the same in both runs; what opens the gap is the clamped medium.  The
    remaining maxima of 'plateau' come with its own kink at y = 1, clamped or not.  Bounds: about twice the measured values."""
    (sm, sx), (pm, px) = SPREAD[yline]
    inside = spread_errors("samples", 0, 0.9)
    assert np.median(inside) <= 6e-4 and inside.max() <= 1.1e-3
    samples, plateau = spread_errors("samples", 0, yline), spread_errors("plateau", 0, yline)
    carried = {k: spread_errors(k, 1, yline) for k in ("samples", "plateau")}
    print(f"y = {yline}: samples clamped {np.median(samples):.2e} / {samples.max():.2e}, carried on "
          f"{np.median(carried['samples']):.2e} / {carried['samples'].max():.2e}; plateau clamped {np.median(plateau):.2e} / "
          f"{plateau.max():.2e}, carried on {np.median(carried['plateau']):.2e} / {carried['plateau'].max():.2e}")
    assert len(samples) >= 300 and len(plateau) >= 300
    assert np.median(samples) <= 2 * sm and samples.max() <= 2 * sx
    assert np.median(plateau) <= 2 * pm and plateau.max() <= 2 * px
    assert np.median(carried["samples"]) <= 2e-4
    # consistent at the edge: the clamp changes nothing; inconsistent: the median is 20x and more above it
    assert abs(np.median(plateau) - np.median(carried["plateau"])) <= 0.01 * np.median(carried["plateau"])
    assert np.median(samples) >= 20 * np.median(plateau)
