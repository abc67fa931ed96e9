"""GPU: x-invariant ("layered") fields -- media whose samples depend on y alone (include/rtmi.h, rtmi_field_layered).  The field
build's detection; the rule the fast-form fp64 step kernels look such a field up by (the row alone: rtmi_debug_field_lookup_layered)
against the general lookup (the cell's polynomial: rtmi_debug_field_lookup); one result per field whichever schedule, flavour or
field path runs the batch; and those runs against the oracle."""
import numpy as np
import pytest

from conftest import LIMITS
from test_gpu_parity import REL, relerr

pytestmark = pytest.mark.gpu

R = 700                        # two full 256-ray bundles and a partial one; 11 waves: a plain op6 run is the few-waves kernel


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


def small_samples():
    """Z = f(y) on a 16 x 24 grid: a smooth v(z)-style profile"""
    x = np.linspace(-1.0, 2.0, 16); y = np.linspace(0.5, 2.5, 24)
    fy = 1.0 / (1.0 + 0.4 * y + 0.1 * np.sin(2.0 * y))
    Z = np.repeat(fy[:, None], len(x), axis=1)
    delta = 0.5 * ((x[1] - x[0]) + (y[1] - y[0]))
    return x, y, Z, delta


class Case:
    def __init__(self, name, field, ofield, step, max_size, box, x0, y0, th):
        self.name, self.field, self.ofield = name, field, ofield
        self.step, self.max_size, self.box, self.x0, self.y0, self.th = step, max_size, box, x0, y0, th
        self._oracle, self._plain = {}, {}


@pytest.fixture(scope="module")
def cases(rb, oracle_fields):
    from oracle import rt_oracle as O
    x, y, Z, delta = small_samples()
    Fs = rb.Field.from_samples(x, y, Z, delta)
    # the box reaches 0.01 past the grid's rim on every side: the last lookups of a ray that leaves are clamped (quirk Q4);
    # a fan from inside the grid in every direction, 150 rows: rays along the long side are truncated
    small = Case("16x24", Fs, O.Field.from_samples(x, y, Z, delta), 0.01, 150, (x[0] - 0.01, x[-1] + 0.01, y[0] - 0.01, y[-1] + 0.01),
                 0.4, 1.3, np.pi - (np.arange(R) + 0.5) * (2.0 * np.pi / R))
    Fv = rb.Field.build("vert_heterogeneous")
    lim = LIMITS["vert_heterogeneous"]
    vert = Case("vert_heterogeneous", Fv, oracle_fields("vert_heterogeneous"), 4 * rb.DELTA_S, 900, lim, -2.0, -2.0,
                np.linspace(0, np.pi / 2, R))
    yield {"16x24": small, "vert_heterogeneous": vert}
    Fs.close(); Fv.close()


def plain(rb, c, m):
    """the plain run of case c with op m -> (rows, d_ray, final), computed once"""
    if m not in c._plain:
        c._plain[m] = trace(rb, c, m, "plain")
    return c._plain[m]


def trace(rb, c, m, how):
    kw = dict(launch_mode="plain")
    if how == "sliced":
        kw = dict(launch_mode="sliced", slice_steps=64)
    elif how == "refill":
        kw = dict(launch_mode="refill")
    elif how == "global":
        kw = dict(launch_mode="plain", field_path=1)
    b = rb.Batch(c.field, rb.METHODS[m], c.step, c.max_size, c.box, 1, c.th, c.x0, c.y0, **kw)
    if how == "per_ray":
        b.set_per_ray(c.step, c.max_size)
    if how == "stepped":
        for _ in range(c.max_size - 1):
            b.step(1)
        b.sync()
    else:
        b.run()
    out = (b.rows(), b.d_ray(), b.final())
    if how in ("plain", "sliced", "refill"):
        assert b.stats()["launch_mode_used"] == how
    b.close()
    return out


# ---------------------------------------------------------------- 1. selection
def test_selection(rb):
    x, y, Z, delta = small_samples()

    def layered(x, y, Z):
        F = rb.Field.from_samples(x, y, Z, delta)
        v = F.layered
        F.close()
        return v

    assert layered(x, y, Z) == 1
    Zb = Z.copy()
    Zb.view(np.uint64)[7, 5] ^= np.uint64(1)                 # one value's last bit
    assert layered(x, y, Zb) == 0
    xs = np.linspace(0.5, 2.5, 24); ys = np.linspace(-1.0, 2.0, 16)
    fx = 1.0 / (1.0 + 0.4 * xs + 0.1 * np.sin(2.0 * xs))
    assert layered(xs, ys, np.repeat(fx[None, :], len(ys), axis=0)) == 0         # Z = f(x): y-invariant media are out of scope
    for scen, want in (("vert_heterogeneous", 1), ("fisheye", 0), ("interface", 0)):
        F = rb.Field.build(scen)
        assert F.layered == want, scen
        if not want:
            with pytest.raises(Exception):
                F.lookup_layered([0.0], [0.0])
        F.close()


# ---------------------------------------------------------------- 2. the rule against the general lookup
def lookup_points(x, y, N=20000, seed=3):
    """inside the grid, on grid lines of either axis, in the rim cells (corners and the grid's own corners included), and up
    to 0.3 outside the grid on both axes"""
    rng = np.random.default_rng(seed)
    k = N // 5
    rim = lambda a: np.where(rng.random(k) < 0.5, rng.uniform(a[0], a[2], k), rng.uniform(a[-3], a[-1], k))      # noqa: E731
    px = [rng.uniform(x[0], x[-1], k), rng.choice(x, k), rng.uniform(x[0], x[-1], k), rim(x)]
    py = [rng.uniform(y[0], y[-1], k), rng.uniform(y[0], y[-1], k), rng.choice(y, k), rim(y)]
    cx, cy = np.meshgrid(x[[0, 1, -2, -1]], y[[0, 1, -2, -1]])
    px.append(cx.ravel()); py.append(cy.ravel())
    rest = N - 4 * k - cx.size
    px.append(rng.uniform(x[0] - 0.3, x[-1] + 0.3, rest)); py.append(rng.uniform(y[0] - 0.3, y[-1] + 0.3, rest))
    return np.concatenate(px), np.concatenate(py)


@pytest.mark.parametrize("name", ["vert_heterogeneous", "16x24"])
def test_rule_against_the_general_lookup(rb, cases, name):
    """Measured on MI355X (differences relative to max |Z| and to the largest gradient-spline coefficient): see DESIGN.md 5.1.1."""
    F = cases[name].field
    x, y, Z, cdy, cdx = F.arrays()
    px, py = lookup_points(x, y)
    assert len(px) == 20000
    n1, gx1, gy1 = F.lookup_layered(px, py)
    n0, gx0, gy0 = F.lookup_fast(px, py)
    nscale, gscale = np.abs(Z).max(), max(np.abs(cdx).max(), np.abs(cdy).max())
    en, ex, ey = np.abs(n1 - n0).max() / nscale, np.abs(gx1 - gx0).max() / gscale, np.abs(gy1 - gy0).max() / gscale
    print(f"{name}: layered rule vs general lookup on {len(px)} points: n {en:.2e}, dn/dx {ex:.2e}, dn/dy {ey:.2e}")
    assert np.all(gx1.view(np.uint64) == 0)                  # dn/dx = +0
    assert en < 1e-13 and ex < 1e-13 and ey < 1e-13


# ---------------------------------------------------------------- 3. one result per field, and the oracle
HOWS = ["sliced", "refill", "global", "per_ray", "stepped"]


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("m", [6, 1])
@pytest.mark.parametrize("name", ["16x24", "vert_heterogeneous"])
def test_one_result_per_field(rb, cases, name, m, how):
    c = cases[name]
    rows0, d0, fin0 = plain(rb, c, m)
    rows, d, fin = trace(rb, c, m, how)
    assert np.array_equal(d, d0), np.flatnonzero(d[2] != d0[2])[:8]
    assert np.array_equal(fin, fin0)
    assert np.array_equal(rows, rows0)


@pytest.mark.parametrize("m", [6, 1])
@pytest.mark.parametrize("name", ["16x24", "vert_heterogeneous"])
def test_against_the_oracle(rb, cases, name, m):
    from oracle import rt_oracle as O
    c = cases[name]
    rows, d, fin = plain(rb, c, m)
    o = O.trazar(c.ofield, m, 1, c.step, c.max_size, c.box, c.x0, c.y0, c.th, record_stride=1, nthreads=16)
    bad = np.flatnonzero(d[2] != o["d_ray"][2])
    assert bad.size == 0, f"step counts differ on rays {bad[:8]}"
    err = max(relerr(fin, o["final"]), relerr(d[:2], o["d_ray"][:2]), relerr(rows, o["s_ray"]))
    trunc = int(np.sum(d[2] == c.max_size - 1))
    x, y = c.field.arrays()[:2]
    live = np.arange(rows.shape[0])[:, None] <= d[2][None, :]
    off = int((((rows[:, 0] < x[0]) | (rows[:, 0] > x[-1]) | (rows[:, 1] < y[0]) | (rows[:, 1] > y[-1])) & live).sum())
    print(f"{name} op{m}: largest relative error against the oracle {err:.2e}; {trunc} rays truncated, {off} rows off the grid")
    assert err < REL
    if name == "16x24":
        assert off > 0 and trunc > 0
