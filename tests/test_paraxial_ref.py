"""CPU: the numpy restatement of rtmi_paraxial (tests/paraxial_ref.py) on the oracle's trajectories, against what the
mathematics says: a homogeneous medium, the circular rays of vert_heterogeneous (closed form), the foci of the fisheye, and
the symplectic invariant.  No GPU involved; these validate the propagator before the device is compared with it."""
import numpy as np
import pytest

import crossing_ref as X
import paraxial_ref as P
from conftest import LIMITS

SIGMA = 0.05293304824724534
DELTA = SIGMA / 3
DELTA_S = SIGMA / 20
VERT = LIMITS["vert_heterogeneous"]
FISH = LIMITS["fisheye"]


def genz_axes(lim):
    xi, xs, yi, ys = lim
    qx, qy = int((xs - xi + 6) / DELTA + 1), int((ys - yi + 6) / DELTA + 1)
    return np.linspace(xi - 3, xs + 3, qx), np.linspace(yi - 3, ys + 3, qy)


def trace(F, m, step, max_size, box, x0, y0, th):
    from oracle import rt_oracle as O
    o = O.trazar(F, m, 1, step, max_size, box, x0, y0, th, record_stride=1, nthreads=8)
    return o["s_ray"], o["d_ray"][2].astype(np.int64)


def test_homogeneous_medium_spreads_linearly():
    from oracle import rt_oracle as O
    x, y = genz_axes(VERT)
    n = 1.37
    F = O.Field.from_samples(x, y, np.full((len(y), len(x)), n), DELTA)
    th = np.linspace(0.1, 1.4, 7)
    s, last = trace(F, 6, DELTA_S, 600, VERT, -2.0, -2.0, th)
    S = P.SplineField(*F.arrays())
    cnt, _, end = P.paraxial(s, last, S)
    r = np.arange(len(th))
    arc = np.array([np.sum(np.hypot(np.diff(s[:last[k] + 1, 0, k]), np.diff(s[:last[k] + 1, 1, k]))) for k in r])
    assert np.all(last > 100)
    assert np.max(np.abs(end[4] - arc) / arc) <= 1e-13          # J = s, to the rounding of ~600 sums
    assert np.max(np.abs(end[3] - 1.0)) <= 1e-15                # P2 = 1
    assert np.max(np.abs(end[0] - 1.0)) <= 1e-15 and np.max(np.abs(end[1])) <= 1e-15
    assert np.all(end[6] == 0)
    assert np.max(np.abs(end[5] - 1.0 / np.sqrt(n * arc)) * np.sqrt(n * arc)) <= 1e-13


@pytest.mark.parametrize("div", [1, 2])
def test_vert_heterogeneous_op6_against_the_closed_form(div):
    """The bound is the traced rays' own distance from the exact circles (up to 3.4e-4 of the radius): the
    field is a fit of samples, and the rays it gives are not the exact arcs.  It does not shrink with DELTA_S."""
    from oracle import rt_oracle as O
    F = O.Field("vert_heterogeneous", VERT, DELTA)
    step = DELTA_S / div
    th = np.linspace(0.05, 1.5, 16)
    s, last = trace(F, 6, step, int(np.ceil(80 / step) + 1), VERT, -2.0, -2.0, th)
    S = P.SplineField(*F.arrays())
    line = (1.0, 0.0, 4.0)
    cnt, atl, end = P.paraxial(s, last, S, line=line, kmax=2)
    r = np.arange(len(th))
    Jc = P.vert_closed_form(th, s[last, 0, r], s[last, 1, r])
    assert np.max(np.abs(np.abs(end[4]) - Jc)) / np.max(Jc) <= 5e-4
    c2, out = X.crossings(s, last, line, 2)
    assert np.array_equal(c2, cnt)
    ok = cnt > 0
    assert ok.sum() >= 5
    Jl = P.vert_closed_form(th, out[0, 1], out[0, 2])
    assert np.max(np.abs(np.abs(atl[0, 4]) - Jl)[ok]) / np.max(Jl[ok]) <= 5e-4
    assert np.all(end[6] == 0)                                  # no caustic on a circle that stays below its top


def test_fisheye_kmah_counts_the_foci():
    from oracle import rt_oracle as O
    F = O.Field("fisheye", FISH, DELTA)
    step = 2 * np.pi / 303
    th = np.linspace(np.pi / 2 - 0.35, np.pi / 2 + 0.35, 15)
    s, last = trace(F, 6, step, 10 * 304, FISH, 1.0, 0.0, th)
    S = P.SplineField(*F.arrays())
    cnt, atl, end = P.paraxial(s, last, S, line=(1.0, 0.0, 0.0), kmax=4)
    assert np.all(cnt >= 3)
    for m in range(3):
        assert np.all(atl[m, 6] == m), m
        # J changes sign at each focus between two crossings of x = 0
        assert np.all(np.sign(atl[m, 4]) == (-1) ** m), m
    assert np.all(end[6] >= 3)


@pytest.mark.parametrize("scen,m", [("vert_heterogeneous", 6), ("fisheye", 6), ("interface", 6), ("interface", 3)])
def test_tube_matrix_has_determinant_one(scen, m):
    from oracle import rt_oracle as O
    F = O.Field(scen, LIMITS[scen], DELTA)
    if scen == "fisheye":
        s, last = trace(F, m, 2 * np.pi / 303, 10 * 304, FISH, 1.0, 0.0, np.linspace(np.pi / 2 - 0.4, np.pi / 2 + 0.4, 9))
    else:
        s, last = trace(F, m, DELTA_S, int(np.ceil(80 / DELTA_S) + 1), LIMITS[scen], -2.0, -2.0,
                        np.linspace(0.05, 1.5 if scen != "interface" else np.pi / 2, 9))
    _, atl, end = P.paraxial(s, last, P.SplineField(*F.arrays()), line=(0.0, 1.0, 0.5), kmax=2)
    det = end[0] * end[3] - end[2] * end[1]
    assert np.max(np.abs(det - 1.0)) <= 1e-12
    d2 = atl[:, 0] * atl[:, 3] - atl[:, 2] * atl[:, 1]
    assert np.nanmax(np.abs(d2 - 1.0)) <= 1e-12
