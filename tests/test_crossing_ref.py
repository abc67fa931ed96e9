"""CPU: the numpy restatement of rtmi_crossings (tests/crossing_ref.py) against exact geometry and its edge cases, and the
argument errors of rtmi_crossings / rtmi_two_point, which are reported before any device work."""
import ctypes as C

import numpy as np
import pytest

import crossing_ref as X
from raytracing_amd import _lib


def circle_rows(rho, phi, n=1.0):
    """Rows of a ray running counter-clockwise on the circle of radius rho about the origin in a medium of index n: exact
    positions, angles and momenta; T = n * arclength."""
    s = np.zeros((len(phi), 6, 1))
    s[:, 0, 0] = rho * np.cos(phi)
    s[:, 1, 0] = rho * np.sin(phi)
    th = phi + np.pi / 2
    s[:, 2, 0] = n * np.cos(th)
    s[:, 3, 0] = n * np.sin(th)
    s[:, 4, 0] = n * rho * (phi - phi[0])
    s[:, 5, 0] = th
    return s


def rows_of(points, thetas, T=None):
    """[rows, 6, 1] from explicit points and angles (unit momentum along the angle)."""
    p = np.asarray(points, dtype=np.float64)
    th = np.asarray(thetas, dtype=np.float64)
    s = np.zeros((len(p), 6, 1))
    s[:, 0, 0], s[:, 1, 0] = p[:, 0], p[:, 1]
    s[:, 2, 0], s[:, 3, 0] = np.cos(th), np.sin(th)
    s[:, 4, 0] = np.arange(len(p), dtype=np.float64) if T is None else T
    s[:, 5, 0] = th
    return s


@pytest.mark.parametrize("c", [0.3, -0.55, 0.8])
def test_circle_crossing_matches_the_exact_intersection(c):
    rho, n = 1.3, 1.7
    phi = np.arange(0, 3.0, 2e-3) - 0.1           # from just below the x axis, counter-clockwise past pi/2
    s = circle_rows(rho, phi, n)
    cnt, out = X.crossings(s, [len(phi) - 1], (1.0, 0.0, c), kmax=2)
    assert cnt[0] == 1                             # x = c is crossed once, going left (x decreasing)
    yx = np.sqrt(rho * rho - c * c)
    d = X.as_dict(cnt, out)
    assert abs(d["x"][0, 0] - c) <= 1e-12 and abs(d["y"][0, 0] - yx) <= 1e-12
    assert abs(d["u"][0, 0] - yx) <= 1e-12         # u = a' y - b' x with (a', b') = (1, 0)
    phic = np.arctan2(yx, c)
    assert abs(d["T"][0, 0] - n * rho * (phic - phi[0])) <= 1e-12
    dth = d["theta"][0, 0] - (phic + np.pi / 2)
    assert abs(np.arctan2(np.sin(dth), np.cos(dth))) <= 1e-9        # atan2's range: the same direction modulo 2 pi
    i = int(d["s"][0, 0])
    assert phi[i] <= phic <= phi[i + 1]


def test_oblique_line_on_a_circle():
    rho = 2.0
    phi = np.arange(0, 6.25, 1e-3)                 # crosses at phi = 2.336 and 6.161
    s = circle_rows(rho, phi)
    a, b, c = 1.0, 2.0, 1.5                        # x + 2 y = 1.5, normalised by sqrt(5)
    cnt, out = X.crossings(s, [len(phi) - 1], (a, b, c), kmax=4)
    assert cnt[0] == 2
    d = X.as_dict(cnt, out)
    for k in range(2):
        x, y = d["x"][k, 0], d["y"][k, 0]
        assert abs(x * x + y * y - rho * rho) <= 1e-11
        assert abs((a * x + b * y - c) / np.sqrt(5.0)) <= 1e-12
        assert abs(d["u"][k, 0] - (a * y - b * x) / np.sqrt(5.0)) <= 1e-15 * 4
    assert d["s"][0, 0] < d["s"][1, 0]


def test_ray_starting_on_the_line_does_not_cross_at_row_0():
    s = rows_of([(0, 0), (1, 0.1), (2, 0.2)], [0.1, 0.1, 0.1])
    cnt, _ = X.crossings(s, [2], (0.0, 1.0, 0.0))
    assert cnt[0] == 0
    # ... but it does when it comes back through the line
    s = rows_of([(0, 0), (1, 0.1), (2, -0.1)], [0.1, -0.2, -0.2])
    cnt, out = X.crossings(s, [2], (0.0, 1.0, 0.0))
    assert cnt[0] == 1 and 1 < out[0, 5, 0] < 2


def test_row_exactly_on_the_line_counts_once():
    s = rows_of([(0, -1), (0, 0), (0, 1)], [np.pi / 2] * 3)
    cnt, out = X.crossings(s, [2], (0.0, 1.0, 0.0))
    assert cnt[0] == 1
    assert out[0, 5, 0] == 1.0 and out[0, 1, 0] == 0.0 and out[0, 2, 0] == 0.0 and out[0, 3, 0] == 1.0


def test_final_step_leaving_the_box_across_its_edge():
    # the last row lies beyond the box top y = 1 (the reference's loop writes the row that left the box, then stops)
    s = rows_of([(0, 0.8), (0, 0.9), (0, 1.05)], [np.pi / 2] * 3, T=[0, 0.1, 0.25])
    cnt, out = X.crossings(s, [2], (0.0, 1.0, 1.0))
    assert cnt[0] == 1
    assert abs(out[0, 2, 0] - 1.0) <= 1e-15 and abs(out[0, 3, 0] - 0.2) <= 1e-15
    # rows past the last written one (zeros, as np.zeros leaves them) are never read
    s2 = np.concatenate([s, np.zeros((3, 6, 1))])
    cnt2, out2 = X.crossings(s2, [2], (0.0, 1.0, 1.0))
    assert cnt2[0] == 1 and np.array_equal(out2, out, equal_nan=True)


def test_more_crossings_than_kmax_are_counted_not_stored():
    phi = np.arange(0, 4 * np.pi, 1e-2)
    s = circle_rows(1.0, phi)
    cnt, out = X.crossings(s, [len(phi) - 1], (0.0, 1.0, 0.25), kmax=2)
    assert cnt[0] == 4
    assert np.isfinite(out[:2]).all()
    cnt3, out3 = X.crossings(s, [len(phi) - 1], (0.0, 1.0, 0.25), kmax=6)
    assert cnt3[0] == 4 and np.array_equal(out3[:2], out) and np.isnan(out3[4:]).all()


def test_truncated_ray_counts_minus_one():
    s = rows_of([(0, -1), (0, 0.5), (0, 1)], [np.pi / 2] * 3)
    cnt, out = X.crossings(s, [3], (0.0, 1.0, 0.0))
    assert cnt[0] == -1 and np.isnan(out).all()


def test_argument_errors_do_not_touch_the_gpu():
    """Every check below comes before the library dereferences a handle or calls HIP, so a placeholder handle is enough."""
    L = _lib.lib()
    fake = C.c_void_p(1)
    line = np.array([0.0, 1.0, 0.0])
    zero = np.zeros(3)
    cnt = np.zeros(4, dtype=np.int32)
    out = np.zeros(4 * 6 * 4)
    ip = lambda a: a.ctypes.data_as(_lib._ip)          # noqa: E731
    assert L.rtmi_crossings(None, _lib.dptr(line), 4, ip(cnt), _lib.dptr(out)) == -1
    assert L.rtmi_crossings(fake, None, 4, ip(cnt), _lib.dptr(out)) == -1
    assert L.rtmi_crossings(fake, _lib.dptr(line), 0, ip(cnt), _lib.dptr(out)) == -1
    assert b"kmax" in L.rtmi_last_error()
    assert L.rtmi_crossings(fake, _lib.dptr(zero), 4, ip(cnt), _lib.dptr(out)) == -1
    assert b"line" in L.rtmi_last_error()

    p = _lib.Params()
    p.method = 6; p.dtype = 0; p.gamma = p.gamma_step = 1.0; p.step = 0.01; p.max_size = 100
    p.box[0], p.box[1], p.box[2], p.box[3] = -2.0, 5.0, -2.5, 1.0
    sx, sy = np.array([-2.0]), np.array([-2.0])
    th = np.linspace(0.1, 1.4, 8)
    ru = np.linspace(-2.0, 0.5, 5)
    c2, b2 = np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int32)
    arr = np.zeros(5 * 4 * 9)

    def tp(pp=p, S=1, M=len(th), J=len(ru), ln=np.array([1.0, 0.0, 4.0]), ru_=ru, f=fake, xs=sx):
        return L.rtmi_two_point(f, C.byref(pp), S, _lib.dptr(xs), _lib.dptr(sy), M, _lib.dptr(th), _lib.dptr(ln), J, _lib.dptr(ru_),
                                None, ip(c2), ip(b2), _lib.dptr(arr), None)
    assert tp(f=None) == -1
    assert tp(xs=None) == -1
    assert tp(J=0) == -1
    assert tp(M=1) == -1
    assert tp(S=0) == -1
    assert tp(ln=zero) == -1 and b"line" in L.rtmi_last_error()
    assert tp(ru_=ru[::-1].copy()) == -1 and b"increasing" in L.rtmi_last_error()
    p32 = _lib.Params.from_buffer_copy(p)
    p32.dtype = 1
    assert tp(pp=p32) == -1 and b"fp64" in L.rtmi_last_error()
    bad = _lib.TwoPointParams()
    bad.max_arrivals = -1
    assert L.rtmi_two_point(fake, C.byref(p), 1, _lib.dptr(sx), _lib.dptr(sy), len(th), _lib.dptr(th), _lib.dptr(line), len(ru),
                            _lib.dptr(ru), C.byref(bad), ip(c2), ip(b2), _lib.dptr(arr), None) == -1
