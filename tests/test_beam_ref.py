"""CPU: the numpy restatement of rtmi_gaussian_beams (tests/beam_ref.py) on the oracle's rows of a constant medium against the
exact Green's function (i/4) H0^(1)(omega n r): the normalisation, the phase and the stationary-phase limit that the device is
then compared with (tests/test_gpu_beams.py); and the cases of tests/beam_cases.py on the oracle's rows of their fan: the
conditions under which the tiles, the cap, the cutoff, the frequency groups and the record's length decide something, which
tests/test_gpu_beam_edges.py asserts again on the device's rows.  No GPU involved."""
import numpy as np
import pytest
from scipy.special import hankel1

import beam_cases as BC
import beam_ref as B
import paraxial_ref as P
from conftest import LIMITS

DELTA_S = 0.05293304824724534 / 20
GRID = (0.0, 0.1, 31, 0.0, 0.1, 31)


@pytest.fixture(scope="module")
def const_fan():
    """n = 1 sampled on [-4, 4]^2, source at the origin, 301 rays over [-0.6, pi/2 + 0.6] to the box's edge"""
    from oracle import rt_oracle as O
    ax = np.linspace(-4.0, 4.0, 81)
    F = O.Field.from_samples(ax, ax, np.ones((81, 81)), 0.1)
    th = np.linspace(-0.6, np.pi / 2 + 0.6, 301)
    box = (-4.0, 4.0, -4.0, 4.0)
    ms = int(np.ceil(6.0 / DELTA_S)) + 1
    c = O.trazar(F, 1, 1, DELTA_S, ms, box, 0.0, 0.0, th, record_stride=0, nthreads=8)
    rows = int(c["d_ray"][2].max()) + 1
    o = O.trazar(F, 1, 1, DELTA_S, ms, box, 0.0, 0.0, th, record_stride=1, rec_rows=rows, nthreads=8)
    s_ray, last = o["s_ray"], o["d_ray"][2].astype(np.int64)
    S = P.SplineField(*F.arrays())
    return s_ray, last, S, th, B.tube_rows(s_ray, last, S)


def compared_nodes():
    X, Y = B.nodes(GRID)
    r, a = np.hypot(X, Y), np.arctan2(Y, X)
    return (r >= 1.0) & (r <= 3.0) & (a >= 0.1) & (a <= np.pi / 2 - 0.1), r


@pytest.mark.parametrize("omega,eps,bound", [(200.0, 1.0, 1e-2), (800.0, 4.0, 1e-3)])
def test_constant_medium_matches_the_hankel_function(const_fan, omega, eps, bound):
    s_ray, last, S, th, tube = const_fan
    u = B.gaussian_beams(s_ray, last, S, th, len(th), GRID, [omega], eps, tube=tube)[0, 0]
    sel, r = compared_nodes()
    ref = 0.25j * hankel1(0, omega * r[sel])
    err = np.abs(u[sel] - ref) / np.abs(ref)
    print(f"omega {omega} eps {eps}: {sel.sum()} nodes, worst {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= bound


def test_a_straight_ray_gives_each_node_one_owning_step(const_fan):
    """d_i = (R - X_i) . t_i: consecutive steps share d_i, so exactly one step of a straight ray owns a node between its ends"""
    s_ray, last, S, th, tube = const_fan
    o = len(th) // 2
    nr = int(last[o]) + 1
    x, y, t = s_ray[:nr, 0, o], s_ray[:nr, 1, o], s_ray[:nr, 5, o]
    X, Y = (a.ravel() for a in B.nodes(GRID))
    d = (X[None, :] - x[:, None]) * np.cos(t)[:, None] + (Y[None, :] - y[:, None]) * np.sin(t)[:, None]
    owners = ((d[:-1] >= 0.0) & (d[1:] < 0.0)).sum(axis=0)
    between = (d[0] >= 0.0) & (d[-1] < 0.0)
    assert between.sum() > 500
    assert np.all(owners[between] == 1) and np.all(owners[~between] == 0)


# ---------------------------------------------------------------- the cases of tests/test_gpu_beam_edges.py bind (beam_cases.py)
@pytest.fixture(scope="module")
def edge_fans(oracle_fields):
    """the oracle's rows of beam_cases' fan, per (sources, rec_rows): s_ray, last (every ray's last written row), the field's
    splines, theta0 and the tube"""
    from oracle import rt_oracle as O
    F = oracle_fields(BC.SCENARIO)
    S = P.SplineField(*F.arrays())
    step, ms = BC.fan_params(DELTA_S)
    cache = {}

    def get(case):
        key = (BC.CASES[case].get("sources"), BC.CASES[case].get("rec_rows"))
        if key not in cache:
            th, x0, y0, _ = BC.launch(case)
            o = O.trazar(F, BC.METHOD, 1, step, ms, LIMITS[BC.SCENARIO], x0, y0, th, record_stride=1, rec_rows=key[1] or ms,
                         nthreads=8)
            s_ray, last = o["s_ray"], o["d_ray"][2].astype(np.int64)
            cache[key] = (s_ray, last, S, th, B.tube_rows(s_ray, last, S))
        return cache[key]
    return get


@pytest.mark.parametrize("case", list(BC.CASES))
def test_the_edge_cases_bind_on_the_oracles_rows(edge_fans, case):
    s_ray, last, S, th, tube = edge_fans(case)
    cn = {}
    u = BC.restate(case, s_ray, last, S, th, counts=cn, tube=tube)
    extra = {}
    if case == "short_record":
        extra["last_raw"] = last
        extra["u_full"] = BC.restate(case, *edge_fans("cap_wide")[:4], tube=edge_fans("cap_wide")[4])
    if case == "taper":
        extra["u_plain"] = BC.restate(case, s_ray, last, S, th, tube=tube, edge_taper=0.0)
    rows = np.minimum(last, s_ray.shape[0] - 1)
    turn = min(float(np.min(np.cos(np.diff(s_ray[:r + 1, 5, o])))) for o, r in enumerate(rows))
    print(f"{case}: rays end at rows {last.min()} .. {last.max()}, smallest cos of a turn {turn:.6f}, counts {cn}, "
          f"{int((u == 0).sum())} of {u.size} outputs exactly 0, max|u| {np.abs(u).max():.3e}")
    assert turn >= B.COS_TURN                  # the turn rule removes no step, so `capped` counts plain steps
    BC.check_binds(case, u, cn, **extra)


def test_counts_leave_the_result_unchanged(edge_fans):
    s_ray, last, S, th, tube = edge_fans("cap_wide")
    a = BC.restate("cap_wide", s_ray, last, S, th, tube=tube)
    b = BC.restate("cap_wide", s_ray, last, S, th, tube=tube, counts={})
    assert np.array_equal(a.view(np.float64), b.view(np.float64))
