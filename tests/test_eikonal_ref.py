"""CPU: the restatement of the eikonal continuation (tests/eikonal_ref.py; rtmi_eikonal_fill) against the
truth and against the rules of its definition.  Errors are fractions of the table's largest T; each bound is the figure the
restatement itself gives (in the comment beside it), rounded up to one digit.  The device is held to the restatement bit for bit
in tests/test_gpu_eikonal.py, the host arithmetic of rt_eikonal.h in tests/test_eikonal_host.py."""
import functools

import numpy as np
import pytest

import eikonal_ref as R

SOURCES = ((-1.97, -2.03), (1.513, -0.77))
GRIDS = {71: (-2.0, 7.0 / 70, 71, -2.5, 3.5 / 56, 57), 141: (-2.0, 7.0 / 140, 141, -2.5, 3.5 / 112, 113)}


def medium(nx):
    """n = 1 / (18 + 2 y) at the nodes of the nx-wide grid, and the nodes"""
    X, Y = R.nodes(GRIDS[nx])
    return X, Y, 1.0 / (18.0 + 2.0 * Y)


def launch_angle(X, Y, xs, ys, v0=18.0, g=2.0):
    """The launch angle from +x of the ray from (xs, ys) to each node in v = v0 + g y: the ray is an arc of the circle through
    both points whose centre lies on y = -v0 / g"""
    yc = -v0 / g
    with np.errstate(all="ignore"):
        xc = ((X * X - xs * xs) + (Y - yc) ** 2 - (ys - yc) ** 2) / (2.0 * (X - xs))
    tx, ty = -(ys - yc) * np.ones_like(X), xs - xc
    sgn = np.sign(tx * (X - xs) + ty * (Y - ys))
    th = np.arctan2(sgn * ty, sgn * tx)
    return np.where(X == xs, np.where(Y > ys, np.pi / 2, -np.pi / 2), th)


@functools.lru_cache(maxsize=None)
def gradient_error(case, nx, k):
    """point: no table; shadow: the table exact but for a disc of radius 0.7 round (3, -1); wedge: the table exact on the launch
    angles 0.05 .. 1.5 only.  -> (the largest error at the nodes the call filled) / (the largest T), rounds, clean"""
    g = GRIDS[nx]
    X, Y, n = medium(nx)
    xs, ys = SOURCES[k]
    truth = R.gradient_truth(X, Y, xs, ys)
    if case == "point":
        tin = None
    elif case == "shadow":
        tin = np.where((X - 3.0) ** 2 + (Y + 1.0) ** 2 <= 0.49, np.nan, truth)
    else:
        th = launch_angle(X, Y, xs, ys)
        tin = np.where((th >= 0.05) & (th <= 1.5), truth, np.nan)
    T, rounds, clean, filled, _ = R.solve_one(g, n, xs, ys, 1.0 / (18.0 + 2.0 * ys), T=tin)
    assert not np.isnan(T).any() and filled.sum() > 0
    if tin is not None:
        assert R.same_bits(T[filled == 0], tin[filled == 0])
    return float(np.max(np.abs(T - truth)[filled == 1]) / truth.max()), rounds, clean


#       case, source -> bound at 71 x 57, bound at 141 x 113
BOUNDS = {("point", 0): (2e-2, 8e-3),       # 1.191e-2, 7.326e-3
          ("point", 1): (2e-2, 2e-2),       # 1.889e-2, 1.128e-2
          ("shadow", 0): (1e-4, 5e-5),      # 9.217e-5, 4.694e-5
          ("shadow", 1): (4e-3, 2e-3),      # 3.674e-3, 1.945e-3
          ("wedge", 0): (7e-3, 5e-3)}       # 6.281e-3, 4.318e-3


@pytest.mark.parametrize("case,k", sorted(BOUNDS))
def test_gradient_medium_against_the_closed_form(case, k):
    coarse, r71, c71 = gradient_error(case, 71, k)
    fine, r141, c141 = gradient_error(case, 141, k)
    print(f"{case} source {k}: 71 x 57 {coarse:.3e}, 141 x 113 {fine:.3e}, ratio {fine / coarse:.3f}")
    assert coarse <= BOUNDS[case, k][0] and fine <= BOUNDS[case, k][1]
    assert fine / coarse < 0.75                              # first order
    assert (r71, c71, r141, c141) == (2, 1, 2, 1)            # a smooth medium: one round and the clean one


@pytest.mark.parametrize("k,bound", [(0, 2e-2), (1, 2e-2)])        # 1.163e-2, 1.947e-2
def test_constant_medium_beyond_the_ball(k, bound):
    g = GRIDS[71]
    X, Y, _ = medium(71)
    xs, ys = SOURCES[k]
    T, rounds, clean, filled, _ = R.solve_one(g, np.ones_like(X), xs, ys, 1.0)
    truth = np.hypot(X - xs, Y - ys)
    u, v = (X - xs) / g[1], (Y - ys) / g[4]
    ball = u * u + v * v <= 4.0
    err = np.max(np.abs(T - truth)[~ball]) / truth.max()
    print(f"constant medium, source {k}: {err:.3e}")
    assert err <= bound and filled.all() and (rounds, clean) == (2, 1)
    assert np.allclose(T[ball], truth[ball], rtol=1e-15, atol=0)      # the ball is the truth of a constant medium


# ------------------------------------------------------------------------------------------------ the rules of the definition
SMALL = (0.0, 0.5, 12, -1.0, 0.25, 9)


def small_medium():
    X, Y = R.nodes(SMALL)
    return X, Y, 1.0 + 0.1 * X + 0.05 * Y


def test_covered_nodes_keep_their_bits():
    X, Y, n = small_medium()
    rng = np.random.default_rng(5)
    tin = np.where(rng.random(n.shape) < 0.4, rng.random(n.shape) * 3.0, np.nan)
    tin[2, 3], tin[4, 4], tin[0, 0] = -0.0, np.inf, -np.inf             # a finite seed; two inputs that are free
    T, rounds, clean, filled, _ = R.solve_one(SMALL, n, 1.3, -0.2, 1.1, T=tin)
    seeded = np.isfinite(tin)
    assert R.same_bits(T[seeded], tin[seeded]) and not filled[seeded].any()
    assert np.isfinite(T).all() and filled[~seeded].all() and clean == 1


def test_obstacles_and_sealed_pockets_stay_nan():
    X, Y, n = small_medium()
    n[3:8, 5] = n[3, 5:10] = n[7, 5:10] = n[3:8, 9] = 0.0              # a sealed box of obstacles ...
    n[0, 11], n[1, 11] = np.nan, -1.0
    tin = np.full(n.shape, np.nan)
    tin[3, 5] = 7.0                                                     # an obstacle's input is its output, and no seed
    T, rounds, clean, filled, _ = R.solve_one(SMALL, n, 0.6, -0.7, 1.0, T=tin)
    obstacle = ~(np.isfinite(n) & (n > 0))
    pocket = np.zeros(n.shape, dtype=bool)
    pocket[4:7, 6:9] = True                                             # ... and the free nodes inside it
    assert R.same_bits(T[obstacle], tin[obstacle])
    assert np.isnan(T[pocket]).all() and not filled[pocket].any() and not filled[obstacle].any()
    rest = ~obstacle & ~pocket
    assert np.isfinite(T[rest]).all() and filled[rest].all()
    # a seed inside the pocket fills it, and nothing leaks through the wall
    tin[5, 7] = 1.0
    T2 = R.solve_one(SMALL, n, 0.6, -0.7, 1.0, T=tin)[0]
    assert np.isfinite(T2[pocket]).all() and R.same_bits(T2[rest], T[rest])


def test_source_off_the_grid_without_a_table():
    X, Y, n = small_medium()
    T, rounds, clean, filled, changes = R.solve_one(SMALL, n, 40.0, 3.0, 1.0)
    assert np.isnan(T).all() and (rounds, clean, changes) == (0, 1, 0) and not filled.any()


def test_negative_ball_gives_no_ball():
    X, Y, n = small_medium()
    T, rounds, clean, filled, _ = R.solve_one(SMALL, n, 1.3, -0.2, 1.1, ball=-1.0)
    assert np.isnan(T).all() and rounds == 0 and not filled.any()
    # ball 0 on a source at a node: that node alone, T = 0, and the solve runs from it
    T0, rounds, clean, filled, _ = R.solve_one(SMALL, n, 1.5, -0.5, 1.1, ball=0.0)
    assert T0[2, 3] == 0.0 and np.isfinite(T0).all() and rounds == 2 and filled.all()
    # the same source off the nodes: no node is within 0 cells
    assert np.isnan(R.solve_one(SMALL, n, 1.51, -0.5, 1.1, ball=0.0)[0]).all()


def test_update_branches():
    inf = R.INF
    assert R.update(0.5, 0.25, inf, inf, 1.0) == inf
    assert R.update(0.5, 0.25, 1.0, inf, 2.0) == 2.0 and R.update(0.5, 0.25, inf, 1.0, 2.0) == 1.5
    assert R.update(0.5, 0.25, 1.0, 2.0, 2.0) == 2.0                  # ta == b: one-sided along x
    assert R.update(0.5, 0.25, 1.5, 1.0, 2.0) == 1.5                  # tb == a: one-sided along y
    t = R.update(0.5, 0.5, 1.0, 1.0, 2.0)                              # two-sided: a + h s / sqrt(2)
    assert abs(t - (1.0 + 0.5 * 2.0 / np.sqrt(2.0))) < 1e-15


# ------------------------------------------------------------------------------------------- a medium that needs several rounds
@pytest.mark.parametrize("flip,rounds", [(True, 7), (False, 7)])
def test_winding_corridor_needs_several_rounds(flip, rounds):
    """The medium of the device's several-round test: the round count is asserted here, so that test cannot quietly become a
    one-round case"""
    n, (ix, iy) = R.winding_corridor(flip=flip)
    assert n.shape == (27, 31)
    g = (0.0, 1.0, 31, 0.0, 1.0, 27)
    T, r, clean, filled, _ = R.solve_one(g, n, ix + 0.25, iy - 0.125, 1.0)
    assert r == rounds >= 3 and clean == 1 and filled.all()
    # the first arrival follows the corridor: at its nodes T is far below one wall's 1000
    assert T[n == 1.0].max() < 500.0
    capped = R.solve_one(g, n, ix + 0.25, iy - 0.125, 1.0, max_rounds=1)
    assert capped[1:3] == (1, 0) and not R.same_bits(capped[0], T)
