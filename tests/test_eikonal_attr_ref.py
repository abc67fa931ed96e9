"""CPU: the restatement of launch angle, direction and spreading at eikonal-filled nodes (tests/eikonal_attr_ref.py; DESIGN.md
section 38) against its own rules and against closed forms.  The sweeps in either round order and one pass over the nodes sorted
by T give the same bits; a homogeneous medium and the gradient medium give the figures of the design note, each bound being the
measured figure rounded up to one digit; the seeded disc is first order (the error ratio between 71 x 57 and 141 x 113 is under
0.75, section 34's criterion); behind a wall every node that descends from one node has that node's launch angle and G is 0 where
the four neighbours share it; seeds that are NaN or infinite are skipped; a node without a usable parent is NaN and still has a
direction.  The device against this restatement: tests/test_gpu_eikonal_attr.py."""
import functools
import math

import numpy as np
import pytest

import eikonal_attr_ref as A
import eikonal_lin_ref as L
import eikonal_ref as R
import kirchhoff_aa_ref as KA
import paraxial_ref as P


def wrapn(d):
    return (d + np.pi) % (2.0 * np.pi) - np.pi


# ------------------------------------------------------------------------------------------------------------- the pieces
def test_wrap_at_pi_and_beside():
    pi = math.pi
    up, down = math.nextafter(pi, math.inf), math.nextafter(pi, 0.0)
    assert A.wrap(pi) == pi and A.wrap(down) == down and A.wrap(up) == up - 2.0 * pi < 0.0
    assert A.wrap(-pi) == -pi + 2.0 * pi == pi and A.wrap(-down) == -down and A.wrap(-up) == -up + 2.0 * pi
    assert A.wrap(0.0) == 0.0 and math.isnan(A.wrap(math.nan)) and A.wrap(math.inf) == math.inf and A.wrap(-math.inf) == -math.inf
    assert A.PI == float.fromhex("0x1.921fb54442d18p+1") and A.TWO_PI == float.fromhex("0x1.921fb54442d18p+2")


def test_gathers_differences_and_the_ball():
    # two parents: the weighted mean along the shorter arc; across the cut the result leaves (-pi, pi] and is not wrapped again
    assert A.combine(True, 1.0, True, 2.0, 0.25) == 1.25
    assert A.combine(True, 3.0, True, -3.0, 0.75) == 3.0 + 0.75 * (-6.0 + 2.0 * math.pi) > math.pi
    # one parent, or one usable parent: its value; a parent the code does not name is not read
    assert A.combine(True, 1.5, False, 9.0, 0.3) == 1.5 and A.combine(False, 9.0, True, -2.0, 0.3) == -2.0
    assert A.combine(True, math.nan, True, 0.5, 0.3) == 0.5 and A.combine(True, 0.5, True, math.inf, 0.3) == 0.5
    assert A.combine(True, -math.inf, True, 0.25, 0.3) == 0.25
    for case in ((False, 1.0, False, 1.0), (True, math.nan, True, math.inf), (True, math.nan, False, 1.0)):
        assert math.isnan(A.combine(*case, 0.3))
    assert math.isnan(A.combine(True, 1.0, True, 2.0, math.nan))
    assert A.weight(L.XPARENT | L.YPARENT, 0.25, 0.75) == 0.75 and A.weight(L.XPARENT, 1.0, 0.0) == 0.0
    # every neighbour pattern of the difference
    assert A.diff(True, 1.0, 5.0, True, 2.0, 0.25) == 1.0 / 0.5 and A.diff(False, 1.0, 1.5, True, 2.0, 0.25) == 0.5 / 0.25
    assert A.diff(True, 1.0, 1.5, False, 2.0, 0.25) == 0.5 / 0.25 and A.diff(False, 1.0, 1.5, False, 2.0, 0.25) == 0.0
    assert A.diff(True, 3.0, 0.0, True, -3.0, 0.5) == (-6.0 + 2.0 * math.pi) / 1.0
    # m == 0: J is +inf and G is 0; J == 0 (the source node): G is +inf
    assert A.spread(0.0, 0.0) == math.inf and A.amp(0.5, math.inf) == 0.0 and A.amp(0.5, 0.0) == math.inf
    assert A.spread(3.0, 4.0) == 1.0 / 5.0 and A.amp(0.5, 8.0) == 1.0 / math.sqrt(4.0)
    assert A.ball_dir(3.0, 4.0, 5.0) == (3.0 / 5.0, 4.0 / 5.0) and A.ball_dir(0.0, 0.0, 0.0) == (0.0, 0.0)
    # the direction: + for a west or south parent, - for an east or north one; no parent: NaN
    assert A.free_dir(0.5, 0.25, L.XPARENT, 2.0, 1.0, 0.0) == (1.0, 0.0)
    assert A.free_dir(0.5, 0.25, L.XPARENT | L.XEAST, 2.0, 1.0, 0.0) == (-1.0, 0.0)
    px, py = A.free_dir(0.5, 0.25, L.XPARENT | L.YPARENT | L.YNORTH, 2.0, 0.5, 1.5)
    assert px == 3.0 / math.sqrt(13.0) and py == -2.0 / math.sqrt(13.0)
    assert all(math.isnan(v) for v in A.free_dir(0.5, 0.25, 0, 2.0, 0.0, 0.0))
    assert all(math.isnan(v) for v in A.free_dir(0.5, 0.25, L.XPARENT, 2.0, 2.0, 0.0))


# ------------------------------------------------------------------------------------- the schedule changes no bit
@functools.lru_cache(maxsize=None)
def named(name):
    return L.filled(getattr(L, name)())


def seeds_theta0(fill, seed):
    """launch angles in (-pi, pi] at every node; only the seeds' are read"""
    return np.random.default_rng(seed).uniform(-3.1, 3.1, fill["T"].shape)


@pytest.mark.parametrize("name", ["gradient_case", "corridor_case", "disc_case", "walls_case"])
def test_sweeps_in_either_order_and_one_sorted_pass_give_the_same_bits(name):
    grid, n, src, ns, fill, nets = named(name)
    th = seeds_theta0(fill, 11)
    want = A.solve(grid, n, src, ns, fill, theta0=th, nets=nets)
    assert want["converged"].all()
    for order in ("other", "sorted"):
        got = A.solve(grid, n, src, ns, fill, theta0=th, nets=nets, order=order)
        assert all(L.same_but_nan(got[k], want[k]) for k in A.KEYS), (name, order)
    cls = np.array([net.cls for net in nets]).reshape(fill["T"].shape)
    keep = (cls == L.DEAD) | (cls == L.SEED)
    assert R.same_bits(want["theta0"][keep], th[keep]) and np.isnan(want["J"][keep]).all() and np.isnan(want["px"][keep]).all()
    if name == "corridor_case":
        assert (want["rounds"] > 3).all()
        capped = A.solve(grid, n, src, ns, fill, theta0=th, nets=nets, max_rounds=1)
        assert (capped["rounds"] == 1).all() and not capped["converged"].any() and np.isnan(capped["theta0"][cls == L.FREE]).any()


# ----------------------------------------------------------------------------------------------- a homogeneous medium
# From the ball alone the launch angle is poor, and J and G poorer (the near-source singularity of a first-order scheme rides along
# the rays): these are the measured figures rounded up, not a claim of accuracy.
#           ball: theta0 max, theta0 median, theta max beyond 0.3, J median, G median, G 95th percentile
HOMOGENEOUS = {2.0: (3e-1, 7e-2, 7e-2, 4e-1, 2e-1, 5e-1), 8.0: (4e-2, 2e-2, 7e-2, 5e-2, 3e-2, 9e-2)}


@pytest.mark.parametrize("ball", [2.0, 8.0])
def test_homogeneous_medium_from_a_ball(ball):
    grid = (-1.0, 0.05, 41, -0.8, 0.04, 37)
    X, Y = R.nodes(grid)
    n, src, ns = np.full(X.shape, 0.5), np.array([[0.013, -0.021]]), np.array([0.5])
    fill = R.solve(grid, n, src, ns, ball=ball)
    o = A.solve(grid, n, src, ns, fill, ball=ball)
    assert fill["filled"].all() and o["converged"].all() and all(np.isfinite(o[k]).all() for k in A.KEYS)
    r, tt = np.hypot(X - src[0, 0], Y - src[0, 1]), np.arctan2(Y - src[0, 1], X - src[0, 0])
    far = r > 0.3
    e0, e1 = np.abs(wrapn(o["theta0"][0] - tt)), np.abs(wrapn(np.arctan2(o["py"][0], o["px"][0]) - tt))
    eJ, eG = np.abs(o["J"][0] - r) / r, np.abs(o["G"][0] * np.sqrt(0.5 * r) - 1.0)
    got = (e0.max(), np.median(e0), e1[far].max(), np.median(eJ[far]), np.median(eG[far]), np.percentile(eG[far], 95))
    print(f"homogeneous, ball {ball}: theta0 max {got[0]:.3e} median {got[1]:.3e} rad, theta max {got[2]:.3e} rad, "
          f"J median {got[3]:.3e}, G median {got[4]:.3e} 95 % {got[5]:.3e}")
    assert all(g <= b for g, b in zip(got, HOMOGENEOUS[ball])), got
    # inside the ball the values are the closed forms themselves (numpy's arctan2 is not libm's to the last bit)
    ball_nodes = np.array(o["nets"][0].cls).reshape(X.shape) == L.BALL
    assert ball_nodes.sum() > 4 and np.abs(o["theta0"][0][ball_nodes] - tt[ball_nodes]).max() < 1e-15
    assert np.allclose(o["J"][0][ball_nodes], r[ball_nodes], rtol=1e-15)


# -------------------------------------------------------------------------------------------------- the gradient medium
def test_closed_forms_agree_with_the_projects_own():
    """gradient_theta0 against kirchhoff_aa_ref.closed_theta0 at a surface position, and |J| = v_r sinh(g T) / g against
    paraxial_ref.vert_closed_form, which is signed for rays that leave to the left"""
    grid = L.GRADIENT_GRID
    X, Y = R.nodes(grid)
    mine = A.gradient_theta0(X, Y, 1.3, -2.5)
    theirs = KA.closed_theta0(np.array([1.3]), -2.5, (grid[0], grid[1], grid[2], grid[3], grid[4], grid[5]))[0]
    ok = (X > 1.3) & (Y > -2.5)                      # where the sign of xc - xs is the sign of X - xs
    assert np.abs(wrapn(mine - theirs))[ok].max() < 1e-12
    for xs, ys in L.GRADIENT_SOURCES:
        th, J = A.gradient_theta0(X, Y, xs, ys), A.gradient_J(X, Y, xs, ys)
        away = np.hypot(X - xs, Y - ys) > 0.2
        assert np.abs(np.abs(P.vert_closed_form(th, X, Y, xs, ys)) - J)[away].max() < 1e-9 * J[away].max()


@functools.lru_cache(maxsize=None)
def disc(shape):
    """the seeded disc on `shape` nodes: per source the largest theta0 error over the filled nodes and the median and the 95th
    percentile of G's relative error there"""
    grid, n, src, ns, T, th, Jc = A.seeded_disc(shape)
    fill = R.solve(grid, n, src, ns, T=T)
    Gc = 1.0 / np.sqrt(n[None] * Jc)
    seeds = fill["filled"] == 0
    o = A.solve(grid, n, src, ns, fill, theta0=np.where(seeds, th, np.nan), J=np.where(seeds, Jc, np.nan), G=np.where(seeds, Gc, np.nan))
    assert o["converged"].all() and R.same_bits(o["theta0"][seeds], th[seeds])
    out = []
    for s in range(2):
        f = fill["filled"][s] == 1
        assert np.isfinite(o["theta0"][s][f]).all() and np.isfinite(o["G"][s][f]).all()
        ge = np.abs(o["G"][s][f] - Gc[s][f]) / Gc[s][f]
        out.append((np.abs(wrapn(o["theta0"][s][f] - th[s][f])).max(), np.median(ge), np.percentile(ge, 95)))
    return out


# measured: 71 x 57   (1.041e-3, 2.987e-3, 1.505e-2) and (2.355e-2, 1.345e-2, 1.192e-1)
#           141 x 113 (5.394e-4, 1.449e-3, 6.791e-3) and (1.292e-2, 6.176e-3, 7.956e-2); the maximum of G is not asserted: the
# outliers are the spikes where the disc's two flanks meet
DISC_BOUNDS = {(71, 57): ((2e-3, 3e-3, 2e-2), (3e-2, 2e-2, 2e-1)), (141, 113): ((6e-4, 2e-3, 7e-3), (2e-2, 7e-3, 8e-2))}


def test_seeded_disc_is_first_order_in_theta0_and_G():
    coarse, fine = disc((71, 57)), disc((141, 113))
    for s in range(2):
        print(f"disc, source {s}: theta0 max {coarse[s][0]:.3e} -> {fine[s][0]:.3e} rad, G median {coarse[s][1]:.3e} -> "
              f"{fine[s][1]:.3e}, 95 % {coarse[s][2]:.3e} -> {fine[s][2]:.3e}")
        for shape, got in (((71, 57), coarse[s]), ((141, 113), fine[s])):
            assert all(g <= b for g, b in zip(got, DISC_BOUNDS[shape][s])), (shape, s, got)
        assert all(fine[s][k] < 0.75 * coarse[s][k] for k in range(3)), (s, coarse[s], fine[s])


# measured on 71 x 57 beyond 0.5 of the source, per ball and source: theta0 median, 95th percentile, G median, 95th percentile.  No
# claim that they improve with the grid or with the ball: from the ball alone they do not
BALL_ONLY = {2.0: ((3e-2, 8e-2, 3e-2, 3e-1), (2e-2, 8e-2, 4e-2, 2e-1)), 8.0: ((4e-2, 7e-2, 2e-2, 9e-2), (4e-2, 7e-2, 3e-2, 1e-1))}


@pytest.mark.parametrize("ball", [2.0, 8.0])
def test_ball_only_solves_of_the_gradient_medium(ball):
    grid, n, src, ns, _, th, Jc = A.seeded_disc((71, 57))
    fill = R.solve(grid, n, src, ns, ball=ball)
    o = A.solve(grid, n, src, ns, fill, ball=ball)
    Gc = 1.0 / np.sqrt(n[None] * Jc)
    X, Y = R.nodes(grid)
    for s in range(2):
        far = np.hypot(X - src[s, 0], Y - src[s, 1]) > 0.5
        e, ge = np.abs(wrapn(o["theta0"][s] - th[s]))[far], (np.abs(o["G"][s] - Gc[s]) / Gc[s])[far]
        got = (np.median(e), np.percentile(e, 95), np.median(ge), np.percentile(ge, 95))
        print(f"ball {ball}, source {s}: theta0 median {got[0]:.3e} 95 % {got[1]:.3e} rad, G median {got[2]:.3e} 95 % {got[3]:.3e}")
        assert all(g <= b for g, b in zip(got, BALL_ONLY[ball][s])), (ball, s, got)


# --------------------------------------------------------------------------------------------------------- behind a wall
def roots_of(net, th, cut):
    """per node the set of nodes its launch angle descends from, the nodes of `cut`, the seeds and the ball being their own"""
    nx = net.nx
    roots = {}
    for x in sorted(net.live, key=lambda x: net.T[x]):
        if not math.isfinite(th[x]):
            roots[x] = frozenset()
        elif net.cls[x] != L.FREE or x in cut:
            roots[x] = frozenset([x])
        else:
            p, r = net.par[x], frozenset()
            if p & L.XPARENT:
                r |= roots[x + 1 if p & L.XEAST else x - 1]
            if p & L.YPARENT:
                r |= roots[x + nx if p & L.YNORTH else x - nx]
            roots[x] = r
    return roots


def test_behind_a_wall_the_launch_angle_is_the_gap_nodes_and_G_is_zero():
    grid, n, src, ns, fill, nets = named("walls_case")
    o = A.solve(grid, n, src, ns, fill, nets=nets)
    net, nx = nets[0], grid[2]
    th, G = o["theta0"][0].reshape(-1), o["G"][0].reshape(-1)
    gap = {j * nx + 12 for j in range(4)}            # the NaN wall stands in column 12 from row 4 upwards
    assert all(net.cls[x] == L.FREE for x in gap) and all(net.cls[j * nx + 12] == L.DEAD for j in range(4, 29))
    roots = roots_of(net, th, gap)
    behind = [x for x in net.free if 12 < x % nx < 25 and x not in gap]
    single = [x for x in behind if len(roots[x]) == 1]
    assert all(roots[x] <= gap for x in behind) and len(single) > 50
    assert {next(iter(roots[x])) for x in single} == {3 * nx + 12}             # the gap's corner, where the first arrival bends
    assert all(L.bits(th[x]) == L.bits(th[next(iter(roots[x]))]) for x in single)
    # a pure diffraction: G is 0 where all four neighbours share the node's value
    flat = [x for x in behind if 0 < x // nx < grid[5] - 1 and all(L.bits(th[y]) == L.bits(th[x]) for y in (x - 1, x + 1, x - nx, x + nx))]
    assert len(flat) > 20 and all(G[x] == 0.0 and o["J"][0].reshape(-1)[x] == math.inf for x in flat)


# ------------------------------------------------------------------------------------------- seeds that cannot be used
def test_nan_and_infinite_seeds_are_skipped_and_a_node_without_a_usable_parent_is_nan():
    """one row: the source's ball on the left, then seeds, then free nodes; and two rows, where the second parent takes over"""
    grid = (0.0, 1.0, 9, 0.0, 1.0, 2)
    n = np.ones((2, 9))
    src, ns = np.array([[0.0, 0.0]]), np.ones(1)
    T = np.full((1, 2, 9), np.nan)
    T[0, :, 3:5] = np.array([[3.0, 4.0], [3.2, 4.2]])                    # seeds at columns 3 and 4 of both rows
    fill = R.solve(grid, n, src, ns, T=T, ball=1.0)
    assert fill["filled"][0, :, 5:].all() and not fill["filled"][0, :, 3:5].any()
    for bad in (math.nan, math.inf, -math.inf):
        th = np.full((1, 2, 9), np.nan)
        th[0, :, 3] = 0.25
        th[0, 0, 4], th[0, 1, 4] = bad, 0.5                              # row 0's seed cannot be used, row 1's can
        o = A.solve(grid, n, src, ns, fill, theta0=th, ball=1.0)
        net = o["nets"][0]
        assert net.cls[5] == L.FREE and net.par[5] == L.XPARENT and net.par[9 + 5] & L.XPARENT
        # row 0 right of the bad seed descends from it alone: NaN in theta0, J and G, and still a direction, (1, 0)
        assert np.isnan(o["theta0"][0, 0, 5:]).all() and np.isnan(o["J"][0, 0, 5:]).all() and np.isnan(o["G"][0, 0, 5:]).all()
        assert (o["px"][0, 0, 5:] == 1.0).all() and (o["py"][0, 0, 5:] == 0.0).all()
        assert L.bits(o["theta0"][0, 0, 4]) == L.bits(bad)               # the seed keeps its bits
        # row 1 carries 0.5 on, and the bad values above it are no neighbours of its differences: a flat line, G = 0
        assert (o["theta0"][0, 1, 5:] == 0.5).all() and (o["G"][0, 1, 6:8] == 0.0).all()
        # the node right of the usable seed differences against it: wrap(0.5 - 0.5) / 2 along x, nothing usable above
        assert o["J"][0, 1, 5] == math.inf


# ------------------------------------------------------------------------------------------------------------ a shock line
def test_a_shock_line_behind_a_block_touches_two_rows_of_nodes():
    """A homogeneous medium with a block in the way: behind it the arrivals round its two sides meet on a line, the launch angle
    jumps there, and the central difference spans the jump at the nodes on either side of the line, where G spikes.  Measured: 70
    of 3 628 nodes beyond the ball, 1.93 %, two rows wide, G ten times its neighbours'.  This is the documented price of central
    differences; the test records how far it reaches."""
    grid = (0.0, 0.1, 71, 0.0, 0.1, 57)
    X, Y = R.nodes(grid)
    n = np.ones(X.shape)
    n[20:37, 30:36] = np.nan
    src, ns = np.array([[1.03, 2.84]]), np.ones(1)
    fill = R.solve(grid, n, src, ns, ball=8.0)
    o = A.solve(grid, n, src, ns, fill, ball=8.0)
    th, G = o["theta0"][0], o["G"][0]
    live = np.isfinite(th)
    far = live & (np.hypot(X - src[0, 0], Y - src[0, 1]) > 1.0)
    jump = np.zeros(th.shape, dtype=bool)
    jump[:, 1:-1] |= np.abs(wrapn(th[:, 2:] - th[:, :-2])) > 0.3
    jump[1:-1, :] |= np.abs(wrapn(th[2:, :] - th[:-2, :])) > 0.3
    touched = jump & far
    share = touched.sum() / far.sum()
    behind = X > 3.6
    ratio = np.median(G[touched & behind]) / np.median(G[far & ~touched & behind])
    print(f"shock line: {int(touched.sum())} of {int(far.sum())} nodes, {share:.3e}; G on it over G beside it {ratio:.3e}")
    assert touched.sum() > 0 and share <= 2e-2 and ratio > 5.0
    assert len(set(np.argwhere(touched & behind)[:, 0])) == 2 and np.isfinite(G[far]).all()
