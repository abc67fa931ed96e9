"""CPU: the restatement of the source-factored eikonal scheme (tests/eikonal_factored_ref.py; rtmi_eikonal_params.scheme,
DESIGN.md section 39) against the truth, against the plain scheme's restatement (tests/eikonal_ref.py) and against the rules of
its definition.  Errors are fractions of the table's largest T; each bound is the figure the restatement itself gives (in the
comment beside it), rounded up to one digit.  The device is held to the restatement bit for bit in
tests/test_gpu_eikonal_factored.py, the host arithmetic of rt_eikonal.h in tests/test_eikonal_factored_host.py."""
import functools

import numpy as np
import pytest

import eikonal_factored_ref as F
import eikonal_ref as R
from test_eikonal_ref import launch_angle


@functools.lru_cache(maxsize=None)
def solved(case, nx, k, scheme):
    """point: no table; const: no table, n = 0.05 everywhere; shadow: the table exact but for a disc of radius 0.7 round (3, -1);
    wedge: the table exact on the launch angles 0.05 .. 1.5 only.
    -> (the largest error at the nodes the call filled) / (the largest T), rounds, clean"""
    g = F.GRIDS[nx]
    X, Y, n = F.gradient_medium(g)
    xs, ys = F.SOURCES[k]
    ns = 1.0 / (18.0 + 2.0 * ys)
    truth = R.gradient_truth(X, Y, xs, ys)
    tin = None
    if case == "const":
        n, ns = np.full_like(X, 0.05), 0.05
        truth = 0.05 * np.hypot(X - xs, Y - ys)
    elif case == "shadow":
        tin = np.where((X - 3.0) ** 2 + (Y + 1.0) ** 2 <= 0.49, np.nan, truth)
    elif case == "wedge":
        th = launch_angle(X, Y, xs, ys)
        tin = np.where((th >= 0.05) & (th <= 1.5), truth, np.nan)
    T, rounds, clean, filled, _ = F.solve_one(g, n, xs, ys, ns, T=tin, scheme=scheme)
    assert not np.isnan(T).any() and filled.sum() > 0
    if tin is not None:
        assert R.same_bits(T[filled == 0], tin[filled == 0])
    return float(np.max(np.abs(T - truth)[filled == 1]) / truth.max()), rounds, clean


#   source -> (bound at 71 x 57, bound at 141 x 113), (rounds at 71 x 57, at 141 x 113)
POINT = {0: ((3e-3, 2e-3), (11, 12)),       # 2.026e-3, 1.028e-3
         1: ((3e-3, 2e-3), (8, 11))}        # 2.161e-3, 1.112e-3


@pytest.mark.parametrize("k", sorted(POINT))
def test_gradient_medium_from_the_ball_alone(k):
    bounds, rounds = POINT[k]
    got = []
    for nx, bound, want_rounds in zip((71, 141), bounds, rounds):
        err, r, clean = solved("point", nx, k, F.FACTORED)
        plain, rp, cp = solved("point", nx, k, F.PLAIN)
        print(f"point source {k}, {nx}: plain {plain:.3e} ({rp} rounds), factored {err:.3e} ({r} rounds), ratio {plain / err:.2f}")
        assert err <= bound
        assert err <= 0.25 * plain                       # the restatement's ratios are 5.9 to 10.1
        assert clean == 1 and r <= R.DEFAULT_ROUNDS and r == want_rounds and (rp, cp) == (2, 1)
        got.append(err)
    assert got[1] / got[0] < 0.75                        # still first order


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("nx,rounds", [(71, (12, 9)), (141, (12, 11))])
def test_constant_medium_is_exact_to_rounding(nx, rounds, k):
    err, r, clean = solved("const", nx, k, F.FACTORED)
    print(f"constant medium, source {k}, {nx}: {err:.3e} ({r} rounds)")        # 1.6e-15 to 4.4e-15; plain: 1.2e-2 and 1.9e-2
    assert err <= 1e-12 and clean == 1 and r == rounds[k]


#       case, source -> bound at 71 x 57, bound at 141 x 113, rounds
TABLES = {("wedge", 0): (2e-3, 7e-4, (7, 12)),      # 1.201e-3, 6.450e-4; plain 6.281e-3, 4.318e-3
          ("shadow", 1): (4e-4, 2e-4, (5, 5)),      # 3.113e-4, 1.772e-4; plain 3.674e-3, 1.945e-3
          ("shadow", 0): (2e-4, 9e-5, (3, 3))}      # 1.652e-4, 8.573e-5; plain 9.217e-5, 4.694e-5: worse -- that far from the
#                                                     source T0 corrects nothing that the table's own seeds have not settled


@pytest.mark.parametrize("case,k", sorted(TABLES))
def test_seeded_tables(case, k):
    b71, b141, rounds = TABLES[case, k]
    for nx, bound, want_rounds in ((71, b71, rounds[0]), (141, b141, rounds[1])):
        err, r, clean = solved(case, nx, k, F.FACTORED)
        print(f"{case} source {k}, {nx}: plain {solved(case, nx, k, F.PLAIN)[0]:.3e}, factored {err:.3e} ({r} rounds)")
        assert err <= bound and clean == 1 and r == want_rounds


@pytest.mark.parametrize("flip,rounds", [(True, 7), (False, 7)])
def test_winding_corridor_is_clean_in_both_senses(flip, rounds):
    n, (ix, iy) = R.winding_corridor(flip=flip)
    g = (0.0, 1.0, 31, 0.0, 1.0, 27)
    T, r, clean, filled, _ = F.solve_one(g, n, ix + 0.25, iy - 0.125, 1.0)
    assert r == rounds and clean == 1 and filled.all() and T[n == 1.0].max() < 500.0
    assert not R.same_bits(T, R.solve_one(g, n, ix + 0.25, iy - 0.125, 1.0)[0])


def test_the_rounds_decay_geometrically():
    """The corrected scheme is not strictly causal in T: the largest decrease of any node falls by 10 to 100 times per round"""
    g = F.GRIDS[71]
    X, Y, n = F.gradient_medium(g)
    xs, ys = F.SOURCES[0]
    hist = []
    T, rounds, clean, _, _ = F.solve_one(g, n, xs, ys, 1.0 / (18.0 + 2.0 * ys), history=hist)
    print(" ".join(f"{h:.1e}" for h in hist))           # 3.2e-02 1.7e-04 2.4e-05 1.8e-06 5.6e-08 9.2e-10 8.6e-12 4.9e-14 ...
    assert len(hist) == rounds == 11 and hist[-1] == 0.0
    assert all(b < 0.2 * a for a, b in zip(hist[1:7], hist[2:8])) and hist[7] < 1e-12 * T.max()


# ------------------------------------------------------------------------------------------------ where factoring is left out
SMALL = (0.0, 0.5, 12, -1.0, 0.25, 9)


def small_medium():
    X, Y = R.nodes(SMALL)
    return X, Y, 1.0 + 0.1 * X + 0.05 * Y


@pytest.mark.parametrize("n_src", [0.0, -1.0, np.nan, np.inf])
def test_an_obstacle_n_src_has_the_bits_of_plain(n_src):
    X, Y, n = small_medium()
    rng = np.random.default_rng(5)
    tin = np.where(rng.random(n.shape) < 0.2, rng.random(n.shape) * 3.0, np.nan)
    a = F.solve_one(SMALL, n, 1.3, -0.2, n_src, T=tin, scheme=F.FACTORED)
    b = R.solve_one(SMALL, n, 1.3, -0.2, n_src, T=tin)
    assert R.same_bits(a[0], b[0]) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[1] >= 2
    # the update itself, too
    assert F.update(SMALL, 3, 2, 1.3, -0.2, n_src, 1.0, 1.2, 1.3, 1.1, 0.9) == R.update(0.5, 0.25, 1.0, 1.1, 0.9)


def test_a_free_node_on_the_source_takes_the_plain_update():
    """ball < 0, a source on node (3, 2) and a seeded table: that node is free and rr == 0 there"""
    X, Y, n = small_medium()
    xs, ys, ns = 1.5, -0.5, 1.1
    tin = np.full(n.shape, np.nan)
    tin[2, 5], tin[6, 1] = 1.3, 2.9
    T, rounds, clean, filled, _ = F.solve_one(SMALL, n, xs, ys, ns, T=tin, ball=-1.0)
    assert clean == 1 and filled[2, 3] == 1 and F.t0(SMALL, 3, 2, xs, ys, ns)[3] == 0.0
    # at the fixed point the node's value is the plain update of its neighbours' final values, not the corrected one
    l, r, dn, up = T[2, 2], T[2, 4], T[1, 3], T[3, 3]
    assert T[2, 3] == R.update(0.5, 0.25, R.fmin(l, r), R.fmin(dn, up), n[2, 3]) == F.update(SMALL, 3, 2, xs, ys, ns, l, r, dn, up, n[2, 3])
    # its neighbour's value is the corrected update, which differs from the plain one
    l, r, dn, up = T[3, 2], T[3, 4], T[2, 3], T[4, 3]
    assert T[3, 3] == F.update(SMALL, 3, 3, xs, ys, ns, l, r, dn, up, n[3, 3]) != R.update(0.5, 0.25, R.fmin(l, r), R.fmin(dn, up), n[3, 3])


def test_scheme_0_is_the_plain_restatement_and_others_are_refused():
    X, Y, n = small_medium()
    a = F.solve_one(SMALL, n, 1.3, -0.2, 1.1, scheme=F.PLAIN)
    b = R.solve_one(SMALL, n, 1.3, -0.2, 1.1)
    assert R.same_bits(a[0], b[0]) and a[1:3] == b[1:3]
    with pytest.raises(ValueError):
        F.solve_one(SMALL, n, 1.3, -0.2, 1.1, scheme=2)
    both = F.solve(SMALL, n, [[1.3, -0.2], [0.2, 0.9]], [1.1, 1.2])
    for s, (xs, ys, ns) in enumerate(((1.3, -0.2, 1.1), (0.2, 0.9, 1.2))):
        one = F.solve_one(SMALL, n, xs, ys, ns)
        assert R.same_bits(both["T"][s], one[0]) and both["rounds"][s] == one[1] and both["converged"][s] == one[2]


def test_readings_and_the_solve_agree():
    """The solve keeps T0, px and py in tables; readings() evaluates them afresh: the same bits, since T0 is a function of the node
    alone.  At the fixed point every free node's value is not above its fresh update."""
    X, Y, n = small_medium()
    xs, ys, ns = 1.3, -0.2, 1.1
    T, rounds, clean, filled, _ = F.solve_one(SMALL, n, xs, ys, ns)
    assert clean == 1
    u, v = (X - xs) / SMALL[1], (Y - ys) / SMALL[4]
    ball = u * u + v * v <= 4.0
    hit = 0
    for j in range(9):
        for i in range(12):
            if ball[j, i]:
                continue
            l = T[j, i - 1] if i > 0 else np.inf
            r = T[j, i + 1] if i < 11 else np.inf
            dn = T[j - 1, i] if j > 0 else np.inf
            up = T[j + 1, i] if j < 8 else np.inf
            t = F.update(SMALL, i, j, xs, ys, ns, l, r, dn, up, n[j, i])
            assert not t < T[j, i]
            hit += t == T[j, i]
    assert hit > 0.9 * (~ball).sum()
