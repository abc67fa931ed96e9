"""CPU: the restatement of the linearised eikonal fill (tests/eikonal_lin_ref.py; rtmi_eikonal_tangent, rtmi_eikonal_adjoint,
DESIGN.md section 35) against the rules of its definition: the sweeps find the bits of one pass over the nodes sorted by T in
either round order; the adjoint is the tangent's transpose; T is homogeneous of degree 1 in (n, n_src) (Euler); central
differences of whole re-solves; seeds chain through dT_seed and lam; the strict-parent rule.  Each bound is the figure the
restatement itself gives (in the comment beside it), rounded up to one digit.  The device is held to the restatement bit for bit
in tests/test_gpu_eikonal_lin.py, the host arithmetic of rt_eikonal_lin.h in tests/test_eikonal_lin_host.py."""
import functools
import math

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_ref as R

CASES = ("gradient_case", "corridor_case", "disc_case", "walls_case")


@functools.lru_cache(maxsize=None)
def case(name):
    return L.filled(getattr(L, name)())


def draws(name, s, n, net):
    """dn, dn_src, dT_seed and r of source s of a case: dn 10 % of n times a normal draw, the rest normal draws"""
    rng = np.random.default_rng(1000 * CASES.index(name) + s)
    ok = np.isfinite(n)
    dn = np.where(ok, 0.1 * np.where(ok, n, 0.0) * rng.standard_normal(n.shape), 0.0)
    seeds = np.array(net.cls).reshape(n.shape) == L.SEED
    return dn, 0.1 * rng.standard_normal(), np.where(seeds, rng.standard_normal(n.shape), 0.0), rng.standard_normal(n.shape), seeds


@pytest.mark.parametrize("name", CASES)
def test_sweeps_in_either_round_order_give_the_pass_sorted_by_T(name):
    grid, n, src, ns, fill, nets = case(name)
    assert fill["converged"].all()
    for s, net in enumerate(nets):
        dn, dns, seed, r, _ = draws(name, s, n, net)
        want_t = net.tangent(dn, dns, seed, order="sorted")[0]
        want_a = net.adjoint(r, order="sorted")[:3]
        for order in ("sweeps", "other"):
            dT, rounds, clean, _ = net.tangent(dn, dns, seed, order=order)
            assert clean == 1 and R.same_bits(dT, want_t), (name, s, order)
            lam, g, g_src, rounds, clean, _ = net.adjoint(r, order=order)
            assert clean == 1 and R.same_bits(lam, want_a[0]) and R.same_bits(g, want_a[1]) and L.bits(g_src) == L.bits(want_a[2])


def test_the_walls_case_has_every_class_and_dead_nodes_are_zero():
    grid, n, src, ns, fill, nets = case("walls_case")
    for s, net in enumerate(nets):
        cls = np.array(net.cls).reshape(n.shape)
        assert {L.DEAD, L.SEED, L.FREE, L.BALL} == set(cls.reshape(-1))
        assert (cls[~(np.isfinite(n) & (n > 0))] == L.DEAD).all() and (cls[9:14, 31:35] == L.DEAD).all()      # the sealed pocket
        dn, dns, seed, r, seeds = draws("walls_case", s, n, net)
        dT = net.tangent(dn, dns, seed)[0]
        lam, g, _, _, _, _ = net.adjoint(np.where(cls == L.DEAD, np.nan, r))          # r at dead nodes is ignored
        assert (dT[cls == L.DEAD] == 0).all() and (lam[cls == L.DEAD] == 0).all() and np.isfinite(lam).all()
        assert R.same_bits(dT[seeds], seed[seeds]) and (g[cls <= L.SEED] == 0).all()


TRANSPOSE_BOUND = 3e-15         # 2.798e-15, the gradient medium's first source


def test_adjoint_is_the_transpose_of_the_tangent():
    """<J v, r> = <v, J^T r> with v = (dn, dn_src, dT_seed): the difference over |<J v, r>|, both sums exact (math.fsum)"""
    worst = 0.0
    for name in CASES:
        grid, n, src, ns, fill, nets = case(name)
        for s, net in enumerate(nets):
            dn, dns, seed, r, seeds = draws(name, s, n, net)
            live = np.array(net.cls).reshape(n.shape) != L.DEAD
            dT = net.tangent(dn, dns, seed)[0]
            lam, g, g_src, _, _, _ = net.adjoint(r)
            lhs = math.fsum((dT * r)[live])
            rhs = math.fsum(list((g * dn).reshape(-1)) + [g_src * dns] + list((lam * seed)[seeds]))
            err = abs(lhs - rhs) / abs(lhs)
            print(f"transpose, {name} source {s}: {err:.3e}")
            worst = max(worst, err)
    assert worst <= TRANSPOSE_BOUND


def test_seeds_chain_through_lam_and_dT_seed():
    """the disc case, the medium held fixed: the tangent's response to moving the seeds alone is what lam at the seeds predicts"""
    grid, n, src, ns, fill, nets = case("disc_case")
    for s, net in enumerate(nets):
        _, _, seed, r, seeds = draws("disc_case", s, n, net)
        assert seeds.sum() > 3000 and len(net.free) > 200
        dT = net.tangent(np.zeros_like(n), 0.0, seed)[0]
        assert np.abs(dT[~seeds]).max() > 0.1                       # the disc does move with its rim
        lam = net.adjoint(r)[0]
        lhs, rhs = math.fsum((dT * r).reshape(-1)), math.fsum((lam * seed)[seeds])
        print(f"seeds, source {s}: {abs(lhs - rhs) / abs(lhs):.3e}")
        assert abs(lhs - rhs) <= TRANSPOSE_BOUND * abs(lhs)


EULER_BOUND = 4e-13             # 3.671e-13, the gradient medium's first source


def ball_only(name):
    grid, n, src, ns, T = getattr(L, name)()
    return L.filled((grid, n, src, ns, None))


def test_euler_identity_on_ball_only_solves():
    """T is homogeneous of degree 1 in (n, n_src): J n + J_src n_src = T at every filled node, as a fraction of the largest T"""
    worst = 0.0
    for name in ("gradient_case", "corridor_case", "walls_case"):
        grid, n, src, ns, fill, nets = ball_only(name)
        for s, net in enumerate(nets):
            dT = net.tangent(np.where(np.isfinite(n), n, 0.0), ns[s])[0]
            got = fill["filled"][s] == 1
            err = float(np.max(np.abs(dT - fill["T"][s])[got]) / np.max(fill["T"][s][got]))
            print(f"Euler, {name} source {s}: {err:.3e}")
            worst = max(worst, err)
    assert worst <= EULER_BOUND


DIFFERENCE_BOUND = 5e-8         # 4.674e-8, the walls' second source


def test_central_differences_of_whole_re_solves():
    """(T(n + eps dn) - T(n - eps dn)) / (2 eps) against J dn on ball-only solves, eps 1e-6, dn 10 % of n times a normal draw and
    n_src moved likewise: the largest difference at a filled node as a fraction of the largest |J dn|"""
    eps, worst = 1e-6, 0.0
    for name in ("gradient_case", "walls_case"):
        grid, n, src, ns, fill, nets = ball_only(name)
        for s, net in enumerate(nets):
            dn, dns, _, _, _ = draws(name, s, n, net)
            dns *= ns[s]
            dT = net.tangent(dn, dns)[0]
            Tp = R.solve_one(grid, n + eps * dn, src[s, 0], src[s, 1], ns[s] + eps * dns)[0]
            Tm = R.solve_one(grid, n - eps * dn, src[s, 0], src[s, 1], ns[s] - eps * dns)[0]
            got = fill["filled"][s] == 1
            diff = np.abs((Tp - Tm) / (2 * eps) - dT)[got]
            err = float(diff.max() / np.abs(dT[got]).max())
            print(f"central differences, {name} source {s}: {err:.3e}")
            worst = max(worst, err)
    assert worst <= DIFFERENCE_BOUND


def test_corridor_needs_more_than_three_rounds():
    """The medium of the device's several-round test: the round counts are asserted here, so that test cannot quietly become a
    one-round case"""
    grid, n, src, ns, fill, nets = case("corridor_case")
    dn, dns, _, r, _ = draws("corridor_case", 0, n, nets[0])
    t, a = L.tangent(nets, dn), L.adjoint(nets, np.stack([r] * 3))
    assert (t["rounds"] > 3).all() and (a["rounds"] > 3).all() and t["converged"].all() and a["converged"].all()
    capped = L.tangent(nets, dn, max_rounds=1)
    assert (capped["rounds"] == 1).all() and not capped["converged"].any() and not R.same_bits(capped["dT"], t["dT"])


def test_strict_parent_rule_fires_where_the_spacing_is_absorbed():
    """a seed of 1.0 and spacings of 1e-20: a + gdx s == a, every filled node has its neighbour's T, none may name it a parent"""
    grid = (0.0, 1e-20, 6, 0.0, 1e-20, 2)
    n = np.ones((2, 6))
    T = np.full((1, 2, 6), np.nan)
    T[0, 0, 0] = 1.0
    fill = R.solve(grid, n, [[50.0, 50.0]], [1.0], T=T)
    assert (fill["T"] == 1.0).all() and fill["filled"].sum() == 11
    net = L.nets(grid, n, [[50.0, 50.0]], [1.0], fill)[0]
    assert net.cls[0] == L.SEED and all(c == L.FREE for c in net.cls[1:])
    assert not any(net.par) and not any(net.ca) and not any(net.cb)
    dn = np.arange(12.0).reshape(2, 6)
    dT, rounds, clean, _ = net.tangent(dn, 0.0, np.full((2, 6), 7.0))
    assert dT[0, 0] == 7.0 and np.array_equal(dT.reshape(-1)[1:], 1e-20 * dn.reshape(-1)[1:]) and clean == 1
    lam = net.adjoint(np.ones((2, 6)))[0]
    assert (lam == 1.0).all()
    # the same table on spacings that are not absorbed: every filled node has a parent
    grid2 = (0.0, 0.5, 6, 0.0, 0.5, 2)
    fill2 = R.solve(grid2, n, [[50.0, 50.0]], [1.0], T=T)
    net2 = L.nets(grid2, n, [[50.0, 50.0]], [1.0], fill2)[0]
    assert all(net2.par[1:])


TOMOGRAPHY_FRACTION_BOUND = 5e-2        # 4.712e-2


def test_one_tomography_step_on_the_restatement():
    """the step of the device's end-to-end test on the restatement: the figure its bound comes from"""
    grid, n0, n_true, src, rec, idx, w = L.tomography_case()

    def solve(n, ns):
        f = R.solve(grid, n, src, ns)
        assert f["converged"].all() and f["filled"].all()
        return f["T"], (n, ns, f)

    before, after, step = L.tomography_step(solve, lambda st: L.dense_jacobian(L.nets(grid, st[0], src, st[1], st[2]), rec, idx, w))
    print(f"tomography step: rms residual {before:.4e} -> {after:.4e} s, fraction {after / before:.4e}")
    assert after <= TOMOGRAPHY_FRACTION_BOUND * before
