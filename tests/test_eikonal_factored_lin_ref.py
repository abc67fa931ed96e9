"""CPU: the restatement of the factored update linearised (tests/eikonal_factored_lin_ref.py; rtmi_eikonal_params.scheme =
RTMI_EIKONAL_FACTORED_LIN) against what defines a derivative: central differences of whole factored
re-solves, beside which the plain linearisation of the same factored table (tests/eikonal_lin_ref.py, what the tangent and adjoint
gave before) is at least 100 times worse, and 1000 times for dn_src; the adjoint is the tangent's transpose with the full g_src; the
fallbacks (rr == 0, an obstacle's n_src) give the plain linearisation's numbers; the corridor needs more than three rounds; one
damped LSQR step on factored tables gains more with the consistent Jacobian.  Each bound is the figure the restatement itself gives
(in the comment beside it), rounded up to one digit.  The device is held to the restatement bit for bit in
tests/test_gpu_eikonal_factored_lin.py, the host arithmetic of rt_eikonal_lin.h in tests/test_eikonal_factored_lin_host.py."""
import functools
import math

import numpy as np
import pytest

import eikonal_factored_lin_ref as FL
import eikonal_factored_ref as F
import eikonal_lin_ref as L
import eikonal_ref as R


@functools.lru_cache(maxsize=None)
def case(name, ball_only=True):
    """(grid, n, src, n_src, the factored fill, the plain networks about it, the factored networks, the seeds' table or None)"""
    grid, n, src, ns, T = getattr(L, name)()
    T = None if ball_only else T
    return FL.filled((grid, n, src, ns, T)) + (T,)


def gradient_perturbations(s):
    """the four perturbations of source s of the gradient case: (name, dn, dn_src)"""
    grid, n, src, ns, fill, _, _, _ = case("gradient_case")
    X, Y = R.nodes(grid)
    rng = np.random.default_rng(40 + s)
    return [("smooth", 0.1 * n * np.exp(-((X - 1.0) ** 2 + (Y + 1.0) ** 2)), 0.0),
            ("rough", 0.1 * n * rng.standard_normal(n.shape), 0.0),
            ("dn_src", np.zeros_like(n), 0.1 * ns[s]),
            ("scaling", 0.1 * n, 0.1 * ns[s])]


def difference_errors(name, s, dn, dns, ball_only=True, eps=1e-6):
    """(the factored linearisation's, the plain one's) largest difference from central differences of factored re-solves at a
    filled node of source s, as fractions of the largest |dT| of the differences"""
    grid, n, src, ns, fill, plain, fact, T = case(name, ball_only)
    seeds = None if T is None else T[s]
    Tp = F.solve_one(grid, n + eps * dn, src[s, 0], src[s, 1], ns[s] + eps * dns, T=seeds)[0]
    Tm = F.solve_one(grid, n - eps * dn, src[s, 0], src[s, 1], ns[s] - eps * dns, T=seeds)[0]
    got = fill["filled"][s] == 1
    fd = ((Tp - Tm) / (2 * eps))[got]
    out = []
    for net in (fact[s], plain[s]):
        dT, _, clean, _ = net.tangent(dn, dns)
        assert clean == 1
        out.append(float(np.abs(dT[got] - fd).max() / np.abs(fd).max()))
    return out


#                 the factored linearisation's bound; the plain one is at least this many times worse
GRADIENT_BOUNDS = {"smooth": (3e-8, 100),        # 2.023e-8 and 9.445e-9; the plain linearisation 8.530e-3 and 1.445e-2
                   "rough": (5e-8, 100),         # 4.067e-8 and 2.330e-8; 2.677e-1 and 1.128e-1
                   "dn_src": (6e-7, 1000),       # 5.076e-7 and 1.464e-7; 1.177 and 0.8576
                   "scaling": (5e-9, 100)}       # 4.867e-9 and 4.893e-9; 1.426e-2 and 1.824e-2


@pytest.mark.parametrize("kind", ["smooth", "rough", "dn_src", "scaling"])
def test_central_differences_on_the_gradient_medium(kind):
    bound, worse = GRADIENT_BOUNDS[kind]
    for s in range(2):
        dn, dns = next((d, ds) for k, d, ds in gradient_perturbations(s) if k == kind)
        err, plain = difference_errors("gradient_case", s, dn, dns)
        print(f"central differences, gradient source {s}, {kind}: factored {err:.3e}, plain {plain:.3e}")
        assert err <= bound and plain >= worse * err


WALLS_BOUND = 4e-8             # 3.817e-8 and 1.618e-8; the plain linearisation 2.379e-1 and 1.470e-1
DISC_BOUND = 4e-8              # 3.538e-8 and 1.453e-8; 3.959e-2 and 6.534e-2


@pytest.mark.parametrize("name, bound", [("walls_case", "WALLS_BOUND"), ("disc_case", "DISC_BOUND")])
def test_central_differences_with_obstacles_and_on_the_disc_medium(name, bound):
    """factored solves of the walls' and the disc case, their seeds held fixed, dn 10 % of n times a normal draw and n_src moved
    likewise; the plain linearisation at least 100 times worse"""
    grid, n, src, ns, fill, plain, fact, T = case(name, False)
    for s in range(len(src)):
        rng = np.random.default_rng(70 + s)
        ok = np.isfinite(n)
        dn = np.where(ok, 0.1 * np.where(ok, n, 0.0) * rng.standard_normal(n.shape), 0.0)
        err, pl = difference_errors(name, s, dn, 0.1 * ns[s] * rng.standard_normal(), ball_only=False)
        print(f"central differences, {name} source {s}: factored {err:.3e}, plain {pl:.3e}")
        assert err <= globals()[bound] and pl >= 100 * err


TRANSPOSE_BOUND = 2e-14         # 1.133e-14, the walls' second source


def test_adjoint_is_the_transpose_of_the_tangent_with_the_full_g_src():
    """<J v, r> = <v, J^T r> with v = (dn, dn_src, dT_seed), g_src over the free nodes and the ball: the difference over
    |<J v, r>|, both sums exact (math.fsum)"""
    worst = 0.0
    for name, ball_only in (("gradient_case", True), ("corridor_case", True), ("walls_case", False), ("disc_case", False)):
        grid, n, src, ns, fill, plain, fact, T = case(name, ball_only)
        for s, net in enumerate(fact):
            rng = np.random.default_rng(90 + s)
            ok = np.isfinite(n)
            dn = np.where(ok, 0.1 * np.where(ok, n, 0.0) * rng.standard_normal(n.shape), 0.0)
            dns = 0.1 * rng.standard_normal()
            cls = np.array(net.cls).reshape(n.shape)
            seeds = cls == L.SEED
            seed, r = np.where(seeds, rng.standard_normal(n.shape), 0.0), rng.standard_normal(n.shape)
            dT, _, clean_t, _ = net.tangent(dn, dns, seed)
            lam, g, g_src, _, clean_a, _ = net.adjoint(r)
            assert clean_t == 1 and clean_a == 1
            free_share = sum(net.csrc[x] * lam.reshape(-1)[x] for x in net.free)
            assert name == "corridor_case" or abs(free_share) > 0.1 * abs(g_src)          # the free nodes carry g_src
            lhs = math.fsum((dT * r)[cls != L.DEAD])
            rhs = math.fsum(list((g * dn).reshape(-1)) + [g_src * dns] + list((lam * seed)[seeds]))
            err = abs(lhs - rhs) / abs(lhs)
            print(f"transpose, {name} source {s}: {err:.3e}")
            worst = max(worst, err)
    assert worst <= TRANSPOSE_BOUND


def test_corridor_needs_more_than_three_rounds_and_the_gradient_medium_as_many_as_its_fill():
    grid, n, src, ns, fill, plain, fact, T = case("corridor_case")
    rng = np.random.default_rng(5)
    dn, r = rng.standard_normal(n.shape), rng.standard_normal(n.shape)
    t, a = FL.tangent(fact, dn), FL.adjoint(fact, np.stack([r] * 3))
    assert (t["rounds"] > 3).all() and (a["rounds"] > 3).all() and t["converged"].all() and a["converged"].all()
    capped = FL.tangent(fact, dn, max_rounds=1)
    assert (capped["rounds"] == 1).all() and not capped["converged"].any() and not R.same_bits(capped["dT"], t["dT"])
    grid, n, src, ns, fill, plain, fact, T = case("gradient_case")
    t, p = FL.tangent(fact, 0.1 * n, 0.1 * ns), L.tangent(plain, 0.1 * n, 0.1 * ns)
    print("rounds on the gradient medium: fill", fill["rounds"], "factored tangent", t["rounds"], "plain tangent", p["rounds"])
    assert (t["rounds"] >= 7).all() and (t["rounds"] <= 11).all() and (p["rounds"] <= 3).all() and t["converged"].all()


def test_the_corrected_readings_keep_parents_that_the_raw_rule_would_drop():
    """On the gradient medium some free nodes have a raw parent that is not below them; the rule on the corrected reading keeps
    it, and never fires there"""
    grid, n, src, ns, fill, plain, fact, T = case("gradient_case")
    raw_not_below = 0
    for s, net in enumerate(fact):
        T = net.T
        for x in net.free:
            p = net.par[x]
            assert p == plain[s].par[x] | p                  # every parent the plain rule kept is kept, on the same side
            if p & L.XPARENT:
                raw_not_below += not T[x + 1 if p & L.XEAST else x - 1] < T[x]
            if p & L.YPARENT:
                raw_not_below += not T[x + net.nx if p & L.YNORTH else x - net.nx] < T[x]
        assert all(net.par[x] for x in net.free)
    print("parents whose raw reading is not below the node:", raw_not_below)
    assert raw_not_below > 50


def test_fallbacks_give_the_plain_linearisation():
    """an obstacle's n_src: every free node; a source on a node: that node alone, were it free (it is of the ball: csrc is the
    ball's) -- and coef() at rr == 0 is eikonal_lin_ref.coef with csrc 0"""
    grid, n, src, ns, T = L.walls_case()
    for bad in (-1.0, math.nan, math.inf, 0.0):
        fill = F.solve(grid, n, src, [bad, bad], T=T)
        for a, b in zip(L.nets(grid, n, src, [bad, bad], fill), FL.nets(grid, n, src, [bad, bad], fill)):
            assert a.free and (a.par, a.ca, a.cb, a.cs, a.cls) == (b.par, b.ca, b.cb, b.cs, b.cls) and not any(b.csrc[x] for x in b.free)
            rng = np.random.default_rng(3)
            dn, r = np.where(np.isfinite(n), rng.standard_normal(n.shape), 0.0), rng.standard_normal(n.shape)
            assert R.same_bits(a.tangent(dn, 0.25)[0], b.tangent(dn, 0.25)[0])
            la, ga, sa = a.adjoint(r)[:3]
            lb, gb, sb = b.adjoint(r)[:3]
            assert R.same_bits(la, lb) and R.same_bits(ga, gb) and sa == sb == 0.0
    g = (0.0, 0.5, 9, 0.0, 0.25, 7)
    got = FL.coef(g, 4, 3, 2.0, 0.75, 1.5, 1.0, 1.25, 0.9, 2.0, 1.5, 1.2)
    assert got == L.coef(0.5, 0.25, 1.0, 1.25, 0.9, 2.0, 1.5, 1.2)[:3] + (0.0,) + L.coef(0.5, 0.25, 1.0, 1.25, 0.9, 2.0, 1.5, 1.2)[3:]
    assert got[4] == L.XPARENT | L.YPARENT
    moved = FL.coef(g, 4, 3, 2.0 + 1e-3, 0.75, 1.5, 1.0, 1.25, 0.9, 2.0, 1.5, 1.2)
    assert moved[3] != 0.0 and moved[:3] != got[:3]


def test_the_sparse_jacobian_is_the_sweeps_jacobian():
    """the rows of eikonal_factored_lin_ref.jacobian against adjoint sweeps of the restatement, to rounding"""
    grid, n0, n_true, src, rec, idx, w = L.tomography_case()
    src, idx, w = src[[0, 5]], idx[[0, 5]], w[[0, 5]]
    ns = (n0.reshape(-1)[idx] * w).sum(axis=1)
    nets = FL.nets(grid, n0, src, ns, F.solve(grid, n0, src, ns))
    J = FL.jacobian(nets, rec[[3, 20]], idx, w)
    for s, net in enumerate(nets):
        for k, x in enumerate(rec[[3, 20]]):
            r = np.zeros(n0.size)
            r[x] = 1.0
            _, g, g_src, _, clean, _ = net.adjoint(r)
            row = g.reshape(-1).copy()
            np.add.at(row, idx[s], g_src * w[s])
            assert clean == 1 and np.abs(J[2 * s + k] - row).max() <= 1e-13 * np.abs(row).max()


LSQR_FRACTION_BOUND = 5e-2      # 4.1476e-2; the plain Jacobian of the same tables 6.7876e-2


def test_one_lsqr_step_gains_more_with_the_consistent_jacobian():
    """eikonal_lin_ref's damped LSQR step on factored tables of its eight sources, with the dense Jacobian: the rms residual
    after over before, under the factored linearisation and under the plain one of the same tables"""
    b0, a0, _ = FL.tomography_step("plain")
    b1, a1, _ = FL.tomography_step("factored")
    print(f"LSQR step on factored tables: plain Jacobian {a0 / b0:.4e}, factored Jacobian {a1 / b1:.4e}")
    assert b0 == b1 and a1 / b1 <= LSQR_FRACTION_BOUND and a1 / b1 < a0 / b0
