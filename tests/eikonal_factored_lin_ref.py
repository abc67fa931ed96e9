"""The factored eikonal update linearised, restated (rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED_LIN on rtmi_eikonal_tangent,
rtmi_eikonal_adjoint and all that goes through them, include/rtmi.h; raytracing_amd/csrc/rt_eikonal_lin.h) in
plain Python floats, on top of eikonal_lin_ref (classes, seeds, ball nodes, dead nodes, the gathers and the sweep orders) and
eikonal_factored_ref (the corrected readings).  Every product, sum, quotient and sqrt below is one rounded fp64 operation.

For a free node x = (i, j) of a source whose n_src is no obstacle's, with rr[x] != 0 (F.t0's expressions):
    the parents are chosen on the raw readings (east iff r < l, north iff up < dn); a, b are F.readings' corrected readings
    ca, cb, cs, the branch and the strict-parent rule are eikonal_lin_ref.coef's on a and b (the rule tests a < t, b < t)
    ka = (rr[x] - rr[x-parent]) +- gdx (dx / rr[x]), + for east;  kb = (rr[x] - rr[y-parent]) +- gdy (dy / rr[x]), + for north
    csrc = the sum from +0.0 of ca ka (where the node has an x-parent) and cb kb (where it has a y-parent)
Every other free node has eikonal_lin_ref's coefficients and csrc = 0.
Tangent: a free node's constant term is (cs dn) + (csrc dn_src); the gather is eikonal_lin_ref's.
Adjoint: the gather is eikonal_lin_ref's; g_src = the sum from +0.0 over the rows in ascending j of each row's sum from +0.0,
over i ascending, of csrc lam at its free nodes and nodes of the ball.
The corrected network is not provably acyclic, so the bits are those of eikonal_lin_ref's sweep orders from its starting values,
capped by max_rounds; clean = 0 means the last sweep's values.  order="sorted" does not apply."""
import math

import numpy as np

import eikonal_factored_ref as F
import eikonal_lin_ref as L
import eikonal_ref as R

INF = math.inf
DEAD, SEED, FREE, BALL = L.DEAD, L.SEED, L.FREE, L.BALL
bits = L.bits


def coef(grid, i, j, xs, ys, n_src, l, r, dn, up, s, t):
    """(ca, cb, cs, csrc, parents) of free node (i, j) whose value is t, from its four raw neighbour readings"""
    gdx, gdy = grid[1], grid[4]
    _, dx, dy, rr = F.t0(grid, i, j, xs, ys, n_src)
    if R.obstacle(n_src) or rr == 0.0:
        ca, cb, cs, par = L.coef(gdx, gdy, l, r, dn, up, s, t)
        return ca, cb, cs, 0.0, par
    east, north = r < l, up < dn
    a, b = F.readings(grid, i, j, xs, ys, n_src, l, r, dn, up)
    # the corrected reading on the side the raw readings chose, +inf on the other: coef's min and its side are then a, b and that side
    ca, cb, cs, par = L.coef(gdx, gdy, INF if east else a, a if east else INF, INF if north else b, b if north else INF, s, t)
    csrc = 0.0
    if par & L.XPARENT:
        d = rr - F.t0(grid, i + 1 if east else i - 1, j, xs, ys, n_src)[3]
        p = gdx * (dx / rr)
        ka = d + p if east else d - p
        csrc = csrc + ca * ka
    if par & L.YPARENT:
        d = rr - F.t0(grid, i, j + 1 if north else j - 1, xs, ys, n_src)[3]
        p = gdy * (dy / rr)
        kb = d + p if north else d - p
        csrc = csrc + cb * kb
    return ca, cb, cs, csrc, par


class Net(L.Net):
    """One source's network of the factored update: eikonal_lin_ref.Net with the free nodes' coefficients replaced"""

    def __init__(self, grid, n, xs, ys, n_src, T, filled, ball=2.0):
        super().__init__(grid, n, xs, ys, n_src, T, filled, ball)
        gx0, gdx, nx, gy0, gdy, ny = grid
        g = (float(gx0), float(gdx), int(nx), float(gy0), float(gdy), int(ny))
        nx, ny = g[2], g[5]
        nl = [float(v) for v in np.asarray(n, dtype=np.float64).reshape(-1)]
        tl = self.T
        rd = [L.read(nl[x], tl[x]) for x in range(self.nn)]
        xs, ys, n_src = float(xs), float(ys), float(n_src)
        for x in self.free:
            i, j = x % nx, x // nx
            l = rd[x - 1] if i > 0 else INF
            r = rd[x + 1] if i + 1 < nx else INF
            dn = rd[x - nx] if j > 0 else INF
            up = rd[x + nx] if j + 1 < ny else INF
            self.ca[x], self.cb[x], self.cs[x], self.csrc[x], self.par[x] = coef(g, i, j, xs, ys, n_src, l, r, dn, up, nl[x], tl[x])

    def run(self, gather, v, nodes, adjoint, order, max_rounds):
        assert order != "sorted", "the corrected network is not ordered by T"
        return super().run(gather, v, nodes, adjoint, order, max_rounds)

    def tangent(self, dn, dn_src=0.0, dT_seed=None, order="sweeps", max_rounds=0):
        """(dT [ny, nx], rounds, clean, changes)"""
        nn, nx = self.nn, self.nx
        dnl = [float(v) for v in np.asarray(dn, dtype=np.float64).reshape(-1)]
        sd = None if dT_seed is None else [float(v) for v in np.asarray(dT_seed, dtype=np.float64).reshape(-1)]
        dn_src = float(dn_src)
        v, k = [0.0] * nn, [0.0] * nn
        for x in range(nn):
            c = self.cls[x]
            if c == SEED:
                v[x] = 0.0 if sd is None else sd[x]
            elif c == BALL:
                v[x] = (0.0 + self.cs[x] * dnl[x]) + self.csrc[x] * dn_src
            elif c == FREE:
                k[x] = self.cs[x] * dnl[x] + self.csrc[x] * dn_src
        par, ca, cb = self.par, self.ca, self.cb

        def gather(x):
            p = par[x]
            acc = 0.0
            if p & L.XPARENT:
                acc = acc + ca[x] * v[x + 1 if p & L.XEAST else x - 1]
            if p & L.YPARENT:
                acc = acc + cb[x] * v[x + nx if p & L.YNORTH else x - nx]
            return acc + k[x]

        rounds, clean, changes = self.run(gather, v, self.free, False, order, max_rounds)
        return np.array(v).reshape(self.ny, nx), rounds, clean, changes

    def adjoint(self, r, order="sweeps", max_rounds=0):
        """(lam [ny, nx], g [ny, nx], g_src, rounds, clean, changes)"""
        lam, g, _, rounds, clean, changes = super().adjoint(r, order, max_rounds)
        v = lam.reshape(-1)
        g_src = 0.0
        for j in range(self.ny):
            row = 0.0
            for x in range(j * self.nx, (j + 1) * self.nx):
                if self.cls[x] >= FREE:
                    row = row + self.csrc[x] * float(v[x])
            g_src = g_src + row
        return lam, g, g_src, rounds, clean, changes


def nets(grid, n, sources, n_src, fill, ball=2.0):
    """the network of every source of a fill result (a dict with T and filled [S, ny, nx])"""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_src, dtype=np.float64).reshape(-1)
    return [Net(grid, n, src[s, 0], src[s, 1], ns[s], fill["T"][s], fill["filled"][s], ball) for s in range(len(src))]


tangent, adjoint = L.tangent, L.adjoint         # over a list of networks, of either kind


def filled(case, max_rounds=0):
    """(grid, n, src, n_src, the factored fill of the restatement, the plain networks, the factored networks) of a case"""
    grid, n, src, ns, T = case
    fill = F.solve(grid, n, src, ns, T=T, max_rounds=max_rounds)
    return grid, n, src, ns, fill, L.nets(grid, n, src, ns, fill), nets(grid, n, src, ns, fill)


# -------------------------------------------------------------------------------------------- the Jacobian at receiver nodes
def jacobian(nets_, rec, idx, w):
    """The dense Jacobian of the networks' fixed point at the receiver nodes `rec`, n_src chained through the bilinear weights
    (idx, w): one sparse solve per source with the transposed network, which agrees with the sweeps to rounding and costs a
    fraction of them.  Rows s R + k."""
    from scipy.sparse import csr_matrix, identity
    from scipy.sparse.linalg import splu
    nn, nx = nets_[0].nn, nets_[0].nx
    J = np.zeros((len(nets_) * len(rec), nn))
    for s, net in enumerate(nets_):
        rows, cols, vals = [], [], []
        for x in net.free:
            p = net.par[x]
            if p & L.XPARENT:
                rows.append(x), cols.append(x + 1 if p & L.XEAST else x - 1), vals.append(net.ca[x])
            if p & L.YPARENT:
                rows.append(x), cols.append(x + nx if p & L.YNORTH else x - nx), vals.append(net.cb[x])
        P = csr_matrix((vals, (rows, cols)), shape=(nn, nn))
        E = np.zeros((nn, len(rec)))
        E[rec, np.arange(len(rec))] = 1.0
        lam = splu((identity(nn, format="csc") - P.T.tocsc())).solve(E)            # [nn, R]: the adjoint states
        cls = np.array(net.cls)
        cs = np.where(cls >= FREE, np.array(net.cs), 0.0)
        csrc = np.where(cls >= FREE, np.array(net.csrc), 0.0)
        block = J[s * len(rec):(s + 1) * len(rec)]
        block += (lam * cs[:, None]).T
        g_src = csrc @ lam                                                         # [R]
        for q in range(4):
            np.add.at(block, (np.arange(len(rec)), np.full(len(rec), idx[s, q])), g_src * w[s, q])
    return J


def tomography_step(linearise, sources=range(8)):
    """eikonal_lin_ref.tomography_step's damped LSQR step on factored tables of `sources` of its case, with the Jacobian of the
    plain linearisation about them ("plain") or of the factored one ("factored").  -> (rms before, after, the step [ny, nx])"""
    from scipy.sparse.linalg import lsqr
    grid, n0, n_true, src, rec, idx, w = L.tomography_case()
    src, idx, w = src[list(sources)], idx[list(sources)], w[list(sources)]
    at = lambda T: T.reshape(len(src), -1)[:, rec].reshape(-1)      # noqa: E731
    ns = lambda n: (n.reshape(-1)[idx] * w).sum(axis=1)             # noqa: E731

    def solve(n):
        f = F.solve(grid, n, src, ns(n))
        assert f["converged"].all() and f["filled"].all()
        return f

    data = at(solve(n_true)["T"])
    f0 = solve(n0)
    r0 = data - at(f0["T"])
    make = {"plain": L.nets, "factored": nets}[linearise]
    J = jacobian(make(grid, n0, src, ns(n0), f0), rec, idx, w)
    step = lsqr(J, r0, damp=L.TOMO_DAMP, iter_lim=L.TOMO_ITERS, atol=0.0, btol=0.0)[0].reshape(n0.shape)
    r1 = data - at(solve(n0 + step)["T"])
    rms = lambda r: float(np.sqrt(np.mean(r * r)))                  # noqa: E731
    return rms(r0), rms(r1), step
