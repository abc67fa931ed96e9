"""First-arrival eikonal tomography restated (rtmi_eikonal_tomo_*, include/rtmi.h; raytracing_amd/csrc/rt_eikonal_tomo.h;
DESIGN.md section 36) in plain Python floats over tests/eikonal_lin_ref.py: the cell weights of a point, the sample, the live
rows, the lists of the transposed product, both products, the residual and the stacked operator of the solver.  Every product
and sum below is one rounded fp64 operation.  Arrays go in and out as numpy, the arithmetic runs on Python floats.  Test
infrastructure."""
import functools
import math

import numpy as np

import eikonal_lin_ref as L
import eikonal_ref as R
import tomo_basis_ref as TB
import tomo_ref as TR


def axis(u, n):
    """(i0, i1, f) of coordinate u on an axis of n nodes"""
    top = max(n - 2, 0)
    fl = math.floor(u) if math.isfinite(u) else (top if u > 0 else 0)
    i0 = min(max(fl, 0), top)
    i1 = min(i0 + 1, n - 1)
    return i0, i1, (u - float(i0) if i1 > i0 else 0.0)


def cell(grid, x, y, source=False):
    """(idx [4], w [4], inside) of the point (x, y); a source that is not inside has i0 = j0 = 0 and four weights +0.0"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    gx0, gdx, gy0, gdy, nx, ny = float(gx0), float(gdx), float(gy0), float(gdy), int(nx), int(ny)
    u = (float(x) - gx0) / gdx
    v = (float(y) - gy0) / gdy
    inside = 0.0 <= u <= float(nx - 1) and 0.0 <= v <= float(ny - 1)
    zero = source and not inside
    if zero:
        u = v = 0.0
    i0, i1, fu = axis(u, nx)
    j0, j1, fv = axis(v, ny)
    idx = [j0 * nx + i0, j0 * nx + i1, j1 * nx + i0, j1 * nx + i1]
    gu = 1.0 - fu
    gv = 1.0 - fv
    w = [0.0] * 4 if zero else [gu * gv, fu * gv, gu * fv, fu * fv]
    return idx, w, inside


def cells(grid, points, source=False):
    """(idx [P, 4] int64, w [P, 4], inside [P] bool) of points [P, 2]"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    out = [cell(grid, x, y, source) for x, y in pts]
    return (np.array([c[0] for c in out], dtype=np.int64).reshape(-1, 4), np.array([c[1] for c in out]).reshape(-1, 4),
            np.array([c[2] for c in out], dtype=bool))


def receiver_ok(grid, x, y):
    gx0, gdx, nx, gy0, gdy, ny = grid
    return (math.isfinite(x) and math.isfinite(y) and float(gx0) <= x <= float(gx0) + float(int(nx) - 1) * float(gdx)
            and float(gy0) <= y <= float(gy0) + float(int(ny) - 1) * float(gdy))


def sample(v, idx, w):
    """((w0 v0 + w1 v1) + w2 v2) + w3 v3 on a list (or flat array) v"""
    return ((w[0] * float(v[idx[0]]) + w[1] * float(v[idx[1]])) + w[2] * float(v[idx[2]])) + w[3] * float(v[idx[3]])


def lists(idx, take=None):
    """(node, off, pair): the (point, corner) pairs 4 k + c sorted by node and then by pair, with the touched nodes and offsets"""
    idx = np.asarray(idx).reshape(-1, 4)
    allp = sorted((int(idx[k, c]), 4 * k + c) for k in range(len(idx)) if take is None or take[k] for c in range(4))
    node, off, pair = [], [], []
    for p, (x, pr) in enumerate(allp):
        if p == 0 or x != allp[p - 1][0]:
            node.append(x)
            off.append(p)
        pair.append(pr)
    off.append(len(allp))
    return np.array(node, dtype=np.int32), np.array(off, dtype=np.int32), np.array(pair, dtype=np.int32)


class NotConverged(RuntimeError):
    pass


class Operator:
    """The handle restated: nets of every source, the weights, the live rows and both products"""

    def __init__(self, grid, n, sources, n_src, fill, receivers, ball=2.0, max_rounds=0):
        self.grid = grid
        self.nx, self.ny = int(grid[2]), int(grid[5])
        self.nn = self.nx * self.ny
        self.n = np.asarray(n, dtype=np.float64)
        self.src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
        self.rec = np.asarray(receivers, dtype=np.float64).reshape(-1, 2)
        self.S, self.R = len(self.src), len(self.rec)
        self.max_rounds = max_rounds
        self.fill = fill
        self.nets = L.nets(grid, n, self.src, n_src, fill, ball)
        self.ridx, self.rw, _ = cells(grid, self.rec)
        self.sidx, self.sw, self.inside = cells(grid, self.src, source=True)
        self.rlist = lists(self.ridx)
        self.live = np.array([[all(net.cls[x] != L.DEAD for x in self.ridx[k]) for k in range(self.R)] for net in self.nets], dtype=bool)
        self.live_per = self.live.sum(axis=1)

    @property
    def shape(self):
        return self.S * self.R, self.nn

    def dn_src(self, dn):
        dn = np.asarray(dn, dtype=np.float64).reshape(-1)
        return [sample(dn, self.sidx[s], self.sw[s]) if self.inside[s] else 0.0 for s in range(self.S)]

    def apply(self, dn):
        """y [S R] = A dn"""
        dn = np.asarray(dn, dtype=np.float64).reshape(self.ny, self.nx)
        ds = self.dn_src(dn)
        y = np.zeros(self.S * self.R)
        for s, net in enumerate(self.nets):
            dT, _, clean, _ = net.tangent(dn, ds[s], None, max_rounds=self.max_rounds)
            if not clean:
                raise NotConverged("tangent")
            dT = dT.reshape(-1)
            for k in range(self.R):
                if self.live[s, k]:
                    y[s * self.R + k] = sample(dT, self.ridx[k], self.rw[k])
        return y

    def spread(self, y, s):
        """r_s [nn]: the gather over the (receiver, corner) list; a dead row's entry is not read"""
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        node, off, pair = self.rlist
        r = np.zeros(self.nn)
        w = self.rw.reshape(-1)
        for q, x in enumerate(node):
            acc = 0.0
            for p in range(off[q], off[q + 1]):
                pr = int(pair[p])
                k = pr >> 2
                if self.live[s, k]:
                    acc = acc + float(w[pr]) * float(y[s * self.R + k])
            r[x] = acc
        return r

    def transpose(self, y, parts=False):
        """G [nn] = A^T y; with parts also the per-source g [S, nn] and g_src [S]"""
        gs, gsrc = [], []
        for s, net in enumerate(self.nets):
            _, g, g_src, _, clean, _ = net.adjoint(self.spread(y, s), max_rounds=self.max_rounds)
            if not clean:
                raise NotConverged("adjoint")
            gs.append(g.reshape(-1))
            gsrc.append(g_src)
        G = self.reduce(gs, gsrc)
        return (G, np.array(gs), np.array(gsrc)) if parts else G

    def reduce(self, gs, gsrc, sidx=None, sw=None, inside=None):
        """G from the sources' g and g_src: the sum over s in increasing order, then the (source, corner) list"""
        sidx = self.sidx if sidx is None else sidx
        sw = self.sw if sw is None else sw
        inside = self.inside if inside is None else inside
        node, off, pair = lists(sidx, inside)
        G = [0.0] * self.nn
        for g in gs:
            for x in range(self.nn):
                G[x] = G[x] + float(g[x])
        w = np.asarray(sw).reshape(-1)
        for q, x in enumerate(node):
            for p in range(off[q], off[q + 1]):
                pr = int(pair[p])
                G[x] = G[x] + float(w[pr]) * float(gsrc[pr >> 2])
        return np.array(G)

    def residual(self, picks):
        picks = np.asarray(picks, dtype=np.float64).reshape(-1)
        res = np.zeros(self.S * self.R)
        for s in range(self.S):
            T = self.fill["T"][s].reshape(-1)
            for k in range(self.R):
                p = float(picks[s * self.R + k])
                if self.live[s, k] and not math.isnan(p):
                    res[s * self.R + k] = p - sample(T, self.ridx[k], self.rw[k])
        return res

    def dense(self):
        """A as a dense [S R, nn] matrix, row by row through the transposed product"""
        J = np.zeros(self.shape)
        for row in range(self.S * self.R):
            e = np.zeros(self.S * self.R)
            e[row] = 1.0
            J[row] = self.transpose(e)
        return J

    def dense_by_nodes(self):
        """A as a dense matrix in numpy arithmetic (not bit-defined): one adjoint solve per (source, touched node with a weight),
        combined with the receivers' weights, n_src chained through the sources' weights"""
        J = np.zeros(self.shape)
        for s, net in enumerate(self.nets):
            rows = {}
            for k in range(self.R):
                if not self.live[s, k]:
                    continue
                for c in range(4):
                    x, w = int(self.ridx[k, c]), float(self.rw[k, c])
                    if w == 0.0:
                        continue
                    if x not in rows:
                        r = np.zeros(self.nn)
                        r[x] = 1.0
                        _, g, g_src, _, _, _ = net.adjoint(r, order="sorted")
                        row = g.reshape(-1).copy()
                        if self.inside[s]:
                            np.add.at(row, self.sidx[s], g_src * self.sw[s])
                        rows[x] = row
                    J[s * self.R + k] += w * rows[x]
        return J

    def stacked(self, d1=None, d2=None):
        """(matvec, rmatvec, rows of the regulariser) of [A | Dx | Dy | Dxx | Dyy] on the node grid, as tomo_basis_ref.stacked"""
        d1, d2 = TB._present(d1), TB._present(d2)
        rows, gx, gy = self.S * self.R, self.nx, self.ny
        n1, nr = TB.n_reg(gx, gy, d1, d2)

        def mv(s):
            s = np.asarray(s, dtype=np.float64).reshape(-1)
            parts = [self.apply(s)]
            if d1 is not None:
                parts.append(TR.diff_forward(s, gx, gy, *d1))
            if d2 is not None:
                parts.append(TB.diff2_forward(s, gx, gy, *d2))
            return np.concatenate(parts)

        def rmv(u):
            u = np.asarray(u, dtype=np.float64).reshape(-1)
            g = self.transpose(u[:rows])
            if d1 is not None and d2 is not None:
                return g + (TR.diff_transpose(u[rows:rows + n1], gx, gy, *d1) + TB.diff2_transpose(u[rows + n1:], gx, gy, *d2))
            if d1 is not None:
                return g + TR.diff_transpose(u[rows:], gx, gy, *d1)
            if d2 is not None:
                return g + TB.diff2_transpose(u[rows:], gx, gy, *d2)
            return g
        return mv, rmv, nr


def operator(case, receivers, max_rounds=0):
    """the Operator of an eikonal_lin_ref case (grid, n, src, n_src, T) with the restatement's own fill"""
    grid, n, src, ns, fill, _ = L.filled(case)
    return Operator(grid, n, src, ns, fill, receivers, max_rounds=max_rounds)


# ------------------------------------------------------------------------------------------------ cases for the tests
def at(grid, u, v):
    """the point at node coordinates (u, v), clipped to the grid"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    u, v = min(max(u, 0.0), nx - 1.0), min(max(v, 0.0), ny - 1.0)
    return [gx0 + u * gdx, gy0 + v * gdy]


def shape_receivers(grid):
    """Eight receivers: on a node, on an edge, two in one cell, on the last column, on the last row, in the corner cell, on the
    corner node"""
    nx, ny = grid[2], grid[5]
    uv = [(2.0, 3.0), (2.5, 3.0), (1.25, 1.5), (1.75, 1.25), (nx - 1.0, 2.5), (1.5, ny - 1.0), (nx - 1.3, ny - 1.4), (nx - 1.0, ny - 1.0)]
    return np.array([at(grid, u, v) for u, v in uv])


SHAPE_GRIDS = {"13x11": (0.5, 0.25, 13, -1.0, 0.2, 11), "1x9": (0.5, 0.25, 1, -1.0, 0.2, 9), "9x1": (0.5, 0.25, 9, -1.0, 0.2, 1),
               "65x63": (0.5, 0.05, 65, -1.0, 0.04, 63)}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(grid, n, src, n_src, receivers, Operator) on a smooth medium: one source on a node, one inside a cell, one outside the
    grid (S = 3; on 65 x 63 two more inside, S = 5)"""
    grid = SHAPE_GRIDS[name]
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = R.nodes(grid)
    med = lambda x, y: 1.0 + 0.25 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2)      # noqa: E731
    n = med(X, Y)
    src = [at(grid, 1.0, 2.0), at(grid, nx / 2 - 0.3, ny / 2 - 0.6), [gx0 - 0.6 * gdx, gy0 - 0.7 * gdy]]
    if name == "65x63":
        src += [at(grid, 50.4, 10.2), at(grid, 7.7, 55.5)]
    src = np.array(src)
    ns = med(src[:, 0], src[:, 1])
    fill = R.solve(grid, n, src, ns)
    rec = shape_receivers(grid)
    return grid, n, src, ns, rec, Operator(grid, n, src, ns, fill, rec)


WALLS_RECEIVERS = np.array([[-1.0 + 0.1 * 3.5, 0.5 + 0.125 * 19.5],        # a corner is n = inf: dead for both sources
                            [-1.0 + 0.1 * 32.5, 0.5 + 0.125 * 11.5],       # in the sealed pocket: unreached
                            [-1.0 + 0.1 * 5.25, 0.5 + 0.125 * 4.5], [-1.0 + 0.1 * 18.0, 0.5 + 0.125 * 20.0],
                            [-1.0 + 0.1 * 20.5, 0.5 + 0.125 * 2.0],        # a corner is n = 0
                            [-1.0 + 0.1 * 30.75, 0.5 + 0.125 * 25.25], [-1.0 + 0.1 * 36.0, 0.5 + 0.125 * 28.0],
                            [-1.0 + 0.1 * 11.5, 0.5 + 0.125 * 2.5]])


@functools.lru_cache(maxsize=None)
def walls():
    """(grid, n, src, n_src, fill, receivers, Operator) of eikonal_lin_ref.walls_case with receivers that give dead and live rows"""
    grid, n, src, ns, fill, _ = L.filled(L.walls_case())
    return grid, n, src, ns, fill, WALLS_RECEIVERS, Operator(grid, n, src, ns, fill, WALLS_RECEIVERS)


# ------------------------------------------------------------------------------------ the off-node tomography step
def tomography_receivers():
    """eikonal_lin_ref.tomography_case's receivers moved half a cell along their edges: [R, 2] coordinates"""
    grid, _, _, _, rec, _, _ = L.tomography_case()
    gx0, gdx, nx, gy0, gdy, ny = grid
    pts = []
    for x in rec:
        i, j = int(x) % nx, int(x) // nx
        if i == nx - 1:                                     # the east edge; the corner node moves down, the others up
            pts.append([gx0 + i * gdx, gy0 + (j + 0.5 if j < ny - 1 else j - 0.5) * gdy])
        else:
            pts.append([gx0 + min(i + 0.5, nx - 1.0) * gdx, gy0 + j * gdy])
    return np.array(pts)


def tomography_hooks(solve_tables, jacobian):
    """The (solve, jacobian) pair that eikonal_lin_ref.tomography_step wants, for receivers off the nodes: tomography_step reads
    a table at its receiver nodes, so solve returns a table that holds at receiver k's node the sample at the moved receiver k.
    solve_tables(n, n_src) -> (T [S, ny, nx], state)"""
    grid, _, _, src, rec, _, _ = L.tomography_case()
    pts = tomography_receivers()
    ridx, rw, _ = cells(grid, pts)

    def solve(n, n_src):
        T, state = solve_tables(n, n_src)
        flat = T.reshape(len(src), -1)
        out = np.zeros_like(flat)
        for s in range(len(src)):
            for k, x in enumerate(rec):
                out[s, x] = sample(flat[s], ridx[k], rw[k])
        return out, state
    return solve, jacobian


TOMO_BOUND = 0.05       # the residual fraction of one off-node step: the restatement's own 0.0467 rounded up to one digit


@functools.lru_cache(maxsize=None)
def solver_case():
    """(grid, n, src, n_src, receivers, Operator, picks) for the solver on 13 x 11: an obstacle node next to receiver 3, so that
    every source has a dead row, and a pick that is absent"""
    grid = SHAPE_GRIDS["13x11"]
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = R.nodes(grid)
    med = lambda x, y: 1.0 + 0.25 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2)      # noqa: E731
    n = med(X, Y)
    n[6, 7] = np.nan
    src = np.array([at(grid, 1.0, 2.0), at(grid, 10.3, 8.6), [gx0 - 0.6 * gdx, gy0 + 4.2 * gdy]])
    ns = med(src[:, 0], src[:, 1])
    fill = R.solve(grid, n, src, ns)
    rec = np.array([at(grid, u, v) for u, v in [(12.0, 1.5), (11.5, 9.0), (4.25, 10.0), (7.5, 6.5), (2.0, 7.0), (9.75, 3.25), (9.25, 3.75)]])
    op = Operator(grid, n, src, ns, fill, rec)
    truth = n * (1.0 + 0.05 * np.exp(-((X - 2.0) ** 2 + (Y - 0.0) ** 2) / 0.5))
    op_true = Operator(grid, truth, src, ns, R.solve(grid, truth, src, ns), rec)
    picks = -op_true.residual(np.zeros(op.S * op.R))
    picks[op.R + 1] = np.nan
    return grid, n, src, ns, rec, op, picks
