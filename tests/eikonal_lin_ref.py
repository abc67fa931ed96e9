"""The linearised eikonal fill restated (rtmi_eikonal_tangent, rtmi_eikonal_adjoint, include/rtmi.h;
raytracing_amd/csrc/rt_eikonal_lin.h) in plain Python floats over tests/eikonal_ref.py: every product, sum,
quotient and sqrt below is one rounded fp64 operation.  Arrays go in and out as numpy, the arithmetic runs on Python lists.
order= picks the schedule that finds the fixed point: "sweeps" (the definition, which also defines rounds), "other" (the other
map's sweep orders) and "sorted" (one pass over the nodes sorted by T, upwards for the tangent, downwards for the adjoint)."""
import math
import struct

import numpy as np

import eikonal_ref as R

INF = math.inf
DEAD, SEED, FREE, BALL = 0, 1, 2, 3
XPARENT, XEAST, YPARENT, YNORTH = 1, 2, 4, 8


def bits(v):
    return struct.pack("<d", v)


def read(s, t):
    """what a node with slowness s and value t reads as when it is a neighbour"""
    return t if (not R.obstacle(s)) and math.isfinite(t) else INF


def coef(gdx, gdy, l, r, dn, up, s, t):
    """(ca, cb, cs, parents) of a free node whose value is t"""
    a = r if r < l else l
    b = up if up < dn else dn
    if a == INF and b == INF:
        return 0.0, 0.0, 0.0, 0
    ta = a + gdx * s
    tb = b + gdy * s
    ca = cb = cs = 0.0
    if b == INF or ta <= b:
        branch = 0
    elif a == INF or tb <= a:
        branch = 1
    else:
        wx = 1.0 / (gdx * gdx)
        wy = 1.0 / (gdy * gdy)
        A = wx + wy
        B = a * wx + b * wy
        e = a - b
        d = A * (s * s) - (wx * wy) * (e * e)
        q = math.sqrt(d) if d > 0.0 else 0.0
        if q > 0.0:
            tt = (B + q) / A
            ca = (wx * (tt - a)) / q
            cb = (wy * (tt - b)) / q
            cs = s / q
            branch = 2
        else:
            branch = 1 if tb < ta else 0
    if branch == 0:
        ca, cs = 1.0, gdx
    elif branch == 1:
        cb, cs = 1.0, gdy
    par = 0
    if branch != 1:
        if a < t:
            par |= XPARENT | (XEAST if r < l else 0)
        else:
            ca = 0.0
    if branch != 0:
        if b < t:
            par |= YPARENT | (YNORTH if up < dn else 0)
        else:
            cb = 0.0
    return ca, cb, cs, par


class Net:
    """One source's network: per node cls, par, ca, cb, cs, csrc (lists in node order)"""

    def __init__(self, grid, n, xs, ys, n_src, T, filled, ball=2.0):
        gx0, gdx, nx, gy0, gdy, ny = grid
        gx0, gdx, gy0, gdy, nx, ny = float(gx0), float(gdx), float(gy0), float(gdy), int(nx), int(ny)
        g = (gx0, gdx, nx, gy0, gdy, ny)
        nl = [float(v) for v in np.asarray(n, dtype=np.float64).reshape(-1)]
        tl = [float(v) for v in np.asarray(T, dtype=np.float64).reshape(-1)]
        fl = [int(v) for v in np.asarray(filled).reshape(-1)]
        nn = nx * ny
        assert len(nl) == len(tl) == len(fl) == nn
        xs, ys, n_src, ball = float(xs), float(ys), float(n_src), float(ball)
        self.nx, self.ny, self.nn, self.T = nx, ny, nn, tl
        self.cls, self.par = [DEAD] * nn, [0] * nn
        self.ca, self.cb, self.cs, self.csrc = [0.0] * nn, [0.0] * nn, [0.0] * nn, [0.0] * nn
        rd = [read(nl[x], tl[x]) for x in range(nn)]
        for j in range(ny):
            for i in range(nx):
                x = j * nx + i
                if rd[x] == INF:
                    continue
                if not fl[x]:
                    self.cls[x] = SEED
                    continue
                if R.init(g, i, j, nl[x], math.nan, xs, ys, n_src, ball)[0] == R.BALL:
                    X = gx0 + float(i) * gdx
                    Y = gy0 + float(j) * gdy
                    dx = X - xs
                    dy = Y - ys
                    self.cs[x] = self.csrc[x] = 0.5 * math.sqrt(dx * dx + dy * dy)
                    self.cls[x] = BALL
                    continue
                l = rd[x - 1] if i > 0 else INF
                r = rd[x + 1] if i + 1 < nx else INF
                dn = rd[x - nx] if j > 0 else INF
                up = rd[x + nx] if j + 1 < ny else INF
                self.ca[x], self.cb[x], self.cs[x], self.par[x] = coef(gdx, gdy, l, r, dn, up, nl[x], tl[x])
                self.cls[x] = FREE
        self.free = [x for x in range(nn) if self.cls[x] == FREE]
        self.live = [x for x in range(nn) if self.cls[x] != DEAD]

    def orders(self, adjoint, nodes):
        """the four sweeps of a round over `nodes` (a list in node order), as lists"""
        nx, ny = self.nx, self.ny
        rows = [[] for _ in range(ny)]
        for x in nodes:
            rows[x // nx].append(x)
        out = []
        for k in range(4):
            xup = k in (1, 2) if adjoint else k in (0, 3)
            yup = k >= 2 if adjoint else k < 2
            seq = []
            for j in (range(ny) if yup else range(ny - 1, -1, -1)):
                seq.extend(rows[j] if xup else reversed(rows[j]))
            out.append(seq)
        return out

    def run(self, gather, v, nodes, adjoint, order, max_rounds):
        """sweep v in place to the fixed point of gather; (rounds, clean, changes)"""
        if not self.free:
            return 0, 1, 0
        if order == "sorted":
            for x in sorted(nodes, key=lambda x: self.T[x], reverse=adjoint):
                v[x] = gather(x)
            assert all(bits(gather(x)) == bits(v[x]) for x in nodes), "one pass in the order of T is not the fixed point"
            return 1, 1, 0
        seqs = self.orders(adjoint if order == "sweeps" else not adjoint, nodes)
        cap = max_rounds if max_rounds > 0 else R.DEFAULT_ROUNDS
        rounds, clean, changes = 0, 1, 0
        while rounds < cap:
            rounds += 1
            changed = 0
            for seq in seqs:
                for x in seq:
                    t = gather(x)
                    if bits(t) != bits(v[x]):
                        v[x] = t
                        changed += 1
            changes += changed
            clean = int(changed == 0)
            if clean:
                break
        return rounds, clean, changes

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
                k[x] = self.cs[x] * dnl[x]
        par, ca, cb = self.par, self.ca, self.cb

        def gather(x):
            p = par[x]
            acc = 0.0
            if p & XPARENT:
                acc = acc + ca[x] * v[x + 1 if p & XEAST else x - 1]
            if p & YPARENT:
                acc = acc + cb[x] * v[x + nx if p & YNORTH else x - nx]
            return acc + k[x]

        rounds, clean, changes = self.run(gather, v, self.free, False, order, max_rounds)
        return np.array(v).reshape(self.ny, nx), rounds, clean, changes

    def adjoint(self, r, order="sweeps", max_rounds=0):
        """(lam [ny, nx], g [ny, nx], g_src, rounds, clean, changes)"""
        nn, nx, ny = self.nn, self.nx, self.ny
        rl = [float(v) for v in np.asarray(r, dtype=np.float64).reshape(-1)]
        v = [rl[x] if self.cls[x] != DEAD else 0.0 for x in range(nn)]
        par, ca, cb = self.par, self.ca, self.cb
        XE, YN = XPARENT | XEAST, YPARENT | YNORTH

        def gather(x):
            i, j = x % nx, x // nx
            acc = rl[x]
            if i > 0 and par[x - 1] & XE == XE:
                acc = acc + ca[x - 1] * v[x - 1]
            if i + 1 < nx and par[x + 1] & XE == XPARENT:
                acc = acc + ca[x + 1] * v[x + 1]
            if j > 0 and par[x - nx] & YN == YN:
                acc = acc + cb[x - nx] * v[x - nx]
            if j + 1 < ny and par[x + nx] & YN == YPARENT:
                acc = acc + cb[x + nx] * v[x + nx]
            return acc

        rounds, clean, changes = self.run(gather, v, self.live, True, order, max_rounds)
        g = [self.cs[x] * v[x] if self.cls[x] >= FREE else 0.0 for x in range(nn)]
        g_src = 0.0
        for x in range(nn):
            if self.cls[x] == BALL:
                g_src = g_src + self.csrc[x] * v[x]
        return np.array(v).reshape(ny, nx), np.array(g).reshape(ny, nx), g_src, rounds, clean, changes


def nets(grid, n, sources, n_src, fill, ball=2.0):
    """the network of every source of a fill result (a dict with T and filled [S, ny, nx])"""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_src, dtype=np.float64).reshape(-1)
    return [Net(grid, n, src[s, 0], src[s, 1], ns[s], fill["T"][s], fill["filled"][s], ball) for s in range(len(src))]


def tangent(nets_, dn, dn_src=None, dT_seed=None, max_rounds=0):
    """dict of dT [S, ny, nx], rounds [S], converged [S], changes"""
    S = len(nets_)
    out = {"dT": [], "rounds": np.zeros(S, dtype=np.int32), "converged": np.zeros(S, dtype=np.int32), "changes": 0}
    for s, net in enumerate(nets_):
        v, r, c, ch = net.tangent(dn, 0.0 if dn_src is None else np.asarray(dn_src, dtype=np.float64).reshape(-1)[s],
                                  None if dT_seed is None else np.asarray(dT_seed)[s], max_rounds=max_rounds)
        out["dT"].append(v)
        out["rounds"][s], out["converged"][s] = r, c
        out["changes"] += ch
    out["dT"] = np.stack(out["dT"]) if S else np.zeros((0, 0, 0))
    return out


def adjoint(nets_, r, max_rounds=0):
    """dict of lam, g [S, ny, nx], g_src [S], rounds [S], converged [S], changes"""
    S = len(nets_)
    out = {"lam": [], "g": [], "g_src": np.zeros(S), "rounds": np.zeros(S, dtype=np.int32), "converged": np.zeros(S, dtype=np.int32),
           "changes": 0}
    for s, net in enumerate(nets_):
        lam, g, gs, rr, c, ch = net.adjoint(np.asarray(r)[s], max_rounds=max_rounds)
        out["lam"].append(lam)
        out["g"].append(g)
        out["g_src"][s], out["rounds"][s], out["converged"][s] = gs, rr, c
        out["changes"] += ch
    out["lam"], out["g"] = np.stack(out["lam"]), np.stack(out["g"])
    return out


def same_but_nan(a, b):
    """NaN at the same places and the same bits everywhere else (a NaN's payload is the processor's, not the definition's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.isnan(a)
    return a.shape == b.shape and np.array_equal(na, np.isnan(b)) and R.same_bits(np.where(na, 0.0, a), np.where(na, 0.0, b))


# ---------------------------------------------------------------------------------------------- media and fills for the tests
GRADIENT_GRID = (-2.0, 7.0 / 70, 71, -2.5, 3.5 / 56, 57)
GRADIENT_SOURCES = ((-1.97, -2.03), (1.513, -0.77))
CORRIDOR_GRID = (0.0, 1.0, 31, 0.0, 1.0, 27)
WALLS_GRID = (-1.0, 0.1, 37, 0.5, 0.125, 29)


def gradient_case():
    """the 71 x 57 gradient medium of DESIGN.md section 34, n = 1 / (18 + 2 y), with both of its sources, from the ball alone"""
    X, Y = R.nodes(GRADIENT_GRID)
    n = 1.0 / (18.0 + 2.0 * Y)
    src = np.array(GRADIENT_SOURCES)
    ns = 1.0 / (18.0 + 2.0 * src[:, 1])
    return GRADIENT_GRID, n, src, ns, None


def corridor_case():
    """the winding corridor with three sources: its outer end, the middle, a far corner"""
    n, (ix, iy) = R.winding_corridor()
    src = np.array([[ix + 0.25, iy - 0.125], [15.0, 13.0], [29.0 - 0.5, 1.0 + 0.375]])
    return CORRIDOR_GRID, n, src, np.ones(3), None


def disc_case():
    """the gradient medium with a table that is the closed form everywhere but in a disc of radius 0.7 round (3, -1)"""
    grid, n, src, ns, _ = gradient_case()
    X, Y = R.nodes(grid)
    T = np.stack([np.where((X - 3.0) ** 2 + (Y + 1.0) ** 2 <= 0.49, np.nan, R.gradient_truth(X, Y, xs, ys)) for xs, ys in src])
    return grid, n, src, ns, T


def walls_case():
    """a smooth medium with a wall of NaN and a wall of negative n, each with a gap, a sealed pocket behind obstacles of every
    kind, and a few seeds"""
    X, Y = R.nodes(WALLS_GRID)
    n = 1.0 + 0.2 * (X + 1.0) + 0.3 * np.exp(-((X - 0.8) ** 2 + (Y - 2.2) ** 2))
    n[4:29, 12] = np.nan
    n[0:22, 25] = -1.0
    n[8:15, 30] = n[8, 30:36] = n[14, 30:36] = n[8:15, 35] = 0.0
    n[20, 3], n[2, 20] = np.inf, 0.0
    src = np.array([[-0.43, 1.31], [2.21, 3.87]])
    ns = 1.0 + 0.2 * (src[:, 0] + 1.0) + 0.3 * np.exp(-((src[:, 0] - 0.8) ** 2 + (src[:, 1] - 2.2) ** 2))
    T = np.full((2,) + n.shape, np.nan)
    T[0, 25, 5:9], T[1, 3, 15:18], T[1, 10, 12] = 2.5, 1.75, 1.0          # seeds; the last on an obstacle, which is no seed
    return WALLS_GRID, n, src, ns, T


def filled(case, max_rounds=0):
    """(grid, n, src, n_src, fill result of the restatement, the networks) of a case"""
    grid, n, src, ns, T = case
    fill = R.solve(grid, n, src, ns, T=T, max_rounds=max_rounds)
    return grid, n, src, ns, fill, nets(grid, n, src, ns, fill)


# ------------------------------------------------------------------------------------ one Gauss-Newton step of tomography
def source_weights(sources, grid):
    """the bilinear weights of each source's cell, for sources inside the grid: (idx [S, 4] node indices, w [S, 4])"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    u, v = (src[:, 0] - gx0) / gdx, (src[:, 1] - gy0) / gdy
    i0 = np.clip(np.floor(u).astype(np.int64), 0, nx - 2)
    j0 = np.clip(np.floor(v).astype(np.int64), 0, ny - 2)
    fu, fv = u - i0, v - j0
    idx = np.stack([j0 * nx + i0, j0 * nx + i0 + 1, (j0 + 1) * nx + i0, (j0 + 1) * nx + i0 + 1], axis=1)
    return idx, np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], axis=1)


def tomography_case():
    """The 71 x 57 gradient medium as the background, the truth a Gaussian slowness anomaly of 4 % on it, eight sources just
    inside the west and south edges, receivers at every fourth node of the east and north edges; n_src is the bilinear
    interpolation of n, so that it follows the medium.  -> grid, n0, n_true, src, receivers (node indices), idx, w"""
    grid = GRADIENT_GRID
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = R.nodes(grid)
    n0 = 1.0 / (18.0 + 2.0 * Y)
    n_true = n0 * (1.0 + 0.04 * np.exp(-((X - 1.6) ** 2 + (Y + 0.8) ** 2) / 0.8 ** 2))
    src = np.array([[gx0 + 0.35 * gdx, gy0 + (7.3 + 14 * k) * gdy] for k in range(4)] +
                   [[gx0 + (8.6 + 17 * k) * gdx, gy0 + 0.4 * gdy] for k in range(4)])
    rec = np.array([j * nx + nx - 1 for j in range(0, ny, 4)] + [(ny - 1) * nx + i for i in range(0, nx - 1, 4)])
    idx, w = source_weights(src, grid)
    return grid, n0, n_true, src, rec, idx, w


TOMO_DAMP, TOMO_ITERS = 1e-3, 40


def tomography_step(solve, jacobian):
    """One damped LSQR step from the background: solve(n, n_src) -> (T [S, ny, nx], state), jacobian(state) -> a matrix or
    LinearOperator [S R, ny nx].  -> (rms residual before, after, the step [ny, nx])"""
    from scipy.sparse.linalg import lsqr
    grid, n0, n_true, src, rec, idx, w = tomography_case()
    at = lambda T: T.reshape(len(src), -1)[:, rec].reshape(-1)      # noqa: E731
    ns = lambda n: (n.reshape(-1)[idx] * w).sum(axis=1)             # noqa: E731
    data = at(solve(n_true, ns(n_true))[0])
    T0, state = solve(n0, ns(n0))
    r0 = data - at(T0)
    step = lsqr(jacobian(state), r0, damp=TOMO_DAMP, iter_lim=TOMO_ITERS, atol=0.0, btol=0.0)[0].reshape(n0.shape)
    n1 = n0 + step
    r1 = data - at(solve(n1, ns(n1))[0])
    rms = lambda r: float(np.sqrt(np.mean(r * r)))                  # noqa: E731
    return rms(r0), rms(r1), step


def dense_jacobian(nets_, rec, idx, w):
    """The restatement's Jacobian at the receivers, one adjoint solve per row, n_src chained through the bilinear weights"""
    nn = nets_[0].nn
    J = np.zeros((len(nets_) * len(rec), nn))
    for s, net in enumerate(nets_):
        for k, x in enumerate(rec):
            r = np.zeros(nn)
            r[x] = 1.0
            _, g, g_src, _, _, _ = net.adjoint(r, order="sorted")
            row = J[s * len(rec) + k]
            row += g.reshape(-1)
            np.add.at(row, idx[s], g_src * w[s])
    return J
